"""The three systems tests/test_gpu_longrows.py runs the solver loops on, each with dense rows: a KKT matrix for MINRES, a symmetric positive
definite arrow matrix for ConjugateGradient and a tall matrix with a dense column for LSQR.  tests/test_longrows_cpu.py checks on the CPU
that they are what they claim to be (definiteness, convergence of the MINRES restatement)."""
import numpy as np

from sparse_matrix_math_amd import generators as gen


def from_dense(D, dtype):
    mask = D != 0
    start = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    return start, np.nonzero(mask)[1].astype(np.int32), D[mask].astype(dtype)


def poisson_dense(n):
    s, p, v = gen.poisson2d(n, dtype=np.float64)
    D = np.zeros((n * n, n * n))
    D[np.repeat(np.arange(n * n), np.diff(s)), p] = v
    return D


def kkt_system(dtype):
    """[[H, Bt], [B, 0]] with H = poisson2d(24) and two dense constraint rows"""
    H = poisson_dense(24)
    n = len(H)
    rng = np.random.default_rng(51)
    B = rng.uniform(0.5, 1.5, (2, n)) / 16
    D = np.block([[H, B.T], [B, np.zeros((2, 2))]])
    csr = from_dense(D, dtype)
    return csr, gen.row_sums(csr[0], csr[2]), D


def arrow_system(dtype):
    """poisson2d(24) plus one dense row and its column, the diagonal raised: symmetric positive definite"""
    H = poisson_dense(24)
    n = len(H)
    D = np.zeros((n + 1, n + 1))
    D[:n, :n] = H + np.eye(n)
    D[n, :n] = D[:n, n] = 0.03125
    D[n, n] = 2.0
    csr = from_dense(D, dtype)
    return csr, gen.row_sums(csr[0], csr[2]), D


def tall_system(dtype):
    """300 x 40, a few entries per row and one dense column (the intercept): a dense row of the transpose"""
    s, p, v = gen.random_rows(300, 40, 2, 5, seed=52)
    D = np.zeros((300, 40))
    D[np.repeat(np.arange(300), np.diff(s)), p] = v
    D[:, 7] = 0.25
    csr = from_dense(D, dtype)
    x_true = np.random.default_rng(53).uniform(-1, 1, 40)
    return csr, from_dense(D.T.copy(), dtype), (D @ x_true).astype(dtype), D
