"""The matrices and right-hand sides of the MINRES tests (tests/test_minres_cpu.py, tests/test_gpu_minres.py): symmetric, all but one
indefinite, all small.  Built from sparse_matrix_math_amd.generators.

  shifted2d_16    poisson2d(16, 16) - 1.0 I    256 rows, 19 negative eigenvalues, smallest |lambda| 0.044
  shifted2d_16b   poisson2d(16, 16) - 3.1 I    256 rows, 83 negative eigenvalues
  shifted2d_12    poisson2d(12, 12) - 1.0 I    144 rows
  spd             poisson2d(32, 32)            1024 rows, positive definite
  saddle          [[K, B^T], [B, 0]], K = poisson2d(12, 12), B 24 x 144 with rows +e(6 j) - e(6 j + 3): disjoint supports, so full rank;
                  168 rows, 24 negative eigenvalues, and the last 24 rows store NO diagonal entry

The right-hand sides are seeded uniform in [-1, 1): the row sums excite only a few eigenvectors on these symmetric grids and MINRES
then ends in about ten steps."""
import numpy as np

from sparse_matrix_math_amd import generators as gen

SHIFTED = {"shifted2d_16": (16, 1.0), "shifted2d_16b": (16, 3.1), "shifted2d_12": (12, 1.0)}
NAMES = ("shifted2d_16", "shifted2d_16b", "shifted2d_12", "spd", "saddle")
INDEFINITE = ("shifted2d_16", "shifted2d_16b", "shifted2d_12", "saddle")
# negative eigenvalues (numpy.linalg.eigvalsh); the saddle matrix has as many as B has rows
NEGATIVE = {"shifted2d_16": 19, "shifted2d_16b": 83, "saddle": 24}
SADDLE_K, SADDLE_B = 12, 24


def shifted2d(n, sigma, dtype=np.float64):
    """poisson2d(n, n) - sigma I: the diagonal is stored in every row, so the shift is a subtraction on it"""
    start, pos, val = gen.poisson2d(n, n, dtype=dtype)
    val = val.copy()
    rows = np.repeat(np.arange(len(start) - 1), np.diff(start))
    val[pos == rows] -= np.dtype(dtype).type(sigma)
    return start, pos, val


def saddle(dtype=np.float64):
    start, pos, val = gen.poisson2d(SADDLE_K, SADDLE_K, dtype=dtype)
    nk = len(start) - 1
    rows = [[(int(pos[k]), float(val[k])) for k in range(start[r], start[r + 1])] for r in range(nk)]
    for j in range(SADDLE_B):
        plus, minus = 6 * j, 6 * j + 3
        rows[plus].append((nk + j, 1.0))
        rows[minus].append((nk + j, -1.0))
        rows.append([(plus, 1.0), (minus, -1.0)])
    out_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    out_pos = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    out_val = np.array([v for r in rows for _, v in r], dtype=dtype)
    return out_start, out_pos, out_val


def matrix(name, dtype=np.float64):
    if name in SHIFTED:
        return shifted2d(*SHIFTED[name], dtype=dtype)
    if name == "spd":
        return gen.poisson2d(32, 32, dtype=dtype)
    if name == "saddle":
        return saddle(dtype)
    raise KeyError(name)


def unshifted(name, dtype=np.float64):
    """the positive definite relative a preconditioner is built on: the Laplacian without the shift"""
    n = SHIFTED[name][0]
    return gen.poisson2d(n, n, dtype=dtype)


def rhs(name, dtype=np.float64, seed=0):
    rows = len(matrix(name, dtype)[0]) - 1
    return np.random.default_rng(1000 + seed + NAMES.index(name)).uniform(-1.0, 1.0, rows).astype(dtype)


def dense(csr):
    start, pos, val = csr
    rows = len(start) - 1
    out = np.zeros((rows, rows), dtype=np.float64)
    r = np.repeat(np.arange(rows), np.diff(start))
    out[r, pos] = val
    return out
