"""The Chebyshev preconditioner without a GPU: the CPU restatement (tests/chebyshev_restatement.py, the definition the device code is
compared with) is the polynomial include/smm_hip.h says it is, is symmetric for a symmetric matrix and halves ConjugateGradient's
iteration count; the public surfaces (Python enum, exported symbols, the drop-in C++ header) exist."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from chebyshev_restatement import coefficients, diagonal, gershgorin, make_apply, pcg, power_bound
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "chebyshev_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/gmres_helpers.py for tests/cpp/chebyshev_case.cpp"""
    exe = tmp_path / "chebyshev_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def spd5(dtype):
    """tests/test_gpu_cgs.py's 5 x 5 matrix: symmetric, strictly diagonally dominant, small dyadic values"""
    dense = np.array([[4.5, -1.25, 0, 0, -0.25], [-1.25, 5.0, -0.75, 0, 0], [0, -0.75, 4.25, -1.5, 0], [0, 0, -1.5, 6.0, -0.5], [-0.25, 0, 0, -0.5, 3.5]])
    start = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int32)
    pos = np.nonzero(dense)[1].astype(np.int32)
    return start, pos, dense[dense != 0].astype(dtype)


def dense_of(csr):
    start, pos, val = csr
    n = len(start) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(start)), pos] = val
    return A


def inverse_matrix(oracle, csr, degree, lmin, lmax):
    """M^-1 column by column: the restatement applied to the unit vectors"""
    n = len(csr[0]) - 1
    fn = make_apply(oracle, csr, degree, lmin, lmax)
    return np.stack([fn(e) for e in np.eye(n)], axis=1)


CASES = {"spd5": lambda: spd5(np.float64), "poisson2d_6": lambda: gen.poisson2d(6, dtype=np.float64)}


@pytest.mark.parametrize("degree", [0, 1, 2, 5])
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_the_chebyshev_polynomial(oracle, name, degree):
    """I - M^-1 A is a polynomial in D^-1 A: its eigenvalues are T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma) over the eigenvalues
    lambda of D^-1 A, to 1e-12 in fp64 (both spectra through the symmetric similarity D^1/2 . D^-1/2); M^-1 is symmetric."""
    csr = CASES[name]()
    A = dense_of(csr)
    n = len(A)
    lmax = gershgorin(csr)
    lmin = lmax / 30
    Minv = inverse_matrix(oracle, csr, degree, lmin, lmax)
    asym = float(np.max(np.abs(Minv - Minv.T)))
    root = np.sqrt(diagonal(csr))
    lam = np.linalg.eigvalsh(A / np.outer(root, root))
    E = np.eye(n) - Minv @ A
    S = E * np.outer(root, 1 / root)  # D^1/2 E D^-1/2: symmetric
    got = np.sort(np.linalg.eigvalsh((S + S.T) / 2))
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    cheb = np.polynomial.chebyshev.Chebyshev.basis(degree + 1)
    want = np.sort(cheb((theta - lam) / delta) / cheb(theta / delta))
    err = float(np.max(np.abs(got - want)))
    print(name, degree, "max eigenvalue error", err, "asymmetry of M^-1", asym, "largest |residual polynomial|", float(np.max(np.abs(want))))
    assert err <= 1e-12
    assert asym <= 1e-14 * float(np.max(np.abs(Minv)))
    assert float(np.max(np.abs(S - S.T))) <= 1e-12
    assert lam.max() <= lmax * (1 + 1e-14)  # Gershgorin is a bound


def test_pcg_needs_at_most_half_the_iterations(oracle):
    """poisson2d_32 in fp64 at eps 1e-8 from x0 = 0, b = A 1: degree 3 against the oracle's ConjugateGradient (measured: 21 against 65)"""
    eps = 1e-8
    csr = gen_matrices(np.float64)["poisson2d_32"]
    b = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(len(b))
    st_ref, _, it_ref, _ = oracle.cg(csr, b, zero, -1, eps)
    lmax = gershgorin(csr)
    st, x, it, rr = pcg(oracle, csr, b, zero, -1, eps, make_apply(oracle, csr, 3, lmax / 30, lmax))
    print("iterations", it, "unpreconditioned", it_ref, "r.r", rr, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0 and rr < eps * eps
    assert 0 < it <= it_ref // 2
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
def test_bounds_and_coefficients(oracle, dtype):
    """the 5-point Laplacian: every interior row sums to 8 / 4; the power heuristic stays below Gershgorin; the coefficients' recurrence"""
    csr = gen_matrices(dtype)["poisson2d_32"]
    assert gershgorin(csr) == 2.0
    assert 1.5 < power_bound(oracle, csr, 10) <= 2.0
    inv_theta, c1, c2 = coefficients(2, 0.5, 1.5, dtype)
    # theta = 1, delta = 0.5, sigma = 2: rho = 1/2, 2/7, 7/26
    assert inv_theta == dtype(1.0) and c1[1] == dtype((2 / 7) * 0.5) and c2[1] == dtype(2 * (1.0 / (4.0 - 0.5)) / 0.5)
    assert len(c1) == len(c2) == 3 and all(isinstance(c, dtype) for c in c1 + c2)


def test_public_surface():
    """the enum member and the two entry points: what the parent of this feature does not have"""
    assert host.SolverPreconditioner.CHEBYSHEV == 7
    assert host.SolverPreconditioner["CHEBYSHEV"].value == 7
    assert (host.CHEB_BOUND_GERSHGORIN, host.CHEB_BOUND_POWER, host.CHEB_BOUND_USER) == (0, 1, 2)
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in ("smm_hip_precond_create_chebyshev", "smm_hip_precond_chebyshev_info"):
            assert hasattr(lib, name), (name, fma)
            assert name in _lib.exported_symbols()
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    assert "#define SMM_PRECOND_CHEBYSHEV 7" in header
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, host.SolverPreconditioner.JACOBI, degree=2)  # refused before the handle is touched


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::ChebyshevPreconditioner<float> / <double> through ConjugateGradient, BiCGStab and GMRES; -Wall -Werror.  Without a GPU every
    call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {f"{t}-{s}" for t in ("float", "double") for s in ("cg", "bicgstab", "gmres")}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip) == (0, 0), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name.startswith("float") else 1e-6)
        else:
            assert (status, hip) == (1, -3), words
