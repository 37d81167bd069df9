"""lobpcg without a GPU: the CPU restatement of the algorithm (tests/lobpcg_restatement.py, the definition the GPU driver is compared with)
meets on every case of tests/lobpcg_cases.py every bound that tests/test_gpu_lobpcg.py puts on the GPU's answer, within half the
iteration cap; its edge paths give what the contract says; the restatements of the two block kernels agree with fp64; the new symbols
are declared, exported and bound; and the argument checks answer SMM_HIP_ERR_INVALID before a device is asked for."""
import ctypes
import os
import re
import subprocess

import lobpcg_cases as cases
import numpy as np
import pytest
from lobpcg_restatement import DIVERGED, LARGEST, MAX_ITERATIONS_REACHED, SMALLEST, SUCCESS, block_axpy, gram, lobpcg, orthonormalise, start_block

from sparse_matrix_math_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
WHICH = {"LA": LARGEST, "SA": SMALLEST}
NEW_SYMBOLS = [f"smm_hip_{base}_{suf}" for base in ("lobpcg", "lobpcg_dev", "multi_gram_dev", "multi_block_axpy_dev") for suf in ("f32", "f64")]
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def working(csr, dtype):
    return cases.dense(csr).astype(dtype)


def test_the_case_list():
    assert len(cases.combos()) == 22 and ("chain_96", "LA", 1) not in cases.combos()
    assert all(3 * k <= cases.ROWS[name] and k <= cases.MAX_K for name, _, k in cases.combos())
    ev = np.linalg.eigvalsh(cases.dense(cases.lap2d_16x16()))
    assert abs(ev[1] - ev[2]) <= 1e-12 and abs(ev[4] - ev[5]) <= 1e-12 and ev[6] - ev[5] >= 0.05  # two double values among six, a clean cut


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k", cases.combos(), ids=_ID)
def test_restatement_meets_the_gpu_bounds(name, which, k, dtype):
    """against numpy.linalg.eigvalsh of the dense matrix: the bounds of tests/test_gpu_lobpcg.py as ratios, all <= 1; at most 500
    iterations, half the cap; the orthonormality ratio stays under ORTH_WORST, from which the GPU test takes its bound"""
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    lam = cases.exact(name)
    norm_a = float(np.max(np.abs(lam)))
    r = lobpcg(working(cases.matrix(name, dtype), dtype), k, WHICH[which], cases.MAX_ITERATIONS, tol)
    w, X = r["w"].astype(np.float64), r["X"].astype(np.float64)
    a64 = cases.dense(cases.matrix(name))
    err = float(np.max(np.abs(w - cases.wanted(lam, which, k)))) / (10 * tol * norm_a)
    res = float(np.max(np.linalg.norm(a64 @ X - X * w, axis=0))) / (10 * tol * norm_a)
    rn = float(np.max(r["residuals"])) / (tol * norm_a)
    orth = float(np.max(np.abs(X.T @ X - np.eye(k)))) / eps
    print(name, which, k, np.dtype(dtype).name, "iterations", r["iterations"], "err / (10 tol |A|)", err, "true residual / (10 tol |A|)", res, "rn / (tol |A|)", rn,
          "max|X^T X - I| / eps", orth)
    assert r["status"] == SUCCESS and r["nconv"] == k
    assert err <= 1 and res <= 1 and rn <= 1
    assert r["iterations"] <= 500
    assert r["matvecs"] <= k + k * r["iterations"] and r["applies"] == 0
    assert orth <= cases.ORTH_WORST[np.dtype(dtype)]
    assert np.all(np.diff(w) < 0) if which == "LA" else np.all(np.diff(w) > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_restatement_multiple_eigenvalues(dtype):
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    csr = cases.lap2d_16x16(dtype)
    lam = np.linalg.eigvalsh(cases.dense(cases.lap2d_16x16()))
    r = lobpcg(working(csr, dtype), 6, SMALLEST, cases.MAX_ITERATIONS, tol)
    print("lap2d_16x16", np.dtype(dtype).name, r["iterations"])
    assert r["status"] == SUCCESS and float(np.max(np.abs(r["w"].astype(np.float64) - lam[:6]))) <= 10 * tol * lam[-1]
    a = working(cases.triple_diagonal(dtype), dtype)
    for which, value, rows in ((LARGEST, 5.0, slice(0, 40)), (SMALLEST, 1.0, slice(20, 60))):
        r = lobpcg(a, 3, which, cases.MAX_ITERATIONS, tol)
        X = r["X"].astype(np.float64)
        assert r["status"] == SUCCESS and float(np.max(np.abs(r["w"].astype(np.float64) - value))) <= 10 * tol * 5.0
        assert float(np.max(np.abs(X[rows]))) <= 100 * eps  # inside the eigenspace: nothing on the rows of the other values


def test_restatement_edges():
    for dtype in DTYPES:  # every start block is an invariant subspace: the residual is the normalisation's rounding, a few eps
        r = lobpcg(np.eye(50, dtype=dtype), 3, SMALLEST, 10, cases.TOL[np.dtype(dtype)])
        assert r["status"] == SUCCESS and r["iterations"] == 0 and r["matvecs"] == 3
        assert float(np.max(r["residuals"])) <= 8 * float(np.finfo(dtype).eps)
    r = lobpcg(np.diag(np.arange(1.0, 25.0)), 8, SMALLEST, cases.MAX_ITERATIONS, 1e-10)  # 3k == rows: S spans everything
    assert r["status"] == SUCCESS and float(np.max(np.abs(r["w"] - np.arange(1.0, 9.0)))) <= 1e-8
    a = working(cases.matrix("chain_96"), np.float64)
    X0 = start_block(96, 4, 0, np.float64)
    one, two = lobpcg(a, 4, SMALLEST, 1000, 1e-10), lobpcg(a, 4, SMALLEST, 1000, 1e-10, X0=X0)
    assert np.array_equal(one["X"], two["X"]) and np.array_equal(one["w"], two["w"])
    X0[:, 2] = X0[:, 0]
    assert lobpcg(a, 4, SMALLEST, 1000, 1e-10, X0=X0)["status"] == DIVERGED and orthonormalise(X0) is None
    r = lobpcg(a, 4, SMALLEST, 3, 1e-10)
    assert r["status"] == MAX_ITERATIONS_REACHED and r["iterations"] == 3 and r["nconv"] < 4
    bad = a.copy()
    bad[0, 0] = np.nan
    assert lobpcg(bad, 2, SMALLEST, 5, 1e-10)["status"] == DIVERGED
    sgs = np.tril(a) @ np.diag(1.0 / np.diag(a)) @ np.triu(a)  # the symmetric Gauss-Seidel matrix: a preconditioner cuts the count
    with_m = lobpcg(a, 4, SMALLEST, 1000, 1e-10, M=lambda v: np.linalg.solve(sgs, v))
    assert with_m["status"] == SUCCESS and with_m["iterations"] < one["iterations"] and with_m["matvecs"] == 4 + with_m["applies"]


def test_block_kernels_restated():
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        eps = float(np.finfo(dtype).eps)
        V = rng.uniform(-1, 1, (257, 17)).astype(dtype)
        W = rng.uniform(-1, 1, (257, 24)).astype(dtype)
        exact = V.astype(np.float64).T @ W.astype(np.float64)
        bound = 257 * eps * (np.abs(V).astype(np.float64).T @ np.abs(W).astype(np.float64))
        assert np.all(np.abs(gram(V, W).astype(np.float64) - exact) <= bound)
        H = rng.uniform(-1, 1, (17, 24)).astype(dtype)
        got = block_axpy(V, H, W)
        exact = W.astype(np.float64) - V.astype(np.float64) @ H.astype(np.float64)
        bound = 18 * eps * (np.abs(W).astype(np.float64) + np.abs(V).astype(np.float64) @ np.abs(H).astype(np.float64))
        assert got.dtype == dtype and np.all(np.abs(got.astype(np.float64) - exact) <= bound)


def test_exports_and_wrappers():
    """what the parent of this feature does not have"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smm_hip.h")).read(), flags=re.S)
    so = os.path.join(LIB, "libsmm_hip.so")
    if not os.path.exists(so):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    for fma in (False, True):
        exported = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(fma=fma)], capture_output=True, text=True, timeout=120).stdout
        for name in NEW_SYMBOLS:
            assert re.search(r" T " + name + r"$", exported, re.M), (name, fma)
            assert name in _lib.exported_symbols()
            assert f"{name}(" in text
    for define in ("#define SMM_LOBPCG_MAX_K 8", "#define SMM_LOBPCG_MAX_BASIS 24"):
        assert define in text
    lib = _lib.load()
    assert len(lib.smm_hip_lobpcg_f32.argtypes) == 18 and len(lib.smm_hip_lobpcg_dev_f64.argtypes) == 19
    assert len(lib.smm_hip_multi_gram_dev_f32.argtypes) == 10 and len(lib.smm_hip_multi_block_axpy_dev_f64.argtypes) == 10
    assert lib.smm_hip_lobpcg_f32.argtypes[4] is ctypes.c_float and lib.smm_hip_lobpcg_dev_f64.argtypes[4] is ctypes.c_double
    import sparse_matrix_math_amd as smm

    for name in ("lobpcg", "lobpcg_dev", "multi_gram_dev", "multi_block_axpy_dev"):
        assert callable(getattr(smm, name))
    assert (smm.LOBPCG_MAX_K, smm.LOBPCG_MAX_BASIS) == (cases.MAX_K, cases.MAX_BASIS) == (8, 24)
    assert smm.LobpcgInfo._fields == ("residuals", "nconv", "iterations", "matvecs", "applies", "status")
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus lobpcg(const CSRMatrix<T>& a, int k, int which, T* eigenvalues," in drop_in


def test_argument_checks_answer_before_a_device_is_asked_for():
    """SMM_HIP_ERR_INVALID with a message that starts with the entry point's name, on a machine with or without a GPU, outputs untouched.
    (Every check that needs a matrix handle needs a device to make one: tests/test_gpu_lobpcg.py has those.)"""
    lib = _lib.load()
    P = ctypes.c_void_p
    w = np.full(4, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(5)]
    refs = [ctypes.byref(i) for i in ints]
    assert lib.smm_hip_lobpcg_f64(None, 2, 1, 10, 0.0, None, None, 0, 0, w.ctypes.data_as(P), None, 0, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    assert lib.smm_hip_lobpcg_dev_f32(None, 2, 1, 10, 0.0, None, None, 0, 0, None, None, 0, None, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    assert np.all(w == 7.0) and all(i.value == -5 for i in ints)
    fake = P(4096)  # never dereferenced: the check comes first
    for fn, who in ((lib.smm_hip_multi_gram_dev_f64, "multi_gram:"), (lib.smm_hip_multi_block_axpy_dev_f32, "multi_block_axpy:")):
        for n, m, l, ldv, ldw, ldg, v, ww, gg in ((-1, 4, 4, 64, 64, 4, fake, fake, fake), (64, 0, 4, 64, 64, 4, fake, fake, fake), (64, 4, 0, 64, 64, 4, fake, fake, fake),
                                                  (64, 25, 4, 64, 64, 25, fake, fake, fake), (64, 4, 25, 64, 64, 4, fake, fake, fake), (64, 4, 4, 63, 64, 4, fake, fake, fake),
                                                  (64, 4, 4, 64, 63, 4, fake, fake, fake), (64, 4, 4, 64, 64, 3, fake, fake, fake), (64, 4, 4, 64, 64, 4, None, fake, fake),
                                                  (64, 4, 4, 64, 64, 4, fake, None, fake), (64, 4, 4, 64, 64, 4, fake, fake, None)):
            # (multi_gram: V, ldV, W, ldW, G, ldG;  multi_block_axpy: V, ldV, H, ldH, W, ldW)
            args = (n, m, l, v, ldv, ww, ldw, gg, ldg, None) if who == "multi_gram:" else (n, m, l, v, ldv, gg, ldg, ww, ldw, None)
            assert fn(*args) == _lib.SMM_HIP_ERR_INVALID, (who, n, m, l, ldv, ldw, ldg)
            assert lib.smm_hip_last_error().decode().startswith(who)
    assert lib.smm_hip_multi_block_axpy_dev_f64(0, 4, 4, None, 64, fake, 4, None, 64, None) == _lib.SMM_HIP_OK  # nothing to do: no device either
