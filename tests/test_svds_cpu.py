"""svds without a GPU: the test matrices are what tests/svds_cases.py says they are, the CPU restatement of the algorithm
(tests/svds_restatement.py, the definition the GPU driver is compared with) meets on them every bound that tests/test_gpu_svds.py puts
on the GPU's answer, with the restart counts and the loss of orthogonality that svds_cases.py records; its breakdown paths give what the
contract says; the new symbols are declared, exported and bound; and the argument checks answer SMM_HIP_ERR_INVALID before a device is
asked for."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import svds_cases as cases
from svds_restatement import ALPHA, BETA, DIVERGED, MAX_ITERATIONS_REACHED, SUCCESS, resolve_ncv, svds

from sparse_matrix_math_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
NEW_SYMBOLS = [f"smm_hip_{base}_{suf}" for base in ("svds", "svds_dev") for suf in ("f32", "f64")]
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def working(csr_case, dtype):
    rows, cols, csr = csr_case
    return cases.lsqr_cases.dense(csr, cols).astype(dtype)


def orth_loss(Q):
    Q = Q.astype(np.float64)
    return float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))))


def test_the_cases_are_what_the_table_says():
    assert cases.NAMES == tuple(cases.SHAPE)
    for name in cases.NAMES:
        for dtype in DTYPES:
            rows, cols, csr = cases.matrix(name, dtype)
            assert csr[2].dtype == dtype and (rows, cols) == cases.SHAPE[name] == cases.dense(name, dtype).shape
        gap = float(np.min(-np.diff(cases.exact(name)[:7])))
        print(name, "smallest gap among the leading seven singular values", gap)
        assert gap >= 1e-3  # no multiple wanted singular values
    assert np.array_equal(cases.dense("grad2d_33x29_t"), cases.dense("grad2d_33x29").T)
    assert len(cases.combos()) == 14 and set(cases.combos()) == set(cases.RESTARTS)
    assert ("grad2d_33x29", 1, 8) not in cases.combos()  # 73 restarts in the prototype: left out on purpose


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,k,ncv", cases.combos(), ids=_ID)
def test_restatement_meets_the_gpu_bounds(name, k, ncv, dtype):
    """against numpy.linalg.svd of the dense fp64 matrix: the bounds of tests/test_gpu_svds.py, the recorded restart count"""
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    sigma = cases.exact(name)
    norm_a = float(sigma[0])
    r = svds(cases.dense(name, dtype).astype(dtype), k, ncv, cases.MAX_RESTARTS, tol)
    s, U, V = r["s"].astype(np.float64), r["U"].astype(np.float64), r["V"].astype(np.float64)
    a64 = cases.dense(name)
    err = float(np.max(np.abs(s - sigma[:k])))
    res = np.maximum(np.linalg.norm(a64 @ V - U * s, axis=0), np.linalg.norm(a64.T @ U - V * s, axis=0))
    rho = r["residuals"].astype(np.float64)
    loss = max(orth_loss(U), orth_loss(V))
    print(name, k, ncv, np.dtype(dtype).name, "restarts", r["restarts"], "err", err, "res", float(np.max(res)), "rho", float(np.max(rho)),
          "true residual / max(rho, eps |A|)", float(np.max(res / np.maximum(rho, eps * norm_a))), "true residual / (tol |A|)",
          float(np.max(res)) / (tol * norm_a), "orth / eps", loss / eps)  # the second ratio is what the factor 10 of the residual bound has to cover
    assert r["status"] == SUCCESS and r["nconv"] == k
    assert r["restarts"] == cases.RESTARTS[(name, k, ncv)][0 if dtype == np.float64 else 1]
    assert 0 < r["restarts"] <= 30  # the cap of 100 stays more than three times away
    assert r["matvecs"] == 2 * (ncv + r["restarts"] * (ncv - (k + (ncv - k) // 2)))
    assert err <= 10 * tol * norm_a and float(np.max(res)) <= 10 * tol * norm_a and float(np.max(rho)) <= tol * norm_a
    assert loss <= cases.ORTH_LOSS_EPS[np.dtype(dtype)] * eps
    assert np.all(np.diff(s) < 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_restatement_breakdowns(dtype):
    eps = float(np.finfo(dtype).eps)
    history = []
    r = svds(working(cases.identity_over_zero(), dtype), 3, 8, 100, 0.0, history=history)
    assert r["status"] == SUCCESS and np.max(np.abs(r["s"] - 1)) <= 4 * eps
    assert history == [(1, 0, BETA), (2, 1, BETA), (3, 2, BETA)] and r["restarts"] == 2 and r["matvecs"] == 6
    assert max(orth_loss(r["U"]), orth_loss(r["V"])) <= 100 * eps

    want = np.array([3.0, 2.0, 1.0]) * np.sqrt(80.0)
    a = working(cases.blocks_rank3(), dtype)
    r = svds(a, 3, 8, 100, 0.0)
    assert r["status"] == SUCCESS and r["nconv"] == 3 and np.max(np.abs(r["s"].astype(np.float64) - want)) <= 10 * eps * want[0]
    assert max(orth_loss(r["U"]), orth_loss(r["V"])) <= 100 * eps and np.max(np.abs(r["V"][24:])) <= 100 * eps
    history = []
    r = svds(a, 4, 8, 5, 0.0, history=history)
    print(np.dtype(dtype).name, "rank 3, k = 4:", r["status"], r["nconv"], r["s"], history)
    assert np.all(np.isfinite(r["s"])) and np.all(np.isfinite(r["U"])) and np.all(np.isfinite(r["V"]))
    assert np.max(np.abs(r["s"][:3].astype(np.float64) - want)) <= 10 * eps * want[0]
    if r["status"] == SUCCESS:
        assert r["s"][3] <= 100 * eps * r["s"][0]
    else:
        assert r["status"] == MAX_ITERATIONS_REACHED and r["nconv"] == 3

    v0 = np.zeros(192, dtype=dtype)
    v0[[3, 50, 100]] = [1.0, 2.0, 3.0]
    history = []
    r = svds(working(cases.diagonal(np.arange(1.0, 193.0)), dtype), 2, 0, 100, 0.0, v0=v0, history=history)
    assert r["status"] == SUCCESS and r["restarts"] == 0 and len(history) == 1 and history[0][0] == 3 and history[0][2] in (ALPHA, BETA)
    assert np.max(np.abs(r["s"].astype(np.float64) - [101.0, 51.0])) <= 10 * eps * 101


def test_restatement_edges():
    a = cases.dense("tall")
    r = svds(a, 4, 20, 0, 1e-10)  # no restart allowed: the best available triplets, with their estimates
    assert r["status"] == MAX_ITERATIONS_REACHED and r["restarts"] == 0 and r["matvecs"] == 40 and r["nconv"] < 4
    assert len(r["s"]) == 4 and np.all(np.diff(r["s"]) < 0) and float(np.max(r["residuals"])) > 1e-10 * 8
    assert svds(a, 2, 0, 5, 1e-10, v0=np.zeros(144))["status"] == DIVERGED  # a start vector without a direction
    bad = a.copy()
    bad[0, 0] = np.nan
    assert svds(bad, 2, 0, 5, 1e-10)["status"] == DIVERGED
    r = svds(np.zeros((30, 20)), 2, 8, 3, 0.0)  # the zero matrix: alpha-breakdowns at 0, no triplet, never a number that is not finite
    assert r["status"] == MAX_ITERATIONS_REACHED and r["nconv"] == 0 and len(r["s"]) == 0 and r["restarts"] == 3
    assert resolve_ncv(168, 144, 4, 0) == 20 and resolve_ncv(168, 144, 12, 0) == 25 and resolve_ncv(10, 300, 4, 0) == 10 and resolve_ncv(96, 96, 4, 30) == 30


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
    assert "#define SMM_SVDS_MAX_NCV 64" in text
    lib = _lib.load()
    assert len(lib.smm_hip_svds_f32.argtypes) == 18 and len(lib.smm_hip_svds_dev_f64.argtypes) == 19
    assert lib.smm_hip_svds_f32.argtypes[5] is ctypes.c_float and lib.smm_hip_svds_dev_f64.argtypes[5] is ctypes.c_double
    import sparse_matrix_math_amd as smm

    for name in ("svds", "svds_dev"):
        assert callable(getattr(smm, name))
    assert callable(smm.CSRMatrix.norm2)
    assert smm.SVDS_MAX_NCV == 64
    assert smm.SvdsInfo._fields == smm.EigshInfo._fields == ("residuals", "nconv", "restarts", "matvecs", "status")
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus svds(const CSRMatrix<T>& a, int k, T* singularValues," in drop_in and "T norm2(T tol" in drop_in


def test_argument_checks_answer_before_a_device_is_asked_for():
    """SMM_HIP_ERR_INVALID with a message that starts with the entry point's name, on a machine with or without a GPU, outputs untouched.
    (Every check that needs a matrix handle needs a device to make one: tests/test_gpu_svds.py has those.)"""
    lib = _lib.load()
    P = ctypes.c_void_p
    s = np.full(4, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(4)]
    refs = [ctypes.byref(i) for i in ints]
    assert lib.smm_hip_svds_f64(None, None, 2, 0, 10, 0.0, None, 0, s.ctypes.data_as(P), None, 0, None, 0, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("svds:")
    assert lib.smm_hip_svds_dev_f32(None, None, 2, 0, 10, 0.0, None, 0, None, None, 0, None, 0, None, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("svds:")
    assert np.all(s == 7.0) and all(i.value == -5 for i in ints)
