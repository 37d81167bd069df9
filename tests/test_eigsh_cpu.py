"""eigsh without a GPU: the test matrices are what tests/eigsh_cases.py says they are, the CPU restatement of the algorithm
(tests/eigsh_restatement.py, the definition the GPU driver is compared with) meets on them every bound that tests/test_gpu_eigsh.py puts
on the GPU's answer, well inside the restart cap; its breakdown paths give what the contract says; the new symbols are declared, exported
and bound; and the argument checks answer SMM_HIP_ERR_INVALID before a device is asked for."""
import ctypes
import os
import re
import subprocess

import eigsh_cases as cases
import numpy as np
import pytest
from eigsh_restatement import DIVERGED, LARGEST, MAX_ITERATIONS_REACHED, SMALLEST, SUCCESS, eigsh, hash_vector, resolve_ncv, rotate

from sparse_matrix_math_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
WHICH = {"LA": LARGEST, "SA": SMALLEST}
NEW_SYMBOLS = [f"smm_hip_{base}_{suf}" for base in ("eigsh", "eigsh_dev", "multi_rotate_dev") for suf in ("f32", "f64")]
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def working(name, dtype):
    return cases.dense(cases.matrix(name, dtype)).astype(dtype)


def test_the_cases_are_what_the_table_says():
    assert cases.NAMES == tuple(cases.ROWS)
    for name in cases.NAMES:
        for dtype in DTYPES:
            csr = cases.matrix(name, dtype)
            a = cases.dense(csr)
            assert csr[2].dtype == dtype and a.shape == (cases.ROWS[name],) * 2 and np.array_equal(a, a.T)
        ev = cases.exact(name)
        ends = [ev[-5:]] + ([ev[:5]] if "SA" in cases.ENDS[name] else [])
        gap = min(float(np.min(np.diff(e))) for e in ends)
        print(name, "smallest gap among the five wanted values at the tested ends", gap)
        assert gap >= 3e-3  # no multiple wanted eigenvalues
    assert float(np.min(np.diff(cases.exact("diag_sq_300")[:5]))) >= 0.01 - 1e-12
    ev = cases.exact("shifted_16x12")
    assert (ev < 0).any() and (ev > 0).any()
    assert len(cases.combos()) == 22


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k,ncv", cases.combos(), ids=_ID)
def test_restatement_meets_the_gpu_bounds(name, which, k, ncv, dtype):
    """against numpy.linalg.eigvalsh of the dense matrix: the bounds of tests/test_gpu_eigsh.py, the restart count far inside the cap"""
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    lam = cases.exact(name)
    norm_a = float(np.max(np.abs(lam)))
    r = eigsh(working(name, dtype), k, WHICH[which], ncv, cases.MAX_RESTARTS, tol)
    w, X = r["w"].astype(np.float64), r["X"].astype(np.float64)
    a64 = cases.dense(cases.matrix(name))
    err = float(np.max(np.abs(w - cases.wanted(lam, which, k))))
    res = np.linalg.norm(a64 @ X - X * w, axis=0)
    rho = r["residuals"].astype(np.float64)
    print(name, which, k, ncv, np.dtype(dtype).name, "restarts", r["restarts"], "err", err, "res", float(np.max(res)), "rho", float(np.max(rho)),
          "true residual / max(rho, eps |A|)", float(np.max(res / np.maximum(rho, eps * norm_a))))
    assert r["status"] == SUCCESS and r["nconv"] == k
    assert r["restarts"] <= 30  # the cap of 100 stays more than three times away
    assert r["matvecs"] == ncv + r["restarts"] * (ncv - (k + (ncv - k) // 2))
    assert err <= 10 * tol * norm_a and float(np.max(res)) <= 10 * tol * norm_a and float(np.max(rho)) <= tol * norm_a
    assert float(np.max(np.abs(X.T @ X - np.eye(k)))) <= 100 * eps
    assert np.all(np.diff(w) < 0) if which == "LA" else np.all(np.diff(w) > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_restatement_breakdowns(dtype):
    eps = float(np.finfo(dtype).eps)
    history = []
    r = eigsh(np.eye(50, dtype=dtype), 3, LARGEST, 8, 100, 0.0, history=history)
    assert r["status"] == SUCCESS and np.max(np.abs(r["w"] - 1)) <= 4 * eps
    assert history == [(1, 0, True), (2, 1, True), (3, 2, True)] and r["restarts"] == 2 and r["matvecs"] == 3
    X = r["X"].astype(np.float64)
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 100 * eps

    r = eigsh(np.diag(np.repeat([1.0, 2.0, 5.0], 20)).astype(dtype), 3, LARGEST, 0, 100, 0.0)
    X = r["X"].astype(np.float64)
    assert r["status"] == SUCCESS and np.max(np.abs(r["w"].astype(np.float64) - 5)) <= 10 * eps * 5
    assert np.max(np.abs(X.T @ X - np.eye(3))) <= 100 * eps and np.max(np.abs(X[:40])) <= 100 * eps

    v0 = np.zeros(192, dtype=dtype)
    v0[[3, 50, 100]] = [1.0, 2.0, 3.0]
    history = []
    r = eigsh(np.diag(np.arange(1.0, 193.0)).astype(dtype), 2, LARGEST, 0, 100, 0.0, v0=v0, history=history)
    assert r["status"] == SUCCESS and history == [(3, 0, True)] and r["matvecs"] == 3
    assert np.max(np.abs(r["w"].astype(np.float64) - [101.0, 51.0])) <= 10 * eps * 101


def test_restatement_edges():
    a = working("chain_96", np.float64)
    r = eigsh(a, 4, LARGEST, 20, 0, 1e-10)  # no restart allowed: the best available pairs, with their estimates
    assert r["status"] == MAX_ITERATIONS_REACHED and r["restarts"] == 0 and r["matvecs"] == 20 and r["nconv"] < 4
    assert len(r["w"]) == 4 and np.all(np.diff(r["w"]) < 0) and float(np.max(r["residuals"])) > 1e-10 * 4
    assert eigsh(a, 2, LARGEST, 0, 5, 1e-10, v0=np.zeros(96))["status"] == DIVERGED  # a start vector without a direction
    bad = a.copy()
    bad[0, 0] = np.nan
    assert eigsh(bad, 2, LARGEST, 0, 5, 1e-10)["status"] == DIVERGED
    assert resolve_ncv(96, 4, 0) == 20 and resolve_ncv(96, 12, 0) == 25 and resolve_ncv(10, 4, 0) == 10 and resolve_ncv(96, 4, 30) == 30


def test_hash_vector_is_the_shadow_generator():
    """the element formula of IDR(s)'s shadow space (tests/idrs_restatement.py), column `col` of seed `seed`"""
    from idrs_restatement import raw_shadow

    for seed in (0, 2011):
        raw = raw_shadow(300, 3, seed, np.float64)
        for col in range(3):
            assert np.array_equal(hash_vector(300, seed, col, np.float64), raw[col])
            assert np.array_equal(hash_vector(300, seed, col, np.float32).astype(np.float64), raw[col])  # exact in fp32


def test_rotate_is_the_product():
    rng = np.random.default_rng(1)
    for dtype in DTYPES:
        V = rng.uniform(-1, 1, (37, 20)).astype(dtype)
        Y = rng.uniform(-1, 1, (20, 12)).astype(dtype)
        exact = V.astype(np.float64) @ Y.astype(np.float64)
        bound = 20 * float(np.finfo(dtype).eps) * (np.abs(V).astype(np.float64) @ np.abs(Y).astype(np.float64))
        assert np.all(np.abs(rotate(V, Y).astype(np.float64) - exact) <= bound)


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
    for define in ("#define SMM_EIGSH_LARGEST 0", "#define SMM_EIGSH_SMALLEST 1", "#define SMM_EIGSH_MAX_NCV 64"):
        assert define in text
    lib = _lib.load()
    assert len(lib.smm_hip_eigsh_f32.argtypes) == 16 and len(lib.smm_hip_eigsh_dev_f64.argtypes) == 17 and len(lib.smm_hip_multi_rotate_dev_f32.argtypes) == 8
    assert lib.smm_hip_eigsh_f32.argtypes[5] is ctypes.c_float and lib.smm_hip_eigsh_dev_f64.argtypes[5] is ctypes.c_double
    import sparse_matrix_math_amd as smm

    for name in ("eigsh", "eigsh_dev", "multi_rotate_dev"):
        assert callable(getattr(smm, name))
    assert (smm.EIGSH_LARGEST, smm.EIGSH_SMALLEST, smm.EIGSH_MAX_NCV) == (0, 1, 64)
    assert smm.EigshInfo._fields == ("residuals", "nconv", "restarts", "matvecs", "status")
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus eigsh(const CSRMatrix<T>& a, int k, int which, T* eigenvalues," in drop_in


def test_argument_checks_answer_before_a_device_is_asked_for():
    """SMM_HIP_ERR_INVALID with a message that starts with the entry point's name, on a machine with or without a GPU, outputs untouched.
    (Every check that needs a matrix handle needs a device to make one: tests/test_gpu_eigsh.py has those.)"""
    lib = _lib.load()
    P = ctypes.c_void_p
    w = np.full(4, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(4)]
    refs = [ctypes.byref(i) for i in ints]
    assert lib.smm_hip_eigsh_f64(None, 2, 0, 0, 10, 0.0, None, 0, w.ctypes.data_as(P), None, 0, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("eigsh:")
    assert lib.smm_hip_eigsh_dev_f32(None, 2, 0, 0, 10, 0.0, None, 0, None, None, 0, None, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("eigsh:")
    assert np.all(w == 7.0) and all(i.value == -5 for i in ints)
    Y = np.eye(4)
    y = Y.ctypes.data_as(P)
    fake = P(4096)  # never dereferenced: the check comes first
    for n, m, l, ld, ldy, v, yy in ((-1, 4, 4, 64, 4, fake, y), (64, 4, 0, 64, 4, fake, y), (64, 3, 4, 64, 4, fake, y), (64, 65, 4, 64, 65, fake, y),
                                    (64, 4, 4, 63, 4, fake, y), (64, 4, 4, 64, 3, fake, y), (64, 4, 4, 64, 4, fake, None), (64, 4, 4, 64, 4, None, y)):
        assert lib.smm_hip_multi_rotate_dev_f64(n, m, l, v, ld, yy, ldy, None) == _lib.SMM_HIP_ERR_INVALID, (n, m, l, ld, ldy)
        assert lib.smm_hip_last_error().decode().startswith("multi_rotate:")
    assert lib.smm_hip_multi_rotate_dev_f32(0, 4, 4, None, 64, y, 4, None) == _lib.SMM_HIP_OK  # nothing to do: no device either
