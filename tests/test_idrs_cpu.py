"""IDR(s) without a GPU: the CPU restatement (tests/idrs_restatement.py, the definition the GPU loop is compared with) converges, its
generated shadow space is the stated hash made orthonormal, the library exports the new entry points, the fixed-step cases of
tests/test_gpu_idrs.py are well enough conditioned to be compared, and tests/cpp/idrs_case.cpp compiles and links against the drop-in
header for float and double with -Wall -Werror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from idrs_helpers import FIXED, LIB, ROOT, SEED, build_case, matrix, near_breakdown, reference, shadow_space
from idrs_restatement import idrs, raw_shadow, shadow, shadow_hash

from sparse_matrix_math_amd import _lib

NEW_SYMBOLS = [f"smm_hip_idrs{kind}_{suf}" for kind in ("", "_dev", "_shadow_dev") for suf in ("f32", "f64")]


@pytest.mark.parametrize("s", [1, 4, 8])
@pytest.mark.parametrize("mname", ["poisson2d_32", "convdiff3d_12"])
def test_restatement_converges_to_ones(oracle, mname, s):
    """the bounds of tests/test_cgs_cpu.py; s = 1 is mathematically BiCGStab"""
    eps = 1e-6
    csr, b = matrix(mname, np.float64)
    st, x, it, rr = idrs(oracle, csr, b, np.zeros(len(b)), -1, eps, s, shadow_space(oracle, len(b), s, np.float64))
    print(mname, s, "SpMVs", it, "r.r", rr, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == 0 and 0 < it < len(b)
    assert rr <= eps * eps  # it left by the residual test, not by the step count
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


def test_restatement_edges(oracle):
    csr, b = matrix("poisson2d_32", np.float64)
    rows = len(b)
    P = shadow_space(oracle, rows, 4, np.float64)
    st, x, it, _ = idrs(oracle, csr, b, np.zeros(rows), 0, 1e-6, 4, P)
    assert (st, it) == (2, 0) and not x.any()
    ones = np.ones(rows)
    st, x, it, rr = idrs(oracle, csr, b, ones, -1, 1e-6, 4, P)
    assert (st, it, rr) == (0, 0, 0.0) and np.array_equal(x, ones)
    # -1 means rows
    free = idrs(oracle, csr, b, np.zeros(rows), -1, 1e-6, 4, P)
    capped = idrs(oracle, csr, b, np.zeros(rows), rows, 1e-6, 4, P)
    assert free[0] == capped[0] == 0 and free[2] == capped[2] and np.array_equal(free[1], capped[1])
    # the rotation [[0, 1], [-1, 0]] with b = e1, s = 1 and P = e1: M[0][0] = p . A r = 0 at the first step
    rot = (np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([1.0, -1.0]))
    e1 = np.array([1.0, 0.0])
    st, x, it, rr = idrs(oracle, rot, e1, np.zeros(2), -1, 1e-6, 1, e1.reshape(1, 2))
    assert (st, it, rr) == (1, 0, 1.0) and not x.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
def test_generated_shadow_space(oracle, dtype):
    """the raw values are the stated hash, exact in both dtypes; the finished columns are orthonormal to 16 u"""
    rows, s = 1000, 8
    raw = raw_shadow(rows, s, SEED, dtype)
    for col, row in ((0, 0), (3, 999), (7, 500)):
        h = shadow_hash(SEED, col, row)
        assert float(raw[col, row]) == ((h >> 40) + 0.5) * 2.0 ** -23 - 1  # (the right side is exact in fp64)
    assert np.array_equal(raw.astype(np.float64), raw_shadow(rows, s, SEED, np.float64))
    assert np.all(np.abs(raw) < 1)
    P = shadow(oracle, rows, s, SEED, dtype).astype(np.float64)
    gram = P @ P.T
    worst = float(np.max(np.abs(gram - np.eye(s))))
    print(np.dtype(dtype).name, "max|P^T P - I|", worst, "16 u", 16 * float(np.finfo(dtype).eps))
    assert worst <= 16 * float(np.finfo(dtype).eps)


def test_hash_values_are_pinned():
    assert shadow_hash(0, 0, 0) == 0x238275BC38FCBE91
    assert shadow_hash(2011, 3, 1000) == 0xD8BAFDF0B47E8D8E
    assert shadow_hash(2 ** 63 + 5, 7, 123456789) == 0xB151BA2DF94CAB15


def test_exports_and_wrappers():
    """what the parent of this feature does not have"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smm_hip.h")).read(), flags=re.S)
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), (name, fma)
            assert name in _lib.exported_symbols()
            assert f"{name}(" in text
    assert "#define SMM_IDRS_MAX_S 8" in text
    lib = _lib.load()
    assert len(lib.smm_hip_idrs_f32.argtypes) == 11 and len(lib.smm_hip_idrs_dev_f64.argtypes) == 14 and len(lib.smm_hip_idrs_shadow_dev_f32.argtypes) == 6
    assert lib.smm_hip_idrs_f32.argtypes[4] is ctypes.c_float and lib.smm_hip_idrs_dev_f64.argtypes[4] is ctypes.c_double
    import sparse_matrix_math_amd as smm

    for name in ("IDRs", "idrs_dev", "idrs_shadow_dev"):
        assert callable(getattr(smm, name))
    assert smm.IDRS_MAX_S == 8


@pytest.mark.parametrize("mname,s,dtype,it", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_step_cases_are_well_conditioned(oracle, mname, s, dtype, it):
    """the condition inside test_gpu_cgs.allowed, on the restatement alone: a condition on the inputs, not a measurement"""
    csr, b = matrix(mname, dtype)
    st, x, k, sens, _ = reference(oracle, mname, csr, b, it, s)
    scale = max(1.0, float(np.max(np.abs(x))))
    print(mname, s, np.dtype(dtype).name, it, "sensitivity", sens, "cap", 1e-2 * scale)
    assert (st, k) == (2, it)
    assert sens <= 1e-2 * scale


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_near_breakdown_iteration_count_is_stable(oracle, jacobi):
    """convdiff3d(32, 0.3) in fp32, s = 4: the restatement's own iteration counts under a one-ulp change of b stay within half of the
    allowance the GPU comparison uses (max(2, it // 5)), so that comparison is about the kernels"""
    _, _, _, _, it, moved = near_breakdown(oracle, jacobi)
    print("iterations", it, "perturbed", moved)
    assert max(abs(m - it) for m in moved) <= max(2, it // 5) // 2


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::IDRs<float> / <double>, with and without a preconditioner object; -Wall -Werror.  Without a GPU the call reports DIVERGED
    with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double", "float-jacobi", "double-jacobi"}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip) == (0, 0), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name.startswith("float") else 1e-6)
        else:
            assert (status, hip) == (1, -3), words
