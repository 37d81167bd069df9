"""The transpose / symmetry / BiCG additions without a GPU: the library exports the new entry points and the ctypes table loads; the
CPU restatement of BiCG (tests/bicg_restatement.py, the definition the GPU loop is compared with) is pinned to the reference's
BiCGSymmetric -- with At = A it returns the oracle's status and x bit for bit, and the real reference's recorded DIVERGED decisions --,
converges on a matrix that is not symmetric, and is well enough conditioned on the fixed-pass cases the GPU test compares it on; and
tests/cpp/bicg_case.cpp compiles and links against the drop-in header with -Wall -Werror."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from bicg_restatement import bicg, sensitivity, transpose
from conftest import bicgsymmetric_cases
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "bicg_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
SYMMETRIC = ("poisson2d_32", "banded_2000")

# the fixed-pass cases tests/test_gpu_bicg.py compares with the restatement: (matrix, dtype, passes).  Every one of them passes
# test_fixed_cases_are_well_conditioned below; a case that did not would be taken out here with its measured sensitivity (fp64 stays).
FIXED = [(m, dt, it) for m in ("poisson2d_32", "convdiff3d_12") for dt, passes in ((np.float64, (1, 3, 10)), (np.float32, (1, 3))) for it in passes]

NEW_SYMBOLS = ["smm_hip_csr_transpose_create", "smm_hip_csr_transpose_refresh_f32", "smm_hip_csr_transpose_refresh_f64", "smm_hip_csr_is_symmetric",
               "smm_hip_csr_get_pattern", "smm_hip_bicg_f32", "smm_hip_bicg_f64", "smm_hip_bicg_dev_f32", "smm_hip_bicg_dev_f64"]

_REF = {}


def case(mname, dtype):
    """(csr, its host transpose, b = row sums), made once"""
    key = (mname, np.dtype(dtype).name)
    if key not in _REF:
        csr = gen_matrices(dtype)[mname]
        _REF[key] = (csr, transpose(csr), gen.row_sums(csr[0], csr[2]))
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def build_case(tmp_path):
    """the g++ line of tests/test_cgs_cpu.py"""
    exe = tmp_path / "bicg_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_abi_exports_and_ctypes_signatures():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by libsmm_hip.so"
        assert name in _lib.exported_symbols()
    assert lib.smm_hip_bicg_f64.argtypes[5] is ctypes.c_double and lib.smm_hip_bicg_dev_f32.argtypes[5] is ctypes.c_float
    assert len(lib.smm_hip_bicg_f32.argtypes) == 9 and len(lib.smm_hip_bicg_dev_f64.argtypes) == 10
    assert len(lib.smm_hip_csr_transpose_refresh_f32.argtypes) == 3 and len(lib.smm_hip_csr_is_symmetric.argtypes) == 3
    import sparse_matrix_math_amd as smm

    for name in ("BiCG", "bicg_dev"):
        assert callable(getattr(smm, name))
    for name in ("transpose", "transpose_refresh", "isSymmetric"):
        assert callable(getattr(smm.CSRMatrix, name))


def test_host_transpose_of_the_known_matrix():
    """the helper itself, on the 5 x 4 matrix with an empty last row: against the dense transpose"""
    from conftest import kat_matrix

    start, pos, val = kat_matrix(np.float64)
    dense = np.zeros((5, 4))
    for r in range(5):
        dense[r, pos[start[r]:start[r + 1]]] = val[start[r]:start[r + 1]]
    st, pt, vt = transpose((start, pos, val), cols=4)
    back = np.zeros((4, 5))
    for r in range(4):
        assert np.all(np.diff(pt[st[r]:st[r + 1]]) > 0)
        back[r, pt[st[r]:st[r + 1]]] = vt[st[r]:st[r + 1]]
    np.testing.assert_array_equal(back, dense.T)
    assert st[-1] == 10 and len(st) == 5


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("mname", SYMMETRIC)
def test_restatement_with_at_equal_a_is_bicgsymmetric(oracle, mname, dtype):
    """a full solve and 9 fixed passes at eps = 1e-30: the oracle's status and x, bit for bit -- with the same arrays as At and with the
    host transpose (the same bits, the matrix being symmetric)"""
    csr, csr_t, b = case(mname, dtype)
    for a, b_ in zip(csr, csr_t):
        np.testing.assert_array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b_) if b_.dtype.kind == "f" else b_)
    zero = np.zeros(len(b), dtype=dtype)
    for maxit, eps in ((-1, 1e-3 if dtype == np.float32 else 1e-6), (9, 1e-30)):
        st_ref, x_ref, it_ref = oracle.bicgsymmetric(csr, b, zero, maxit, dtype(eps))
        for at in (csr, csr_t):
            st, x, it, _ = bicg(oracle, csr, at, b, zero, maxit, eps)
            assert (st, it) == (st_ref, it_ref), (mname, maxit)
            np.testing.assert_array_equal(bits(x), bits(x_ref))
        if maxit == 9:
            assert it_ref == 9


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_restatement_returns_the_reference_decisions(oracle, golden_v2, dtype):
    """every recorded BiCGSymmetric case of the real reference (both DIVERGED branches and SUCCESS): its status and its x bit for bit"""
    seen = set()
    for name, csr, b, maxit, eps, st_ref, x_ref in bicgsymmetric_cases(golden_v2, dtype):
        st, x, _, _ = bicg(oracle, csr, csr, b.copy(), np.zeros(len(b), dtype=dtype), maxit, dtype(eps))
        assert st == st_ref, name
        np.testing.assert_array_equal(x, x_ref, err_msg=name)
        seen.add(st_ref)
    assert seen == {0, 1}


def test_restatement_converges_on_a_matrix_that_is_not_symmetric(oracle):
    csr, csr_t, b = case("convdiff3d_12", np.float64)
    assert not np.array_equal(csr[2], csr_t[2])
    st, x, it, rr = bicg(oracle, csr, csr_t, b, np.zeros(len(b)), -1, 1e-6)
    err = float(np.max(np.abs(x - 1)))
    print("convdiff3d_12 fp64 passes", it, "r.r", rr, "max|x - 1|", err)
    assert st == 0 and 0 < it < len(b)
    assert rr <= 1e-6 * 1e-6
    assert err <= 1e-5


@pytest.mark.parametrize("mname,dtype,it", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_cases_are_well_conditioned(oracle, mname, dtype, it):
    """the condition tests/test_gpu_cgs.py's `allowed` puts on a restatement before it compares a GPU result with it, asserted here on
    the CPU: the restatement's own x moves by at most 1e-2 of its scale under one-ulp changes of b"""
    csr, csr_t, b = case(mname, dtype)
    st, x, k, _ = bicg(oracle, csr, csr_t, b, np.zeros(len(b), dtype=dtype), it, 0.0)
    sens = sensitivity(oracle, csr, csr_t, b, it, x)
    scale = max(1.0, float(np.max(np.abs(x))))
    print(mname, np.dtype(dtype).name, it, "sensitivity", sens, "scale", scale)
    assert st == 0 and k == it
    assert sens <= 1e-2 * scale


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::transpose, SMM::isSymmetric and both overloads of SMM::BiCG for float and double (function pointers in the case); -Wall
    -Werror.  Without a GPU every call reports its failure: DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double"}
    for name, words in lines.items():
        status, hip, noat, sym, tsym = int(words[2]), int(words[4]), int(words[10]), int(words[12]), int(words[14])
        if os.path.exists("/dev/kfd"):
            assert (status, hip, noat, sym, tsym) == (0, 0, 0, 0, 1), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name == "float" else 1e-6)
            assert float.fromhex(words[16]) == -2.0
        else:
            assert (status, hip, noat, sym, tsym) == (1, -3, 1, 0, 0), words
