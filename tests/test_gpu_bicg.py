"""BiCG for general matrices on the GPU (csrc/smm_solvers_bicg.hip) through the C ABI: fixed passes and converged runs against the CPU
restatement (tests/bicg_restatement.py), THE BIT RULE -- with `at` giving the bits of `a` the solve is smm.BiCGSymmetric's, bit for
bit --, at=None, the reference's recorded DIVERGED decisions, the edge semantics, the frozen loop, the device-pointer form on offset
views, the fma flavour and the drop-in C++ header."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from bicg_restatement import bicg, sensitivity
from bicg_restatement import transpose as host_transpose
from conftest import bicgsymmetric_cases
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from test_bicg_cpu import FIXED, build_case, case
from test_gpu_cgs import allowed
from test_gpu_solvers import RTOL
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID

_REF = {}


def reference(oracle, mname, dtype, it, tag=""):
    """(status, x, iterations, sensitivity) of the restatement after `it` fixed passes from x0 = 0, computed once per case and oracle"""
    key = (tag, mname, np.dtype(dtype).name, it)
    if key not in _REF:
        csr, csr_t, b = case(mname, dtype)
        st, x, k, _ = bicg(oracle, csr, csr_t, b, np.zeros(len(b), dtype=dtype), it, 0.0)
        _REF[key] = (st, x, k, sensitivity(oracle, csr, csr_t, b, it, x))
    return _REF[key]


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def worst(x, ref):
    return float(np.max(np.abs(x.astype(np.float64) - ref.astype(np.float64))))


@pytest.mark.parametrize("mname,dtype,it", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_passes_match_the_restatement(smm, oracle, mname, dtype, it):
    csr, _, b = case(mname, dtype)
    st_ref, x_ref, it_ref, sens = reference(oracle, mname, dtype, it)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    T = A.transpose()
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.BiCG(A, b.copy(), x, it, 0.0, at=T, info=info)
    err = worst(x, x_ref)
    print(mname, np.dtype(dtype).name, it, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert int(st) == st_ref == 0 and info["iterations"] == it_ref == it
    assert err <= tol
    assert info["resnorm2"] >= 0


@pytest.mark.parametrize("mname", ["convdiff3d_12", "poisson2d_32"])
def test_converged_fp64(smm, oracle, mname):
    """the rule of test_gpu_cgs.test_converged_fp64 for the pass count"""
    eps = 1e-6
    csr, csr_t, b = case(mname, np.float64)
    st_ref, _, it_ref, _ = bicg(oracle, csr, csr_t, b, np.zeros(len(b)), -1, eps)
    A = make(smm, csr)
    T = A.transpose()
    x = np.zeros(len(b))
    info = {}
    st = smm.BiCG(A, b.copy(), x, -1, eps, at=T, info=info)
    print(mname, "passes", info["iterations"], "restatement", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))), "r.r", info["resnorm2"])
    assert int(st) == st_ref == 0
    assert float(np.max(np.abs(x - 1))) <= 10 * eps
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    assert info["resnorm2"] <= eps * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("mname", ["poisson2d_32", "banded_2000"])
def test_bit_rule_bicg_is_bicgsymmetric(smm, mname, dtype):
    """at = A and at = A.transpose() of a symmetric matrix, a full solve and 9 passes at eps = 1e-30: status, iterations and x of
    smm.BiCGSymmetric on the same GPU, bit for bit.  Holds under the SMM_WITH_STD_FMA flavour too (both loops use the plain forms)."""
    csr, _, b = case(mname, dtype)
    A = make(smm, csr)
    T = A.transpose()
    assert A.isSymmetric() == (True, True)
    for maxit, eps in ((-1, 1e-3 if dtype == np.float32 else 1e-6), (9, 1e-30)):
        x_ref = np.zeros(len(b), dtype=dtype)
        info_ref = {}
        st_ref = smm.BiCGSymmetric(A, b.copy(), x_ref, maxit, eps, info=info_ref)
        assert info_ref["iterations"] == 9 or maxit == -1
        for name, at in (("A", A), ("A.transpose()", T), ("None", None)):
            x = np.zeros(len(b), dtype=dtype)
            info = {}
            st = smm.BiCG(A, b.copy(), x, maxit, eps, at=at, info=info)
            assert (int(st), info["iterations"]) == (int(st_ref), info_ref["iterations"]), (name, maxit)
            np.testing.assert_array_equal(bits(x), bits(x_ref), err_msg=f"at = {name}, maxIterations {maxit}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_at_none_gives_the_bits_of_the_explicit_transpose(smm, dtype):
    csr, _, b = case("convdiff3d_12", dtype)
    A = make(smm, csr)
    T = A.transpose()
    got = []
    for at in (T, None):
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        st = smm.BiCG(A, b.copy(), x, 7, 0.0, at=at, info=info)
        got.append((int(st), info["iterations"], info["resnorm2"], x))
    assert got[0][:3] == got[1][:3] and got[0][1] == 7
    np.testing.assert_array_equal(bits(got[0][3]), bits(got[1][3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_diverged_heuristics_match_reference(smm, golden_v2, dtype):
    """every recorded BiCGSymmetric case of the real reference with at = A: the reference's status; x compared as
    test_gpu_solvers.test_bicgsymmetric_diverged_heuristics_match_reference compares it"""
    tol = RTOL[dtype]
    statuses = set()
    for name, csr, b, maxit, eps, st_ref, x_ref in bicgsymmetric_cases(golden_v2, dtype):
        n = len(b)
        A = smm.CSRMatrix(n, n, *csr)
        x = np.zeros(n, dtype=dtype)
        st = smm.BiCG(A, b.copy(), x, maxit, dtype(eps), at=A)
        assert int(st) == st_ref, name
        scale = max(float(np.max(np.abs(x_ref))), 1.0)
        bound = 50 * tol if len(b) == 2 else max(50 * tol, 20 * eps, 0.05 if st_ref == 1 else 0.0)
        assert float(np.max(np.abs(x - x_ref))) <= bound * scale, name
        statuses.add(int(st))
    assert statuses == {0, 1}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_edge_semantics(smm, oracle, dtype):
    csr, csr_t, b = case("convdiff3d_12", dtype)
    rows = len(b)
    A = make(smm, csr)
    T = A.transpose()
    info = {}
    # maxIterations == 0: the body runs once, then iterations (1) > maxIterations (0)
    x = np.zeros(rows, dtype=dtype)
    st = smm.BiCG(A, b.copy(), x, 0, 1e-6, at=T, info=info)
    st_ref, x_ref, it_ref, _ = bicg(oracle, csr, csr_t, b, np.zeros(rows, dtype=dtype), 0, 1e-6)
    assert int(st) == st_ref == 2 and info["iterations"] == it_ref == 1
    assert worst(x, x_ref) <= RTOL[dtype] * max(1.0, float(np.max(np.abs(x_ref))))
    # rows == 0 returns cleanly, with what ConjugateGradientSquared reports for rows == 0
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    z = np.zeros(0, dtype=dtype)
    info_c = {}
    st_c = smm.ConjugateGradientSquared(E, z, z, -1, 1e-6, info=info_c)
    for at in (E, E.transpose(), None):
        st = smm.BiCG(E, z, z, -1, 1e-6, at=at, info=info)
        assert (int(st), info["iterations"]) == (int(st_c), info_c["iterations"]) == (2, 1)
    # an `at` of the wrong shape, dtype or entry count; a matrix that is not square: SMM_HIP_ERR_INVALID, x untouched
    other = np.float64 if dtype == np.float32 else np.float32
    small = gen_matrices(dtype)["poisson2d_32"]
    fewer = (csr[0].copy(), csr[1][:-1].copy(), csr[2][:-1].copy())
    fewer[0][-1] -= 1
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2, dtype=dtype))
    bad = (("wrong shape", A, make(smm, small)), ("wrong dtype", A, make(smm, tuple(a.astype(other) if a.dtype.kind == "f" else a for a in csr_t))),
           ("wrong nnz", A, make(smm, fewer)), ("a is not square", W, W.transpose()), ("a is not square, no at", W, None))
    for name, a, at in bad:
        x = np.full(a.rows, 7, dtype=dtype)
        with pytest.raises(smm.SmmHipError) as e:
            smm.BiCG(a, np.ones(a.rows, dtype=dtype), x, 3, 0.0, at=at)
        assert e.value.code == INVALID, name
        assert np.all(x == 7), name
    # null vectors, a null matrix; the outputs are optional
    lib = _lib.load()
    suf = "f32" if dtype == np.float32 else "f64"
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st_i, it_i = ctypes.c_int(), ctypes.c_int()
    x = np.zeros(rows, dtype=dtype)
    fn = getattr(lib, f"smm_hip_bicg_{suf}")
    assert fn(A._h, T._h, None, p(x), 1, 0.0, ctypes.byref(st_i), ctypes.byref(it_i), None) == INVALID
    assert fn(None, T._h, p(x), p(x), 1, 0.0, ctypes.byref(st_i), ctypes.byref(it_i), None) == INVALID
    bb = b.copy()
    assert fn(A._h, T._h, p(bb), p(x), 3, 0.0, None, None, None) == 0
    _, x_ref, _, sens = reference(oracle, "convdiff3d_12", dtype, 3)
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_frozen_loop(smm, dtype):
    """The launches queued behind the pass that left the loop must write nothing: a converged run with a huge maxIterations (the host
    looks at the done flag only every few passes) and a run stopped at the converged count give the same bits."""
    eps = 1e-3 if dtype == np.float32 else 1e-6
    csr, _, b = case("convdiff3d_12", dtype)
    A = make(smm, csr)
    T = A.transpose()
    x1 = np.zeros(len(b), dtype=dtype)
    info1, info2 = {}, {}
    st1 = smm.BiCG(A, b.copy(), x1, -1, eps, at=T, info=info1)
    assert int(st1) == 0 and 4 < info1["iterations"] < len(b) - 8
    x2 = np.zeros(len(b), dtype=dtype)
    st2 = smm.BiCG(A, b.copy(), x2, info1["iterations"], eps, at=T, info=info2)
    assert int(st2) == 0 and info2 == info1
    np.testing.assert_array_equal(bits(x1), bits(x2))


def test_device_pointers_on_offset_views_and_another_stream(smm, oracle):
    """smm_hip_bicg_dev_f64 on a stream of the caller's, b and x views at element alignment inside larger buffers with guard bands"""
    dtype, it = np.float64, 3
    csr, _, b = case("convdiff3d_12", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle, "convdiff3d_12", dtype, it)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved = snapshot(d_b)
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    T = A.transpose(s.cuda_stream)
    st, k, res = host.bicg_dev(A, d_b, d_x, it, 0.0, at=T, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == st_ref == 0 and k == it and res >= 0
    assert worst(d_x.cpu().numpy(), x_ref) <= allowed(x_ref, sens, dtype)
    assert_unchanged(d_b, saved, "b")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")


def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it): against the restatement over the fma oracle by tolerance,
    and the bit rule -- BiCG with at = A and with a built transpose of a symmetric matrix equals BiCGSymmetric bit for bit"""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    dtype, it = np.float64, 3
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    fn = lib.smm_hip_bicg_f64
    fn.argtypes = [P, P, P, P, I, D, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(D)]
    sym = lib.smm_hip_bicgsymmetric_f64
    sym.argtypes = [P, P, P, I, D, ctypes.POINTER(I), ctypes.POINTER(I)]
    lib.smm_hip_csr_transpose_create.argtypes = [P, P, ctypes.POINTER(P)]

    def handles(csr):
        n = len(csr[0]) - 1
        h, t = P(), P()
        assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
        assert lib.smm_hip_csr_transpose_create(h, None, ctypes.byref(t)) == 0, lib.smm_hip_last_error()
        return h, t

    csr, _, b = case("convdiff3d_12", dtype)
    st_ref, x_ref, _, sens = reference(oracle_fma, "convdiff3d_12", dtype, it, tag="fma")
    h, t = handles(csr)
    st, k, res = I(), I(), D()
    x = np.zeros(len(b), dtype=dtype)
    assert fn(h, t, ptr(b.copy()), ptr(x), it, 0.0, ctypes.byref(st), ctypes.byref(k), ctypes.byref(res)) == 0, lib.smm_hip_last_error()
    assert st.value == st_ref == 0 and k.value == it
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)
    lib.smm_hip_csr_destroy(t)
    lib.smm_hip_csr_destroy(h)
    csr, _, b = case("poisson2d_32", dtype)
    h, t = handles(csr)
    x_sym = np.zeros(len(b), dtype=dtype)
    st_s, k_s = I(), I()
    assert sym(h, ptr(b.copy()), ptr(x_sym), 9, 1e-30, ctypes.byref(st_s), ctypes.byref(k_s)) == 0
    for at in (h, t):
        x = np.zeros(len(b), dtype=dtype)
        assert fn(h, at, ptr(b.copy()), ptr(x), 9, 1e-30, ctypes.byref(st), ctypes.byref(k), None) == 0
        assert (st.value, k.value) == (st_s.value, k_s.value) == (0, 9)
        np.testing.assert_array_equal(bits(x), bits(x_sym))
    lib.smm_hip_csr_destroy(t)
    lib.smm_hip_csr_destroy(h)


def test_cpp_dropin_case_on_the_gpu(golden, oracle, tmp_path):
    """tests/cpp/bicg_case.cpp on mesh1e1_structural_48_48_177 (the goldens' CSR arrays), fp64, as test_gpu_cgs runs its case: SUCCESS and
    x near the golden CG solution of the same asset within 10 * eps; the small built-in systems first"""
    eps = 1e-8
    start, pos = golden["asset/mesh1e1/start"], golden["asset/mesh1e1/positions"]
    val = golden["asset/mesh1e1/values"].astype(np.float64)
    rows = len(start) - 1
    b = gen.row_sums(start, val)
    csr = (start, pos, val)
    st_ref, x_cpu, it_ref, _ = bicg(oracle, csr, host_transpose(csr), b, np.zeros(rows), -1, eps)
    assert st_ref == 0 and it_ref < rows
    np.testing.assert_allclose(x_cpu, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
    path = tmp_path / "mesh1e1.txt"
    with open(path, "w") as f:
        f.write(f"{rows} {len(pos)}\n")
        for r in range(rows):
            for k in range(start[r], start[r + 1]):
                f.write(f"{r} {int(pos[k])} {float(val[k])!r}\n")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for ln in r.stdout.splitlines():
        w = ln.split()
        assert (int(w[2]), int(w[4]), int(w[10]), int(w[12]), int(w[14])) == (0, 0, 0, 0, 1), ln
        np.testing.assert_allclose([float.fromhex(v) for v in w[6:9]], 1.0, rtol=1e-4 if w[0] == "float" else 1e-6)
        assert float.fromhex(w[16]) == -2.0
    r = subprocess.run([str(exe), str(path), repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "status 0 hip 0", lines[0]
    x = np.array([float.fromhex(ln.split()[1]) for ln in lines[1:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
