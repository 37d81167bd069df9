"""Restarted GMRES on the GPU (csrc/smm_solvers_gmres.hip) through the C ABI, against the CPU restatement (tests/gmres_restatement.py;
the method is an addition, so there are no goldens): fixed steps, converged runs, right preconditioning, the edge semantics, the frozen
loop and determinism, a PATTERN case, the device-pointer form on offset views, the fma flavour and the drop-in C++ header.
Tolerances: the `allowed` rule of tests/test_gpu_cgs.py with RTOL of tests/test_gpu_solvers.py."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_helpers import build_case, permuted
from gmres_restatement import gmres, sensitivity
from test_gpu_cgs import allowed, make, worst
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
STEPS = [(1, 30), (3, 30), (10, 30), (10, 4), (25, 8)]  # the last two cross restarts
FIXED = [(m, dt, it, restart) for m in ("poisson2d_32", "banded_2000", "convdiff3d_12") for dt in DTYPES for it, restart in STEPS]

_REF = {}


def matrix(mname, dtype):
    key = ("matrix", mname, np.dtype(dtype).name)
    if key not in _REF:
        csr = gen_matrices(dtype)[mname]
        _REF[key] = (csr, gen.row_sums(csr[0], csr[2]))
    return _REF[key]


def reference(oracle, tag, csr, b, it, restart, apply=None):
    """(status, x, iterations, sensitivity) of the restatement after `it` fixed steps from x0 = 0, computed once per case"""
    key = ("fixed", tag, csr[2].dtype.name, it, restart)
    if key not in _REF:
        st, x, k, _ = gmres(oracle, csr, b, np.zeros(len(b), dtype=b.dtype), it, 0.0, restart, apply)
        _REF[key] = (st, x, k, sensitivity(oracle, csr, b, it, restart, x, apply))
    return _REF[key]


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("mname,dtype,it,restart", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_steps_match_the_restatement(smm, oracle, mname, dtype, it, restart):
    csr, b = matrix(mname, dtype)
    st_ref, x_ref, it_ref, sens = reference(oracle, mname, csr, b, it, restart)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.GMRES(A, b.copy(), x, it, 0.0, restart, info=info)
    err = worst(x, x_ref)
    print(mname, np.dtype(dtype).name, it, restart, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert int(st) == st_ref == 2 and info["iterations"] == it_ref == it
    assert err <= tol
    assert info["resnorm2"] >= 0


@pytest.mark.parametrize("restart", [30, 10])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("mname", ["poisson2d_32", "convdiff3d_12"])
def test_converged(smm, oracle, mname, dtype, restart):
    eps = 1e-6 if dtype == np.float64 else 1e-3
    csr, b = matrix(mname, dtype)
    zero = np.zeros(len(b), dtype=dtype)
    st_ref, _, it_ref, _ = gmres(oracle, csr, b, zero, -1, eps, restart)
    A = make(smm, csr)
    x = zero.copy()
    info = {}
    st = smm.GMRES(A, b.copy(), x, -1, eps, restart, info=info)
    print(mname, np.dtype(dtype).name, restart, "steps", info["iterations"], "restatement", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))), "r.r", info["resnorm2"])
    assert int(st) == st_ref == 0
    assert info["resnorm2"] <= dtype(eps) * dtype(eps)
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    if mname == "poisson2d_32":
        assert float(np.max(np.abs(x.astype(np.float64) - 1))) <= 55 * eps  # |A^-1| = 55 (tests/test_cgs_cpu.py)
    else:
        np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


def oracle_apply(smm, oracle, A, csr, kind):
    """(the library's preconditioner, M^-1 as the oracle applies it for that kind, in A's row order)"""
    P = smm.SolverPreconditioner
    M = A.getPreconditioner(kind)
    if kind == P.JACOBI:
        err, diag = oracle.jacobi_setup(csr)
        assert err == 0
        return M, lambda v: oracle.jacobi_apply(diag, np.ascontiguousarray(v))
    if kind == P.SYMMETRIC_GAUS_SEIDEL:
        return M, lambda v: oracle.sgs_apply(csr, np.ascontiguousarray(v))[1]
    bounds = M.block_bounds()
    order = M.block_rows()[0]
    pcsr = permuted(csr, order)  # the block kinds are defined on P A P^T with contiguous blocks (tests/test_gpu_precond_block.py)
    mcsr = oracle.level_cut_matrix(pcsr, bounds, M.level_cap())[0]
    err, lu = oracle.block_ilu0_factorize(mcsr, bounds)
    assert err == 0

    def apply(v):
        z = np.zeros_like(v)
        z[order] = oracle.block_ilu0_apply(mcsr, bounds, lu, np.ascontiguousarray(v[order]))[1]
        return z

    return M, apply


@pytest.mark.parametrize("kind", ["JACOBI", "SYMMETRIC_GAUS_SEIDEL", "BLOCK_ILU0"])
def test_right_preconditioning(smm, oracle, kind):
    """convdiff3d(20), the size at which tests/test_gpu_precond_block.py builds these kinds for its BiCGStab runs; fp64"""
    dtype, eps, restart = np.float64, 1e-6, 30
    csr = gen.convdiff3d(20, 0.3, dtype=dtype)
    b = gen.row_sums(csr[0], csr[2])
    rows = len(b)
    zero = np.zeros(rows, dtype=dtype)
    A = make(smm, csr)
    M, apply = oracle_apply(smm, oracle, A, csr, getattr(smm.SolverPreconditioner, kind))
    info = {}
    for it in (1, 3, 10):
        st_ref, x_ref, it_ref, sens = reference(oracle, "precond/" + kind, csr, b, it, restart, apply)
        x = zero.copy()
        st = smm.GMRES(A, b.copy(), x, it, 0.0, restart, M, info=info)
        err, tol = worst(x, x_ref), allowed(x_ref, sens, dtype)
        print(kind, it, "max|x - ref|", err, "allowed", tol)
        assert int(st) == st_ref == 2 and info["iterations"] == it_ref == it
        assert err <= tol
    st_ref, _, it_ref, _ = gmres(oracle, csr, b, zero, -1, eps, restart, apply)
    x = zero.copy()
    st = smm.GMRES(A, b.copy(), x, -1, eps, restart, M, info=info)
    plain = {}
    smm.GMRES(A, b.copy(), zero.copy(), -1, eps, restart, info=plain)
    print(kind, "steps", info["iterations"], "restatement", it_ref, "unpreconditioned", plain["iterations"])
    assert int(st) == st_ref == 0 and info["resnorm2"] <= eps * eps
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)
    if kind != "JACOBI":
        assert info["iterations"] < plain["iterations"]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_edge_semantics(smm, oracle, dtype):
    csr, b = matrix("poisson2d_32", dtype)
    rows = len(b)
    A = make(smm, csr)
    info = {}
    # maxIterations == 0 with b != 0
    x = np.zeros(rows, dtype=dtype)
    st = smm.GMRES(A, b.copy(), x, 0, 1e-6, info=info)
    assert int(st) == 2 and info["iterations"] == 0 and not x.any()
    # an exact x0: untouched
    x = np.ones(rows, dtype=dtype)
    st = smm.GMRES(A, b.copy(), x, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 0 and info["resnorm2"] == 0 and np.array_equal(x, np.ones(rows, dtype=dtype))
    # [2] x = 6 from 0: the exact H[1][0] == 0 path
    one = (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([2], dtype=dtype))
    x = np.zeros(1, dtype=dtype)
    st = smm.GMRES(make(smm, one), np.array([6], dtype=dtype), x, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 1 and x[0] == 3 and info["resnorm2"] == 0
    # every stored value zero, b != 0: the column is dropped
    zero_values = (csr[0], csr[1], np.zeros_like(csr[2]))
    x = np.zeros(rows, dtype=dtype)
    st = smm.GMRES(make(smm, zero_values), b.copy(), x, -1, 1e-6, info=info)
    assert int(st) == 1 and info["iterations"] == 1 and not x.any()
    assert gmres(oracle, zero_values, b, np.zeros(rows, dtype=dtype), -1, 1e-6, 30)[::2] == (1, 1)
    # rows == 0
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    z = np.zeros(0, dtype=dtype)
    st = smm.GMRES(E, z, z, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 0
    # restart 0 and 65; a matrix that is not square; the other dtype; null vectors
    for restart in (0, 65):
        with pytest.raises(smm.SmmHipError) as e:
            smm.GMRES(A, b.copy(), np.zeros(rows, dtype=dtype), 1, 0.0, restart)
        assert e.value.code == INVALID
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2, dtype=dtype))
    with pytest.raises(smm.SmmHipError) as e:
        smm.GMRES(W, np.ones(2, dtype=dtype), np.zeros(2, dtype=dtype), 1, 0.0)
    assert e.value.code == INVALID
    lib = _lib.load()
    suf, other = ("f32", "f64") if dtype == np.float32 else ("f64", "f32")
    st_c, it_c = ctypes.c_int(), ctypes.c_int()
    wrong = np.zeros(rows, dtype=np.float64 if dtype == np.float32 else np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert getattr(lib, f"smm_hip_gmres_{other}")(A._h, p(wrong), p(wrong), 1, 0.0, 30, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    x = np.zeros(rows, dtype=dtype)
    fn = getattr(lib, f"smm_hip_gmres_{suf}")
    assert fn(A._h, None, p(x), 1, 0.0, 30, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert fn(None, p(x), p(x), 1, 0.0, 30, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    # the status, iterations and resnorm2 are optional
    bb = b.copy()
    assert fn(A._h, p(bb), p(x), 3, 0.0, 30, None, None, None, None) == 0
    _, x_ref, _, sens = reference(oracle, "poisson2d_32", csr, b, 3, 30)
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


@pytest.mark.parametrize("restart", [30, 10])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_frozen_loop_and_determinism(smm, dtype, restart):
    """The launches queued behind a raised flag must write nothing, and no sum depends on timing: a converged run with maxIterations =
    -1, the same run with maxIterations = its step count and a second identical run give the same bits of x and the same info."""
    eps = 1e-3 if dtype == np.float32 else 1e-6
    csr, b = matrix("poisson2d_32", dtype)
    A = make(smm, csr)
    runs = []
    for maxit in (-1, None, -1):
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        st = smm.GMRES(A, b.copy(), x, runs[0][2]["iterations"] if maxit is None else maxit, eps, restart, info=info)
        runs.append((int(st), x, info))
    st1, x1, info1 = runs[0]
    assert st1 == 0 and 4 < info1["iterations"] < len(b)
    for st, x, info in runs[1:]:
        assert st == 0 and info == info1
        np.testing.assert_array_equal(bits(x), bits(x1))


def test_pattern_family(smm, oracle):
    """convdiff3d(54) in fp64 (157 464 rows, over the 2^20 entries from which a solver adopts the PATTERN family), in the manner of
    test_every_spmv_family_under_the_inplace_subtract: a solve that plans 16 steps and leaves after its first lets the handle adopt; then
    five steps on AUTO and five with STREAM forced at one lane per row."""
    dtype = np.float64
    csr = gen.convdiff3d(54, 0.3, dtype=dtype)
    b = gen.row_sums(csr[0], csr[2])
    n = len(b)
    assert len(csr[1]) > 1 << 20
    _, x_ref, _, sens = reference(oracle, "family/convdiff3d_54", csr, b, 5, 30)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    info = {}
    smm.GMRES(A, b.copy(), np.zeros(n, dtype=dtype), 16, 1e30, info=info)
    assert info["iterations"] == 0  # (r.r <= eps^2 at once: the adoption happened before the loop)
    assert A.get_kernel()[0] == smm.SPMV_PATTERN and A.pattern_info()[0] != 0
    got = {}
    x = np.zeros(n, dtype=dtype)
    st = smm.GMRES(A, b.copy(), x, 5, 0.0, info=info)
    assert int(st) == 2 and info["iterations"] == 5 and A.get_kernel()[0] == smm.SPMV_PATTERN
    got["auto"] = x
    S = make(smm, csr)
    S.set_kernel(smm.SPMV_STREAM, 1)
    x = np.zeros(n, dtype=dtype)
    st = smm.GMRES(S, b.copy(), x, 5, 0.0, info=info)
    assert int(st) == 2 and info["iterations"] == 5 and S.get_kernel() == (smm.SPMV_STREAM, 1)
    got["stream"] = x
    errs = {k: worst(v, x_ref) for k, v in got.items()}
    between = worst(got["auto"], got["stream"])
    print("max|x - ref|", errs, "auto - stream", between, "allowed", tol)
    assert between <= tol and errs["auto"] <= tol and errs["stream"] <= tol


def test_device_pointers_on_offset_views_and_another_stream(smm, oracle):
    """smm_hip_gmres_dev_f64 on a stream of the caller's, b and x views at element alignment inside larger buffers with guard bands"""
    dtype, it, restart = np.float64, 10, 4
    csr, b = matrix("convdiff3d_12", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle, "convdiff3d_12", csr, b, it, restart)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved = snapshot(d_b)
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    st, k, res = host.gmres_dev(A, d_b, d_x, it, 0.0, restart, None, s.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == st_ref == 2 and k == it and res >= 0
    assert worst(d_x.cpu().numpy(), x_ref) <= allowed(x_ref, sens, dtype)
    assert_unchanged(d_b, saved, "b")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")


def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it) against the restatement over the fma oracle.  The
    element-wise lines of the restatement stay a*x+b in NumPy, so this flavour is compared by tolerance only."""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    dtype, it, restart = np.float64, 10, 4
    csr, b = matrix("convdiff3d_12", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle_fma, "fma/convdiff3d_12", csr, b, it, restart)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h = P()
    assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    fn = lib.smm_hip_gmres_f64
    fn.argtypes = [P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_int, P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_double)]
    st, k, res = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    x = np.zeros(n, dtype=dtype)
    assert fn(h, ptr(b.copy()), ptr(x), it, 0.0, restart, None, ctypes.byref(st), ctypes.byref(k), ctypes.byref(res)) == 0, lib.smm_hip_last_error()
    lib.smm_hip_csr_destroy(h)
    assert st.value == st_ref == 2 and k.value == it
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


def test_cpp_dropin_case_on_the_gpu(golden, oracle, tmp_path):
    """tests/cpp/gmres_case.cpp on mesh1e1_structural_48_48_177 (the goldens' CSR arrays), fp64: SUCCESS and x near the golden CG solution
    of the same asset, within 10 * eps as test_reference_asset_cases"""
    eps = 1e-8
    start, pos = golden["asset/mesh1e1/start"], golden["asset/mesh1e1/positions"]
    val = golden["asset/mesh1e1/values"].astype(np.float64)
    rows = len(start) - 1
    b = gen.row_sums(start, val)
    st_ref, x_cpu, it_ref, _ = gmres(oracle, (start, pos, val), b, np.zeros(rows), -1, eps, 30)
    assert st_ref == 0 and it_ref < rows
    np.testing.assert_allclose(x_cpu, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
    path = tmp_path / "mesh1e1.txt"
    with open(path, "w") as f:
        f.write(f"{rows} {len(pos)}\n")
        for r in range(rows):
            for k in range(start[r], start[r + 1]):
                f.write(f"{r} {int(pos[k])} {float(val[k])!r}\n")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe), str(path), repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "status 0 hip 0", lines[0]
    x = np.array([float.fromhex(ln.split()[1]) for ln in lines[1:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
