"""The Chebyshev polynomial preconditioner on the GPU (csrc/smm_precond_cheb.hip) through the C ABI, against its CPU restatement
(tests/chebyshev_restatement.py): the spectral bounds, the apply bit for bit at one lane per row and by the fixed-pass tolerance rule of
tests/test_gpu_cgs.py elsewhere, vector lengths around the 16-byte packs, the device-pointer form on offset views, the three solvers
that take it, the refusals, the frozen loop, the fma flavour and the drop-in C++ header."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from chebyshev_restatement import bicgstab, diagonal, gershgorin, make_apply, pcg, power_bound, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres
from gmres_restatement import sensitivity as gmres_sensitivity
from test_chebyshev_cpu import build_case, spd5
from test_gpu_cgs import allowed, make, worst
from test_gpu_solvers import RTOL
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID, PRECOND = -1, -4  # SMM_HIP_ERR_INVALID, SMM_HIP_ERR_PRECOND
MATRICES = ("poisson2d_32", "banded_2000", "convdiff3d_12")
RATIO = 30.0
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def negated_row5(dtype):
    """spd5 with row 2 multiplied by -1: a negative diagonal entry; D^-1 A is that of spd5"""
    start, pos, val = spd5(dtype)
    val = val.copy()
    val[start[2]:start[3]] *= -1
    return start, pos, val


def matrix(mname, dtype):
    """(csr, b = A 1, a fixed right-hand side for the applies, the Gershgorin bound), made once"""
    def compute():
        if mname == "negated_row5":
            csr = negated_row5(dtype)
        elif mname == "convdiff3d_20":
            csr = gen.convdiff3d(20, 0.3, dtype=dtype)
        elif mname.startswith("banded_rows_"):
            csr = gen.banded_random_spd(int(mname.split("_")[2]), dtype=dtype)
        else:
            csr = gen_matrices(dtype)[mname]
        n = len(csr[0]) - 1
        r = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
        return csr, gen.row_sums(csr[0], csr[2]), r, gershgorin(csr)
    return cached(("matrix", mname, np.dtype(dtype).name), compute)


def applied(oracle, tag, mname, dtype, degree):
    """(z = M^-1 r of the restatement with the default bounds, its sensitivity), made once"""
    def compute():
        csr, _, r, lmax = matrix(mname, dtype)
        fn = make_apply(oracle, csr, degree, lmax / RATIO, lmax)
        z = fn(r)
        return z, sensitivity(fn, r, z)
    return cached(("apply", tag, mname, np.dtype(dtype).name, degree), compute)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mname", MATRICES + ("negated_row5",))
def test_gershgorin_bound_equals_the_restatement(smm, mname, dtype):
    csr, _, _, lmax = matrix(mname, dtype)
    M = make(smm, csr).getPreconditioner(smm.SolverPreconditioner.CHEBYSHEV)
    info = M.chebyshev_info()
    print(mname, np.dtype(dtype).name, info, "restatement", lmax)
    assert info["degree"] == 3 and info["bound"] == 0
    assert info["lambda_max"] == lmax
    assert info["lambda_min"] == lmax / RATIO
    np.testing.assert_array_equal(bits(M.values()), bits(diagonal(csr)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mname", MATRICES)
def test_power_bound_near_the_restatement(smm, oracle, mname, dtype):
    csr, _, _, lmax = matrix(mname, dtype)
    ref = cached(("power", mname, np.dtype(dtype).name), lambda: power_bound(oracle, csr, 10))
    info = make(smm, csr).getPreconditioner("CHEBYSHEV", bound="POWER").chebyshev_info()
    print(mname, np.dtype(dtype).name, info, "restatement", ref, "gershgorin", lmax)
    assert info["bound"] == 1 and 0 < info["lambda_max"] <= lmax
    assert abs(info["lambda_max"] - ref) <= RTOL[dtype] * ref
    assert info["lambda_min"] == info["lambda_max"] / RATIO
    four = make(smm, csr).getPreconditioner("CHEBYSHEV", bound="POWER", power_steps=4, eig_ratio=10).chebyshev_info()
    ref4 = power_bound(oracle, csr, 4)
    assert abs(four["lambda_max"] - ref4) <= RTOL[dtype] * ref4 and four["lambda_min"] == four["lambda_max"] / 10.0


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_user_bounds_are_returned_unchanged(smm, dtype):
    csr, _, _, _ = matrix("poisson2d_32", dtype)
    info = make(smm, csr).getPreconditioner("CHEBYSHEV", degree=5, bound="USER", lambda_min=0.1234567890123, lambda_max=1.987654321)
    assert info.chebyshev_info() == {"degree": 5, "bound": 2, "lambda_min": 0.1234567890123, "lambda_max": 1.987654321}


# ---- apply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mname", MATRICES)
def test_apply_bit_for_bit_at_one_lane_per_row(smm, oracle, mname, dtype, degree):
    csr, _, r, _ = matrix(mname, dtype)
    z_ref, _ = applied(oracle, "plain", mname, dtype, degree)
    A = make(smm, csr)
    A.set_kernel(smm.SPMV_STREAM, 1)
    M = A.getPreconditioner("CHEBYSHEV", degree=degree)
    z = np.full(len(r), np.nan, dtype=dtype)
    saved = r.copy()
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(z_ref))
    np.testing.assert_array_equal(bits(r), bits(saved))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mname,kernel", [(m, None) for m in MATRICES] + [("banded_2000", "vector4"), ("convdiff3d_12", "pattern")])
def test_apply_at_other_lane_counts_by_tolerance(smm, oracle, mname, kernel, dtype):
    """the AUTO choice, four lanes per row (a row's sum is split over lanes) and the PATTERN family at two lanes per row; twice: the
    same bits"""
    degree = 3
    csr, _, r, _ = matrix(mname, dtype)
    z_ref, sens = applied(oracle, "plain", mname, dtype, degree)
    tol = allowed(z_ref, sens, dtype)
    A = make(smm, csr)
    if kernel == "pattern":
        A.set_kernel(smm.SPMV_PATTERN, 2)
    elif kernel == "vector4":
        A.set_kernel(smm.SPMV_VECTOR, 4)
    M = A.getPreconditioner("CHEBYSHEV", degree=degree)
    z = np.zeros(len(r), dtype=dtype)
    M.apply(r, z)
    again = np.zeros(len(r), dtype=dtype)
    M.apply(r, again)
    err = worst(z, z_ref)
    print(mname, kernel, np.dtype(dtype).name, A.get_kernel(), "max|z - ref|", err, "allowed", tol)
    assert err <= tol
    np.testing.assert_array_equal(bits(z), bits(again))
    if kernel == "pattern":
        assert A.get_kernel()[0] == smm.SPMV_PATTERN
    # x = M^-1 (A v): the generic SpMV-then-apply path
    x = np.zeros(len(r), dtype=dtype)
    M.apply_spmv(r, x)
    v = oracle.spmv(csr, 0, None, r)
    lmax = matrix(mname, dtype)[3]
    fn = make_apply(oracle, csr, degree, lmax / RATIO, lmax)
    x_ref = fn(v)
    assert worst(x, x_ref) <= allowed(x_ref, sensitivity(fn, v, x_ref), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("rows", [1, 2, 5, 257, 1027])
def test_vector_tail(smm, oracle, rows, dtype):
    """lengths below, at and off the 16-byte packs and the 1024-pack trips of the element-wise kernels, degree 2, bit for bit"""
    mname = f"banded_rows_{rows}"
    csr, _, r, _ = matrix(mname, dtype)
    z_ref, _ = applied(oracle, "plain", mname, dtype, 2)
    A = make(smm, csr)
    A.set_kernel(smm.SPMV_STREAM, 1)
    M = A.getPreconditioner("CHEBYSHEV", degree=2)
    z = np.full(rows, np.nan, dtype=dtype)
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(z_ref))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_device_pointers_on_offset_views_and_another_stream(smm, oracle, dtype):
    """smm_hip_precond_apply_dev_* with rhs and x at element alignment inside larger buffers with guard bands: the one-element path"""
    mname, degree = "convdiff3d_12", 3
    csr, _, r, _ = matrix(mname, dtype)
    z_ref, _ = applied(oracle, "plain", mname, dtype, degree)
    A = make(smm, csr)
    A.set_kernel(smm.SPMV_STREAM, 1)
    M = A.getPreconditioner("CHEBYSHEV", degree=degree)
    d_r = carve_like(r, fit(1, dtype), device="cuda:0")
    d_z = carve_like(np.zeros(len(r), dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_r.data_ptr() % 16 != 0 and d_z.data_ptr() % 16 != 0
    saved = snapshot(d_r)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    M.apply_dev(d_r, d_z, s.cuda_stream)
    M.take_error(s.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(d_z.cpu().numpy()), bits(z_ref))
    assert_unchanged(d_r, saved, "rhs")
    assert_guards_intact(d_r, "rhs")
    assert_guards_intact(d_z, "x")


# ---- solvers -----------------------------------------------------------------------------------------------------------------
def restated(oracle, solver, mname, dtype, it, eps, oracle_tag="plain"):
    """(status, x, iterations, sensitivity or None) of the restated loop with the degree-3 default preconditioner, made once"""
    def compute():
        csr, b, _, lmax = matrix(mname, dtype)
        fn = make_apply(oracle, csr, 3, lmax / RATIO, lmax)
        zero = np.zeros(len(b), dtype=dtype)
        if solver == "cg":
            solve = lambda bb: pcg(oracle, csr, bb, zero, it, eps, fn)  # noqa: E731
        elif solver == "bicgstab":
            solve = lambda bb: bicgstab(oracle, csr, bb, zero, it, eps, fn)  # noqa: E731
        else:
            solve = lambda bb: gmres(oracle, csr, bb, zero, it, eps, 30, fn)  # noqa: E731
        st, x, k, _ = solve(b)
        sens = None
        if eps == 0.0:
            sens = gmres_sensitivity(oracle, csr, b, it, 30, x, fn) if solver == "gmres" else sensitivity(lambda bb: solve(bb)[1], b, x)
        return st, x, k, sens
    return cached(("solve", oracle_tag, solver, mname, np.dtype(dtype).name, it, eps), compute)


def run(smm, solver, A, b, it, eps, M, dtype):
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    if solver == "cg":
        st = smm.ConjugateGradient(A, b, np.zeros(len(b), dtype=dtype), x, it, eps, M, info=info)
    elif solver == "bicgstab":
        st = smm.BiCGStab(A, b.copy(), x, it, eps, M, info=info)
    else:
        st = smm.GMRES(A, b.copy(), x, it, eps, 30, M, info=info)
    return int(st), x, info


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,mname", [("cg", "poisson2d_32"), ("cg", "banded_2000"), ("bicgstab", "convdiff3d_12"), ("bicgstab", "poisson2d_32"),
                                          ("gmres", "convdiff3d_12"), ("gmres", "banded_2000")])
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, mname, dtype):
    it = 5
    csr, b, _, _ = matrix(mname, dtype)
    st_ref, x_ref, it_ref, sens = restated(oracle, solver, mname, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.CHEBYSHEV)
    st, x, info = run(smm, solver, A, b, it, 0.0, M, dtype)
    err = worst(x, x_ref)
    print(solver, mname, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol, "sensitivity", sens, info)
    assert st == st_ref and info["iterations"] == it_ref == it
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,mname", [("cg", "poisson2d_32"), ("bicgstab", "convdiff3d_20"), ("gmres", "convdiff3d_20")])
def test_converged_runs(smm, oracle, solver, mname, dtype):
    """SUCCESS, the restated loop's iteration count within max(2, ref // 5), and fewer iterations than the same call without M"""
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr, b, _, _ = matrix(mname, dtype)
    st_ref, _, it_ref, _ = restated(oracle, solver, mname, dtype, -1, eps)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.CHEBYSHEV)
    st, x, info = run(smm, solver, A, b, -1, eps, M, dtype)
    st0, _, info0 = run(smm, solver, A, b, -1, eps, None, dtype)
    print(solver, mname, np.dtype(dtype).name, "iterations", info["iterations"], "restated", it_ref, "unpreconditioned", info0["iterations"],
          "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0 and st0 == 0
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5)
    assert info["iterations"] < info0["iterations"]
    if solver != "bicgstab":  # (BiCGStab tests the preconditioned residual; the other two the true one: |x - 1| <= |A^-1| eps, |A^-1| <= 55, tests/test_gmres_cpu.py)
        assert float(np.max(np.abs(x - 1))) <= 55 * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,mname", [("cg", "poisson2d_32"), ("bicgstab", "convdiff3d_12")])
def test_frozen_loop(smm, solver, mname, dtype):
    """The applies queued behind the pass that left the loop must write nothing: a converged run with maxIterations = -1 (the host looks
    at the done flag only every few passes) and a run of exactly that many planned passes give the same bits."""
    eps = 1e-3 if dtype == np.float32 else 1e-8
    csr, b, _, _ = matrix(mname, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.CHEBYSHEV)
    st1, x1, info1 = run(smm, solver, A, b, -1, eps, M, dtype)
    assert st1 == 0 and 2 < info1["iterations"] < len(b) - 8
    st2, x2, info2 = run(smm, solver, A, b, info1["iterations"], eps, M, dtype)
    assert st2 == 0 and info2 == info1
    np.testing.assert_array_equal(bits(x1), bits(x2))


# ---- edges -------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals(smm, dtype):
    start, pos, val = spd5(dtype)
    C = smm.SolverPreconditioner.CHEBYSHEV
    # a stored zero, a 1e-6 and a missing diagonal; an empty row
    for bad in (0.0, 1e-6):
        v = val.copy()
        v[start[3] + 1] = bad  # row 3 holds columns 2, 3, 4
        assert pos[start[3] + 1] == 3
        assert code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(C)) == PRECOND
    keep = np.ones(len(pos), dtype=bool)
    keep[start[3] + 1] = False
    s2 = start.copy()
    s2[4:] -= 1
    assert code_of(lambda: make(smm, (s2, pos[keep], val[keep])).getPreconditioner(C)) == PRECOND
    ragged = gen_matrices(dtype)["ragged_300"]
    assert (np.diff(ragged[0]) == 0).any()
    assert code_of(lambda: make(smm, ragged).getPreconditioner(C)) == PRECOND
    # degree, ratio, USER bounds, bound mode, power steps
    A = make(smm, (start, pos, val))
    for degree in (-1, 65):
        assert code_of(lambda: A.getPreconditioner(C, degree=degree)) == INVALID
    assert A.getPreconditioner(C, degree=64).chebyshev_info()["degree"] == 64
    for ratio in (1.0, 0.5, -3.0, float("nan"), float("inf")):
        assert code_of(lambda: A.getPreconditioner(C, eig_ratio=ratio)) == PRECOND
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.5, float("inf")), (0.5, float("nan"))):
        assert code_of(lambda: A.getPreconditioner(C, bound="USER", lambda_min=lo, lambda_max=hi)) == PRECOND
    assert code_of(lambda: A.getPreconditioner(C, bound=3)) == INVALID
    assert code_of(lambda: A.getPreconditioner(C, bound="POWER", power_steps=0)) == INVALID
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
    assert code_of(lambda: W.getPreconditioner(C)) == INVALID
    # ConjugateGradient still refuses every kind but IC0 and CHEBYSHEV; the batched BiCGStab refuses CHEBYSHEV; so does a foreign matrix
    b = gen.row_sums(start, val)
    x = np.zeros(5, dtype=dtype)
    J = A.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    assert code_of(lambda: smm.ConjugateGradient(A, b, x, x, 5, 1e-6, J)) == INVALID
    M = A.getPreconditioner(C)
    B = np.stack([b, b], axis=1).copy()
    assert code_of(lambda: smm.BiCGStabBatch(A, B, np.zeros_like(B), 5, 1e-6, M)) == INVALID
    other = make(smm, (start, pos, val))
    assert code_of(lambda: smm.ConjugateGradient(other, b, x, x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: smm.BiCGStab(other, b.copy(), x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: M.apply(b, b)) == INVALID  # rhs aliases x
    assert code_of(lambda: J.chebyshev_info()) == INVALID
    # the same handle still solves
    assert int(smm.ConjugateGradient(A, b, x, x, -1, 1e-6 if dtype == np.float64 else 1e-4, M)) == 0
    np.testing.assert_allclose(x, 1.0, rtol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_no_rows(smm, dtype):
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    M = E.getPreconditioner(smm.SolverPreconditioner.CHEBYSHEV)
    assert M.chebyshev_info()["degree"] == 3
    z = np.zeros(0, dtype=dtype)
    M.apply(z, z)
    assert len(M.values()) == 0


# ---- flavour and drop-in -----------------------------------------------------------------------------------------------------
def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it) against the restatement over the fma oracle.  The
    element-wise lines of the restatement stay a*x+b in NumPy, so this flavour is compared by tolerance only."""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    dtype, degree, mname = np.float64, 3, "convdiff3d_12"
    csr, _, r, lmax = matrix(mname, dtype)
    n = len(r)
    z_ref, sens = applied(oracle_fma, "fma", mname, dtype, degree)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h, m = P(), P()
    assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    create = lib.smm_hip_precond_create_chebyshev
    create.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(P)]
    assert create(h, degree, 0, RATIO, 10, 0.0, 0.0, ctypes.byref(m)) == 0, lib.smm_hip_last_error()
    got_lmax = ctypes.c_double()
    info = lib.smm_hip_precond_chebyshev_info
    info.argtypes = [P, P, P, P, ctypes.POINTER(ctypes.c_double)]
    assert info(m, None, None, None, ctypes.byref(got_lmax)) == 0 and got_lmax.value == lmax
    z = np.zeros(n, dtype=dtype)
    lib.smm_hip_precond_apply_f64.argtypes = [P, P, P]
    assert lib.smm_hip_precond_apply_f64(m, ptr(r), ptr(z)) == 0, lib.smm_hip_last_error()
    lib.smm_hip_precond_destroy.argtypes = [P]
    lib.smm_hip_csr_destroy.argtypes = [P]
    lib.smm_hip_precond_destroy(m)
    lib.smm_hip_csr_destroy(h)
    err = worst(z, z_ref)
    print("fma flavour: max|z - ref|", err, "allowed", allowed(z_ref, sens, dtype))
    assert err <= allowed(z_ref, sens, dtype)


def test_cpp_dropin_case_on_the_gpu(golden, tmp_path):
    """tests/cpp/chebyshev_case.cpp on mesh1e1_structural_48_48_177 (the goldens' CSR arrays), fp64: SMM::ConjugateGradient with the
    degree-3 SMM::ChebyshevPreconditioner ends with SUCCESS near the golden CG solution of the same asset, within 10 * eps as
    test_reference_asset_cases (the restated loop: 14 iterations against 21 unpreconditioned, 6.2e-10 from the golden x)"""
    eps = 1e-8
    start, pos = golden["asset/mesh1e1/start"], golden["asset/mesh1e1/positions"]
    val = golden["asset/mesh1e1/values"].astype(np.float64)
    rows = len(start) - 1
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
    assert lines[0] == "status 0 hip 0", lines[0] + r.stderr[-500:]
    x = np.array([float.fromhex(ln.split()[1]) for ln in lines[1:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
