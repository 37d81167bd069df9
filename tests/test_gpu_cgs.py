"""ConjugateGradientSquared on the GPU (csrc/smm_solvers_cgs.hip) through the C ABI, against the CPU restatement of ref:2110-2178 with
the one repair (tests/cgs_restatement.py; the reference's own template cannot be instantiated, so there are no goldens): fixed passes,
converged runs, the edge semantics the reference's text implies, the frozen loop, every SpMV family under the in-place subtract with two
fused dot products, the device-pointer form on offset views, the fma flavour, and the drop-in C++ header."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from cgs_restatement import cgs, perturbed, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from test_cgs_cpu import build_case
from test_gpu_solvers import RTOL
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID

# fixed passes: it in {1, 3} everywhere; it = 10 on poisson2d_32 in both dtypes and on the other two matrices in fp64 only -- in fp32 the
# restatement's own sensitivity after ten passes on banded_2000 / convdiff3d_12 is of the size of x (measured on the CPU: convdiff3d_12
# moves by 6e-2 under a one-ulp change of b with max|x| = 667 and does not converge at all; banded_2000 runs into NaN once its residual
# has bottomed out), so that comparison would pass or fail by luck.  That is the method in fp32, not the kernels.
FIXED = [(m, dt, it) for m in ("poisson2d_32", "banded_2000", "convdiff3d_12") for dt in DTYPES for it in (1, 3, 10)
         if it < 10 or m == "poisson2d_32" or dt == np.float64]

_REF = {}


def matrix(mname, dtype):
    key = ("matrix", mname, np.dtype(dtype).name)
    if key not in _REF:
        csr = gen_matrices(dtype)[mname]
        _REF[key] = (csr, gen.row_sums(csr[0], csr[2]))
    return _REF[key]


def reference(oracle, tag, csr, b, it):
    """(status, x, iterations, sensitivity) of the restatement after `it` fixed passes from x0 = 0, computed once per case"""
    key = ("fixed", tag, csr[2].dtype.name, it)
    if key not in _REF:
        st, x, k, _ = cgs(oracle, csr, b, np.zeros(len(b), dtype=b.dtype), it, 0.0)
        _REF[key] = (st, x, k, sensitivity(oracle, csr, b, it, x))
    return _REF[key]


def allowed(x_ref, sens, dtype):
    """the tolerance rule of the fixed-pass comparisons; the case must be well enough conditioned to mean anything (a condition on
    the restatement, not a measurement of the GPU)"""
    scale = max(1.0, float(np.max(np.abs(x_ref))))
    assert sens <= 1e-2 * scale, ("the restatement itself is too sensitive for this case", sens, scale)
    return max(RTOL[dtype] * scale, 4 * sens)


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


def worst(x, ref):
    return float(np.max(np.abs(x.astype(np.float64) - ref.astype(np.float64))))


@pytest.mark.parametrize("mname,dtype,it", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_passes_match_the_restatement(smm, oracle, mname, dtype, it):
    csr, b = matrix(mname, dtype)
    st_ref, x_ref, it_ref, sens = reference(oracle, mname, csr, b, it)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.ConjugateGradientSquared(A, b.copy(), x, it, 0.0, info=info)
    err = worst(x, x_ref)
    print(mname, np.dtype(dtype).name, it, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert int(st) == st_ref == 0 and info["iterations"] == it_ref == it
    assert err <= tol
    assert info["resnorm2"] >= 0


@pytest.mark.parametrize("mname", ["poisson2d_32", "convdiff3d_12"])
def test_converged_fp64(smm, oracle, mname):
    """the rule of test_config5_nonsymmetric_preconditioned for the pass count"""
    eps = 1e-6
    csr, b = matrix(mname, np.float64)
    st_ref, _, it_ref, _ = cgs(oracle, csr, b, np.zeros(len(b)), -1, eps)
    A = make(smm, csr)
    x = np.zeros(len(b))
    info = {}
    st = smm.ConjugateGradientSquared(A, b.copy(), x, -1, eps, info=info)
    print(mname, "passes", info["iterations"], "restatement", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))), "r.r", info["resnorm2"])
    assert int(st) == st_ref == 0
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    assert info["resnorm2"] <= eps * eps


def test_converged_fp32(smm, oracle):
    """fp32 CGS is fragile: the pass count of the restatement itself moves with a one-ulp change of b, so the GPU's count must lie inside
    the range of the restatement's unperturbed and three perturbed runs, widened by it_ref // 5 on each side"""
    eps = 1e-3
    csr, b = matrix("poisson2d_32", np.float32)
    zero = np.zeros(len(b), dtype=np.float32)
    st_ref, _, it_ref, _ = cgs(oracle, csr, b, zero, -1, eps)
    counts = [it_ref] + [cgs(oracle, csr, perturbed(b, seed), zero, -1, eps)[2] for seed in range(3)]
    A = make(smm, csr)
    x = zero.copy()
    info = {}
    st = smm.ConjugateGradientSquared(A, b.copy(), x, -1, eps, info=info)
    print("passes", info["iterations"], "restatement", counts, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert int(st) == st_ref == 0
    assert float(np.max(np.abs(x - 1))) <= 1e-4
    assert min(counts) - it_ref // 5 <= info["iterations"] <= max(counts) + it_ref // 5, (info, counts)


def spd5(dtype):
    """5 x 5, symmetric and strictly diagonally dominant, every value a small dyadic number (so that b = A 1 and b - A 1 are exact)"""
    dense = np.array([[4.5, -1.25, 0, 0, -0.25], [-1.25, 5.0, -0.75, 0, 0], [0, -0.75, 4.25, -1.5, 0], [0, 0, -1.5, 6.0, -0.5], [-0.25, 0, 0, -0.5, 3.5]])
    start = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int32)
    pos = np.nonzero(dense)[1].astype(np.int32)
    return start, pos, dense[dense != 0].astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_semantics(smm, oracle, dtype):
    """what ref:2110-2178 does at its edges, independent of any summation order"""
    csr, b = matrix("poisson2d_32", dtype)
    rows = len(b)
    A = make(smm, csr)
    info = {}
    # maxIterations == 0: the body runs once, then iterations (1) > maxIterations (0) (ref:2131, 2172-2176)
    x = np.zeros(rows, dtype=dtype)
    st = smm.ConjugateGradientSquared(A, b.copy(), x, 0, 1e-6, info=info)
    st_ref, x_ref, it_ref, _ = cgs(oracle, csr, b, np.zeros(rows, dtype=dtype), 0, 1e-6)
    assert int(st) == st_ref == 2 and info["iterations"] == it_ref == 1
    assert worst(x, x_ref) <= RTOL[dtype] * max(1.0, float(np.max(np.abs(x_ref))))
    # every stored value zero, b != 0: ap.r0 == 0, alpha = inf, q = -inf * 0 + u = NaN (no breakdown test, ref:2134); r = r - A NaN = NaN
    # leaves the loop.  With no stored value at all x is NaN as well, but r = r - (an empty sum) stays b: the loop runs all its passes
    zero_values = (csr[0], csr[1], np.zeros_like(csr[2]))
    no_values = (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    for zero_csr, passes in ((zero_values, 1), (no_values, rows)):
        assert cgs(oracle, zero_csr, b, np.zeros(rows, dtype=dtype), -1, 1e-6)[::2] == (0, passes)
        x = np.zeros(rows, dtype=dtype)
        st = smm.ConjugateGradientSquared(make(smm, zero_csr), b.copy(), x, -1, 1e-6, info=info)
        assert int(st) == 0 and info["iterations"] == passes and np.isnan(x).all()
    # x0 exact: r = 0, rr0 = 0, alpha = 0 / 0 -- the quirk that bicgstab_exact_x0 pins for BiCGStab
    k5 = spd5(dtype)
    K = make(smm, k5)
    ones = np.ones(5, dtype=dtype)
    b5 = gen.row_sums(k5[0], k5[2])
    np.testing.assert_array_equal(oracle.spmv(k5, 2, b5, ones), 0)
    x = ones.copy()
    st = smm.ConjugateGradientSquared(K, b5.copy(), x, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 1 and np.isnan(x).all()
    assert cgs(oracle, k5, b5, ones, -1, 1e-6)[::2] == (0, 1)
    # rows == 1: [2] x = 6 from 0: alpha = 36 / 72, q = 0, x = 3, r = 0 -- exact in one pass
    one = (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([2], dtype=dtype))
    x = np.zeros(1, dtype=dtype)
    st = smm.ConjugateGradientSquared(make(smm, one), np.array([6], dtype=dtype), x, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 1 and x[0] == 3 and info["resnorm2"] == 0
    # rows == 0 returns cleanly, with what BiCGStab reports for rows == 0: one pass over empty vectors, 1 > maxIterations == 0
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    z = np.zeros(0, dtype=dtype)
    info_b = {}
    st_b = smm.BiCGStab(E, z, z, -1, 1e-6, info=info_b)
    st = smm.ConjugateGradientSquared(E, z, z, -1, 1e-6, info=info)
    assert (int(st), info["iterations"]) == (int(st_b), info_b["iterations"]) == (2, 1)
    # a matrix that is not square; a matrix of the other dtype; null vectors
    lib = _lib.load()
    suf, other = ("f32", "f64") if dtype == np.float32 else ("f64", "f32")
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2, dtype=dtype))
    with pytest.raises(smm.SmmHipError) as e:
        smm.ConjugateGradientSquared(W, np.ones(2, dtype=dtype), np.zeros(2, dtype=dtype), 1, 0.0)
    assert e.value.code == INVALID
    st_c, it_c = ctypes.c_int(), ctypes.c_int()
    wrong = np.zeros(rows, dtype=np.float64 if dtype == np.float32 else np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert getattr(lib, f"smm_hip_cgs_{other}")(A._h, p(wrong), p(wrong), 1, 0.0, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    x = np.zeros(rows, dtype=dtype)
    assert getattr(lib, f"smm_hip_cgs_{suf}")(A._h, None, p(x), 1, 0.0, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert getattr(lib, f"smm_hip_cgs_{suf}")(None, p(x), p(x), 1, 0.0, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    # iterations / resnorm2 (and the status) are optional
    bb = b.copy()
    assert getattr(lib, f"smm_hip_cgs_{suf}")(A._h, p(bb), p(x), 3, 0.0, None, None, None) == 0
    _, x_ref, _, sens = reference(oracle, "poisson2d_32", csr, b, 3)
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_loop(smm, dtype):
    """The launches queued behind the pass that left the loop must write nothing: a converged run with maxIterations = -1 (the host
    looks at the done flag only every few passes) and a run of exactly that many planned passes give the same bits."""
    eps = 1e-3 if dtype == np.float32 else 1e-6
    csr, b = matrix("poisson2d_32", dtype)
    A = make(smm, csr)
    x1 = np.zeros(len(b), dtype=dtype)
    info1, info2 = {}, {}
    st1 = smm.ConjugateGradientSquared(A, b.copy(), x1, -1, eps, info=info1)
    assert int(st1) == 0 and 4 < info1["iterations"] < len(b) - 8
    x2 = np.zeros(len(b), dtype=dtype)
    st2 = smm.ConjugateGradientSquared(A, b.copy(), x2, info1["iterations"], eps, info=info2)
    assert int(st2) == 0 and info2 == info1
    np.testing.assert_array_equal(x1.view(np.uint32 if dtype == np.float32 else np.uint64), x2.view(np.uint32 if dtype == np.float32 else np.uint64))


N54 = 54  # 157 464 rows, 1.09 M stored entries: just over the 2^20 from which a solver adopts the PATTERN family


MARCH = (1 << 17, 1 << 17)  # grids from 2^17 rows take the 2.5-D kernels (production: 2^21 rows and more)
PLANES = (128, 72, 17)  # 156 672 rows, 1.07 M entries: planes of 9216 rows (the march along planes needs 8192) and more than 8 of them
BOTH = (np.float32, np.float64)
# name -> (generator, march thresholds or None for production's, keep the constant-diagonal form, the kernel AUTO must end on, the dtypes
# in which the restatement is a reference).  convdiff3d_varying (an addition to the issue's list, for the kernels that read values[]
# without a march) is compared with the restatement in fp64 only: in fp32 the restatement's own x after five passes moves by 8.5e-2
# (max|x| = 64.6) when its dot products -- the reference's sequential sums, here over 157 464 terms -- are summed accurately instead,
# 80 times what one-ulp changes of b predict (1.0e-3) and 4 times the bound; measured on the CPU alone.  The comparison would pass or
# fail by luck, so in fp32 that matrix only has to give the same x on both families.
FAMILY_CASES = {
    "convdiff3d": (lambda dt: gen.convdiff3d(N54, 0.3, dtype=dt), None, True, "spmvPatternConstKernel", BOTH),
    "convdiff3d_varying": (lambda dt: gen.convdiff3d_varying(N54, dtype=dt), None, True, "spmvPatternWaveKernel", (np.float64,)),
    "poisson3d": (lambda dt: gen.poisson3d(N54, dtype=dt), None, True, "spmvPatternConstKernel", BOTH),
    "stencil3d-march": (lambda dt: gen.stencil3d(*PLANES, 6.0, -1.25, -0.75, dtype=dt), MARCH, True, "spmvPatternConstMarchKernel", BOTH),
    "stencil3d-march-values-read": (lambda dt: gen.stencil3d(*PLANES, 6.0, -1.25, -0.75, dtype=dt), MARCH, False, "spmvPatternMasksMarchKernel", BOTH),
}


@pytest.mark.parametrize("name", list(FAMILY_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_every_spmv_family_under_the_inplace_subtract(smm, oracle, dtype, name):
    """r = r - A alphaUQ with out aliasing lhs and dotMode 2 is new to the compressed kernels.  Five fixed passes on a handle left on
    AUTO -- which must really run a PATTERN kernel -- and five with the STREAM family forced at one lane per row; both against the
    restatement by the fixed-pass rule.  A solver adopts the PATTERN family only when it plans at least 16 passes, so the AUTO handle
    first sees one solve that plans 16 and leaves after its first (eps = 1e30): the adoption stays with the handle."""
    make_csr, march, keep_const, expected_kernel, restated = FAMILY_CASES[name]
    csr = make_csr(dtype)
    b = gen.row_sums(csr[0], csr[2])
    n = len(b)
    assert len(csr[1]) > 1 << 20
    _, x_ref, _, sens = reference(oracle, "family/" + name, csr, b, 5)
    tol = allowed(x_ref, sens, dtype)
    host.set_march_min_rows(*(march or (-1, -1)))
    try:
        A = make(smm, csr)
        if not keep_const:
            A.pattern_allow_const(False)
        x = np.zeros(n, dtype=dtype)
        info = {}
        smm.ConjugateGradientSquared(A, b.copy(), x, 16, 1e30, info=info)
        assert info["iterations"] == 1
        family, lanes = A.get_kernel()
        kernel = A.kernel_desc()[0]
        encoding = A.pattern_info()[0]
        print(name, np.dtype(dtype).name, "AUTO ->", family, lanes, kernel, "encoding", encoding)
        assert family == smm.SPMV_PATTERN and kernel == expected_kernel and encoding != 0
        got = {}
        x = np.zeros(n, dtype=dtype)
        st = smm.ConjugateGradientSquared(A, b.copy(), x, 5, 0.0, info=info)
        assert int(st) == 0 and info["iterations"] == 5 and A.get_kernel()[0] == smm.SPMV_PATTERN
        got["auto"] = x
        S = make(smm, csr)
        S.set_kernel(smm.SPMV_STREAM, 1)
        x = np.zeros(n, dtype=dtype)
        st = smm.ConjugateGradientSquared(S, b.copy(), x, 5, 0.0, info=info)
        assert int(st) == 0 and info["iterations"] == 5 and S.get_kernel() == (smm.SPMV_STREAM, 1)
        got["stream"] = x
    finally:
        host.set_march_min_rows(-1, -1)
    errs = {k: worst(v, x_ref) for k, v in got.items()}
    between = worst(got["auto"], got["stream"])
    print(name, "max|x - ref|", errs, "auto - stream", between, "allowed", tol)
    assert between <= tol
    if dtype in restated:
        assert errs["auto"] <= tol and errs["stream"] <= tol


def test_device_pointers_on_offset_views_and_another_stream(smm, oracle):
    """smm_hip_cgs_dev_f64 on a stream of the caller's, b and x views at element alignment inside larger buffers with guard bands"""
    dtype, it = np.float64, 3
    csr, b = matrix("convdiff3d_12", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle, "convdiff3d_12", csr, b, it)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved = snapshot(d_b)
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    st, k, res = host.cgs_dev(A, d_b, d_x, it, 0.0, s.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == st_ref == 0 and k == it and res >= 0
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
    dtype, it = np.float64, 3
    csr, b = matrix("convdiff3d_12", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle_fma, "fma/convdiff3d_12", csr, b, it)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h = P()
    assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    fn = lib.smm_hip_cgs_f64
    fn.argtypes = [P, P, P, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    st, k, res = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    x = np.zeros(n, dtype=dtype)
    assert fn(h, ptr(b.copy()), ptr(x), it, 0.0, ctypes.byref(st), ctypes.byref(k), ctypes.byref(res)) == 0, lib.smm_hip_last_error()
    lib.smm_hip_csr_destroy(h)
    assert st.value == st_ref == 0 and k.value == it
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


def test_cpp_dropin_case_on_the_gpu(golden, oracle, tmp_path):
    """tests/cpp/cgs_case.cpp on mesh1e1_structural_48_48_177 (the goldens' CSR arrays), fp64: SUCCESS and x near the golden CG solution of
    the same asset, within 10 * eps as test_reference_asset_cases -- the restatement converges on it (12 passes on the CPU)"""
    eps = 1e-8
    start, pos = golden["asset/mesh1e1/start"], golden["asset/mesh1e1/positions"]
    val = golden["asset/mesh1e1/values"].astype(np.float64)
    rows = len(start) - 1
    b = gen.row_sums(start, val)
    st_ref, x_cpu, it_ref, _ = cgs(oracle, (start, pos, val), b, np.zeros(rows), -1, eps)
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
