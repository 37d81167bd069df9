"""Precision conversion of a handle and mixed-precision iterative refinement on the GPU (csrc/smm_convert.hip,
csrc/smm_solvers_refine.hip) through the C ABI: the converted bits against NumPy's, the range rule, refresh as a value edit, the four cases
of tests/test_refine_cpu.py against the CPU restatement (tests/refine_restatement.py; the method is an addition, so there are no goldens),
rejection, the edge semantics, determinism, the device-pointer form on offset views and the drop-in C++ header.

ConjugateGradient takes IC0 / CHEBYSHEV / AMG preconditioners only, so for the two CG cases the run "kept a32 plus a float32 Jacobi M" is
the error the inner driver's own check gives (SMM_HIP_ERR_INVALID handed on, x untouched); the kept a32 of those cases is solved with
M = None, and with AMG for poisson2d_32."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from conftest import kat_matrix
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from refine_restatement import DIVERGED, MAX_ITERATIONS_REACHED, SUCCESS, cases, refine, rounded
from test_oracle import gen_matrices
from test_refine_cpu import build_case

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
INVALID = -1  # SMM_HIP_ERR_INVALID
EPS, INNER_EPS = 1e-10, 1e-4
DEV = "cuda:0"
_REF = {}


def csr_of(mname):
    key = ("csr", mname)
    if key not in _REF:
        _REF[key] = kat_matrix(np.float64) if mname == "kat" else gen_matrices(np.float64)[mname]
    return _REF[key]


def shape_of(mname, csr):
    return (5, 4) if mname == "kat" else (len(csr[0]) - 1, len(csr[0]) - 1)


def problem(oracle, case):
    """(csr, b, the restatement's (status, x, outer, inner, rr), sigma_min of the dense matrix), computed once per case"""
    name, mname, inner, restart, rhs = case
    key = ("problem", name)
    if key not in _REF:
        csr = csr_of(mname)
        b = rhs(oracle, csr)
        ref = {jac: refine(oracle, csr, rounded(csr), b, np.zeros(len(b)), EPS, inner, 20, -1, INNER_EPS, restart, jacobi=jac)
               for jac in ([False] if inner == "CG" else [False, True])}
        _REF[key] = (csr, b, ref, sigma_min(mname, csr))
    return _REF[key]


def sigma_min(mname, csr):
    key = ("sigma", mname)
    if key not in _REF:
        import scipy.sparse as sp

        n = len(csr[0]) - 1
        dense = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n)).toarray()
        _REF[key] = float(np.linalg.svd(dense, compute_uv=False)[-1])
    return _REF[key]


def make(smm, csr, shape=None):
    rows, cols = shape or (len(csr[0]) - 1, len(csr[0]) - 1)
    return smm.CSRMatrix(rows, cols, *csr)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def planted(values):
    """the values with the special ones written in: a tie between two floats (rounds to even: 1), a float subnormal, -0.0, NaN, +Inf"""
    v = values.copy()
    special = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -140 * 1.25, -0.0, np.nan, np.inf]
    at = np.linspace(0, len(v) - 1, len(special)).astype(int) if len(v) >= len(special) else np.arange(0)
    for k, s in zip(at, special):
        v[k] = s
    return v, at


def true_residual(csr, b, x):
    """(||b - A x||_2 in float64 NumPy, what a differently ordered evaluation of it may differ by: every row sum and its subtraction carry
    at most (longest row + 2) roundings of 2^-53 relative to |b| + |A| |x|)"""
    import scipy.sparse as sp

    n = len(b)
    A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n))
    r = b - A @ x
    longest = int(np.max(np.diff(csr[0])))
    slack = (longest + 2) * 2.0 ** -53 * float(np.linalg.norm(np.abs(b) + abs(A) @ np.abs(x)))
    return float(np.linalg.norm(r)), slack


# ---- conversion ------------------------------------------------------------------------------------------------------------------------
CONVERT = ["kat", "poisson2d_32", "banded_2000"]


def check_conversion(A, csr, values, at):
    with np.errstate(all="ignore"):
        expect32 = values.astype(np.float32)
    A32 = A.astype(np.float32)
    assert A32.dtype == np.float32 and (A32.rows, A32.cols, A32.nnz) == (A.rows, A.cols, A.nnz)
    got = A32.get_values()
    np.testing.assert_array_equal(got, expect32)
    finite = ~np.isnan(expect32)
    np.testing.assert_array_equal(bits(got)[finite], bits(expect32)[finite])  # (the sign of -0.0 and the subnormal included)
    if len(at):
        assert got[at[0]] == np.float32(1.0) and got[at[1]] == np.float32(1.0 + 2.0 ** -22)  # ties to even, both ways
        assert 0 < got[at[2]] < np.finfo(np.float32).tiny and np.signbit(got[at[3]]) and got[at[3]] == 0
        assert np.isnan(got[at[4]]) and got[at[5]] == np.inf
    start, pos = A32.get_pattern()
    np.testing.assert_array_equal(start, csr[0])
    np.testing.assert_array_equal(pos, csr[1])
    A64 = A32.astype(np.float64)  # exact
    back = A64.get_values()
    np.testing.assert_array_equal(bits(back)[finite], bits(expect32.astype(np.float64))[finite])
    assert np.isnan(back[~finite]).all()
    again = A64.astype(np.float32)  # the round trip, and the copy
    np.testing.assert_array_equal(bits(again.get_values())[finite], bits(expect32)[finite])
    np.testing.assert_array_equal(bits(A32.astype(np.float32).get_values())[finite], bits(expect32)[finite])
    np.testing.assert_array_equal(again.get_pattern()[1], csr[1])
    assert A32.hasSameNonZeroPattern(again)


@pytest.mark.parametrize("mname", CONVERT)
def test_conversion_bits(smm, mname):
    csr = csr_of(mname)
    if mname == "banded_2000":
        assert len(csr[1]) % 64
    values, at = planted(csr[2])
    check_conversion(make(smm, (csr[0], csr[1], values), shape_of(mname, csr)), csr, values, at)


def test_conversion_of_no_rows(smm):
    for rows, cols in ((0, 0), (0, 3)):
        E = smm.CSRMatrix(rows, cols, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64))
        E32 = E.astype(np.float32)
        assert (E32.rows, E32.cols, E32.nnz) == (rows, cols, 0) and E32.get_values().size == 0
        E32.convert_refresh(E)
        assert E32.astype(np.float64).nnz == 0
    csr = csr_of("kat")  # rows without entries at all
    Z = smm.CSRMatrix(5, 4, np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64))
    assert Z.astype(np.float32).nnz == 0 and csr[0][-1] == 10


@pytest.mark.parametrize("residue", [1, 2, 3])
@pytest.mark.parametrize("mname", CONVERT)
def test_conversion_of_caller_owned_arrays_at_odd_offsets(smm, mname, residue):
    """the source's arrays carved at element offsets inside larger buffers with guard bands; then a refresh INTO caller-owned arrays at the
    residue that shares a 16-byte phase with the source after a head of elements, and at one that never does"""
    csr = csr_of(mname)
    rows, cols = shape_of(mname, csr)
    values, at = planted(csr[2])
    d = [carve_like(csr[0], fit(residue, np.int32), fill=len(csr[1]), device=DEV), carve_like(csr[1], fit(residue + 1, np.int32), fill=0, device=DEV),
         carve_like(values, fit(residue, np.float64), device=DEV)]
    saved = [snapshot(t) for t in d]
    A = smm.CSRMatrix.from_device(rows, cols, d[0], d[1], d[2], np.float64)
    check_conversion(A, csr, values, at)
    with np.errstate(all="ignore"):
        expect32 = values.astype(np.float32)
    finite = ~np.isnan(expect32)
    for dst_residue in range(4):
        t = [carve_like(csr[0], 0, fill=len(csr[1]), device=DEV), carve_like(csr[1], 0, fill=0, device=DEV),
             carve_like(np.full(len(values), 7, dtype=np.float32), dst_residue, device=DEV)]
        D = smm.CSRMatrix.from_device(rows, cols, t[0], t[1], t[2], np.float32)
        D.convert_refresh(A)
        got = D.get_values()
        np.testing.assert_array_equal(bits(got)[finite], bits(expect32)[finite])
        assert np.isnan(got[~finite]).all()
        for name, view in zip(("start", "positions", "values"), t):
            assert_guards_intact(view, f"dst {name}")
        W = smm.CSRMatrix.from_device(rows, cols, t[0], t[1], carve_like(np.zeros(len(values)), fit(dst_residue, np.float64), device=DEV), np.float64)
        W.convert_refresh(D)  # widening, asynchronous
        assert_guards_intact(W._keep[2], "widened values")
        np.testing.assert_array_equal(bits(W.get_values())[finite], bits(expect32.astype(np.float64))[finite])
    for name, view, s in zip(("start", "positions", "values"), d, saved):
        assert_unchanged(view, s, name)
        assert_guards_intact(view, name)


def test_range_failure(smm, oracle):
    csr = csr_of("poisson2d_32")
    n = len(csr[0]) - 1
    A = make(smm, csr)
    A32 = A.astype(np.float32)
    A32.set_kernel(smm.SPMV_STREAM, 1)
    x = np.linspace(-1, 1, n).astype(np.float32)
    before = np.zeros(n, dtype=np.float32)
    A32.rMult(x, before)
    kernel, old = A32.get_kernel(), A32.get_values()
    k = len(csr[2]) // 2 + 1
    bad = csr[2].copy()
    bad[k] = 1e300
    bad[k + 40] = -1e300  # the FIRST one is named
    B = make(smm, (csr[0], csr[1], bad))
    with pytest.raises(smm.SmmHipError) as e:
        B.astype(np.float32)
    assert e.value.code == INVALID and f"values[{k}]" in str(e.value)
    with pytest.raises(smm.SmmHipError) as e:
        A32.convert_refresh(B)
    assert e.value.code == INVALID and f"values[{k}]" in str(e.value)
    np.testing.assert_array_equal(bits(A32.get_values()), bits(old))
    assert A32.get_kernel() == kernel
    after = np.zeros(n, dtype=np.float32)
    A32.rMult(x, after)
    np.testing.assert_array_equal(bits(after), bits(before))
    # the largest double that still rounds to a finite float passes, the next one does not
    edge = csr[2].copy()
    edge[k] = np.nextafter(2.0 ** 128 - 2.0 ** 103, 0)
    assert make(smm, (csr[0], csr[1], edge)).astype(np.float32).get_values()[k] == np.finfo(np.float32).max
    edge[k] = 2.0 ** 128 - 2.0 ** 103
    with pytest.raises(smm.SmmHipError):
        make(smm, (csr[0], csr[1], edge)).astype(np.float32)
    # the other refusals of convert_refresh: itself, another shape, another entry count
    for other in (A32, make(smm, csr_of("convdiff3d_12")), make(smm, gen.poisson2d(32, 31, dtype=np.float64))):
        with pytest.raises(smm.SmmHipError) as e:
            A32.convert_refresh(other)
        assert e.value.code == INVALID
    h = ctypes.c_void_p()
    assert _lib.load().smm_hip_csr_convert_create(A._h, 2, None, ctypes.byref(h)) == INVALID and not h
    assert _lib.load().smm_hip_csr_convert_create(None, 0, None, ctypes.byref(h)) == INVALID


def test_refresh_is_a_value_edit(smm, oracle):
    csr = csr_of("poisson2d_32")
    n = len(csr[0]) - 1
    A = make(smm, csr)
    A32 = A.astype(np.float32)
    A32.set_kernel(smm.SPMV_PATTERN, 1)
    x = np.linspace(-1, 1, n).astype(np.float32)
    y = np.zeros(n, dtype=np.float32)
    A32.rMult(x, y)
    assert A32.pattern_info()[0] == 3  # constant diagonals: no values[] read
    np.testing.assert_array_equal(y, oracle.spmv(rounded(csr), 0, None, x))
    A.scale(3)
    rows = np.array([0, 5, 5, 700, n - 1], dtype=np.int32)
    cols = np.array([1, 5, 4, 700 - 32, n - 1], dtype=np.int32)
    vals = np.array([0.1, 1 / 3, -2.7, 1e-3, 12.3])
    assert A.update_entries(rows, cols, vals).all()
    new = A.get_values()
    assert not np.array_equal(new, 3 * csr[2])
    A32.convert_refresh(A)
    assert A32.get_kernel() == (smm.SPMV_PATTERN, 1) and A32.pattern_info()[0] == 1  # the pattern's analysis stays, CONST is gone
    np.testing.assert_array_equal(bits(A32.get_values()), bits(new.astype(np.float32)))
    A32.rMult(x, y)
    np.testing.assert_array_equal(bits(y), bits(oracle.spmv((csr[0], csr[1], new.astype(np.float32)), 0, None, x)))


# ---- refinement ------------------------------------------------------------------------------------------------------------------------
def check_solve(smm, case, csr, b, ref, smin, x, st, info, label):
    st_ref, x_ref, outer_ref, _, _ = ref
    res, slack = true_residual(csr, b, x)
    err = float(np.linalg.norm(x - x_ref))
    print(case[0], label, "status", int(st), "outer", info["outer_iterations"], "restatement", outer_ref, "inner", info["inner_iterations"], "true residual", res,
          "sqrt(resnorm2)", np.sqrt(info["resnorm2"]), "slack", slack, "|x - ref|", err, "bound", 2 * EPS / smin)
    assert int(st) == st_ref == SUCCESS
    assert abs(info["outer_iterations"] - outer_ref) <= 1
    assert res <= EPS
    assert abs(res - np.sqrt(info["resnorm2"])) <= 1e-12 * res + slack
    assert err <= 2 * EPS / smin


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_solves(smm, oracle, case):
    name, mname, inner, restart, _ = case
    csr, b, refs, smin = problem(oracle, case)
    n = len(b)
    if mname == "poisson2d_32":
        assert smin == pytest.approx(0.0181, rel=1e-2)
    if mname == "convdiff3d_12":
        assert smin == pytest.approx(0.236, rel=1e-2)
    A = make(smm, csr)
    info = {}
    x = np.zeros(n)
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, innerEps=INNER_EPS, restart=restart, info=info)
    check_solve(smm, case, csr, b, refs[False], smin, x, st, info, "a32=None")
    A32 = A.astype(np.float32)
    M = A32.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    x = np.zeros(n)
    if inner == "CG":  # (the module's docstring)
        with pytest.raises(smm.SmmHipError) as e:
            smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, a32=A32, M=M, innerEps=INNER_EPS, info=info)
        assert e.value.code == INVALID and not x.any()
        st = smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, a32=A32, innerEps=INNER_EPS, info=info)
        check_solve(smm, case, csr, b, refs[False], smin, x, st, info, "kept a32")
    else:
        st = smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, a32=A32, M=M, innerEps=INNER_EPS, restart=restart, info=info)
        check_solve(smm, case, csr, b, refs[True], smin, x, st, info, "kept a32 + JACOBI")
    if mname == "poisson2d_32":
        # the V-cycle changes how far an inner solve overshoots innerEps, not what it is asked for: the outer count is the restatement's +-1
        G = A32.getPreconditioner("AMG")
        x = np.zeros(n)
        st = smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, a32=A32, M=G, innerEps=INNER_EPS, info=info)
        plain = refs[False][3]
        check_solve(smm, case, csr, b, refs[False], smin, x, st, info, "kept a32 + AMG")
        assert info["inner_iterations"] < plain


def test_what_the_feature_is_for(smm, oracle):
    """a float32 solve asked for 1e-10 stops at float32's floor; refinement on the SAME float32 handle gets there"""
    case = cases()[0]
    csr, b, _, _ = problem(oracle, case)
    n = len(b)
    A = make(smm, csr)
    A32 = make(smm, rounded(csr))
    x32 = np.zeros(n, dtype=np.float32)
    smm.ConjugateGradient(A32, b.astype(np.float32), x32, x32, -1, EPS)
    floor = true_residual(csr, b, x32.astype(np.float64))[0]
    x = np.zeros(n)
    info = {}
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, a32=A32, innerEps=INNER_EPS, info=info)
    res = true_residual(csr, b, x)[0]
    print("float32 CG: true residual", floor, "refined:", res, info)
    assert floor > 1e-6
    assert int(st) == SUCCESS and res <= EPS


def negated(smm, csr):
    return make(smm, (csr[0], csr[1], (-csr[2]).astype(np.float32)))


def test_rejection(smm, oracle):
    csr = csr_of("poisson2d_32")
    b = gen.row_sums(csr[0], csr[2])
    n = len(b)
    A, N32 = make(smm, csr), negated(smm, csr)
    x0 = np.full(n, 0.5)
    st_ref, _, outer_ref, _, rr_ref = refine(oracle, csr, (csr[0], csr[1], (-csr[2]).astype(np.float32)), b, x0, EPS, "CG", 20, 50, INNER_EPS)
    x = x0.copy()
    info = {}
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, a32=N32, maxInner=50, innerEps=INNER_EPS, info=info)
    assert int(st) == st_ref == DIVERGED and info["outer_iterations"] == outer_ref == 0 and info["inner_iterations"] > 0
    np.testing.assert_array_equal(bits(x), bits(x0))
    assert info["resnorm2"] == pytest.approx(rr_ref, rel=1e-12)
    # the device-pointer form on offset views and a stream of the caller's
    d_b = carve_like(b, fit(1, np.float64), device=DEV)
    d_x = carve_like(x0, fit(3, np.float64), device=DEV)
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    saved_b, saved_x = snapshot(d_b), snapshot(d_x)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    st, outer, inner, rr = host.refine_dev(A, d_b, d_x, EPS, a32=N32, maxInner=50, innerEps=INNER_EPS, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == DIVERGED and outer == 0 and inner > 0
    assert_unchanged(d_b, saved_b, "b")
    assert_unchanged(d_x, saved_x, "x")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")
    # ... and a run that accepts its steps there: the host form's bits
    d_x.copy_(torch.zeros(n, dtype=torch.float64))
    A32 = A.astype(np.float32)
    st, outer, inner, rr = host.refine_dev(A, d_b, d_x, EPS, a32=A32, innerEps=INNER_EPS, stream=s.cuda_stream)
    torch.cuda.synchronize()
    x = np.zeros(n)
    assert int(smm.IterativeRefinement(A, b.copy(), x, EPS, a32=A32, innerEps=INNER_EPS, info=info)) == int(st) == SUCCESS
    assert (outer, inner, rr) == (info["outer_iterations"], info["inner_iterations"], info["resnorm2"])
    np.testing.assert_array_equal(bits(d_x.cpu().numpy()), bits(x))
    assert_unchanged(d_b, saved_b, "b")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")


def test_edges(smm, oracle):
    csr = csr_of("poisson2d_32")
    b = gen.row_sums(csr[0], csr[2])
    n = len(b)
    A = make(smm, csr)
    A32 = A.astype(np.float32)
    info = {}
    # an exact start
    x = np.ones(n)
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, a32=A32, info=info)
    assert int(st) == SUCCESS and info == {"outer_iterations": 0, "inner_iterations": 0, "resnorm2": 0.0} and np.array_equal(x, np.ones(n))
    # maxOuter == 0: the start's residual
    x = np.zeros(n)
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, a32=A32, maxOuter=0, info=info)
    assert int(st) == MAX_ITERATIONS_REACHED and info["outer_iterations"] == info["inner_iterations"] == 0 and not x.any()
    assert info["resnorm2"] == pytest.approx(float(np.dot(b, b)), rel=1e-12)
    # maxOuter == 1: one accepted step, not enough
    st = smm.IterativeRefinement(A, b.copy(), x, EPS, a32=A32, maxOuter=1, info=info)
    assert int(st) == MAX_ITERATIONS_REACHED and info["outer_iterations"] == 1 and EPS * EPS < info["resnorm2"] < 1e-4 * float(np.dot(b, b))
    # a NaN in b
    nan_b = b.copy()
    nan_b[n // 2] = np.nan
    x0 = np.linspace(0, 1, n)
    x = x0.copy()
    st = smm.IterativeRefinement(A, nan_b, x, EPS, a32=A32, info=info)
    assert int(st) == DIVERGED and info["outer_iterations"] == 0 and np.isnan(info["resnorm2"])
    np.testing.assert_array_equal(bits(x), bits(x0))
    # rows == 0
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64))
    z = np.zeros(0)
    for a32 in (None, E.astype(np.float32)):
        st = smm.IterativeRefinement(E, z, z, EPS, a32=a32, info=info)
        assert int(st) == SUCCESS and info == {"outer_iterations": 0, "inner_iterations": 0, "resnorm2": 0.0}
    # every SMM_HIP_ERR_INVALID of the header; x keeps its bits
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2))
    other_shape = make(smm, csr_of("convdiff3d_12")).astype(np.float32)
    other_nnz = make(smm, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.float32)))
    M = A32.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    refused = [dict(maxOuter=-1), dict(inner=3), dict(inner=-1), dict(a32=A), dict(a32=other_shape), dict(a32=other_nnz), dict(M=M),
               dict(inner="GMRES", a32=A32, restart=0), dict(inner="BICGSTAB", a32=A32, M=other_shape.getPreconditioner(smm.SolverPreconditioner.JACOBI))]
    for kwargs in refused:
        x = x0.copy()
        with pytest.raises(smm.SmmHipError) as e:
            smm.IterativeRefinement(A, b.copy(), x, EPS, **kwargs)
        assert e.value.code == INVALID, kwargs
        np.testing.assert_array_equal(bits(x), bits(x0))
    for a in (A32, W):  # the wrong dtype for `a`; a matrix that is not square
        with pytest.raises(smm.SmmHipError) as e:
            smm.IterativeRefinement(a, np.ones(a.rows), np.zeros(a.rows), EPS)
        assert e.value.code == INVALID
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    x = x0.copy()
    bb = b.copy()
    assert lib.smm_hip_refine_f64(None, None, p(bb), p(x), 0, 20, -1, EPS, INNER_EPS, 30, None, None, None, None, None) == INVALID
    assert lib.smm_hip_refine_f64(A._h, None, None, p(x), 0, 20, -1, EPS, INNER_EPS, 30, None, None, None, None, None) == INVALID
    assert lib.smm_hip_refine_f64(A._h, None, p(bb), None, 0, 20, -1, EPS, INNER_EPS, 30, None, None, None, None, None) == INVALID
    assert lib.smm_hip_refine_dev_f64(A._h, None, None, None, 0, 20, -1, EPS, INNER_EPS, 30, None, None, None, None, None, None) == INVALID
    np.testing.assert_array_equal(bits(x), bits(x0))
    # the outputs are optional
    x = np.zeros(n)
    assert lib.smm_hip_refine_f64(A._h, A32._h, p(bb), p(x), 0, 20, -1, EPS, INNER_EPS, 30, None, None, None, None, None) == 0
    assert true_residual(csr, b, x)[0] <= EPS


@pytest.mark.parametrize("case", [cases()[0], cases()[3]], ids=lambda c: c[0])
def test_two_runs_give_the_same_bits(smm, oracle, case):
    _, _, inner, restart, _ = case
    csr, b, _, _ = problem(oracle, case)
    A = make(smm, csr)
    A32 = A.astype(np.float32)
    runs = []
    for _ in range(2):
        x = np.zeros(len(b))
        info = {}
        st = smm.IterativeRefinement(A, b.copy(), x, EPS, inner=inner, a32=A32, innerEps=INNER_EPS, restart=restart, info=info)
        runs.append((int(st), info, x))
    assert runs[0][0] == runs[1][0] == SUCCESS and runs[0][1] == runs[1][1]
    np.testing.assert_array_equal(bits(runs[0][2]), bits(runs[1][2]))


def test_cpp_dropin_case_on_the_gpu(golden, tmp_path):
    """tests/cpp/refine_case.cpp: its 3 x 3 system (as tests/test_refine_cpu.py reads it), then mesh1e1_structural_48_48_177 (the goldens'
    CSR arrays) in double: SUCCESS and x near the golden CG solution of the same asset, within 10 * eps as test_reference_asset_cases"""
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
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert int(lines["roundtrip"][1]) == 1
    for name in ("kept", "call"):
        words = lines[name]
        assert (int(words[2]), int(words[4])) == (0, 0) and 1 <= int(words[6]) <= 6, words
        np.testing.assert_allclose([float.fromhex(w) for w in words[8:11]], 1.0, rtol=1e-11)
    r = subprocess.run([str(exe), str(path), repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[0] == "status 0 hip 0", out[0]
    x = np.array([float.fromhex(ln.split()[1]) for ln in out[1:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
