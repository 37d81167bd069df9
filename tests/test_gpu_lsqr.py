"""LSQR on the GPU (csrc/smm_solvers_lsqr.hip) through the C ABI, against the CPU restatement of the loop that include/smm_hip.h states
(tests/lsqr_restatement.py) and against numpy.linalg.lstsq: fixed passes, converged runs, the minimum-norm property, the two estimates,
the same bits twice, the three ways to give the transpose, a nonzero start, every SpMV family, the refusals, the edges, the
device-pointer form on offset views of a wide AND a tall matrix, the fma flavour and the drop-in C++ header.  The matrices are those of
tests/lsqr_cases.py.

A fixed-pass run (eps = 0) stops at the pass limit with both estimates above eps^2 = 0, which the status rule of the contract calls
MAX_ITERATIONS_REACHED: that is what these tests expect of it, and what the restatement returns."""
import ctypes
import subprocess

import lsqr_cases as cases
import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from lsqr_restatement import lsqr, perturbed, sensitivity
from test_gpu_solvers import RTOL
from test_lsqr_cpu import build_case

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
DAMPS = [0.0, cases.DAMP]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
EPS = cases.EPS

_REF = {}


def system(name, dtype):
    """(rows, cols, csr, csr of the transpose, b)"""
    key = ("system", name, np.dtype(dtype).name)
    if key not in _REF:
        rows, cols, csr = cases.matrix(name, dtype)
        _REF[key] = (rows, cols, csr, cases.transposed(csr, cols), cases.rhs(name, dtype))
    return _REF[key]


def reference(oracle, name, dtype, it, damp, fma=False):
    """(status, x, iterations, reason, res, arn, sensitivity) of the restatement after `it` fixed passes from x0 = 0, once per case"""
    key = ("fixed", name, np.dtype(dtype).name, it, damp, fma)
    if key not in _REF:
        rows, cols, csr, csr_t, b = system(name, dtype)
        out = lsqr(oracle, csr, csr_t, b, np.zeros(cols, dtype=dtype), it, 0.0, damp)
        _REF[key] = out + (sensitivity(oracle, csr, csr_t, b, it, damp, out[1]),)
    return _REF[key]


def converged(oracle, name, dtype, damp):
    key = ("converged", name, np.dtype(dtype).name, damp)
    if key not in _REF:
        rows, cols, csr, csr_t, b = system(name, dtype)
        _REF[key] = lsqr(oracle, csr, csr_t, b, np.zeros(cols, dtype=dtype), -1, EPS[dtype], damp)
    return _REF[key]


def answer(name, dtype, damp):
    key = ("answer", name, np.dtype(dtype).name, damp)
    if key not in _REF:
        _REF[key] = cases.lstsq(name, dtype) if damp == 0 else cases.damped(name, damp, dtype)
    return _REF[key]


def allowed(x_ref, sens, dtype):
    """the tolerance rule of tests/test_gpu_cgs.py"""
    scale = max(1.0, float(np.max(np.abs(x_ref))))
    assert sens <= 1e-2 * scale, ("the restatement itself is too sensitive for this case", sens, scale)
    return max(RTOL[dtype] * scale, 4 * sens)


def make(smm, rows, cols, csr):
    return smm.CSRMatrix(rows, cols, *csr)


def worst(x, ref):
    return float(np.max(np.abs(x.astype(np.float64) - ref.astype(np.float64))))


def true_quantities(csr, cols, b, x, damp, x0=None):
    """(||b - A x||^2 + damp^2 ||x - x0||^2, ||At (b - A x) - damp^2 (x - x0)||) in fp64"""
    a = cases.dense(csr, cols)
    x = x.astype(np.float64)
    dx = x if x0 is None else x - x0.astype(np.float64)
    r = b.astype(np.float64) - a @ x
    return float(r @ r + damp * damp * (dx @ dx)), float(np.linalg.norm(a.T @ r - damp * damp * dx))


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("it", [1, 3, 10])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_fixed_passes_match_the_restatement(smm, oracle, name, dtype, it, damp):
    rows, cols, csr, csr_t, b = system(name, dtype)
    st_ref, x_ref, it_ref, why_ref, res_ref, arn_ref, sens = reference(oracle, name, dtype, it, damp)
    tol = allowed(x_ref, sens, dtype)
    x = np.zeros(cols, dtype=dtype)
    info = {}
    st = smm.LSQR(make(smm, rows, cols, csr), b.copy(), x, it, 0.0, damp, info=info)
    err = worst(x, x_ref)
    print(name, np.dtype(dtype).name, it, "damp", damp, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert info["iterations"] == it_ref == it
    assert int(st) == st_ref == MAX_ITERATIONS_REACHED and info["reason"] == why_ref == 0
    assert err <= tol
    assert info["resnorm2"] > 0 and info["arnorm2"] > 0


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_converged_fp64(smm, oracle, name, damp):
    dtype = np.float64
    eps = EPS[dtype]
    rows, cols, csr, csr_t, b = system(name, dtype)
    st_ref, x_ref, it_ref, why_ref, _, _ = converged(oracle, name, dtype, damp)
    ref = answer(name, dtype, damp)
    own = worst(x_ref, ref)  # the restatement's own error: the yardstick
    x = np.zeros(cols)
    info = {}
    st = smm.LSQR(make(smm, rows, cols, csr), b.copy(), x, -1, eps, damp, info=info)
    err = worst(x, ref)
    _, atr = true_quantities(csr, cols, b, x, damp)
    bound = max(4 * own, RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))))
    print(name, "damp", damp, "steps", info["iterations"], "restatement", it_ref, "reason", info["reason"], "max|x - lstsq|", err, "restatement's", own, "bound", bound,
          "true |At r|", atr)
    assert int(st) == st_ref == SUCCESS and info["reason"] == why_ref
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    assert err <= bound
    assert atr <= 10 * eps
    assert (info["resnorm2"] <= eps * eps) if why_ref == 1 else (info["arnorm2"] <= eps * eps)


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_converged_fp32(smm, oracle, name, damp):
    """the step count must lie inside the range of the restatement's unperturbed and three perturbed runs, widened by max(2, it_ref // 5)"""
    dtype = np.float32
    eps = EPS[dtype]
    rows, cols, csr, csr_t, b = system(name, dtype)
    zero = np.zeros(cols, dtype=dtype)
    st_ref, x_ref, it_ref, why_ref, _, _ = converged(oracle, name, dtype, damp)
    counts = [it_ref] + [lsqr(oracle, csr, csr_t, perturbed(b, seed), zero, -1, eps, damp)[2] for seed in range(3)]
    ref = answer(name, dtype, damp)
    own = worst(x_ref, ref)
    x = zero.copy()
    info = {}
    st = smm.LSQR(make(smm, rows, cols, csr), b.copy(), x, -1, eps, damp, info=info)
    err = worst(x, ref)
    _, atr = true_quantities(csr, cols, b, x, damp)
    bound = max(4 * own, RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))))
    print(name, "damp", damp, "steps", info["iterations"], "restatement", counts, "reason", info["reason"], "max|x - lstsq|", err, "restatement's", own, "bound", bound,
          "true |At r|", atr)
    assert int(st) == st_ref == SUCCESS and info["reason"] == why_ref
    slack = max(2, it_ref // 5)
    assert min(counts) - slack <= info["iterations"] <= max(counts) + slack, (info, counts)
    assert err <= bound
    assert atr <= 100 * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_the_minimum_norm_answer(smm, oracle, dtype):
    """grad2d_12: x orthogonal to the constants; sparse_random: x[17] == 0 exactly (column 17 is empty); wide: x in the range of At"""
    eps = EPS[dtype]
    for name in ("grad2d_12", "sparse_random", "wide"):
        rows, cols, csr, csr_t, b = system(name, dtype)
        x_ref = converged(oracle, name, dtype, 0.0)[1]
        ref = answer(name, dtype, 0.0)
        bound = max(4 * worst(x_ref, ref), RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))))
        x = np.zeros(cols, dtype=dtype)
        assert int(smm.LSQR(make(smm, rows, cols, csr), b.copy(), x, -1, eps)) == SUCCESS
        a = cases.dense(csr, cols)
        null = np.linalg.svd(a)[2][cases.RANK[name]:]  # an orthonormal basis of the null space
        inside = float(np.max(np.abs(null @ x.astype(np.float64))))
        print(name, np.dtype(dtype).name, "largest null-space component", inside, "bound", bound * np.sqrt(cols))
        assert inside <= bound * np.sqrt(cols)  # (a unit vector against an x that is off by `bound` per element)
        if name == "grad2d_12":
            assert abs(float(np.sum(x.astype(np.float64)))) <= bound * cols
        if name == "sparse_random":
            assert x[cases.EMPTY_COL] == 0.0


def test_the_residual_estimate_never_grows(smm):
    rows, cols, csr, csr_t, b = system("tall", np.float64)
    A = make(smm, rows, cols, csr)
    At = A.transpose()
    seen = []
    for k in range(1, 13):
        x = np.zeros(cols)
        info = {}
        smm.LSQR(A, b.copy(), x, k, 0.0, at=At, info=info)
        assert info["iterations"] == k
        seen.append(info["resnorm2"])
    print("resnorm2 by pass limit", seen)
    assert all(seen[k + 1] <= seen[k] for k in range(len(seen) - 1))
    assert seen[0] <= float(np.dot(b, b))


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_estimates_follow_the_true_quantities(smm, oracle, name, dtype, damp):
    """after 10 fixed steps: |resnorm2 - (||r||^2 + damp^2 ||x||^2)| and |arnorm2 - ||At r - damp^2 x||^2|, each at most 4 x the largest such
    gap of the restatement's own runs (b unperturbed and perturbed by one unit in the last place, three sign patterns)"""
    it = 10
    rows, cols, csr, csr_t, b = system(name, dtype)
    zero = np.zeros(cols, dtype=dtype)
    gap_res, gap_arn = 0.0, 0.0
    for bb in [b] + [perturbed(b, seed) for seed in range(3)]:
        _, x_ref, _, _, res_ref, arn_ref = lsqr(oracle, csr, csr_t, bb, zero, it, 0.0, damp)
        t_res, t_atr = true_quantities(csr, cols, bb, x_ref, damp)
        gap_res = max(gap_res, abs(float(res_ref) - t_res))
        gap_arn = max(gap_arn, abs(float(arn_ref) - t_atr * t_atr))
    x = zero.copy()
    info = {}
    smm.LSQR(make(smm, rows, cols, csr), b.copy(), x, it, 0.0, damp, info=info)
    t_res, t_atr = true_quantities(csr, cols, b, x, damp)
    got_res, got_arn = abs(info["resnorm2"] - t_res), abs(info["arnorm2"] - t_atr * t_atr)
    print(name, np.dtype(dtype).name, "damp", damp, "resnorm2", info["resnorm2"], "true", t_res, "gap", got_res, "restatement's", gap_res, "| arnorm2", info["arnorm2"],
          "true", t_atr * t_atr, "gap", got_arn, "restatement's", gap_arn)
    assert got_res <= 4 * gap_res
    assert got_arn <= 4 * gap_arn


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_same_bits_twice(smm, dtype):
    rows, cols, csr, csr_t, b = system("tall", dtype)
    A = make(smm, rows, cols, csr)
    runs = []
    for _ in range(2):
        x = np.zeros(cols, dtype=dtype)
        info = {}
        st = smm.LSQR(A, b.copy(), x, -1, EPS[dtype], cases.DAMP, info=info)
        runs.append((int(st), info["iterations"], info["reason"], info["resnorm2"], info["arnorm2"], x))
    assert runs[0][:5] == runs[1][:5] and runs[0][0] == SUCCESS
    np.testing.assert_array_equal(bits(runs[0][5]), bits(runs[1][5]))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_the_three_ways_to_give_the_transpose(smm, dtype):
    """at=None and at=A.transpose() on the tall matrix; at=None, at=A.transpose() and at=A on poisson2d(12, 12), whose transpose has its
    bits: the same bits each time"""
    def run(A, b, cols, at):
        x = np.zeros(cols, dtype=dtype)
        info = {}
        st = smm.LSQR(A, b.copy(), x, 25, 0.0, at=at, info=info)
        return (int(st), info["iterations"], info["resnorm2"], info["arnorm2"]), x

    rows, cols, csr, csr_t, b = system("tall", dtype)
    A = make(smm, rows, cols, csr)
    first, x_none = run(A, b, cols, None)
    second, x_kept = run(A, b, cols, A.transpose())
    assert first == second and first[1] == 25
    np.testing.assert_array_equal(bits(x_none), bits(x_kept))

    csr = gen.poisson2d(12, 12, dtype=dtype)
    n = len(csr[0]) - 1
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(dtype)
    S = make(smm, n, n, csr)
    assert S.isSymmetric() == (True, True)
    got = [run(S, b, n, at) for at in (None, S.transpose(), S)]
    assert got[0][0] == got[1][0] == got[2][0]
    np.testing.assert_array_equal(bits(got[0][1]), bits(got[1][1]))
    np.testing.assert_array_equal(bits(got[0][1]), bits(got[2][1]))


@pytest.mark.parametrize("name", cases.CONSISTENT)
def test_a_nonzero_start(smm, oracle, name):
    """consistent cases: the undamped answer from x0 != 0 is x0 plus the minimum-norm correction (convdiff2d_12: THE solution, unchanged);
    with damp > 0 it is the correction x - x0 that is damped, not x"""
    dtype = np.float64
    eps = EPS[dtype]
    rows, cols, csr, csr_t, b = system(name, dtype)
    a = cases.dense(csr, cols)
    A = make(smm, rows, cols, csr)
    x0 = np.random.default_rng(3).uniform(-1, 1, cols)
    want = x0 + np.linalg.lstsq(a, b - a @ x0, rcond=1e-10)[0]
    own = worst(lsqr(oracle, csr, csr_t, b, x0, -1, eps)[1], want)  # the restatement's own error from the same start: the yardstick
    bound = max(4 * own, RTOL[dtype] * max(1.0, float(np.max(np.abs(want)))))
    x = x0.copy()
    info = {}
    st = smm.LSQR(A, b.copy(), x, -1, eps, info=info)
    print(name, "from x0: steps", info["iterations"], "max|x - (x0 + dx)|", worst(x, want), "bound", bound)
    assert int(st) == SUCCESS and info["reason"] == 1 and worst(x, want) <= bound
    if name == "convdiff2d_12":
        assert worst(x, answer(name, dtype, 0.0)) <= bound
    # three fixed steps against the restatement from the same start
    st_ref, x_ref, it_ref, _, _, _ = lsqr(oracle, csr, csr_t, b, x0, 3, 0.0)
    x = x0.copy()
    st = smm.LSQR(A, b.copy(), x, 3, 0.0, info=info)
    assert int(st) == st_ref and info["iterations"] == it_ref == 3
    assert worst(x, x_ref) <= RTOL[dtype] * max(1.0, float(np.max(np.abs(x_ref))))
    damp = cases.DAMP
    want = x0 + np.linalg.solve(a.T @ a + damp * damp * np.eye(cols), a.T @ (b - a @ x0))
    own = worst(lsqr(oracle, csr, csr_t, b, x0, -1, eps, damp)[1], want)
    bound = max(4 * own, RTOL[dtype] * max(1.0, float(np.max(np.abs(want)))))
    x = x0.copy()
    st = smm.LSQR(A, b.copy(), x, -1, eps, damp, info=info)
    res, atr = true_quantities(csr, cols, b, x, damp, x0)
    print(name, "damped from x0: steps", info["iterations"], "max|x - (x0 + dx)|", worst(x, want), "|At r - damp^2 dx|", atr)
    assert int(st) == SUCCESS and info["reason"] == 2 and worst(x, want) <= bound
    assert atr <= 10 * eps and abs(info["resnorm2"] - res) <= 1e-10 * res
    assert worst(x, answer(name, dtype, damp)) > 1e-3


FAMILIES = [("STREAM", 1), ("STREAM", 2), ("STREAM", 4), ("PATTERN", 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["tall", "sparse_random", "convdiff2d_12"])
def test_every_spmv_family(smm, oracle, name, dtype):
    """both handles forced to one family; PATTERN where the analysis takes the matrix and its transpose (a refusal is printed)"""
    it = 10
    rows, cols, csr, csr_t, b = system(name, dtype)
    _, x_ref, _, _, _, _, sens = reference(oracle, name, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    ran = []
    for family, lanes in FAMILIES:
        A = make(smm, rows, cols, csr)
        At = A.transpose()
        try:
            A.set_kernel(getattr(smm, "SPMV_" + family), lanes)
            At.set_kernel(getattr(smm, "SPMV_" + family), lanes)
        except smm.SmmHipError as e:
            assert family == "PATTERN", (family, lanes, str(e))
            print(name, family, lanes, "refused:", e)
            continue
        x = np.zeros(cols, dtype=dtype)
        info = {}
        smm.LSQR(A, b.copy(), x, it, 0.0, at=At, info=info)
        assert info["iterations"] == it
        assert A.get_kernel() == (getattr(smm, "SPMV_" + family), lanes) == At.get_kernel()
        err = worst(x, x_ref)
        print(name, family, lanes, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol)
        assert err <= tol, (family, lanes)
        ran.append(family)
    assert ran.count("STREAM") == 3


def test_refusals(smm):
    lib = _lib.load()
    dtype = np.float64
    rows, cols, csr, csr_t, b = system("tall", dtype)
    A = make(smm, rows, cols, csr)
    At = A.transpose()
    A32 = make(smm, rows, cols, system("tall", np.float32)[2])
    other = make(smm, *system("grad2d_12", dtype)[:3])
    fewer_start = csr_t[0].copy()  # the shape of the transpose, one entry short
    fewer_start[-1] -= 1
    fewer = make(smm, cols, rows, (fewer_start, csr_t[1][:-1].copy(), csr_t[2][:-1].copy()))
    offers = {
        "a wrong-shape at": dict(at=other),
        "A itself as at, A not square": dict(at=A),
        "an at of the other dtype": dict(at=A32.transpose()),
        "an at with another entry count": dict(at=fewer),
        "a negative damp": dict(damp=-0.5),
        "a NaN damp": dict(damp=float("nan")),
        "an infinite damp": dict(damp=float("inf")),
        "a negative eps": dict(eps=-1e-8),
        "a NaN eps": dict(eps=float("nan")),
    }
    for what, kw in offers.items():
        x = np.full(cols, 0.25)
        info = {}
        with pytest.raises(smm.SmmHipError) as e:
            smm.LSQR(A, b.copy(), x, 1, kw.get("eps", 0.0), kw.get("damp", 0.0), at=kw.get("at"), info=info)
        message = lib.smm_hip_last_error().decode()
        print(what, "->", message)
        assert e.value.code == INVALID and message.startswith("lsqr:"), (what, message)
        assert np.all(x == 0.25) and not info, what
    # the same handles are taken once they fit
    x = np.zeros(cols)
    assert int(smm.LSQR(A, b.copy(), x, 1, 0.0, at=At)) == MAX_ITERATIONS_REACHED
    # null vectors, a null matrix, vectors of the other dtype's matrix: the outputs stay unwritten
    st_c, it_c, why_c, res_c = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_double(-7.0)
    out = (ctypes.byref(st_c), ctypes.byref(it_c), ctypes.byref(why_c), ctypes.byref(res_c), None)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    x = np.full(cols, 0.25)
    bb = b.copy()
    assert lib.smm_hip_lsqr_f64(A._h, None, None, p(x), 1, 0.0, 0.0, *out) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("lsqr:")
    assert lib.smm_hip_lsqr_f64(A._h, None, p(bb), None, 1, 0.0, 0.0, *out) == INVALID
    assert lib.smm_hip_lsqr_f64(None, None, p(bb), p(x), 1, 0.0, 0.0, *out) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("lsqr:")
    assert lib.smm_hip_lsqr_f64(A32._h, None, p(bb), p(x), 1, 0.0, 0.0, *out) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("lsqr:")
    assert lib.smm_hip_lsqr_dev_f64(A._h, None, None, None, 1, 0.0, 0.0, None, *out) == INVALID
    assert (st_c.value, it_c.value, why_c.value, res_c.value) == (-7, -7, -7, -7.0) and np.all(x == 0.25)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_edges(smm, oracle, dtype):
    lib = _lib.load()
    suf = "f32" if dtype == np.float32 else "f64"
    fn = getattr(lib, f"smm_hip_lsqr_{suf}")
    CT = ctypes.c_float if dtype == np.float32 else ctypes.c_double
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rows, cols, csr, csr_t, b = system("tall", dtype)
    A = make(smm, rows, cols, csr)
    info = {}
    # maxIterations == 0: no step, x keeps its bits, the status of the start values
    x0 = np.random.default_rng(5).uniform(-1, 1, cols).astype(dtype)
    x = x0.copy()
    st = smm.LSQR(A, b.copy(), x, 0, EPS[dtype], info=info)
    assert (int(st), info["iterations"], info["reason"]) == (MAX_ITERATIONS_REACHED, 0, 0) and info["resnorm2"] > 0 and info["arnorm2"] > 0
    np.testing.assert_array_equal(bits(x), bits(x0))
    # b == 0 from x = 0: reason 1 at once
    x = np.zeros(cols, dtype=dtype)
    st = smm.LSQR(A, np.zeros(rows, dtype=dtype), x, -1, EPS[dtype], info=info)
    assert (int(st), info["iterations"], info["reason"], info["resnorm2"]) == (SUCCESS, 0, 1, 0.0) and not x.any()
    # b orthogonal to the range of A, exactly: the unit vector of an empty row -- At b is 0 bit for bit, reason 2 at once
    rows_s, cols_s, csr_s, _, _ = system("sparse_random", dtype)
    S = make(smm, rows_s, cols_s, csr_s)
    unit = np.zeros(rows_s, dtype=dtype)
    unit[cases.EMPTY_ROW] = 1.0
    x = np.zeros(cols_s, dtype=dtype)
    st = smm.LSQR(S, unit, x, -1, EPS[dtype], info=info)
    assert (int(st), info["iterations"], info["reason"], info["resnorm2"], info["arnorm2"]) == (SUCCESS, 0, 2, 1.0, 0.0) and not x.any()
    # rows == 0, cols == 0: nothing is read or written through b / x
    one = np.zeros(1, dtype=np.int32)
    none_i, none_v = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)
    for (r, c), why in (((0, 3), 1), ((3, 0), 2), ((0, 0), 1)):
        E = smm.CSRMatrix(r, c, np.zeros(r + 1, dtype=np.int32) if r else one, none_i, none_v)
        st_c, it_c, why_c, res_c, arn_c = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), CT(-1), CT(-1)
        assert fn(E._h, None, None, None, -1, dtype(1e-6), dtype(0), ctypes.byref(st_c), ctypes.byref(it_c), ctypes.byref(why_c), ctypes.byref(res_c),
                  ctypes.byref(arn_c)) == 0, lib.smm_hip_last_error()
        assert (st_c.value, it_c.value, why_c.value, res_c.value, arn_c.value) == (SUCCESS, 0, why, 0.0, 0.0)
        xb, xx = np.full(r, 0.5, dtype=dtype), np.full(c, 0.5, dtype=dtype)
        assert int(smm.LSQR(E, xb, xx, -1, 1e-6)) == SUCCESS and np.all(xb == 0.5) and np.all(xx == 0.5)
    # no entries: reason 2 at once (reason 1 for b == 0), x untouched
    Z = smm.CSRMatrix(3, 2, np.zeros(4, dtype=np.int32), none_i, none_v)
    x = np.full(2, 0.5, dtype=dtype)
    st = smm.LSQR(Z, np.ones(3, dtype=dtype), x, -1, 1e-6, info=info)
    assert (int(st), info["iterations"], info["reason"], info["resnorm2"], info["arnorm2"]) == (SUCCESS, 0, 2, 3.0, 0.0) and np.all(x == 0.5)
    st = smm.LSQR(Z, np.zeros(3, dtype=dtype), x, -1, 1e-6, cases.DAMP, at=Z.transpose(), info=info)
    assert (int(st), info["iterations"], info["reason"]) == (SUCCESS, 0, 1) and np.all(x == 0.5)
    # the outputs are optional; more steps than cols are allowed and stay finite
    x = np.zeros(cols, dtype=dtype)
    bb = b.copy()
    assert fn(A._h, None, p(bb), p(x), 3, dtype(0), dtype(0), None, None, None, None, None) == 0
    x = np.zeros(cols, dtype=dtype)
    st = smm.LSQR(A, b.copy(), x, 2 * cols, 0.0, info=info)
    assert info["iterations"] > cols and np.isfinite(x).all()
    assert worst(x, answer("tall", dtype, 0.0)) <= (1e-2 if dtype == np.float32 else 1e-8)


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_device_pointers_on_offset_views_and_another_stream(smm, oracle, name, damp):
    """smm_hip_lsqr_dev_f64 on a stream of the caller's: b (rows elements) and x (cols elements) are views at element alignment inside
    larger buffers with NaN guard bands -- on a wide AND a tall matrix, so a length taken from the wrong dimension reads a NaN or writes
    a guard"""
    dtype, it = np.float64, 3
    rows, cols, csr, csr_t, b = system(name, dtype)
    st_ref, x_ref, _, _, _, _, sens = reference(oracle, name, dtype, it, damp)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(cols, dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved = snapshot(d_b)
    A = smm.CSRMatrix.from_device(rows, cols, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    for at in (None, A.transpose(s.cuda_stream)):
        d_x.zero_()
        torch.cuda.synchronize()
        st, k, why, res, arn = host.lsqr_dev(A, d_b, d_x, it, 0.0, damp, at, s.cuda_stream)
        torch.cuda.synchronize()
        assert int(st) == st_ref == MAX_ITERATIONS_REACHED and (k, why) == (it, 0) and res > 0 and arn > 0
        assert worst(d_x.cpu().numpy(), x_ref) <= allowed(x_ref, sens, dtype)
        assert_unchanged(d_b, saved, "b")
        assert_guards_intact(d_b, "b")
        assert_guards_intact(d_x, "x")
    # a start that is not zero takes the set-up SpMV: x is read over cols elements, b over rows
    x0 = np.random.default_rng(9).uniform(-1, 1, cols)
    _, x_ref, _, _, _, _ = lsqr(oracle, csr, csr_t, b, x0, it, 0.0, damp)
    d_x.copy_(torch.from_numpy(x0))
    torch.cuda.synchronize()
    st, k, why, res, arn = host.lsqr_dev(A, d_b, d_x, it, 0.0, damp, None, s.cuda_stream)
    torch.cuda.synchronize()
    assert k == it and worst(d_x.cpu().numpy(), x_ref) <= RTOL[dtype] * max(1.0, float(np.max(np.abs(x_ref))))
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
    dtype, it = np.float64, 10
    rows, cols, csr, csr_t, b = system("tall", dtype)
    st_ref, x_ref, _, _, _, _, sens = reference(oracle_fma, "tall", dtype, it, cases.DAMP, fma=True)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h = P()
    assert lib.smm_hip_csr_create_f64(rows, cols, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    fn = lib.smm_hip_lsqr_f64
    I, D = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [P, P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double, I, I, I, D, D]
    st, k, why, res, arn = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    x = np.zeros(cols, dtype=dtype)
    rc = fn(h, None, ptr(b.copy()), ptr(x), it, 0.0, cases.DAMP, ctypes.byref(st), ctypes.byref(k), ctypes.byref(why), ctypes.byref(res), ctypes.byref(arn))
    assert rc == 0, lib.smm_hip_last_error()
    lib.smm_hip_csr_destroy(h)
    assert st.value == st_ref == MAX_ITERATIONS_REACHED and k.value == it
    assert np.isfinite(x).all() and worst(x, x_ref) <= allowed(x_ref, sens, dtype)


def test_cpp_dropin_case_on_the_gpu(tmp_path):
    """tests/cpp/lsqr_case.cpp: SMM::LSQR on `tall` built in the case itself, float and double: SUCCESS by reason 2 (b is inconsistent), a
    count below cols, ||At r|| formed by the case in double under the bound of the converged tests, and a residual that is not small"""
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double"}
    for name, w in lines.items():
        status, hip, steps, reason, atr, res = int(w[2]), int(w[4]), int(w[6]), int(w[8]), float.fromhex(w[10]), float.fromhex(w[12])
        assert (status, hip, reason) == (SUCCESS, 0, 2), w
        assert 0 < steps < 144
        assert atr <= (100 * 1e-3 if name == "float" else 10 * 1e-8)
        assert res > 0.5
