"""The aggregation multigrid preconditioner on the GPU (csrc/smm_precond_amg.hip) through the C ABI, against its CPU restatement
(tests/amg_restatement.py): the hierarchy's structure exactly, its values bit for bit, the coarse inverse, the cycle bit for bit at one
lane per row and by the fixed-pass tolerance rule of tests/test_gpu_cgs.py elsewhere, the device-pointer form on offset views, the three
solvers that take it, refresh, the refusals and edges, the frozen loop, the fma flavour and the drop-in C++ header."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from amg_cases import NAMES as GRAPH_CASES
from amg_cases import case as graph_case
from amg_restatement import coarse_inverse, dense_of, hierarchy, make_apply, operator_complexity, products
from chebyshev_restatement import bicgstab, diagonal, gershgorin, pcg, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres
from gmres_restatement import sensitivity as gmres_sensitivity
from test_amg_cpu import build_case, case
from test_chebyshev_cpu import spd5
from test_gpu_cgs import allowed, make, worst
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID, PRECOND = -1, -4  # SMM_HIP_ERR_INVALID, SMM_HIP_ERR_PRECOND
CASES = ("poisson2d_32", "stencil3d_12", "convdiff3d_12", "convdiff3d_20", "spd5", "poisson2d_32_c48")
FIXED_STEPS = 5  # the passes of the fixed-step comparisons with the restated loops
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def reference(name, dtype):
    """(csr, keyword arguments, the restated hierarchy, b = A 1, a fixed right-hand side), made once; the names of tests/amg_cases.py
    (tests/test_gpu_amg_graphs.py) are served as well"""
    def compute():
        csr, kw = (graph_case if name in GRAPH_CASES else case)(name, dtype)
        n = len(csr[0]) - 1
        return csr, kw, hierarchy(csr, **kw), gen.row_sums(csr[0], csr[2]), np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    return cached(("ref", name, np.dtype(dtype).name), compute)


def triple(m):
    return (*m.get_pattern(), m.get_values())


def library_levels(M):
    """the library's hierarchy in the restatement's form, every matrix read back from the device: the cycle restated on the library's
    own operators (their values are compared with the restatement's separately)"""
    info = M.amg_info()
    out = []
    for l in range(info["levels"]):
        A, P, R = M.amg_level(l)
        a = triple(A)
        lv = {"A": a, "diag": diagonal(a), "lam": gershgorin(a) if len(a[0]) > 1 else 1.0}
        if P is not None:
            lv["P"], lv["R"] = triple(P), triple(R)
        out.append(lv)
    return out


def one_lane_per_row(smm, M):
    for l in range(M.amg_info()["levels"]):
        for m in M.amg_level(l):
            if m is not None:
                m.set_kernel(smm.SPMV_STREAM, 1)


def assert_same_csr(got, want, what, values=True):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what}: start")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: positions")
    if values:
        np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg=f"{what}: values")


# ---- the hierarchy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", CASES)
def test_structure_is_exact(smm, name, dtype):
    csr, kw, ref, _, _ = reference(name, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", **kw)
    info = M.amg_info()
    print(name, np.dtype(dtype).name, info)
    assert info["levels"] == len(ref)
    assert info["rows"] == [len(v["A"][0]) - 1 for v in ref]
    assert info["nnz"] == [len(v["A"][1]) for v in ref]
    assert info["operator_complexity"] == operator_complexity(ref)
    assert M.kind == smm.SolverPreconditioner.AMG
    for l, lv in enumerate(ref):
        Al, Pl, Rl = M.amg_level(l)
        assert_same_csr(Al.get_pattern(), lv["A"], f"A_{l}", values=False)
        if "P" in lv:
            np.testing.assert_array_equal(M.amg_aggregates(l), lv["agg"])
            assert_same_csr(Pl.get_pattern(), lv["P"], f"P_{l}", values=False)
            assert_same_csr(Rl.get_pattern(), lv["R"], f"R_{l}", values=False)
            assert (Pl.rows, Pl.cols, Rl.rows, Rl.cols) == (len(lv["agg"]), lv["n_c"], lv["n_c"], len(lv["agg"]))
        else:
            assert Pl is None and Rl is None and l == len(ref) - 1
    np.testing.assert_array_equal(bits(M.values()), bits(diagonal(csr)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("poisson2d_32", "convdiff3d_20", "poisson2d_32_c48"))
def test_values_are_bit_for_bit(smm, name, dtype):
    """level 0's products against the restatement outright; deeper levels with the restatement fed the library's own A_l"""
    csr, kw, ref, _, _ = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    for l, lv in enumerate(ref[:-1]):
        Al, Pl, Rl = M.amg_level(l)
        a = triple(Al)
        if l == 0:
            assert_same_csr(a, csr, "A_0")
            P, R, A_next = lv["P"], lv["R"], ref[1]["A"]
        else:
            fed = {"diag": diagonal(a), "lam": gershgorin(a), "agg": lv["agg"], "n_c": lv["n_c"]}
            P, R, _, A_next = products(a, fed)
        assert_same_csr(triple(Pl), P, f"P_{l}")
        assert_same_csr(triple(Rl), R, f"R_{l}")
        assert_same_csr(triple(M.amg_level(l + 1)[0]), A_next, f"A_{l + 1}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("poisson2d_32", "convdiff3d_20", "spd5"))
def test_coarse_inverse(smm, name, dtype):
    """|Inv A_L - I|_max against the same figure of np.linalg.inv (double) rounded to T: the margin is 8 x that rounding"""
    csr, kw, _, _, _ = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    levels = M.amg_info()["levels"]
    a = triple(M.amg_level(levels - 1)[0])
    dense = dense_of(a)
    n = len(dense)
    inv = M.amg_coarse_inverse()
    assert inv.shape == (n, n) and inv.dtype == np.dtype(dtype)
    ref = np.linalg.inv(dense)
    rounding = float(np.max(np.abs(ref.astype(dtype).astype(np.float64) @ dense - np.eye(n))))
    got = float(np.max(np.abs(inv.astype(np.float64) @ dense - np.eye(n))))
    print(name, np.dtype(dtype).name, "rows", n, "cond", float(np.linalg.cond(dense)), "|Inv A - I|", got, "reference rounded to T", rounding)
    assert got <= 8 * rounding


# ---- apply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", CASES)
def test_apply_bit_for_bit_at_one_lane_per_row(smm, oracle, name, dtype):
    csr, kw, _, _, r = reference(name, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", **kw)
    one_lane_per_row(smm, M)
    fn = make_apply(oracle, library_levels(M), M.amg_coarse_inverse())
    z = np.full(len(r), np.nan, dtype=dtype)
    saved = r.copy()
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(fn(r)))
    np.testing.assert_array_equal(bits(r), bits(saved))


def applied(oracle, name, dtype, tag="plain"):
    """(the restated cycle on the restated hierarchy, z = M^-1 r, its sensitivity), made once"""
    def compute():
        _, _, ref, _, r = reference(name, dtype)
        fn = make_apply(oracle, ref, coarse_inverse(ref[-1]["A"]))
        z = fn(r)
        return fn, z, sensitivity(fn, r, z)
    return cached(("apply", tag, name, np.dtype(dtype).name), compute)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("poisson2d_32", "convdiff3d_20", "poisson2d_32_c48", "spd5"))
def test_apply_at_the_auto_choice_by_tolerance(smm, oracle, name, dtype):
    csr, kw, _, _, r = reference(name, dtype)
    fn, z_ref, sens = applied(oracle, name, dtype)
    tol = allowed(z_ref, sens, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    z = np.zeros(len(r), dtype=dtype)
    M.apply(r, z)
    again = np.zeros(len(r), dtype=dtype)
    M.apply(r, again)
    err = worst(z, z_ref)
    print(name, np.dtype(dtype).name, "max|z - ref|", err, "allowed", tol, "sensitivity", sens)
    assert err <= tol
    np.testing.assert_array_equal(bits(z), bits(again))
    x = np.zeros(len(r), dtype=dtype)  # x = M^-1 (A v): the generic SpMV-then-apply path
    M.apply_spmv(r, x)
    v = oracle.spmv(csr, 0, None, r)
    x_ref = fn(v)
    assert worst(x, x_ref) <= allowed(x_ref, sensitivity(fn, v, x_ref), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_device_pointers_on_offset_views_and_another_stream(smm, oracle, dtype):
    name = "convdiff3d_20"
    csr, kw, _, _, r = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    one_lane_per_row(smm, M)
    z_ref = make_apply(oracle, library_levels(M), M.amg_coarse_inverse())(r)
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
def restated(oracle, solver, name, dtype, it, eps):
    """(status, x, iterations, sensitivity or None) of the restated loop with the restated cycle, made once"""
    def compute():
        csr, _, _, b, _ = reference(name, dtype)
        fn = applied(oracle, name, dtype)[0]
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
    return cached(("solve", solver, name, np.dtype(dtype).name, it, eps), compute)


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
@pytest.mark.parametrize("solver,name", [("cg", "poisson2d_32"), ("cg", "stencil3d_12"), ("bicgstab", "convdiff3d_12"), ("gmres", "convdiff3d_12")])
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, name, dtype):
    it = FIXED_STEPS
    csr, kw, _, b, _ = reference(name, dtype)
    st_ref, x_ref, it_ref, sens = restated(oracle, solver, name, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.AMG, **kw)
    st, x, info = run(smm, solver, A, b, it, 0.0, M, dtype)
    err = worst(x, x_ref)
    print(solver, name, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol, "sensitivity", sens, info)
    assert st == st_ref and info["iterations"] == it_ref == it
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name", [("cg", "poisson2d_32"), ("cg", "poisson2d_32_c48"), ("bicgstab", "convdiff3d_20"), ("gmres", "convdiff3d_20")])
def test_converged_runs(smm, oracle, solver, name, dtype):
    """SUCCESS, the restated loop's iteration count within max(2, ref // 5), and fewer iterations than the same call without M"""
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr, kw, _, b, _ = reference(name, dtype)
    st_ref, _, it_ref, _ = restated(oracle, solver, name, dtype, -1, eps)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.AMG, **kw)
    st, x, info = run(smm, solver, A, b, -1, eps, M, dtype)
    st0, _, info0 = run(smm, solver, A, b, -1, eps, None, dtype)
    print(solver, name, np.dtype(dtype).name, "iterations", info["iterations"], "restated", it_ref, "unpreconditioned", info0["iterations"],
          "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0 and st0 == 0
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5)
    assert info["iterations"] < info0["iterations"]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name", [("cg", "poisson2d_32"), ("bicgstab", "convdiff3d_20")])
def test_frozen_loop(smm, solver, name, dtype):
    """The applies queued behind the pass that left the loop must write nothing: a converged run with maxIterations = -1 and a run of
    exactly that many planned passes give the same bits."""
    eps = 1e-3 if dtype == np.float32 else 1e-8
    csr, kw, _, b, _ = reference(name, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.AMG, **kw)
    st1, x1, info1 = run(smm, solver, A, b, -1, eps, M, dtype)
    assert st1 == 0 and 2 < info1["iterations"] < len(b) - 8
    st2, x2, info2 = run(smm, solver, A, b, info1["iterations"], eps, M, dtype)
    assert st2 == 0 and info2 == info1
    np.testing.assert_array_equal(bits(x1), bits(x2))


# ---- refresh -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refresh_after_scaling_equals_a_fresh_create(smm, dtype):
    """A scaled by 2 changes no strength decision: same structure, and the apply of the refreshed handle equals that of a handle created
    on the scaled matrix, bit for bit at one lane per row"""
    name = "convdiff3d_20"
    csr, kw, ref, _, r = reference(name, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", **kw)
    before = M.amg_info()
    A.scale(2.0)
    M.amg_refresh()
    fresh = A.getPreconditioner("AMG", **kw)
    assert M.amg_info() == before == fresh.amg_info()
    for l in range(before["levels"]):
        for got, want in zip(M.amg_level(l), fresh.amg_level(l)):
            assert (got is None) == (want is None)
            if got is not None:
                assert_same_csr(triple(got), triple(want), f"level {l}")
        if l + 1 < before["levels"]:
            np.testing.assert_array_equal(M.amg_aggregates(l), fresh.amg_aggregates(l))
    np.testing.assert_array_equal(bits(M.amg_coarse_inverse()), bits(fresh.amg_coarse_inverse()))
    one_lane_per_row(smm, M)
    one_lane_per_row(smm, fresh)
    z, z2 = np.zeros(len(r), dtype=dtype), np.zeros(len(r), dtype=dtype)
    M.apply(r, z)
    fresh.apply(r, z2)
    np.testing.assert_array_equal(bits(z), bits(z2))
    np.testing.assert_array_equal(bits(M.values()), bits(fresh.values()))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refresh_after_an_entry_edit_keeps_the_old_aggregates(smm, dtype):
    name = "poisson2d_32_c48"
    csr, kw, ref, _, _ = reference(name, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", **kw)
    start, pos, val = csr
    rows = np.array([3, 200, 777], dtype=np.int32)
    cols = np.array([pos[start[i] + (1 if pos[start[i]] == i else 0)] for i in rows], dtype=np.int32)  # an off-diagonal entry of each row
    new = np.array([-0.875, -1.125, -0.5], dtype=dtype)
    A.update_entries(rows, cols, new)
    M.amg_refresh()
    edited = (start, pos, A.get_values())
    assert (bits(edited[2]) != bits(val)).sum() == 3
    a = edited
    for l, lv in enumerate(ref[:-1]):  # the restatement with the OLD aggregates, level by level on the library's own A_l
        Al, Pl, Rl = M.amg_level(l)
        assert_same_csr(triple(Al), a, f"A_{l}")
        np.testing.assert_array_equal(M.amg_aggregates(l), lv["agg"])
        P, R, _, A_next = products(a, {"diag": diagonal(a), "lam": gershgorin(a), "agg": lv["agg"], "n_c": lv["n_c"]})
        assert_same_csr(triple(Pl), P, f"P_{l}")
        assert_same_csr(triple(Rl), R, f"R_{l}")
        a = triple(M.amg_level(l + 1)[0])
        assert_same_csr(a, A_next, f"A_{l + 1}")
    kept = hierarchy(edited, keep=[lv["agg"] for lv in ref[:-1]], **kw)
    assert [len(v["A"][0]) - 1 for v in kept] == M.amg_info()["rows"]


# ---- edges -------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


def diagonal_matrix(smm, n, dtype):
    return smm.CSRMatrix(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(1.0, 2.0, n).astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals(smm, dtype):
    start, pos, val = spd5(dtype)
    G = smm.SolverPreconditioner.AMG
    for bad in (0.0, 1e-6):  # a stored zero, a 1e-6 and a missing diagonal; an empty row
        v = val.copy()
        v[start[3] + 1] = bad
        assert code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(G)) == PRECOND
    keep = np.ones(len(pos), dtype=bool)
    keep[start[3] + 1] = False
    s2 = start.copy()
    s2[4:] -= 1
    assert code_of(lambda: make(smm, (s2, pos[keep], val[keep])).getPreconditioner(G)) == PRECOND
    ragged = gen_matrices(dtype)["ragged_300"]
    assert code_of(lambda: make(smm, ragged).getPreconditioner(G)) == PRECOND
    # the empty row alone: rows 0 and 2 hold their diagonal, row 1 holds nothing
    hollow = smm.CSRMatrix(3, 3, np.array([0, 1, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([4.0, 5.0], dtype=dtype))
    assert code_of(lambda: hollow.getPreconditioner(G)) == PRECOND
    A = make(smm, (start, pos, val))
    for theta in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        assert code_of(lambda: A.getPreconditioner(G, theta=theta)) == INVALID
    for levels in (0, 17):
        assert code_of(lambda: A.getPreconditioner(G, max_levels=levels)) == INVALID
    for rows in (0, 1025):
        assert code_of(lambda: A.getPreconditioner(G, coarse_rows=rows)) == INVALID
    for degree in (-1, 65):
        assert code_of(lambda: A.getPreconditioner(G, smooth_degree=degree)) == INVALID
    for ratio in (1.0, 0.5, float("nan"), float("inf")):
        assert code_of(lambda: A.getPreconditioner(G, eig_ratio=ratio)) == PRECOND
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
    assert code_of(lambda: W.getPreconditioner(G)) == INVALID
    # the coarsest level above 1024 rows: max_levels 1 on 1728 rows; the message names the sizes
    big = make(smm, case("stencil3d_12", dtype)[0])
    with pytest.raises(_lib.SmmHipError) as e:
        big.getPreconditioner(G, max_levels=1)
    assert e.value.code == PRECOND and "1728" in str(e.value)
    # a foreign matrix, the batched solver, other kinds' queries
    b = gen.row_sums(start, val)
    x = np.zeros(5, dtype=dtype)
    M = A.getPreconditioner(G)
    other = make(smm, (start, pos, val))
    assert code_of(lambda: smm.ConjugateGradient(other, b, x, x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: smm.BiCGStab(other, b.copy(), x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: smm.GMRES(other, b.copy(), x, 5, 1e-6, 5, M)) == INVALID
    B = np.stack([b, b], axis=1).copy()
    assert code_of(lambda: smm.BiCGStabBatch(A, B, np.zeros_like(B), 5, 1e-6, M)) == INVALID
    assert code_of(lambda: M.apply(b, b)) == INVALID
    J = A.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    assert code_of(lambda: J.amg_info()) == INVALID
    assert code_of(lambda: J.amg_refresh()) == INVALID
    assert code_of(lambda: M.amg_aggregates(0)) == INVALID  # the dense solve alone: no aggregates
    assert int(smm.ConjugateGradient(A, b, x, x, -1, 1e-6 if dtype == np.float64 else 1e-4, M)) == 0
    np.testing.assert_allclose(x, 1.0, rtol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_edges(smm, dtype):
    G = smm.SolverPreconditioner.AMG
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    M = E.getPreconditioner(G)
    assert M.amg_info()["rows"] == [0]
    z = np.zeros(0, dtype=dtype)
    M.apply(z, z)
    assert len(M.values()) == 0
    one = smm.CSRMatrix(1, 1, np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([4.0], dtype=dtype))
    M = one.getPreconditioner(G)
    out = np.zeros(1, dtype=dtype)
    M.apply(np.array([2.0], dtype=dtype), out)
    assert M.amg_info()["levels"] == 1 and out[0] == 0.5 and M.amg_coarse_inverse()[0, 0] == 0.25
    # isolated rows: every row is its own root, n_c = n, the stall rule fires: dense only, or refused above 1024 rows
    D = diagonal_matrix(smm, 300, dtype)
    M = D.getPreconditioner(G)
    assert M.amg_info()["levels"] == 1 and M.amg_info()["rows"] == [300]
    r = np.linspace(-1, 1, 300).astype(dtype)
    out = np.zeros(300, dtype=dtype)
    M.apply(r, out)
    np.testing.assert_allclose(out, r / np.linspace(1.0, 2.0, 300).astype(dtype), rtol=4 * np.finfo(dtype).eps)
    assert code_of(lambda: diagonal_matrix(smm, 1025, dtype).getPreconditioner(G)) == PRECOND
    # max_levels = 2 stops a hierarchy that would have three levels
    csr = case("convdiff3d_20", dtype)[0]
    M = make(smm, csr).getPreconditioner(G, max_levels=2)
    assert M.amg_info()["rows"] == [8000, 766]


# ---- flavour and drop-in -----------------------------------------------------------------------------------------------------
def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so against the restatement over the fma oracle, by tolerance only (tests/test_gpu_chebyshev.py::test_fma_flavour)"""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    dtype, name = np.float64, "convdiff3d_12"
    csr, _, ref, _, r = reference(name, dtype)
    n = len(r)
    fn = make_apply(oracle_fma, ref, coarse_inverse(ref[-1]["A"]))
    z_ref = fn(r)
    sens = sensitivity(fn, r, z_ref)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h, m = P(), P()
    assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    create = lib.smm_hip_precond_create_amg
    create.argtypes = [P, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(P)]
    assert create(h, 0.08, 10, 256, 2, 30.0, ctypes.byref(m)) == 0, lib.smm_hip_last_error()
    levels = ctypes.c_int()
    info = lib.smm_hip_precond_amg_info
    info.argtypes = [P, ctypes.POINTER(ctypes.c_int), P, P, ctypes.c_size_t, P]
    assert info(m, ctypes.byref(levels), None, None, 0, None) == 0 and levels.value == len(ref)
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
    """tests/cpp/amg_case.cpp on mesh1e1_structural_48_48_177 (the goldens' CSR arrays), fp64: SMM::ConjugateGradient with the default
    SMM::AMGPreconditioner ends with SUCCESS within 10 * eps of the golden CG solution of the same asset"""
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
    print(r.stderr[-300:])
    lines = r.stdout.splitlines()
    assert lines[0] == "status 0 hip 0", lines[0] + r.stderr[-500:]
    x = np.array([float.fromhex(ln.split()[1]) for ln in lines[1:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, golden["asset/mesh1e1/float64/cg/x"], rtol=10 * eps)
