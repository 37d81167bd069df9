"""The multigrid preconditioner created with near-null-space candidates on the GPU (csrc/smm_precond_amg.hip) through the C ABI, against
its CPU restatement (tests/amg_candidates_restatement.py): dof aggregates, every pattern and the dropped-column counts exactly, T and
B_{l+1} bit for bit, the products by the rule of tests/test_gpu_amg.py, the aggregate-size edges of the QR kernel on forests of stars, the
cycle and the three solvers by the fixed-pass tolerance rule of tests/test_gpu_cgs.py, refresh, the device-pointer form on offset views,
the refusals, the untouched scalar path and the drop-in C++ header."""
import subprocess

import numpy as np
import pytest
import torch
from amg_candidates_restatement import LDS_ROWS, hierarchy, products
from amg_restatement import coarse_inverse, make_apply
from amg_restatement import hierarchy as scalar_hierarchy
from chebyshev_restatement import bicgstab, diagonal, gershgorin, pcg, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres
from gmres_restatement import sensitivity as gmres_sensitivity
from test_amg_candidates_cpu import COARSE_ROWS, build_case, elasticity, with_lone_node
from test_gpu_amg import assert_same_csr, bits, library_levels, one_lane_per_row, triple
from test_gpu_cgs import allowed, make, worst
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
FIXED_STEPS = 5
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def reference(name, dtype):
    """(csr, B, dofs per node, keyword arguments, the restated hierarchy, b = A 1, a fixed right-hand side), made once"""
    def compute():
        if name == "lone":
            csr, B, b = with_lone_node(dtype)
            kw = {"coarse_rows": 8}
        else:
            csr, B, b = elasticity(name, dtype)
            kw = {"coarse_rows": COARSE_ROWS}
        n = len(csr[0]) - 1
        return csr, B, b, kw, hierarchy(csr, B, b, **kw), gen.row_sums(csr[0], csr[2]), np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    return cached(("ref", name, np.dtype(dtype).name), compute)


def create(smm, csr, B, b, **kw):
    A = make(smm, csr)
    return A, A.getPreconditioner("AMG", candidates=B, dofs_per_node=b, **kw)


def check_hierarchy(M, ref, csr, what):
    """dof aggregates, the patterns of T, P, R, A_l and the dropped counts exactly; T and B_l bit for bit; P, R and A_{l+1} bit for bit,
    level 0 against the restatement outright, deeper levels with the restatement fed the library's own A_l"""
    info = M.amg_info()
    assert info["levels"] == len(ref), (what, info)
    assert info["rows"] == [len(v["A"][0]) - 1 for v in ref]
    assert info["nnz"] == [len(v["A"][1]) for v in ref]
    for l, lv in enumerate(ref):
        Al, Pl, Rl = M.amg_level(l)
        got = M.amg_candidates(l)
        assert_same_csr(Al.get_pattern(), lv["A"], f"{what} A_{l}", values=False)
        np.testing.assert_array_equal(bits(np.ascontiguousarray(got["B"])), bits(np.ascontiguousarray(lv["B"])), err_msg=f"{what} B_{l}")
        assert got["dropped"] == lv["dropped"], (what, l)
        if "P" not in lv:
            assert Pl is None and Rl is None and got["T"] is None and l == len(ref) - 1
            continue
        np.testing.assert_array_equal(M.amg_aggregates(l), lv["agg"], err_msg=f"{what} aggregates {l}")
        assert_same_csr(triple(got["T"]), lv["T"], f"{what} T_{l}")
        assert (got["T"].rows, got["T"].cols) == (len(lv["agg"]), lv["n_c"])
        a = triple(Al)
        if l == 0:
            assert_same_csr(a, csr, "A_0")
            P, R, A_next = lv["P"], lv["R"], ref[1]["A"]
        else:
            fed = dict(lv, diag=diagonal(a), lam=gershgorin(a))
            P, R, _, A_next = products(a, fed)
        assert_same_csr(triple(Pl), P, f"{what} P_{l}")
        assert_same_csr(triple(Rl), R, f"{what} R_{l}")
        assert_same_csr(triple(M.amg_level(l + 1)[0]), A_next, f"{what} A_{l + 1}")


# ---- the hierarchy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("e_16x16", "e_4x4x4", "lone"))
def test_structure_and_values(smm, name, dtype):
    csr, B, b, kw, ref, _, _ = reference(name, dtype)
    A, M = create(smm, csr, B, b, **kw)
    print(name, np.dtype(dtype).name, M.amg_info(), "dropped", [v["dropped"] for v in ref])
    assert len(ref) >= 2
    check_hierarchy(M, ref, csr, name)
    np.testing.assert_array_equal(bits(M.values()), bits(diagonal(csr)))
    if name == "lone":
        assert ref[0]["dropped"] == 1


def star_forest(leaves, b, dtype, seed=3):
    """disjoint stars, b dofs per node: the centre of a star with L leaves carries (L + 1) I_b, a leaf 1.5 I_b, an edge -I_b, and every
    node a 0.25 coupling between its own dofs.  Symmetric, strictly diagonally dominant.  With theta = 0.02 every edge is strong
    (b >= theta^2 |N_cc| |N_ll| up to L = 300), so each star is ONE aggregate of (L + 1) b dofs."""
    rows, cols, vals = [], [], []
    node = 0
    for L in leaves:
        c = node
        for j in range(L + 1):
            me = node + j
            for u in range(b):
                for v in range(b):
                    rows.append(me * b + u)
                    cols.append(me * b + v)
                    vals.append((float(L + 1) if j == 0 else 1.5) if u == v else 0.25 / b)
                if j:
                    rows += [me * b + u, c * b + u]
                    cols += [c * b + u, me * b + u]
                    vals += [-1.0, -1.0]
        node += L + 1
    n = node * b
    key = np.array(rows, dtype=np.int64) * n + np.array(cols, dtype=np.int64)
    order = np.argsort(key, kind="stable")
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(np.array(rows)[order], minlength=n), out=start[1:])
    B = np.random.default_rng(seed).uniform(-1, 1, (n, 6)).astype(dtype)
    return (start, np.array(cols, dtype=np.int32)[order], np.array(vals, dtype=dtype)[order]), B


FORESTS = {  # leaves per star; aggregate sizes in dofs are (L + 1) b
    "sub16": (0, 1, 7, 15, 3, 15, 9),                   # every aggregate <= 16 rows: 16 lanes per aggregate
    "sub32": (0, 16, 31, 4, 30),                        # <= 32 rows: 32 lanes per aggregate
    "wave": (0, 63, 64, LDS_ROWS - 1, LDS_ROWS, 299),   # 64 and 65 rows, the LDS-resident limit and one past it (b = 1)
}


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("b,k,mode", [(1, 1, "plain"), (1, 6, "plain"), (1, 6, "duplicate"), (1, 6, "zero"), (2, 3, "plain"), (2, 3, "duplicate"), (2, 3, "zero")])
@pytest.mark.parametrize("forest", sorted(FORESTS))
def test_aggregate_size_edges(smm, forest, b, k, mode, dtype):
    """a single-node aggregate (m = b, below k unless k = 1), 64 / 65 rows, LDS_ROWS and LDS_ROWS + 1 rows (b = 1; with b = 2 the stars
    of 128 and 129 nodes give 256 and 258), k = 1 and k = 6, a duplicated column and a column of zeros (beside others: k >= 2)"""
    def compute():
        leaves = FORESTS[forest]
        if forest == "wave" and b == 2:
            leaves = (0, 31, 32, LDS_ROWS // 2 - 1, LDS_ROWS // 2, 149)
        csr, B6 = star_forest(leaves, b, dtype)
        B = B6[:, :k].copy()
        if mode == "duplicate":
            B[:, k - 1] = B[:, 0]
        if mode == "zero":
            B[:, 1] = 0
        kw = {"theta": 0.02, "coarse_rows": 4, "max_levels": 2}
        ref = hierarchy(csr, B, b, **kw)
        sizes = np.bincount(ref[0]["agg"])
        assert sorted(sizes) == sorted((L + 1) * b for L in leaves), sizes
        return csr, B, kw, ref
    csr, B, kw, ref = cached(("forest", forest, b, k, mode, np.dtype(dtype).name), compute)
    assert len(ref) == 2
    if mode != "plain":
        assert ref[0]["dropped"] >= ref[0]["n_agg"]
    if k > b:
        assert ref[0]["dropped"] >= k - b  # the single node
    A, M = create(smm, csr, B, b, **kw)
    check_hierarchy(M, ref, csr, f"{forest} b={b} k={k} {mode}")


# ---- apply and the solvers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("e_16x16", "lone"))
def test_apply_bit_for_bit_at_one_lane_per_row(smm, oracle, name, dtype):
    csr, B, b, kw, _, _, r = reference(name, dtype)
    A, M = create(smm, csr, B, b, **kw)
    one_lane_per_row(smm, M)
    fn = make_apply(oracle, library_levels(M), M.amg_coarse_inverse())
    z = np.full(len(r), np.nan, dtype=dtype)
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(fn(r)))


def applied(oracle, name, dtype):
    def compute():
        _, _, _, _, ref, _, _ = reference(name, dtype)
        return make_apply(oracle, ref, coarse_inverse(ref[-1]["A"]))
    return cached(("apply", name, np.dtype(dtype).name), compute)


def restated(oracle, solver, name, dtype, it, eps):
    def compute():
        csr, _, _, _, _, b, _ = reference(name, dtype)
        fn = applied(oracle, name, dtype)
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
@pytest.mark.parametrize("solver", ("cg", "bicgstab", "gmres"))
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, dtype):
    name, it = "e_16x16", FIXED_STEPS
    csr, B, b, kw, _, rhs, _ = reference(name, dtype)
    st_ref, x_ref, it_ref, sens = restated(oracle, solver, name, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    A, M = create(smm, csr, B, b, **kw)
    st, x, info = run(smm, solver, A, rhs, it, 0.0, M, dtype)
    err = worst(x, x_ref)
    print(solver, name, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol, "sensitivity", sens, info)
    assert st == st_ref and info["iterations"] == it_ref == it
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_converged_cg(smm, oracle, dtype):
    """elasticity2d(32, 32), b = A 1: SUCCESS, the restated loop's count within max(2, ref // 5), fewer iterations than with
    candidates=None and than without a preconditioner.  Restated: 16 iterations to 1e-8 in fp64 (candidates=None: 44, none: 282)."""
    name = "e_32x32"
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr, B, b, kw, _, rhs, _ = reference(name, dtype)
    st_ref, _, it_ref, _ = restated(oracle, "cg", name, dtype, -1, eps)
    A, M = create(smm, csr, B, b, **kw)
    st, x, info = run(smm, "cg", A, rhs, -1, eps, M, dtype)
    st1, _, info1 = run(smm, "cg", A, rhs, -1, eps, A.getPreconditioner("AMG", **kw), dtype)
    st0, _, info0 = run(smm, "cg", A, rhs, -1, eps, None, dtype)
    print(name, np.dtype(dtype).name, "iterations", info["iterations"], "restated", it_ref, "candidates=None", info1["iterations"], "unpreconditioned",
          info0["iterations"], "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0 and st1 == 0 and st0 == 0
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5)
    assert info["iterations"] < info1["iterations"] < info0["iterations"]


# ---- refresh, the device-pointer form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ("e_16x16", "lone"))
def test_refresh_after_scaling_equals_a_fresh_create(smm, name, dtype):
    """A scaled by 2 on the device changes no strength decision; after amg_refresh every value equals that of a handle created on the
    scaled matrix, and the aggregates, T and every B_l still hold their first bits ("lone": the sum with E is redone as well)"""
    csr, B, b, kw, ref, _, r = reference(name, dtype)
    A, M = create(smm, csr, B, b, **kw)
    before = M.amg_info()
    first = [(M.amg_aggregates(l), triple(M.amg_candidates(l)["T"])) for l in range(before["levels"] - 1)]
    A.scale(2.0)
    M.amg_refresh()
    fresh = A.getPreconditioner("AMG", candidates=B, dofs_per_node=b, **kw)
    assert M.amg_info() == before == fresh.amg_info()
    for l in range(before["levels"]):
        for got, want in zip(M.amg_level(l), fresh.amg_level(l)):
            assert (got is None) == (want is None)
            if got is not None:
                assert_same_csr(triple(got), triple(want), f"level {l}")
        got, want = M.amg_candidates(l), fresh.amg_candidates(l)
        np.testing.assert_array_equal(bits(np.ascontiguousarray(got["B"])), bits(np.ascontiguousarray(want["B"])))
        np.testing.assert_array_equal(bits(np.ascontiguousarray(got["B"])), bits(np.ascontiguousarray(ref[l]["B"])))
        assert got["dropped"] == want["dropped"] == ref[l]["dropped"]
        if l + 1 < before["levels"]:
            np.testing.assert_array_equal(M.amg_aggregates(l), first[l][0])
            assert_same_csr(triple(got["T"]), first[l][1], f"T_{l} kept")
            assert_same_csr(triple(want["T"]), first[l][1], f"T_{l} fresh")
    np.testing.assert_array_equal(bits(M.amg_coarse_inverse()), bits(fresh.amg_coarse_inverse()))
    one_lane_per_row(smm, M)
    one_lane_per_row(smm, fresh)
    z, z2 = np.zeros(len(r), dtype=dtype), np.zeros(len(r), dtype=dtype)
    M.apply(r, z)
    fresh.apply(r, z2)
    np.testing.assert_array_equal(bits(z), bits(z2))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_device_pointers_on_offset_views(smm, dtype):
    name = "e_4x4x4"
    csr, B, b, kw, ref, _, _ = reference(name, dtype)
    n, k = B.shape
    held = carve_like(np.ascontiguousarray(B.T), fit(1, dtype), device="cuda:0")  # (k, n) contiguous: column-major n x k
    d_B = held.t()
    assert d_B.data_ptr() % 16 != 0 and tuple(d_B.shape) == (n, k) and tuple(d_B.stride()) == (1, n)
    saved = snapshot(held)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", candidates=d_B, dofs_per_node=b, stream=s.cuda_stream, **kw)
    torch.cuda.synchronize()
    check_hierarchy(M, ref, csr, "device pointers")
    assert_unchanged(held, saved, "B")
    assert_guards_intact(held, "B")
    with pytest.raises(TypeError):
        A.getPreconditioner("AMG", candidates=held.t().contiguous(), dofs_per_node=b)  # row-major on the device


# ---- refusals, the scalar path, the drop-in header ---------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals(smm, dtype):
    csr, B, b, kw, _, rhs, _ = reference("e_16x16", dtype)
    n = len(rhs)
    A = make(smm, csr)
    wide = np.ones((n, 7), dtype=dtype)
    assert code_of(lambda: A.getPreconditioner("AMG", candidates=wide, dofs_per_node=b)) == INVALID
    assert code_of(lambda: A.getPreconditioner("AMG", candidates=np.ones((n, 0), dtype=dtype), dofs_per_node=b)) == INVALID
    for bad in (0, 5, -1):
        assert code_of(lambda: A.getPreconditioner("AMG", candidates=B, dofs_per_node=bad)) == INVALID
    assert n % 3 != 0 and code_of(lambda: A.getPreconditioner("AMG", candidates=B, dofs_per_node=3)) == INVALID
    for poison in (np.nan, np.inf, -np.inf):
        Bp = B.copy()
        Bp[n // 2, 1] = poison
        assert code_of(lambda: A.getPreconditioner("AMG", candidates=Bp, dofs_per_node=b)) == INVALID
        d = torch.from_numpy(np.ascontiguousarray(Bp.T)).cuda().t()
        assert code_of(lambda: A.getPreconditioner("AMG", candidates=d, dofs_per_node=b)) == INVALID
    assert code_of(lambda: A.getPreconditioner("AMG", candidates=B, dofs_per_node=b, theta=1.0)) == INVALID
    assert code_of(lambda: A.getPreconditioner("AMG", candidates=B, dofs_per_node=b, max_levels=0)) == INVALID
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
    assert code_of(lambda: W.getPreconditioner("AMG", candidates=np.ones((2, 1), dtype=dtype))) == INVALID
    with pytest.raises(ValueError):
        A.getPreconditioner("AMG", candidates=B[:-1], dofs_per_node=b)
    plain = A.getPreconditioner("AMG", **kw)
    assert code_of(lambda: plain.amg_candidates(0)) == INVALID  # created without candidates
    # a column that is zero everywhere is dropped on every aggregate, not refused; CG still converges
    Bz = B.copy()
    Bz[:, 2] = 0
    M = A.getPreconditioner("AMG", candidates=Bz, dofs_per_node=b, **kw)
    info = M.amg_info()
    assert M.amg_candidates(0)["dropped"] == info["rows"][1] // 3
    x = np.zeros(n, dtype=dtype)
    assert int(smm.ConjugateGradient(A, rhs, np.zeros(n, dtype=dtype), x, -1, 1e-8 if dtype == np.float64 else 1e-3, M)) == 0
    if dtype == np.float64:
        np.testing.assert_allclose(x, 1.0, rtol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_candidates_none_is_todays_path(smm, dtype):
    csr = gen_matrices(dtype)["poisson2d_32"]
    ref = scalar_hierarchy(csr)
    A = make(smm, csr)
    M, plain = A.getPreconditioner("AMG", candidates=None), A.getPreconditioner("AMG")
    assert M.amg_info() == plain.amg_info() and M.amg_info()["levels"] == len(ref) >= 2
    for l in range(len(ref)):
        for got, want in zip(M.amg_level(l), plain.amg_level(l)):
            assert (got is None) == (want is None)
            if got is not None:
                assert_same_csr(triple(got), triple(want), f"level {l}")
        if l + 1 < len(ref):
            np.testing.assert_array_equal(M.amg_aggregates(l), ref[l]["agg"])
    np.testing.assert_array_equal(bits(M.amg_coarse_inverse()), bits(plain.amg_coarse_inverse()))


def test_cpp_dropin_case_on_the_gpu(tmp_path):
    """tests/cpp/amg_candidates_case.cpp on elasticity2d(16, 16) with the rigid body modes, fp64: SUCCESS, x = 1, three levels"""
    eps = 1e-10
    csr, B, b, _, ref, _, _ = reference("e_16x16", np.float64)
    start, pos, val = csr
    rows = len(start) - 1
    with open(tmp_path / "matrix.txt", "w") as f:
        f.write(f"{rows} {len(pos)}\n")
        for r in range(rows):
            for k in range(start[r], start[r + 1]):
                f.write(f"{r} {int(pos[k])} {float(val[k])!r}\n")
    with open(tmp_path / "candidates.txt", "w") as f:
        f.write(f"{rows} {B.shape[1]}\n")
        for row in B:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path / "matrix.txt"), str(tmp_path / "candidates.txt"), str(b), repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "status 0 hip 0", lines[0] + r.stderr[-500:]
    assert lines[1] == f"levels {len(ref)} k 3 dropped 0"
    x = np.array([float.fromhex(ln.split()[1]) for ln in lines[2:]])
    assert len(x) == rows
    np.testing.assert_allclose(x, 1.0, rtol=1e-6)
