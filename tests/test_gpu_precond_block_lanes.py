"""BLOCK_ILU0 / BLOCK_SGS under BiCGStab at every lanes-per-row setting of the matrix.

x = M^-1 (A v) has two forms (csrc/smm_precond_block.hip).  ONE launch (blockApplySpmvDev) sums each row of A v as one chain from 0 in
stored order; TWO launches (launchSpmv, then blockApplyDev) sum it in the matrix's configured order: the kernel family and the L pieces
per row of set_kernel, or AUTO's choice.  The two agree bit for bit only at one lane per row, and which one a solve takes is decided per
call (blockFuseSpmv: the block count against 4 x the device's CUs and the partials count, whether the PATTERN analysis has run on the
handle, SMM_HIP_BLOCK_FUSE_SPMV).  tests/test_gpu_precond_block.py pins one lane per row; here both forms run at 2, 4 and 16 lanes and on
AUTO's choice against a reference that depends on neither: A v in float64, rounded once, then the oracle's sequential sweeps on the matrix
M is built from; for the solves the restated BiCGStab of tests/chebyshev_restatement.py with those sweeps as M^-1.  Tolerances: the
fixed-pass rule of tests/test_gpu_cgs.py (allowed / worst) with the restatement's own sensitivity to a one-ulp change of its input;
converged runs by the rule of tests/test_gpu_batched_solvers.py.  Every case prints the kernel, the route and worst / allowed / sens.

b = A x_true with x_true uniform in [0.5, 1.5] (not the row sums: on banded_random_spd the all-ones vector is an eigenvector and the
loop would finish in its first pass).

Measured on an MI355X (256 CUs): AUTO gives banded (STREAM, 2) and every other matrix (STREAM, 1); many_blocks is poisson2d(257) in 1034
blocks (4 x CUs = 1024, partials 2048).  Largest worst / allowed: fp32 0.15 and fp64 0.10, both in test_first_and_later_solves_agree
(BLOCK_SGS after 20 passes); the applies and six-pass solves stay below 0.02.  At L > 1 the two forms do give different bits (104 of
the 120 apply cases)."""
import numpy as np
import pytest
import torch
from chebyshev_restatement import bicgstab, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from test_gpu_cgs import allowed, make, worst
from test_gpu_precond_block import CONTIGUOUS, permuted

from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
STREAM, VECTOR, PATTERN = 2, 1, 3  # smm.SPMV_STREAM, _VECTOR, _PATTERN (asserted in setting())
LANE_SETTINGS = [(STREAM, 2), (STREAM, 4), (VECTOR, 4), (VECTOR, 16), (PATTERN, 2), (0, 0)]  # (0, 0): AUTO
KINDS = ["BLOCK_ILU0", "BLOCK_SGS"]
FIXED_PASSES = 6
BLOCK_ROWS_MIN = 64  # the smallest block_rows a create accepts
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

# name -> (generator, block_rows, partition).  many_blocks is built for the device at hand (many_blocks_side).
MATRICES = {
    "banded": (lambda dt: gen.banded_random_spd(4000, k=12, seed=11, max_offset=90, dtype=dt), None, None),  # 25-entry rows: the tail loop
    "convdiff3d_bricks": (lambda dt: gen.convdiff3d(24, 0.3, dtype=dt), None, None),
    "convdiff3d_rows64": (lambda dt: gen.convdiff3d(24, 0.3, dtype=dt), 64, CONTIGUOUS),
    "ragged": (lambda dt: gen.random_rows(900, 900, 2, 25, seed=9, dtype=dt, diag_dominant=True), 300, None),  # rows shorter than the lane count
    "many_blocks": (lambda dt: gen.poisson2d(many_blocks_side(), dtype=dt), BLOCK_ROWS_MIN, CONTIGUOUS),
}

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


def many_blocks_side():
    """the smallest N at which poisson2d(N) in contiguous blocks of 64 rows -- the smallest a create accepts -- has more than 4 x CUs
    blocks: the one launch is then not taken by the automatic rule (the matrix stays outside the PATTERN family)"""
    n = 1
    while -(-n * n // BLOCK_ROWS_MIN) <= 4 * compute_units():
        n += 1
    return n


def skip_unless_many_blocks_fit(name):
    """no block size gives more than 4 x CUs and at most partials_count() blocks when 4 x CUs is the larger number"""
    if name == "many_blocks" and 4 * compute_units() >= host.partials_count():
        pytest.skip(f"no block count lies above 4 x CUs = {4 * compute_units()} and within partials_count() = {host.partials_count()}")


def case(name, dtype):
    """(csr, x_true, b = A x_true in float64 rounded once, v, A v in float64 rounded once)"""
    def compute():
        csr = MATRICES[name][0](dtype)
        start, pos, val = csr
        n = len(start) - 1
        rowof = np.repeat(np.arange(n), np.diff(start))
        mul = lambda x: np.bincount(rowof, weights=val.astype(np.float64) * x.astype(np.float64)[pos], minlength=n).astype(dtype)  # noqa: E731
        rng = np.random.default_rng(17)
        x_true = rng.uniform(0.5, 1.5, n).astype(dtype)
        v = rng.uniform(-1, 1, n).astype(dtype)
        return csr, x_true, mul(x_true), v, mul(v)
    return cached(("case", name, np.dtype(dtype).name), compute)


def setting(smm, name, dtype, family, lanes):
    """a fresh handle set to (family, lanes) -- (0, 0): left on AUTO -- so that no case inherits a PATTERN analysis from another"""
    assert (smm.SPMV_STREAM, smm.SPMV_VECTOR, smm.SPMV_PATTERN) == (STREAM, VECTOR, PATTERN)
    A = make(smm, case(name, dtype)[0])
    if (family, lanes) != (0, 0):
        A.set_kernel(family, lanes)
        assert A.get_kernel() == (family, lanes)
    return A


def precond(smm, A, name, kind):
    _, block_rows, partition = MATRICES[name]
    return A.getPreconditioner(getattr(smm.SolverPreconditioner, kind), block_rows, None, partition)


def block_inverse(oracle, smm, name, dtype, kind, M):
    """M^-1 as a function of one vector, restated: the oracle's sequential sweeps on the matrix M is built from, in the order of M's
    partition.  Computed once per (matrix, dtype, kind); every later handle must report the same partition."""
    bounds, order, cap = M.block_bounds(), M.block_rows()[0], M.level_cap()

    def compute():
        csr = case(name, dtype)[0]
        mcsr = oracle.level_cut_matrix(permuted(csr, order)[0], bounds, cap)[0]
        lu = oracle.block_ilu0_factorize(mcsr, bounds)[1] if kind == "BLOCK_ILU0" else None

        def fn(r):
            rp = np.ascontiguousarray(r[order])
            z = oracle.block_ilu0_apply(mcsr, bounds, lu, rp)[1] if kind == "BLOCK_ILU0" else oracle.block_sgs_apply(mcsr, bounds, rp)[1]
            out = np.empty_like(z)
            out[order] = z
            return out
        return bounds, order, cap, fn
    b0, o0, c0, fn = cached(("inverse", name, np.dtype(dtype).name, kind), compute)
    assert np.array_equal(b0, bounds) and np.array_equal(o0, order) and c0 == cap
    return fn


def restated_apply(oracle, name, dtype, kind, fn):
    """(x = M^-1 (A v), its sensitivity to a one-ulp change of A v)"""
    def compute():
        av = case(name, dtype)[4]
        ref = fn(av)
        return ref, sensitivity(fn, av, ref)
    return cached(("apply", name, np.dtype(dtype).name, kind), compute)


def restated_solve(oracle, name, dtype, kind, fn, it, eps):
    """(status, x, iterations, sensitivity of x to a one-ulp change of b) of the restated loop from x0 = 0"""
    def compute():
        csr, _, b = case(name, dtype)[:3]
        solve = lambda bb: bicgstab(oracle, csr, bb, np.zeros(len(b), dtype=dtype), it, eps, fn)  # noqa: E731
        st, x, k, _ = solve(b)
        return st, x, k, sensitivity(lambda bb: solve(bb)[1], b, x)
    return cached(("solve", name, np.dtype(dtype).name, kind, it, eps), compute)


def solve(smm, A, M, b, it, eps, dtype):
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.BiCGStab(A, b.copy(), x, it, dtype(eps), M, info=info)
    return int(st), info["iterations"], x


def in_mask_form(A):
    """the PATTERN analysis has run on the handle and found the row-mask encoding: the one launch is then always taken"""
    return A.pattern_info()[0] in (1, 3)


def automatic_route(A, M):
    """what blockFuseSpmv(M, false) decides without the environment switch, from what the handle reports AFTER the solve (the solver
    readies the matrix before it asks)"""
    blocks = len(M.block_bounds()) - 1
    return "fused" if blocks <= host.partials_count() and (in_mask_form(A) or blocks <= 4 * compute_units()) else "unfused"


def true_residual(csr, b, x):
    start, pos, val = csr
    n = len(start) - 1
    ax = np.bincount(np.repeat(np.arange(n), np.diff(start)), weights=val.astype(np.float64) * x.astype(np.float64)[pos], minlength=n)
    return float(np.linalg.norm(b.astype(np.float64) - ax))


def test_the_many_blocks_matrix_takes_two_launches_by_the_automatic_rule(smm):
    """more blocks than 4 x CUs, no more than the partials count, and the matrix outside the PATTERN family: blkMaskForm is false"""
    skip_unless_many_blocks_fit("many_blocks")
    A = setting(smm, "many_blocks", np.float64, STREAM, 2)
    M = precond(smm, A, "many_blocks", "BLOCK_ILU0")
    blocks = len(M.block_bounds()) - 1
    print("many_blocks: poisson2d side", many_blocks_side(), "rows", A.rows, "blocks", blocks, "4 x CUs", 4 * compute_units(), "partials", host.partials_count())
    assert blocks > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert blocks <= smm.host.partials_count()
    assert not in_mask_form(A) and automatic_route(A, M) == "unfused"


def test_auto_resolves_to_more_than_one_lane_on_some_matrix(smm):
    """otherwise the AUTO leg of every test below repeats the one-lane tests of tests/test_gpu_precond_block.py"""
    chosen = {}
    for name in MATRICES:
        if name == "many_blocks" and 4 * compute_units() >= host.partials_count():
            continue
        A = setting(smm, name, np.float64, 0, 0)
        v = case(name, np.float64)[3]
        A.rMult(v, np.zeros_like(v))
        chosen[name] = A.get_kernel()
    print("AUTO:", chosen)
    assert any(lanes > 1 for _, lanes in chosen.values()), chosen


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", list(MATRICES))
def test_apply_spmv_at_every_lane_setting(smm, oracle, name, dtype):
    """M.apply_spmv(v, x) within `allowed` of the restated x at every setting, the same bits on a second call, and the bits of
    M.apply(A.rMult(v)) where -- and only where that is claimed -- the matrix runs one lane per row"""
    skip_unless_many_blocks_fit(name)
    v = case(name, dtype)[3]
    for family, lanes in LANE_SETTINGS:
        A = setting(smm, name, dtype, family, lanes)
        for kind in KINDS:
            M = precond(smm, A, name, kind)
            ref, sens = restated_apply(oracle, name, dtype, kind, block_inverse(oracle, smm, name, dtype, kind, M))
            tol = allowed(ref, sens, dtype)
            x, again, av, two = (np.full(len(v), np.nan, dtype=dtype) for _ in range(4))
            assert M.apply_spmv(v, x) == 0 and M.apply_spmv(v, again) == 0
            A.rMult(v, av)
            assert M.apply(av, two) == 0
            kernel = A.get_kernel()
            err, err_two = worst(x, ref), worst(two, ref)
            same = np.array_equal(bits(x), bits(two))
            print(name, np.dtype(dtype).name, kind, "set", (family, lanes), "kernel", kernel, "pattern", A.pattern_info(), "one launch: worst", err,
                  "two launches: worst", err_two, "allowed", tol, "sens", sens, "same bits" if same else "different bits")
            assert err <= tol and err_two <= tol
            np.testing.assert_array_equal(bits(x), bits(again))
            if kernel[1] == 1:
                np.testing.assert_array_equal(bits(x), bits(two))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", list(MATRICES))
def test_bicgstab_routes_agree_with_the_restated_loop(smm, oracle, name, dtype, monkeypatch):
    """six fixed passes with SMM_HIP_BLOCK_FUSE_SPMV=1 and =0 (read per solve): the restated loop's status and pass count, x within
    `allowed` of its x on either route, and the same bits on both where the matrix runs one lane per row"""
    skip_unless_many_blocks_fit(name)
    b = case(name, dtype)[2]
    for family, lanes in LANE_SETTINGS:
        A = setting(smm, name, dtype, family, lanes)
        for kind in KINDS:
            M = precond(smm, A, name, kind)
            st_ref, x_ref, it_ref, sens = restated_solve(oracle, name, dtype, kind, block_inverse(oracle, smm, name, dtype, kind, M), FIXED_PASSES, 1e-30)
            tol = allowed(x_ref, sens, dtype)
            got = {}
            for route, fuse in (("fused", "1"), ("unfused", "0")):
                monkeypatch.setenv("SMM_HIP_BLOCK_FUSE_SPMV", fuse)
                got[route] = solve(smm, A, M, b, FIXED_PASSES, 1e-30, dtype)
            monkeypatch.delenv("SMM_HIP_BLOCK_FUSE_SPMV", raising=False)
            kernel = A.get_kernel()
            for route, (st, it, x) in got.items():
                err = worst(x, x_ref)
                print(name, np.dtype(dtype).name, kind, "set", (family, lanes), "kernel", kernel, "route", route, "worst", err, "allowed", tol, "sens", sens)
                assert st == st_ref and it == it_ref == FIXED_PASSES
                assert err <= tol
            if kernel[1] == 1:
                np.testing.assert_array_equal(bits(got["fused"][2]), bits(got["unfused"][2]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ["banded", "convdiff3d_bricks", "convdiff3d_rows64", "many_blocks"])
def test_converged_runs_do_not_depend_on_the_route(smm, name, dtype, monkeypatch):
    """maxIterations = -1, eps = 1e-8 (fp64) / 1e-3 (fp32), on AUTO and at (STREAM, 2); fused, unfused and with the switch unset -- the
    automatic rule, which on many_blocks takes the two launches.  Every run ends with SUCCESS; the pass counts of every pair differ by
    at most max(2, it // 5), it being the smaller of the two; the true residual |b - A x|_2, formed in float64, is at most 10 * eps.
    That rule applied in both dtypes: no fp32 run needed the eps / sigma_min bound of tests/test_gpu_ainv.py::test_converged_runs.
    The unset run gives the bits of the route the rule predicts.
    Measured on an MI355X: the largest |b - A x| is 6.3e-3 in fp32 and 7.6e-8 in fp64 (banded, BLOCK_SGS, every route); the pass counts
    agree to one pass everywhere but on many_blocks fp64 at (STREAM, 2): BLOCK_ILU0 405 fused / 353 unfused (allowed 70), BLOCK_SGS
    408 / 399."""
    skip_unless_many_blocks_fit(name)
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr, _, b = case(name, dtype)[:3]
    for family, lanes in ((0, 0), (STREAM, 2)):
        A = setting(smm, name, dtype, family, lanes)
        for kind in KINDS:
            M = precond(smm, A, name, kind)
            got = {}
            for route, fuse in (("fused", "1"), ("unfused", "0"), ("automatic", None)):
                if fuse is None:
                    monkeypatch.delenv("SMM_HIP_BLOCK_FUSE_SPMV", raising=False)
                else:
                    monkeypatch.setenv("SMM_HIP_BLOCK_FUSE_SPMV", fuse)
                got[route] = solve(smm, A, M, b, -1, eps, dtype)
            predicted = automatic_route(A, M)
            kernel = A.get_kernel()
            for route, (st, it, x) in got.items():
                res = true_residual(csr, b, x)
                print(name, np.dtype(dtype).name, kind, "set", (family, lanes), "kernel", kernel, "route", route + (" = " + predicted if route == "automatic" else ""),
                      "status", st, "passes", it, "|b - A x|", res, "bound", 10 * eps)
                assert st == 0
                assert res <= 10 * eps
            routes = list(got)
            for i, first in enumerate(routes):
                for second in routes[i + 1:]:
                    it1, it2 = got[first][1], got[second][1]
                    assert abs(it1 - it2) <= max(2, min(it1, it2) // 5), (first, it1, second, it2)
            if name == "many_blocks":
                assert predicted == "unfused"
            assert got["automatic"][1] == got[predicted][1]
            np.testing.assert_array_equal(bits(got["automatic"][2]), bits(got[predicted][2]))


# convdiff3d_rows64 (an addition: with bricks the create itself runs the PATTERN analysis, with contiguous rows the first solve finds the
# handle not analysed) in fp64 only: in fp32 the restated loop after 20 passes with these weaker blocks is still far from converged
# (|r| = 0.65) and its own x moves by 3.3e-2 under a one-ulp change of b (max|x| = 1.8; measured on the CPU alone), beyond what `allowed`
# accepts from a reference.
FIRST_AND_LATER = [("convdiff3d_bricks", np.float32), ("convdiff3d_bricks", np.float64), ("convdiff3d_rows64", np.float64)]


@pytest.mark.parametrize("name,dtype", FIRST_AND_LATER, ids=ids)
def test_first_and_later_solves_agree(smm, oracle, name, dtype):
    """a fresh AUTO handle and its block preconditioner: two solves back to back with maxIterations = 20 (eps = 1e-30: every pass runs),
    then the PATTERN analysis forced with set_kernel(PATTERN, 0) and a third -- the same status and pass count, each x within `allowed`
    of the restated loop.  With bricks the create has already run the analysis; with contiguous rows the first two solves find the
    handle not analysed and the third finds the row masks."""
    it = 20
    b = case(name, dtype)[2]
    for kind in KINDS:
        A = setting(smm, name, dtype, 0, 0)
        M = precond(smm, A, name, kind)
        st_ref, x_ref, it_ref, sens = restated_solve(oracle, name, dtype, kind, block_inverse(oracle, smm, name, dtype, kind, M), it, 1e-30)
        tol = allowed(x_ref, sens, dtype)
        got = []
        for call in ("first", "second", "after the analysis"):
            if call == "after the analysis":
                A.set_kernel(smm.SPMV_PATTERN, 0)
            before = (A.get_kernel(), A.pattern_info())
            st, k, x = solve(smm, A, M, b, it, 1e-30, dtype)
            err = worst(x, x_ref)
            print(name, np.dtype(dtype).name, kind, call, "kernel, pattern before", before, "route", automatic_route(A, M), "status", st, "passes", k,
                  "worst", err, "allowed", tol, "sens", sens)
            got.append((st, k))
            assert err <= tol
        assert in_mask_form(A)
        assert got[0] == got[1] == got[2] == (st_ref, it_ref) and it_ref == it


@pytest.mark.parametrize("kind", KINDS)
def test_device_entry_point_on_a_side_stream(smm, oracle, kind):
    """smm_hip_bicgstab_dev_f64 with the block preconditioner on a stream of the caller's, the matrix at (STREAM, 2), b and x views at
    element alignment inside larger buffers with guard bands; then take_error on that stream"""
    name, dtype = "banded", np.float64
    b = case(name, dtype)[2]
    A = setting(smm, name, dtype, STREAM, 2)
    M = precond(smm, A, name, kind)
    st_ref, x_ref, it_ref, sens = restated_solve(oracle, name, dtype, kind, block_inverse(oracle, smm, name, dtype, kind, M), FIXED_PASSES, 1e-30)
    tol = allowed(x_ref, sens, dtype)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(len(b), dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 != 0 and d_x.data_ptr() % 16 != 0
    saved = snapshot(d_b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    st, k, _ = host.bicgstab_dev(A, d_b, d_x, FIXED_PASSES, 1e-30, M, s.cuda_stream)
    M.take_error(s.cuda_stream)
    torch.cuda.synchronize()
    err = worst(d_x.cpu().numpy(), x_ref)
    print(name, kind, "kernel", A.get_kernel(), "route", automatic_route(A, M), "worst", err, "allowed", tol, "sens", sens)
    assert int(st) == st_ref and k == it_ref == FIXED_PASSES
    assert err <= tol
    assert_unchanged(d_b, saved, "b")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")
