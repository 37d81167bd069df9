"""Several host threads on shared handles: four threads, released together, each with ITS OWN right-hand side, solve on one matrix
(and one preconditioner, transpose, fp32 copy) at the same time.  A buffer two of them share by mistake then holds visibly foreign
data.  Every result is compared (1) with the CPU reference of that solve at the tolerance the solver's own GPU test uses and (2) bit
for bit with the same call made alone (a repeated solve is deterministic: test_frozen_loop_and_determinism, the "fresh handle"
equalities of tests/test_gpu_csr_update.py).  A round counts only if the four solves overlapped in time; up to ROUNDS rounds are run
and every round is checked, counted or not.

The iteration count is fixed (eps = 1e-30).  Unpreconditioned loops run IT = 36 iterations: the count between 30 and 40 at which
the restated fp32 ConjugateGradientSquared passes the conditioning assertion of test_gpu_cgs.allowed for all four right-hand sides
(at 32 one of them moves by 0.05 when b moves by one unit in the last place).  Under a preconditioner the loops converge in far
fewer steps and then divide rounding noise by rounding noise, which no tolerance can follow: PRECOND_IT = 12, at which every restated
loop used here moves by less than 1e-4 of max|x| under that perturbation.  Both are properties of the CPU restatements alone."""
import threading
import time

import numpy as np
import pytest
from ainv_restatement import FSAI, SPAI
from ainv_restatement import make_apply as ainv_apply
from amg_restatement import coarse_inverse, hierarchy
from amg_restatement import make_apply as amg_apply
from bicg_restatement import bicg
from bicg_restatement import transpose as csr_transpose
from cgs_restatement import cgs
from chebyshev_restatement import bicgstab as restated_bicgstab
from chebyshev_restatement import gershgorin, pcg, sensitivity
from chebyshev_restatement import make_apply as cheb_apply
from gmres_helpers import permuted
from gmres_restatement import gmres
from multicolor_restatement import make_apply as mc_apply
from refine_restatement import refine, rounded
from test_gpu_cgs import allowed, worst
from test_gpu_solvers import RTOL

from sparse_matrix_math_amd import generators as gen

gpu = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
THREADS, ROUNDS = 4, 5
IT, PRECOND_IT, EPS = 36, 12, 1e-30
RESTART = 10
K = 3  # right-hand sides of the batched solvers and of SpMM
AMG_COARSE_ROWS = 64  # 2304 -> ... : at least two levels (asserted)
REFINE_EPS, REFINE_INNER_EPS = 1e-10, 1e-4  # tests/test_gpu_refine.py
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the barrier scheme -----------------------------------------------------------------------------------------------------------
def overlapping(windows):
    """every pair of (begin, end) windows overlaps: the last to begin began before the first to end ended"""
    return max(w[0] for w in windows) < min(w[1] for w in windows)


def concurrently(work, threads=THREADS, rounds=ROUNDS):
    """work(i) in `threads` threads released together, round after round until the windows of one round pairwise overlap.  Returns the
    results of every round run (each is to be checked); fails if no round counted or a thread raised."""
    out = []
    for _ in range(rounds):
        gate = threading.Barrier(threads)
        results, windows, errors = [None] * threads, [None] * threads, []

        def body(i):
            try:
                gate.wait()
                begin = time.perf_counter()
                results[i] = work(i)
                windows[i] = (begin, time.perf_counter())
            except Exception as e:  # noqa: BLE001
                errors.append((i, e))

        pool = [threading.Thread(target=body, args=(i,)) for i in range(threads)]
        for t in pool:
            t.start()
        for t in pool:
            t.join()
        assert not errors, errors
        out.append(results)
        if overlapping(windows):
            print("rounds run", len(out), "windows of the counted round (ms)", [(round(1e3 * (a - windows[0][0]), 2), round(1e3 * (b - windows[0][0]), 2)) for a, b in windows])
            return out
    raise AssertionError(f"no round of {rounds} had {threads} solves overlapping in time: the test cannot say anything")


def test_the_barrier_scheme_overlaps_on_the_first_round():
    """no GPU: the library call stubbed by a sleep of the order of one small solve"""
    assert overlapping([(0, 3), (1, 4), (2, 5)]) and not overlapping([(0, 1), (1, 2), (0, 2)])
    rounds = concurrently(lambda i: (time.sleep(0.02), i)[1])
    assert rounds == [[0, 1, 2, 3]]


# ---- matrices, right-hand sides ---------------------------------------------------------------------------------------------------
def matrix(which, dtype):
    """'spd': gen.poisson2d(48, 48), 2304 rows; 'gen': gen.convdiff3d_varying(14), 2744 rows, non-symmetric"""
    return cached(("matrix", which, np.dtype(dtype).name), lambda: gen.poisson2d(48, 48, dtype=dtype) if which == "spd" else gen.convdiff3d_varying(14, dtype=dtype))


def rhs(n, dtype, i, k=None):
    """thread i's own right-hand side(s)"""
    return np.random.default_rng(i).uniform(-1, 1, n if k is None else (n, k)).astype(dtype)


def make(smm, csr, kernel=None):
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    if kernel is not None:
        A.set_kernel(*kernel)
    return A


# ---- the solvers: the call on the GPU, the same solve on the CPU, the comparison -------------------------------------------------
class Solver:
    """which: the matrix it runs on; gpu(smm, H, b, M, it) -> (status, iterations, x); cpu(oracle, H, b, apply, it) -> (status,
    iterations, x); rule: 'close' (RTOL alone, test_gpu_solvers.close), 'bicgstab' (RTOL or 4 x sensitivity,
    test_gpu_solvers.test_fixed_iterations_match_reference) or 'allowed' (test_gpu_cgs.allowed)"""

    def __init__(self, which, gpu, cpu, rule, batched=False, dtypes=DTYPES):
        self.which, self.gpu, self.cpu, self.rule, self.batched, self.dtypes = which, gpu, cpu, rule, batched, dtypes


def _zeros(b):
    return np.zeros_like(b)


def gpu_cg(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.ConjugateGradient(H["A"], b, _zeros(b), x, it, EPS, M, info=info)
    return int(st), info["iterations"], x


def cpu_cg(oracle, H, b, apply, it):
    st, x, k, _ = oracle.cg(H["csr"], b, _zeros(b), it, EPS) if apply is None else pcg(oracle, H["csr"], b, _zeros(b), it, EPS, apply)
    return int(st), k, x


def gpu_bicgstab(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.BiCGStab(H["A"], b.copy(), x, it, EPS, M, info=info)
    return int(st), info["iterations"], x


def cpu_bicgstab(oracle, H, b, apply, it):
    st, x, k, _ = oracle.bicgstab(H["csr"], b, _zeros(b), it, EPS) if apply is None else restated_bicgstab(oracle, H["csr"], b, _zeros(b), it, EPS, apply)
    return int(st), k, x


def gpu_gmres(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.GMRES(H["A"], b.copy(), x, it, EPS, RESTART, M, info=info)
    return int(st), info["iterations"], x


def cpu_gmres(oracle, H, b, apply, it):
    st, x, k, _ = gmres(oracle, H["csr"], b, _zeros(b), it, EPS, RESTART, apply)
    return int(st), k, x


def gpu_cgs(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.ConjugateGradientSquared(H["A"], b.copy(), x, it, EPS, info=info)
    return int(st), info["iterations"], x


def cpu_cgs(oracle, H, b, apply, it):
    st, x, k, _ = cgs(oracle, H["csr"], b, _zeros(b), it, EPS)
    return int(st), k, x


def gpu_bicg(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.BiCG(H["A"], b.copy(), x, it, EPS, at=H["At"], info=info)
    return int(st), info["iterations"], x


def cpu_bicg(oracle, H, b, apply, it):
    st, x, k, _ = bicg(oracle, H["csr"], H["csr_t"], b, _zeros(b), it, EPS)
    return int(st), k, x


def gpu_bicgstab_batch(smm, H, B, M, it):
    X, info = _zeros(B), {}
    sts = smm.BiCGStabBatch(H["A"], B.copy(), X, it, EPS, M, info=info)
    return tuple(int(s) for s in sts), tuple(int(v) for v in info["iterations"]), X


def gpu_cg_batch(smm, H, B, M, it):
    X, info = _zeros(B), {}
    sts = smm.ConjugateGradientBatch(H["A"], B, _zeros(B), X, it, EPS, info=info)
    return tuple(int(s) for s in sts), tuple(int(v) for v in info["iterations"]), X


def gpu_refine(smm, H, b, M, it):
    x, info = _zeros(b), {}
    st = smm.IterativeRefinement(H["A"], b.copy(), x, REFINE_EPS, inner="CG", a32=H["A32"], innerEps=REFINE_INNER_EPS, info=info)
    return int(st), (info["outer_iterations"], info["inner_iterations"]), x


SOLVERS = {
    "cg": Solver("spd", gpu_cg, cpu_cg, "close"),
    "cg_resident": Solver("spd", gpu_cg, cpu_cg, "close"),
    "bicgstab_mode0": Solver("gen", gpu_bicgstab, cpu_bicgstab, "bicgstab"),
    "bicgstab_mode2": Solver("gen", gpu_bicgstab, cpu_bicgstab, "bicgstab"),
    "gmres": Solver("gen", gpu_gmres, cpu_gmres, "allowed"),
    "cgs": Solver("gen", gpu_cgs, cpu_cgs, "allowed"),
    "bicg": Solver("gen", gpu_bicg, cpu_bicg, "allowed"),
    "bicgstab_batch": Solver("gen", gpu_bicgstab_batch, cpu_bicgstab, "bicgstab", batched=True),
    "cg_batch": Solver("spd", gpu_cg_batch, cpu_cg, "close", batched=True),
    "refine": Solver("spd", gpu_refine, None, "refine", dtypes=[np.float64]),
}
PATTERN_ONE_LANE = "PATTERN, 1"


class modes:
    """the two process-wide switches of the single-launch loops, put back on the way out"""

    def __init__(self, smm, names):
        self.smm, self.names = smm, names

    def __enter__(self):
        host = self.smm.host
        self.before = (host.cg_resident(-1), host.bicgstab_resident(-1))
        if "cg_resident" in self.names:  # REQUIRE: under AUTO a refusal or a barrier time-out would fall back to the three-launch loop quietly
            host.cg_resident(host.CG_RESIDENT_REQUIRE)
        elif "cg" in self.names:
            host.cg_resident(host.CG_RESIDENT_OFF)
        if "bicgstab_mode2" in self.names:
            host.bicgstab_resident(host.CG_RESIDENT_REQUIRE)
        elif "bicgstab_mode0" in self.names:
            host.bicgstab_resident(host.CG_RESIDENT_OFF)

    def __exit__(self, *exc):
        self.smm.host.cg_resident(self.before[0])
        self.smm.host.bicgstab_resident(self.before[1])


def handles(smm, which, dtype, kernel=PATTERN_ONE_LANE, extras=()):
    """the shared handles of one case: the matrix and, on request, its transpose and its fp32 copy"""
    csr = matrix(which, dtype)
    if kernel == PATTERN_ONE_LANE:
        kernel = (smm.SPMV_PATTERN, 1)
    H = {"csr": csr, "A": make(smm, csr, kernel)}
    if "At" in extras:
        H["csr_t"] = cached(("transpose", which, np.dtype(dtype).name), lambda: csr_transpose(csr))
        H["At"] = H["A"].transpose()
        if kernel is not None:
            H["At"].set_kernel(*kernel)
    if "A32" in extras:
        H["A32"] = H["A"].astype(np.float32)
    return H


def extras_of(names):
    return (("At",) if "bicg" in names else ()) + (("A32",) if "refine" in names else ())


def check_against_cpu(oracle, name, tag, H, b, got, apply, it, dtype):
    """assertion (1): thread's (status, iterations, x) against the CPU reference of that solve, made once per (case, right-hand side)"""
    S = SOLVERS[name]
    st, k, x = got
    if S.rule == "refine":
        from test_gpu_refine import true_residual

        csr = H["csr"]
        st_ref, x_ref, outer_ref, _, _ = cached(("cpu", tag), lambda: refine(oracle, csr, rounded(csr), b, _zeros(b), REFINE_EPS, "CG", 20, -1, REFINE_INNER_EPS, 30))
        smin = 4.0 - 4.0 * np.cos(np.pi / 49.0)  # the smallest eigenvalue of the 48 x 48 five-point Laplacian
        res, _ = true_residual(csr, b, x)
        err = float(np.linalg.norm(x - x_ref))
        print(tag, "outer", k[0], "restatement", outer_ref, "true residual", res, "|x - ref|", err, "bound", 2 * REFINE_EPS / smin)
        assert st == st_ref == 0 and abs(k[0] - outer_ref) <= 1  # the rules of tests/test_gpu_refine.py::check_solve
        assert res <= REFINE_EPS and err <= 2 * REFINE_EPS / smin
        return None
    columns = [(b, x, st, k)] if not S.batched else [(np.ascontiguousarray(b[:, j]), x[:, j], st[j], k[j]) for j in range(b.shape[1])]
    tols = []
    for j, (bj, xj, stj, kj) in enumerate(columns):
        def compute():
            st_ref, k_ref, x_ref = S.cpu(oracle, H, bj, apply, it)
            sens = None if S.rule == "close" else sensitivity(lambda bb: S.cpu(oracle, H, bb, apply, it)[2], bj, x_ref)
            return st_ref, k_ref, x_ref, sens

        st_ref, k_ref, x_ref, sens = cached(("cpu", tag, j), compute)
        scale = max(1.0, float(np.max(np.abs(x_ref))))
        tol = RTOL[dtype] * scale if S.rule == "close" else max(RTOL[dtype] * scale, 4 * sens) if S.rule == "bicgstab" else allowed(x_ref, sens, dtype)
        err = worst(xj, x_ref)
        print(tag, "column", j, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
        assert (stj, kj) == (st_ref, k_ref) and kj == it, (tag, j, stj, kj, st_ref, k_ref)
        assert err <= tol, (tag, j, err, tol)
        tols.append(tol)
    return tols


def check_against_solo(tag, got, alone, tols=None):
    """assertion (2): bit for bit what the same call gave alone; tols: per column, where the sums may legitimately differ"""
    assert got[0] == alone[0] and got[1] == alone[1], (tag, got[:2], alone[:2])
    if tols is not None:
        for j, tol in enumerate(tols):
            assert worst(got[2][:, j], alone[2][:, j]) <= tol, (tag, j, tol)
        return
    np.testing.assert_array_equal(bits(got[2]), bits(alone[2]), err_msg=f"{tag}: differs from the same solve made alone")


def run_case(smm, oracle, names, H, dtype, tag, M=None, apply=None, it=IT, solo_H=None, stream_table=False):
    """thread i runs solver names[i] on its own right-hand side; solo_H: other handles for the solves made alone (a fresh-handle case
    must not warm the shared ones); stream_table: the fresh handles' SpMVs build the STREAM family's tile table"""
    n = len(H["csr"][0]) - 1
    B = [rhs(n, dtype, i, K if SOLVERS[names[i]].batched else None) for i in range(THREADS)]
    with modes(smm, [s.split("@")[0] for s in names]):
        alone = [SOLVERS[names[i]].gpu(smm, solo_H or H, B[i], M, it) for i in range(THREADS)]
        rounds = concurrently(lambda i: SOLVERS[names[i]].gpu(smm, H, B[i], M, it))
    tols = {}
    for r, results in enumerate(rounds):
        for i, got in enumerate(results):
            tols[r, i] = check_against_cpu(oracle, names[i], f"{tag}/{names[i]}/{np.dtype(dtype).name}/rhs{i}", H, B[i], got, apply, it, dtype)
    for r, results in enumerate(rounds):
        for i, got in enumerate(results):
            # The batched solvers read the STREAM family's tile table "as it is" (tileTableFor, smm_spmm.hip): on a fresh handle its cut is
            # the first user's, the SpMM's own or an SpMV's, and the partial sums of the fused dot products follow the cut.  Which thread is
            # first is not determined, so there the comparison with the solve made alone is by the bound of the batched solvers' own test
            # (tests/test_gpu_batched_solvers.py: the one assertion (1) used); everywhere else it is bit for bit -- on a PATTERN handle too,
            # where no SpMV builds that table and the cut is always the SpMM's own.
            loose = solo_H is not None and stream_table and SOLVERS[names[i]].batched
            check_against_solo(f"{tag}/{names[i]}/thread {i}/round {r}", got, alone[i], tols[r, i] if loose else None)


# ---- case 1: every solver, unpreconditioned, warm handles ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,dtype", [(s, dt) for s in SOLVERS for dt in SOLVERS[s].dtypes], ids=ids)  # (the refinement solver is an fp64 entry point)
def test_every_solver_on_a_warm_shared_matrix(smm, oracle, name, dtype):
    S = SOLVERS[name]
    H = handles(smm, S.which, dtype, extras=extras_of([name]))
    run_case(smm, oracle, [name] * THREADS, H, dtype, "warm")


MIXED = {"spd": ["cg", "cg_batch", "bicgstab_mode0", "gmres"], "gen": ["bicgstab_mode2", "gmres", "cgs", "bicg"]}


def on(which, name):
    """solver `name` as it runs on matrix `which` (BiCGStab and GMRES take either matrix)"""
    S = SOLVERS[name]
    if S.which == which:
        return name
    alias = f"{name}@{which}"
    SOLVERS.setdefault(alias, Solver(which, S.gpu, S.cpu, S.rule, S.batched, S.dtypes))
    return alias


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("which", list(MIXED))
def test_four_different_solvers_on_one_matrix(smm, oracle, which, dtype):
    names = [on(which, s) for s in MIXED[which]]
    H = handles(smm, which, dtype, extras=extras_of(MIXED[which]))
    run_case(smm, oracle, names, H, dtype, "mixed")


# ---- case 2: first use inside the threads -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("kernel", ["AUTO", "PATTERN_1", "STREAM_4"])
@pytest.mark.parametrize("which", list(MIXED))
def test_first_use_of_a_fresh_matrix_inside_the_threads(smm, oracle, which, kernel, dtype):
    """the lazily built state (tile table, slot-major values of the single-launch form, SpMM tiles) is created under contention; the
    solves made alone run on a second set of handles"""
    kern = {"AUTO": None, "PATTERN_1": (smm.SPMV_PATTERN, 1), "STREAM_4": (smm.SPMV_STREAM, 4)}[kernel]
    # (the single-launch BiCGStab is required only where tests/test_gpu_csr_update.py requires it: PATTERN at one lane per row)
    plain = [("bicgstab_mode0" if s == "bicgstab_mode2" and kernel != "PATTERN_1" else s) for s in MIXED[which]]
    names = [on(which, s) for s in plain]
    solo_H = handles(smm, which, dtype, kern, extras_of(plain))
    H = handles(smm, which, dtype, kern, extras_of(plain))
    run_case(smm, oracle, names, H, dtype, "fresh/" + kernel, solo_H=solo_H, stream_table=kernel != "PATTERN_1")


# (bicgstab_mode2, the required single-launch form, at PATTERN 1 only; at the other settings it would be bicgstab_mode0 again)
FRESH = [(s, k, dt) for s in SOLVERS for k in ("AUTO", "PATTERN_1", "STREAM_4") for dt in SOLVERS[s].dtypes if s != "bicgstab_mode2" or k == "PATTERN_1"]


@gpu
@pytest.mark.parametrize("name,kernel,dtype", FRESH, ids=ids)
def test_first_use_by_four_threads_of_one_solver(smm, oracle, name, kernel, dtype):
    """case 1 on fresh handles: the four threads race for the same lazily built state -- the tile table, the slot-major values of
    the single-launch BiCGStab, the register-resident CG's first use, the SpMM tiles, the transpose's and the fp32 copy's tables"""
    kern = {"AUTO": None, "PATTERN_1": (smm.SPMV_PATTERN, 1), "STREAM_4": (smm.SPMV_STREAM, 4)}[kernel]
    S = SOLVERS[name]
    solo_H = handles(smm, S.which, dtype, kern, extras_of([name]))
    H = handles(smm, S.which, dtype, kern, extras_of([name]))
    run_case(smm, oracle, [name] * THREADS, H, dtype, "fresh/" + kernel, solo_H=solo_H, stream_table=kernel != "PATTERN_1")


# ---- case 3: one shared preconditioner handle --------------------------------------------------------------------------------------
SYMMETRIC_KINDS = ("IC0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "MULTICOLOR_IC0", "FSAI")
GENERAL_KINDS = ("JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS", "SPAI")
# tests/test_gpu_precond_kinds.py::TAKES, with FSAI and SPAI as tests/test_gpu_ainv.py shows them accepted
TAKES = {
    "cg": {"IC0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_IC0", "FSAI"},
    "bicgstab_mode0": {"JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "FSAI", "SPAI"},
    "gmres": {"JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "FSAI", "SPAI"},
    "bicgstab_batch": {"JACOBI"},
}
OFFERS = [(s, k) for s in TAKES for k in SYMMETRIC_KINDS + GENERAL_KINDS if k in TAKES[s]]


def enum_of(smm, kind):
    P = smm.SolverPreconditioner
    return P.SYMMETRIC_GAUS_SEIDEL if kind == "SGS" else P[kind]


def preconditioner(smm, oracle, A, csr, kind):
    """(the library's handle, M^-1 on the CPU as the kind's own test restates it)"""
    dtype = csr[2].dtype
    if kind == "AMG":
        M = A.getPreconditioner("AMG", coarse_rows=AMG_COARSE_ROWS)
        assert M.amg_info()["levels"] >= 2
        levels = hierarchy(csr, coarse_rows=AMG_COARSE_ROWS)
        return M, amg_apply(oracle, levels, coarse_inverse(levels[-1]["A"]))
    M = A.getPreconditioner(enum_of(smm, kind))
    if kind == "CHEBYSHEV":
        lmax = gershgorin(csr)
        return M, cheb_apply(oracle, csr, 3, lmax / 30.0, lmax)
    if kind.startswith("MULTICOLOR_"):
        return M, mc_apply(oracle, csr, kind.split("_")[1])
    if kind in ("FSAI", "SPAI"):
        return M, ainv_apply(oracle, csr, FSAI if kind == "FSAI" else SPAI, 1)
    if kind == "JACOBI":
        err, diag = oracle.jacobi_setup(csr)
        assert err == 0
        return M, lambda v: oracle.jacobi_apply(diag, np.ascontiguousarray(v, dtype=dtype))
    if kind == "SGS":
        return M, lambda v: oracle.sgs_apply(csr, np.ascontiguousarray(v, dtype=dtype))[1]
    if kind in ("ILU0", "IC0"):
        err, f = oracle.ilu0_factorize(csr) if kind == "ILU0" else oracle.ic0_factorize(csr)
        assert err == 0
        fn = oracle.ilu0_apply if kind == "ILU0" else oracle.ic0_apply
        return M, lambda v: fn(csr, f, np.ascontiguousarray(v, dtype=dtype))[1]
    bounds, order = M.block_bounds(), M.block_rows()[0]  # BLOCK_ILU0 / BLOCK_SGS: defined on P A P^T with contiguous blocks
    mcsr = oracle.level_cut_matrix(permuted(csr, order), bounds, M.level_cap())[0]
    if kind == "BLOCK_ILU0":
        err, lu = oracle.block_ilu0_factorize(mcsr, bounds)
        assert err == 0
        sweep = lambda v: oracle.block_ilu0_apply(mcsr, bounds, lu, v)[1]  # noqa: E731
    else:
        sweep = lambda v: oracle.block_sgs_apply(mcsr, bounds, v)[1]  # noqa: E731

    def apply(v):
        z = np.zeros(len(v), dtype=dtype)
        z[order] = sweep(np.ascontiguousarray(np.asarray(v, dtype=dtype)[order]))
        return z

    return M, apply


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,kind", OFFERS, ids=ids)
def test_one_shared_preconditioner_handle(smm, oracle, solver, kind, dtype):
    """the exact kinds keep their scratch per stream and enqueue an apply whole; CHEBYSHEV, AMG, MULTICOLOR_* and FSAI keep one set of
    work vectors in the handle, and an apply of theirs is several launches: without a lock around it the launches of two threads
    interleave on the library stream and one thread's apply reads the other's vector"""
    which = "spd" if kind in SYMMETRIC_KINDS else "gen"
    # BLOCK_*: at several lanes per row the sums depend on the lane count, which the header leaves to the library: one lane per row
    H = handles(smm, which, dtype, (smm.SPMV_STREAM, 1) if kind.startswith("BLOCK_") else PATTERN_ONE_LANE)
    M, apply = preconditioner(smm, oracle, H["A"], H["csr"], kind)
    run_case(smm, oracle, [on(which, solver)] * THREADS, H, dtype, "precond/" + kind, M=M, apply=apply, it=PRECOND_IT)
    M.close()


# ---- case 4: plain operations, per-thread inputs ----------------------------------------------------------------------------------
def check_plain(rounds, alone, want, tag, dtype, exact):
    for r, results in enumerate(rounds):
        for i, got in enumerate(results):
            if exact:
                np.testing.assert_array_equal(bits(got), bits(want[i]), err_msg=f"{tag}: thread {i}, round {r}: not the oracle's bits")
            else:
                np.testing.assert_allclose(got, want[i], rtol=2e-5 if dtype == np.float32 else 1e-13, atol=2e-5 if dtype == np.float32 else 1e-13)
            np.testing.assert_array_equal(bits(got), bits(alone[i]), err_msg=f"{tag}: thread {i}, round {r}: differs from the call made alone")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family,lanes", [("STREAM", 1), ("STREAM", 4), ("VECTOR", 2), ("PATTERN", 1), ("PATTERN", 2)])  # CONFIGS of tests/test_gpu_csr_update.py
def test_host_pointer_spmv_from_threads(smm, oracle, family, lanes, dtype):
    """rMult, 40 calls per thread so that the windows overlap; one lane per row gives the oracle's bits.  More lanes: fp32 by the
    tolerance of tests/test_gpu_misc.py::test_autotune_and_kernel_selection; fp64 by 1e-13 (seven-entry rows of entries below 7 and
    |x| <= 1: a few hundred units of 2^-53 of the row's |a||x| sum, chosen here, no existing test states one)"""
    csr = matrix("gen", dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr, (getattr(smm, "SPMV_" + family), lanes))
    X = [rhs(n, dtype, i) for i in range(THREADS)]
    want = [oracle.spmv(csr, 0, None, x) for x in X]

    def work(i):
        y = np.zeros(n, dtype=dtype)
        for _ in range(40):
            y[:] = 0
            A.rMult(X[i], y)
        return y

    alone = [work(i) for i in range(THREADS)]
    check_plain(concurrently(work), alone, want, f"rMult {family} {lanes}", dtype, lanes == 1)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("fresh", [False, True], ids=["warm", "fresh"])
def test_spmm_and_dot_from_threads(smm, oracle, fresh, dtype):
    """rMultBlock at k = 3 (column j is the SpMV of column j; the STREAM family at one lane per row: the oracle's bits) and dot (its
    partial sums are per stream and the threads share the library stream; compared with the same call made alone and with the float64
    sum at the tolerance of tests/test_gpu_misc.py::test_fused_dot_entry_point)"""
    csr = matrix("gen", dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr, (smm.SPMV_STREAM, 1))
    solo = make(smm, csr, (smm.SPMV_STREAM, 1)) if fresh else A
    X = [rhs(n, dtype, i, K) for i in range(THREADS)]
    want = [np.stack([oracle.spmv(csr, 0, None, np.ascontiguousarray(x[:, j])) for j in range(K)], axis=1) for x in X]

    def spmm(i, m=None):
        out = np.zeros((n, K), dtype=dtype)
        for _ in range(30):
            out[:] = 0
            (m or A).rMultBlock(X[i], out)
        return out

    alone = [spmm(i, solo) for i in range(THREADS)]
    check_plain(concurrently(spmm), alone, want, "rMultBlock", dtype, True)
    if fresh:
        return
    big = 1 << 20  # more than one workgroup's share of the partial sums
    V = [np.random.default_rng(10 + i).uniform(-1, 1, (2, big)).astype(dtype) for i in range(THREADS)]

    def dots(i):
        return np.array([smm.dot(V[i][0], V[i][1]) for _ in range(20)], dtype=dtype)

    alone = [dots(i) for i in range(THREADS)]
    for r, results in enumerate(concurrently(dots)):
        for i, got in enumerate(results):
            exact = float(np.dot(V[i][0].astype(np.float64), V[i][1].astype(np.float64)))
            tol = (1e-4 if dtype == np.float32 else 1e-11) * float(np.abs(V[i][0].astype(np.float64) * V[i][1]).sum())
            assert np.all(np.abs(got.astype(np.float64) - exact) <= tol), (i, r, got, exact)
            np.testing.assert_array_equal(bits(got), bits(alone[i]), err_msg=f"dot: thread {i}, round {r}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["JACOBI", "SGS", "ILU0", "BLOCK_ILU0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "FSAI"])
def test_preconditioner_applies_from_threads(smm, oracle, kind, dtype):
    """apply and apply_spmv (the multicolour kinds have no apply_spmv) of one handle, 20 calls per thread, at one lane per row.  The
    exact kinds (JACOBI, SGS, ILU0, BLOCK_ILU0) give the oracle's bits: apply(r), and apply(oracle.spmv(v)) for apply_spmv.  CHEBYSHEV,
    AMG, MULTICOLOR_SGS and FSAI are compared with a NumPy restatement whose set-up (bounds, hierarchy, colouring, G) is its
    own, not the handle's, so by the tolerance of test_gpu_cgs.allowed; all of them bit for bit with the applies made alone"""
    csr = matrix("spd", dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr, (smm.SPMV_STREAM, 1))
    M, apply = preconditioner(smm, oracle, A, csr, kind)
    if kind == "AMG":
        for l in range(M.amg_info()["levels"]):
            for m in M.amg_level(l):
                if m is not None:
                    m.set_kernel(smm.SPMV_STREAM, 1)
    R = [rhs(n, dtype, i) for i in range(THREADS)]
    fused = not kind.startswith("MULTICOLOR_")

    def work(i):
        z, w = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
        for _ in range(20):
            z[:] = 0
            M.apply(R[i], z)
            if fused:
                w[:] = 0
                M.apply_spmv(R[i], w)
        return np.stack([z, w])

    alone = [work(i) for i in range(THREADS)]
    refs = []
    for i in range(THREADS):
        v = oracle.spmv(csr, 0, None, R[i])
        z_ref, w_ref = apply(R[i]), apply(v)
        refs.append((z_ref, allowed(z_ref, sensitivity(apply, R[i], z_ref), dtype), w_ref, allowed(w_ref, sensitivity(apply, v, w_ref), dtype)))
    for r, results in enumerate(concurrently(work)):
        for i, got in enumerate(results):
            z_ref, z_tol, w_ref, w_tol = refs[i]
            if kind in ("JACOBI", "SGS", "ILU0", "BLOCK_ILU0"):
                np.testing.assert_array_equal(bits(got[0]), bits(z_ref), err_msg=f"{kind}: apply, thread {i}, round {r}: not the oracle's bits")
                np.testing.assert_array_equal(bits(got[1]), bits(w_ref), err_msg=f"{kind}: apply_spmv, thread {i}, round {r}: not the oracle's bits")
            else:
                assert worst(got[0], z_ref) <= z_tol, (kind, i, r)
                if fused:
                    assert worst(got[1], w_ref) <= w_tol, (kind, i, r)
            np.testing.assert_array_equal(bits(got), bits(alone[i]), err_msg=f"{kind}: thread {i}, round {r}: differs from the applies made alone")
    M.close()


# ---- case 5: one exact-kind handle on several streams, from one host thread ------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("kind", ["SGS", "ILU0"])
def test_one_exact_handle_on_several_streams(smm, oracle, kind, dtype):
    """the exact kinds keep their sweep scratch per stream: applies enqueued alternately on two streams with different right-hand
    sides equal the applies made alone, and walking the handle over 9 streams crosses the eviction of the scratch map (8 entries)"""
    import torch

    dev = torch.device("cuda:0")
    csr = matrix("gen", dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    M, apply = preconditioner(smm, oracle, A, csr, kind)
    R = [rhs(n, dtype, i) for i in range(9)]
    d_R = [torch.from_numpy(r).to(dev) for r in R]
    torch.cuda.synchronize()
    want = []
    for i in range(9):
        d_z = torch.zeros(n, dtype=d_R[i].dtype, device=dev)
        M.apply_dev(d_R[i], d_z, None)
        M.take_error(None)
        want.append(d_z.cpu().numpy())
        z_ref = apply(R[i])
        assert worst(want[i], z_ref) <= allowed(z_ref, sensitivity(apply, R[i], z_ref), dtype), (kind, i)
    streams = [torch.cuda.Stream(device=dev) for _ in range(9)]
    d_Z = [[torch.zeros(n, dtype=d_R[0].dtype, device=dev) for _ in range(20)] for _ in range(2)]
    torch.cuda.synchronize()
    for j in range(20):
        for s in range(2):
            M.apply_dev(d_R[s], d_Z[s][j], streams[s].cuda_stream)
    for s in range(2):
        M.take_error(streams[s].cuda_stream)  # synchronises the stream; raises if a sweep ran into its pass limit
        for j in range(20):
            np.testing.assert_array_equal(bits(d_Z[s][j].cpu().numpy()), bits(want[s]), err_msg=f"{kind}: stream {s}, apply {j}")
    d_out = [torch.zeros(n, dtype=d_R[0].dtype, device=dev) for _ in range(10)]
    torch.cuda.synchronize()
    for i, s in enumerate(streams + streams[:1]):
        M.apply_dev(d_R[i % 9], d_out[i], s.cuda_stream)
        M.take_error(s.cuda_stream)
        np.testing.assert_array_equal(bits(d_out[i].cpu().numpy()), bits(want[i % 9]), err_msg=f"{kind}: stream {i} of the walk")
    M.close()
