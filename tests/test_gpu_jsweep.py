"""The iterated triangular sweeps on the GPU (csrc/smm_precond_jsweep.hip) through the C ABI, against their CPU restatement
(tests/jsweep_restatement.py): the applies bit for bit at several step counts, the exact kind's bits at levels - 1 steps, set_sweeps,
refresh, device pointers, the solvers by the fixed-pass tolerance rule of tests/test_gpu_cgs.py, the refusals, the fma flavour and the
drop-in C++ header."""
import ctypes
import subprocess
import threading

import numpy as np
import pytest
import torch
from chebyshev_restatement import sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres
from gmres_restatement import sensitivity as gmres_sensitivity
from jsweep_restatement import IC0, ILU0, SGS, bicgstab, factor, make_apply, pcg
from test_gpu_cgs import allowed, make, worst
from test_jsweep_cpu import CASES, build_case, chain_for, js_matrix, rhs_of

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID, PRECOND = -1, -4  # SMM_HIP_ERR_INVALID, SMM_HIP_ERR_PRECOND
BASES = (SGS, ILU0, IC0)
KIND = {SGS: "JSWEEP_SGS", ILU0: "JSWEEP_ILU0", IC0: "JSWEEP_IC0"}
EXACT = {SGS: "SYMMETRIC_GAUS_SEIDEL", ILU0: "ILU0", IC0: "IC0"}
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


def restated_apply(oracle, name, base, dtype, lower, upper, r):
    """the restatement's z for that case, made once; the factor is the oracle's"""
    csr = js_matrix(name, dtype)
    f = cached(("factor", name, base, np.dtype(dtype).name), lambda: factor(oracle, csr, base))
    return cached(("apply", name, base, np.dtype(dtype).name, lower, upper), lambda: make_apply(oracle, csr, base, lower, upper, values=f)(r))


def apply_of(M, r):
    z = np.full(len(r), np.nan, dtype=r.dtype)
    M.apply(r, z)
    return z


# ---- apply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,base", CASES)
def test_apply_equals_the_restatement_bit_for_bit(smm, oracle, name, base, dtype):
    """1 / 1, 3 / 3, 2 / 5 and levels - 1 steps, changed on one handle; at levels - 1 also the bits of the exact kind on the same matrix"""
    csr = js_matrix(name, dtype)
    n = len(csr[0]) - 1
    r = rhs_of(n, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    info = M.jsweep_info()
    X = A.getPreconditioner(EXACT[base])
    assert (info["sweeps_lower"], info["sweeps_upper"]) == (3, 3) and info["base"] == smm.SolverPreconditioner[EXACT[base]]
    assert (info["levels_lower"], info["levels_upper"]) == M.levels() == X.levels()
    deep = (max(1, info["levels_lower"] - 1), max(1, info["levels_upper"] - 1))
    saved = r.copy()
    for lower, upper in ((3, 3), (1, 1), (2, 5), deep):
        M.jsweep_set_sweeps(lower, upper)
        assert (M.jsweep_info()["sweeps_lower"], M.jsweep_info()["sweeps_upper"]) == (lower, upper)
        z = apply_of(M, r)
        np.testing.assert_array_equal(bits(z), bits(restated_apply(oracle, name, base, dtype, lower, upper, r)))
    np.testing.assert_array_equal(bits(z), bits(apply_of(X, r)))  # exactness
    np.testing.assert_array_equal(bits(r), bits(saved))
    if base != SGS:
        np.testing.assert_array_equal(bits(M.values()), bits(X.values()))
    if n:
        assert code_of(lambda: M.apply(r, r)) == INVALID  # rhs aliases x: refused like the exact kinds
    # a handle created with the counts equals the one they were set on
    M2 = A.getPreconditioner(KIND[base], sweeps=(2, 5))
    np.testing.assert_array_equal(bits(apply_of(M2, r)), bits(restated_apply(oracle, name, base, dtype, 2, 5, r)))
    M1 = A.getPreconditioner(KIND[base], sweeps=1)
    np.testing.assert_array_equal(bits(apply_of(M1, r)), bits(restated_apply(oracle, name, base, dtype, 1, 1, r)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
def test_truncation_on_the_chain(smm, oracle, base, dtype):
    """the 65-row chain, right-hand side of ones: 64 steps are the exact kind, 63 are not (and are the restatement's)"""
    name = chain_for(base)
    csr = js_matrix(name, dtype)
    r = np.ones(65, dtype=dtype)
    A = make(smm, csr)
    want = apply_of(A.getPreconditioner(EXACT[base]), r)
    M = A.getPreconditioner(KIND[base], sweeps=64)
    assert M.levels() == (65, 65)
    np.testing.assert_array_equal(bits(apply_of(M, r)), bits(want))
    M.jsweep_set_sweeps(63)
    z = apply_of(M, r)
    assert not np.array_equal(bits(z), bits(want))
    np.testing.assert_array_equal(bits(z), bits(make_apply(oracle, csr, base, 63, 63)(r)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
def test_refresh_after_value_edits(smm, base, dtype):
    """a handle is a snapshot: the old apply until refreshed, then bit for bit a newly created handle -- after a scale, after an entry batch"""
    name = "poisson2d_9x7" if base == IC0 else "convdiff3d_5"
    csr = js_matrix(name, dtype)
    n = len(csr[0]) - 1
    r = rhs_of(n, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base], sweeps=(2, 4))
    old = apply_of(M, r)
    d = np.arange(0, n, 3, dtype=np.int32)
    for edit in (lambda: A.scale(1.75), lambda: A.update_entries(d, d, np.full(len(d), 0.5, dtype=dtype), add=True)):
        edit()
        np.testing.assert_array_equal(bits(apply_of(M, r)), bits(old))  # stale
        M.jsweep_refresh()
        fresh = A.getPreconditioner(KIND[base], sweeps=(2, 4))
        z = apply_of(M, r)
        np.testing.assert_array_equal(bits(z), bits(apply_of(fresh, r)))
        assert not np.array_equal(bits(z), bits(old))
        if base != SGS:
            np.testing.assert_array_equal(bits(M.values()), bits(fresh.values()))
        old = z
    assert M.jsweep_info()["sweeps_lower"] == 2 and M.jsweep_info()["sweeps_upper"] == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("sweeps", [(3, 3), (2, 3)], ids=ids)
def test_apply_device_pointers_on_offset_views_and_another_stream(smm, oracle, base, sweeps, dtype):
    """both parities of the upper count: the iterates pass through x or through scratch"""
    name = "arrow_300" if base == IC0 else "convdiff3d_5"
    csr = js_matrix(name, dtype)
    n = len(csr[0]) - 1
    r = rhs_of(n, dtype)
    z_ref = restated_apply(oracle, name, base, dtype, sweeps[0], sweeps[1], r)
    M = make(smm, csr).getPreconditioner(KIND[base], sweeps=sweeps)
    d_r = carve_like(r, fit(1, dtype), device="cuda:0")
    d_z = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    saved = snapshot(d_r)
    torch.cuda.synchronize()
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        d_z.fill_(float("nan"))
        torch.cuda.synchronize()
        M.apply_dev(d_r, d_z, s.cuda_stream)
        M.take_error(s.cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(d_z.cpu().numpy()), bits(z_ref))
    assert_unchanged(d_r, saved, "rhs")
    assert_guards_intact(d_r, "rhs")
    assert_guards_intact(d_z, "x")


# ---- solvers -----------------------------------------------------------------------------------------------------------------
def restated(oracle, solver, name, base, dtype, it, eps):
    """(status, x, iterations, sensitivity or None) of the restated loop with 3 / 3 steps, made once"""
    def compute():
        csr = js_matrix(name, dtype)
        b = gen.row_sums(csr[0], csr[2])
        fn = make_apply(oracle, csr, base, 3, 3)
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
    return cached(("solve", solver, name, base, np.dtype(dtype).name, it, eps), compute)


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


SOLVES = [("cg", "poisson2d_24", IC0), ("bicgstab", "convdiff3d_10", ILU0), ("bicgstab", "convdiff3d_10", SGS), ("gmres", "convdiff3d_10", ILU0),
          ("gmres", "convdiff3d_10", SGS)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name,base", SOLVES)
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, name, base, dtype):
    """the fixed-pass rule of tests/test_gpu_cgs.py: 5 passes with eps = 0 against the restated loop, within `allowed`"""
    it = 5
    csr = js_matrix(name, dtype)
    b = gen.row_sums(csr[0], csr[2])
    st_ref, x_ref, it_ref, sens = restated(oracle, solver, name, base, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    st, x, info = run(smm, solver, A, b, it, 0.0, M, dtype)
    err = worst(x, x_ref)
    print(solver, name, base, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol, "sensitivity", sens, info)
    assert st == st_ref and info["iterations"] == it_ref == it
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name,base", [("cg", "poisson2d_24", IC0), ("bicgstab", "convdiff3d_10", ILU0), ("gmres", "convdiff3d_10", SGS)])
def test_converged_runs(smm, oracle, solver, name, base, dtype):
    """SUCCESS, and the restated loop's iteration count within the slack of test_gpu_multicolor.py::test_converged_runs, max(2, ref // 5)"""
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr = js_matrix(name, dtype)
    b = gen.row_sums(csr[0], csr[2])
    st_ref, _, it_ref, _ = restated(oracle, solver, name, base, dtype, -1, eps)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    st, x, info = run(smm, solver, A, b, -1, eps, M, dtype)
    print(solver, name, base, np.dtype(dtype).name, "iterations", info["iterations"], "restated", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5)


def test_refinement_takes_the_kinds(smm):
    """the refinement driver hands M32 to its inner solver: BiCGStab + JSWEEP_ILU0 and CG + JSWEEP_IC0 on the fp32 copy"""
    for name, inner, kind in (("convdiff3d_10", "BICGSTAB", "JSWEEP_ILU0"), ("poisson2d_24", "CG", "JSWEEP_IC0")):
        csr = js_matrix(name, np.float64)
        b = gen.row_sums(csr[0], csr[2])
        A = make(smm, csr)
        A32 = A.astype(np.float32)
        M32 = A32.getPreconditioner(kind)
        x = np.zeros(len(b))
        info = {}
        st = smm.IterativeRefinement(A, b, x, 1e-10, inner=inner, a32=A32, M=M32, info=info)
        print(name, inner, kind, info)
        assert int(st) == 0
        np.testing.assert_allclose(x, 1.0, atol=1e-8)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", (ILU0, SGS))
def test_batched_columns_equal_the_single_vector_runs(smm, oracle, base, dtype):
    """BiCGStabBatch with three different right-hand sides against BiCGStab alone on each column.  The applies of a column are the same
    launches in both; the batched loop adds its dot products from other partial sums than the single loop, which is a perturbation of the
    kind the fixed-pass rule of tests/test_gpu_cgs.py allows for: 5 passes with eps = 0 within `allowed`, from the restated loop's
    sensitivity on that column's b.  Then a converged run: SUCCESS in every column, the single run's count within max(2, count // 5)."""
    name = "convdiff3d_10"
    csr = js_matrix(name, dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    fn = make_apply(oracle, csr, base, 3, 3)
    vs = [np.ones(n, dtype=dtype), (1 + np.arange(n) % 3).astype(dtype), rhs_of(n, dtype)]
    B = np.stack([oracle.spmv(csr, 0, None, v) for v in vs], axis=1).copy()
    zero = np.zeros(n, dtype=dtype)
    for it, eps in ((5, 0.0), (-1, 1e-8 if dtype == np.float64 else 1e-3)):
        X = np.zeros_like(B)
        info = {}
        sts = smm.BiCGStabBatch(A, B.copy(), X, it, eps, M, info=info)
        for j in range(3):
            b = np.ascontiguousarray(B[:, j])
            st1, x1, info1 = run(smm, "bicgstab", A, b, it, eps, M, dtype)
            print(base, np.dtype(dtype).name, "column", j, "passes", it, "batched", info["iterations"][j], "alone", info1["iterations"])
            assert int(sts[j]) == st1 == 0
            if eps == 0.0:
                x_ref = bicgstab(oracle, csr, b, zero, it, 0.0, fn)[1]
                sens = sensitivity(lambda bb: bicgstab(oracle, csr, bb, zero, it, 0.0, fn)[1], b, x_ref)
                tol = allowed(x_ref, sens, dtype)
                err = worst(X[:, j], x1)
                print("   max|x - alone|", err, "allowed", tol)
                assert info["iterations"][j] == info1["iterations"] == it and err <= tol
            else:
                assert abs(int(info["iterations"][j]) - info1["iterations"]) <= max(2, info1["iterations"] // 5)
                np.testing.assert_allclose(X[:, j], vs[j], rtol=0, atol=1e-5 * 3 if dtype == np.float64 else 3e-2)


def test_concurrent_applies_and_solves_on_one_handle(smm):
    """four host threads, a right-hand side each, on one matrix and one JSWEEP_ILU0 handle (unequal step counts: both buffer parities):
    every apply and every solve equals the same call made alone, bit for bit (the rule of tests/test_gpu_concurrent.py)"""
    csr = js_matrix("convdiff3d_10", np.float64)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    M = A.getPreconditioner("JSWEEP_ILU0", sweeps=(3, 2))
    rs = [np.random.default_rng(20 + i).uniform(-1, 1, n) for i in range(4)]

    def solve(r):
        x = np.zeros(n)
        smm.BiCGStab(A, r.copy(), x, 6, 0.0, M)
        return x

    alone = [(apply_of(M, r), solve(r)) for r in rs]
    wrong = []
    gate = threading.Barrier(4)

    def work(i):
        gate.wait()
        for _ in range(8):
            if not np.array_equal(bits(apply_of(M, rs[i])), bits(alone[i][0])):
                wrong.append((i, "apply"))
            if not np.array_equal(bits(solve(rs[i])), bits(alone[i][1])):
                wrong.append((i, "solve"))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not wrong, wrong


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals(smm, dtype):
    start, pos, val = js_matrix("poisson2d_5", dtype)
    P = smm.SolverPreconditioner
    A = make(smm, (start, pos, val))
    b = gen.row_sums(start, val)
    n = len(b)
    # create: the exact kinds' failures with their codes -- not square, a missing diagonal, not positive definite for IC0
    k3 = int(np.nonzero(pos[start[3]:start[4]] == 3)[0][0]) + int(start[3])
    keep = np.ones(len(pos), dtype=bool)
    keep[k3] = False
    s2 = start.copy()
    s2[4:] -= 1
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
    for kind, exact in ((P.JSWEEP_SGS, P.SYMMETRIC_GAUS_SEIDEL), (P.JSWEEP_ILU0, P.ILU0), (P.JSWEEP_IC0, P.IC0)):
        assert code_of(lambda: W.getPreconditioner(kind)) == code_of(lambda: W.getPreconditioner(exact)) == INVALID
        holed = (s2, pos[keep], val[keep])
        assert code_of(lambda: make(smm, holed).getPreconditioner(kind)) == code_of(lambda: make(smm, holed).getPreconditioner(exact)) == PRECOND
    v = val.copy()
    v[k3] = -4.0
    assert code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(P.JSWEEP_IC0)) == code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(P.IC0)) == PRECOND
    # step counts out of range; sweeps= with another kind (refused before the library is asked)
    for bad in (-1, 1025, (3, -2), (2000, 3)):
        assert code_of(lambda: A.getPreconditioner("JSWEEP_ILU0", sweeps=bad)) == INVALID
    with pytest.raises(ValueError):
        A.getPreconditioner("ILU0", sweeps=3)
    S, I, C = (A.getPreconditioner(k) for k in (P.JSWEEP_SGS, P.JSWEEP_ILU0, P.JSWEEP_IC0))
    for bad in ((0, -1), (1025, 1)):
        assert code_of(lambda: I.jsweep_set_sweeps(*bad)) == INVALID
    assert I.jsweep_info()["sweeps_lower"] == 3
    # apply_spmv, set_sweep, the batched entry point, the kinds a solver does not take, a foreign matrix; nothing written
    x = np.full(n, 0.25, dtype=dtype)
    keep_x = x.copy()
    B2 = np.stack([b, b], axis=1).copy()
    X2 = np.full_like(B2, 0.25)
    for M in (S, I, C):
        assert code_of(lambda: M.apply_spmv(b, x)) == INVALID
        assert code_of(lambda: M.set_sweep(1)) == INVALID
        assert code_of(lambda: smm.BiCGStab(make(smm, (start, pos, val)), b.copy(), x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: smm.BiCGStabBatch(A, B2, X2, 5, 1e-6, C)) == INVALID  # (a Cholesky-type factor, as in the single loop)
    assert code_of(lambda: smm.BiCGStab(A, b.copy(), x, 5, 1e-6, C)) == INVALID
    assert code_of(lambda: smm.GMRES(A, b.copy(), x, 5, 1e-6, 30, C)) == INVALID
    assert code_of(lambda: smm.ConjugateGradient(A, b, x, x, 5, 1e-6, I)) == INVALID
    # ConjugateGradient's symmetric-kind check: unequal counts are not a symmetric operator
    C.jsweep_set_sweeps(2, 3)
    assert code_of(lambda: smm.ConjugateGradient(A, b, x, x, 5, 1e-6, C)) == INVALID
    C.jsweep_set_sweeps(3, 3)
    np.testing.assert_array_equal(bits(x), bits(keep_x))
    np.testing.assert_array_equal(bits(X2), bits(np.full_like(B2, 0.25)))
    d_v = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(keep_x, fit(1, dtype), device="cuda:0")
    saved = snapshot(d_x)
    assert code_of(lambda: S.apply_spmv_dev(d_v, d_x)) == INVALID
    torch.cuda.synchronize()
    assert_unchanged(d_x, saved, "x")
    J = A.getPreconditioner(P.JACOBI)
    for call in (J.jsweep_info, lambda: J.jsweep_set_sweeps(2), J.jsweep_refresh):
        assert code_of(call) == INVALID
    # the same handles still solve
    tol = 1e-6 if dtype == np.float64 else 1e-4
    for M in (S, C):
        x = np.zeros(n, dtype=dtype)
        assert int(smm.ConjugateGradient(A, b, x, x, -1, tol, M)) == 0
        np.testing.assert_allclose(x, 1.0, rtol=1e-3)
    x = np.zeros(n, dtype=dtype)
    assert int(smm.BiCGStab(A, b.copy(), x, -1, tol, I)) == 0
    np.testing.assert_allclose(x, 1.0, rtol=1e-3)


def test_row_partitioned_solver_refuses_the_kinds(smm):
    from sparse_matrix_math_amd import distributed as dist

    csr = js_matrix("convdiff3d_5", np.float64)
    n = len(csr[0]) - 1
    comm = dist.NativeComm.single()
    tens = [torch.tensor(a, device="cuda:0") for a in csr]
    D = dist.NativeDistMatrix(comm, n, [0, n], tens[0], tens[1], tens[2], np.float64)
    b = torch.tensor(gen.row_sums(csr[0], csr[2]), device="cuda:0")
    x = torch.full((n,), 0.25, dtype=torch.float64, device="cuda:0")
    for kind in (smm.SolverPreconditioner.JSWEEP_SGS, smm.SolverPreconditioner.JSWEEP_ILU0):
        D.set_precond(kind)
        assert code_of(lambda: D.bicgstab(b, x, 5, 1e-8)) == INVALID
    torch.cuda.synchronize()
    assert bool((x == 0.25).all())
    D.close()
    comm.close()


# ---- flavour and drop-in -----------------------------------------------------------------------------------------------------
def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_ainv.py::test_fma_flavour loads it): one apply per base against the restatement over
    the fma oracle's factor.  The restatement's own lines stay a*x+b in NumPy, so this flavour is compared by that test's tolerance rule."""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    create = lib.smm_hip_precond_create_jsweep
    create.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
    lib.smm_hip_precond_apply_f64.argtypes = [P, P, P]
    lib.smm_hip_precond_destroy.argtypes = [P]
    lib.smm_hip_csr_destroy.argtypes = [P]
    lib.smm_hip_csr_create_f64.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.POINTER(P)]
    dtype = np.float64
    for base, code, name in ((SGS, 3, "convdiff3d_5"), (ILU0, 2, "convdiff3d_5"), (IC0, 4, "poisson2d_9x7")):
        csr = js_matrix(name, dtype)
        n = len(csr[0]) - 1
        r = rhs_of(n, dtype)
        fn = make_apply(oracle_fma, csr, base, 3, 3)
        z_ref = fn(r)
        sens = sensitivity(fn, r, z_ref)
        h, m = P(), P()
        assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
        assert create(h, code, 3, 3, ctypes.byref(m)) == 0, lib.smm_hip_last_error()
        z = np.zeros(n, dtype=dtype)
        assert lib.smm_hip_precond_apply_f64(m, ptr(r), ptr(z)) == 0, lib.smm_hip_last_error()
        lib.smm_hip_precond_destroy(m)
        lib.smm_hip_csr_destroy(h)
        err = worst(z, z_ref)
        print("fma flavour", KIND[base], name, "max|z - ref|", err, "allowed", allowed(z_ref, sens, dtype))
        assert err <= allowed(z_ref, sens, dtype)


def test_cpp_dropin_case_on_the_gpu(tmp_path):
    """tests/cpp/jsweep_case.cpp: SMM::JacobiSweepPreconditioner in BiCGStab (ILU0, SGS) and ConjugateGradient (IC0, SGS) on the 6 x 6
    generated matrix, both dtypes: SUCCESS at x = 1; 6 levels, so setSweeps(5, 5) makes the apply the exact kind's bit for bit"""
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 10
    for ln in lines:
        words = ln.split()
        if "-exact" in words[0]:
            assert words[1:] == ["hip", "0", "levels", "6", "6", "same", "1", "one_step_same", "0"], ln
            continue
        assert words[1:9] == ["status", "0", "hip", "0", "sweeps", "3", "3", "x"], ln
        x = np.array([float.fromhex(w) for w in words[9:]])
        np.testing.assert_allclose(x, 1.0, rtol=1e-3 if "float" in words[0] else 1e-4)
