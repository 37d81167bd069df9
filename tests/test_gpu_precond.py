"""GPU parity of the preconditioner apply kernels (level-scheduled triangular sweeps): bit-identical to the sequential
sweeps of the reference / oracle."""
import numpy as np
import pytest
from test_oracle import gen_matrices, spmv_vectors

from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sgs_apply_bit_identical_to_reference(smm, golden, dtype):
    dn = np.dtype(dtype).name
    rng_rows = {}
    for mname, csr in gen_matrices(dtype).items():
        if mname == "ragged_300":
            continue
        rows = len(csr[0]) - 1
        A = make(smm, csr)
        M = A.getPreconditioner(smm.SolverPreconditioner.SYMMETRIC_GAUS_SEIDEL)
        lhs = spmv_vectors(rows, dtype)[1]
        x = np.zeros(rows, dtype=dtype)
        assert M.apply(lhs, x) == 0
        np.testing.assert_array_equal(x, golden[f"gen/{mname}/{dn}/sgs_apply/x"], err_msg=mname)
        lo, up = M.levels()
        assert lo >= 1 and up >= 1
        rng_rows[mname] = (lo, up)
    assert rng_rows["poisson2d_32"] == (63, 63)  # i + j wavefronts of the 32x32 grid


@pytest.mark.parametrize("dtype", DTYPES)
def test_ic0_matches_reference(smm, golden, dtype):
    dn = np.dtype(dtype).name
    P = smm.SolverPreconditioner
    csr = (golden["ic0_kat/start"], golden["ic0_kat/positions"], golden["ic0_kat/values"].astype(dtype))
    A = smm.CSRMatrix(5, 5, *csr)
    M = A.getPreconditioner(P.IC0)
    x = np.zeros(5, dtype=dtype)
    M.apply(np.ones(5, dtype=dtype), x)
    np.testing.assert_allclose(x, golden["ic0_kat/resRef"], rtol=1e-4)  # test/cpp/cg.cpp:55
    np.testing.assert_array_equal(M.values(), golden[f"ic0_kat/{dn}/values"])
    np.testing.assert_array_equal(x, golden[f"ic0_kat/{dn}/x"])
    for mname in ("poisson2d_32", "banded_2000"):
        csr = gen_matrices(dtype)[mname]
        rows = len(csr[0]) - 1
        A = make(smm, csr)
        M = A.getPreconditioner(P.IC0)
        np.testing.assert_array_equal(M.values(), golden[f"gen/{mname}/{dn}/ic0/values"])
        lhs = spmv_vectors(rows, dtype)[1]
        x = np.zeros(rows, dtype=dtype)
        M.apply(lhs, x)
        np.testing.assert_array_equal(x, golden[f"gen/{mname}/{dn}/ic0/x"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_jacobi_and_ilu0_match_oracle(smm, oracle, dtype):
    """no reference behaviour exists for these two (parity unpinned); the oracle is the textbook algorithm"""
    P = smm.SolverPreconditioner
    for csr in (gen.convdiff3d(14, 0.3, dtype=dtype), gen.banded_random_spd(3000, k=9, seed=3, max_offset=800, dtype=dtype),
                gen.random_rows(500, 500, 2, 25, seed=9, dtype=dtype, diag_dominant=True)):
        rows = len(csr[0]) - 1
        A = make(smm, csr)
        rhs = np.random.default_rng(8).uniform(-1, 1, rows).astype(dtype)
        J = A.getPreconditioner(P.JACOBI)
        e, diag = oracle.jacobi_setup(csr)
        assert e == 0
        np.testing.assert_array_equal(J.values(), diag)
        x = np.zeros(rows, dtype=dtype)
        J.apply(rhs, x)
        np.testing.assert_array_equal(x, oracle.jacobi_apply(diag, rhs))
        I = A.getPreconditioner(P.ILU0)
        e, lu = oracle.ilu0_factorize(csr)
        assert e == 0
        np.testing.assert_array_equal(I.values(), lu)
        I.apply(rhs, x)
        np.testing.assert_array_equal(x, oracle.ilu0_apply(csr, lu, rhs)[1])
        S = A.getPreconditioner(P.SYMMETRIC_GAUS_SEIDEL)
        S.apply(rhs, x)
        np.testing.assert_array_equal(x, oracle.sgs_apply(csr, rhs)[1])


def test_structural_failures(smm):
    """missing / tiny diagonal, leading empty row: create fails with SMM_HIP_ERR_PRECOND (the reference's non-zero
    return of apply, ref:1666-1693)"""
    P = smm.SolverPreconditioner
    bad = [
        (np.array([0, 1, 2], dtype=np.int32), np.array([1, 1], dtype=np.int32), np.array([1.0, 2.0])),
        (np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1.0, 1e-7])),
        (np.array([0, 0, 1], dtype=np.int32), np.array([1], dtype=np.int32), np.array([1.0])),
    ]
    for csr in bad:
        A = smm.CSRMatrix(2, 2, *csr)
        for kind in (P.SYMMETRIC_GAUS_SEIDEL, P.JACOBI):
            with pytest.raises(smm.SmmHipError) as e:
                A.getPreconditioner(kind)
            assert e.value.code == -4
    A = smm.CSRMatrix(2, 2, np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32), np.array([1.0, 2.0, 2.0, 1.0]))
    with pytest.raises(smm.SmmHipError):  # not positive definite
        A.getPreconditioner(P.IC0)
    # IC0 on a pattern that is not symmetric (row 2 holds column 0, row 0 does not hold column 2): refused, not factorised into garbage
    A = smm.CSRMatrix(3, 3, np.array([0, 2, 4, 7], dtype=np.int32), np.array([0, 1, 0, 1, 0, 1, 2], dtype=np.int32),
                      np.array([4.0, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0]))
    with pytest.raises(smm.SmmHipError) as e:
        A.getPreconditioner(P.IC0)
    assert e.value.code == -4 and "symmetric" in str(e.value)
    # ILU0 with a pivot that cancels to zero: [[1, 1], [1, 1]] -> u_11 = 1 - 1 * 1 = 0 (ref:1741-1746: reordering would be needed)
    A = smm.CSRMatrix(2, 2, np.array([0, 2, 4], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32), np.array([1.0, 1.0, 1.0, 1.0]))
    with pytest.raises(smm.SmmHipError) as e:
        A.getPreconditioner(P.ILU0)
    assert e.value.code == -4
    M = smm.CSRMatrix(2, 2, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([2.0, 4.0])).getPreconditioner(P.JACOBI)
    v = np.ones(2)
    with pytest.raises(smm.SmmHipError):  # rhs must not alias x (ref:1667)
        M.apply(v, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_modes_bit_identical(smm, oracle, dtype):
    """the level-scheduled sweeps (one launch per level) and the synchronisation-free sweeps (one launch per sweep, rows wait
    on ready values) walk every row in the reference's order: same bits, and the oracle's sequential sweep's bits; sizes with
    thousands of wavefronts, hundreds of levels, levels smaller and larger than a wavefront"""
    from sparse_matrix_math_amd.host import SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD

    P = smm.SolverPreconditioner
    cases = {
        "convdiff3d_48": gen.convdiff3d(48, 0.3, dtype=dtype),  # 110 592 rows, 142 levels of up to ~1700 rows
        "poisson2d_400x130": gen.poisson2d(400, 130, dtype=dtype),  # 529 levels of <= 130 rows
        "banded": gen.banded_random_spd(50_000, k=6, seed=11, max_offset=3000, dtype=dtype),
        "chain": gen.banded_random_spd(3000, k=1, seed=5, max_offset=2, dtype=dtype),  # tridiagonal: every row its own level
    }
    rng = np.random.default_rng(12)
    for name, csr in cases.items():
        rows = len(csr[0]) - 1
        A = make(smm, csr)
        rhs = rng.uniform(-1, 1, rows).astype(dtype)
        kinds = [P.SYMMETRIC_GAUS_SEIDEL, P.ILU0] + ([P.IC0] if name != "convdiff3d_48" else [])
        for kind in kinds:
            M = A.getPreconditioner(kind)
            out = {}
            for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD):
                M.set_sweep(mode)
                x = np.full(rows, 7, dtype=dtype)
                for _ in range(3):  # repeated applies reuse the ticket counters and the scratch vector
                    M.apply(rhs, x)
                out[mode] = x
            np.testing.assert_array_equal(out[SWEEP_LEVELS], out[SWEEP_SYNCFREE], err_msg=f"{name} {kind}")
            np.testing.assert_array_equal(out[SWEEP_LEVELS], out[SWEEP_SYNCFREE_XCD], err_msg=f"{name} {kind} one XCD")
            if kind == P.SYMMETRIC_GAUS_SEIDEL and rows <= 60_000:
                np.testing.assert_array_equal(out[SWEEP_SYNCFREE], oracle.sgs_apply(csr, rhs)[1], err_msg=name)


def test_sweep_modes_in_solver(smm):
    """a preconditioned BiCGStab / PCG solve gives the same bits whichever way the sweeps are launched; NaN / Inf in rhs travel
    through the synchronisation-free sweep (NaN is not the 'not ready yet' marker) instead of stalling it"""
    from sparse_matrix_math_amd.host import SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD

    P = smm.SolverPreconditioner
    csr = gen.convdiff3d(30, 0.3, dtype=np.float64)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    b = np.random.default_rng(2).uniform(-1, 1, n)
    res = {}
    for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE):
        M = A.getPreconditioner(P.ILU0)
        M.set_sweep(mode)
        x = np.zeros(n)
        info = {}
        st = smm.BiCGStab(A, b, x, 200, 1e-10, M=M, info=info)
        res[mode] = (int(st), info["iterations"], x)
    assert res[SWEEP_LEVELS][:2] == res[SWEEP_SYNCFREE][:2]
    assert res[SWEEP_SYNCFREE][1] < 60
    np.testing.assert_array_equal(res[SWEEP_LEVELS][2], res[SWEEP_SYNCFREE][2])
    spd = gen.poisson2d(90, dtype=np.float64)
    S = make(smm, spd)
    bs = np.random.default_rng(3).uniform(-1, 1, 8100)
    res = {}
    for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE):
        M = S.getPreconditioner(P.IC0)
        M.set_sweep(mode)
        x = np.zeros(8100)
        info = {}
        st = smm.ConjugateGradient(S, bs, np.zeros(8100), x, 500, 1e-10, M=M, info=info)
        res[mode] = (int(st), info["iterations"], x)
    assert res[SWEEP_LEVELS][:2] == res[SWEEP_SYNCFREE][:2] and res[SWEEP_SYNCFREE][0] == 0
    np.testing.assert_array_equal(res[SWEEP_LEVELS][2], res[SWEEP_SYNCFREE][2])
    # non-finite input
    M = S.getPreconditioner(P.SYMMETRIC_GAUS_SEIDEL)
    bad = bs.copy()
    bad[17] = np.nan
    bad[4000] = np.inf
    outs = []
    for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE):
        M.set_sweep(mode)
        x = np.zeros(8100)
        M.apply(bad, x)
        outs.append(x)
    np.testing.assert_array_equal(np.isnan(outs[0]), np.isnan(outs[1]))
    ok = ~np.isnan(outs[0])
    np.testing.assert_array_equal(outs[0][ok], outs[1][ok])
    with pytest.raises(smm.SmmHipError):
        M.set_sweep(9)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ic0_and_ilu0_long_rows_match_oracle(smm, oracle, dtype):
    """rows far longer than a wavefront (the device factorisation shares a row's work over 64 lanes in batches): a dense symmetric
    positive definite block of 200 rows inside a banded matrix -- factor values and one apply bit-identical to the oracle's
    sequential algorithms (the oracle's IC0 is pinned to the real reference bit for bit, tests/test_oracle.py)"""
    P = smm.SolverPreconditioner
    rng = np.random.default_rng(21)
    nb, n = 200, 600
    dense = np.zeros((n, n))
    blk = rng.uniform(-0.5, 0.5, (nb, nb)) / nb
    dense[100:100 + nb, 100:100 + nb] = blk + blk.T
    for i in range(n):
        dense[i, i] = 3.0
        if i + 1 < n:
            dense[i, i + 1] = dense[i + 1, i] = -1.0
        if i + 7 < n:
            dense[i, i + 7] = dense[i + 7, i] = -0.25
    start = np.zeros(n + 1, dtype=np.int32)
    pos, val = [], []
    for r in range(n):
        (c,) = np.nonzero(dense[r])
        pos.extend(c.tolist())
        val.extend(dense[r, c].tolist())
        start[r + 1] = len(pos)
    csr = (start, np.array(pos, dtype=np.int32), np.array(val, dtype=dtype))
    assert np.diff(start).max() > 3 * 64
    A = make(smm, csr)
    rhs = rng.uniform(-1, 1, n).astype(dtype)
    x = np.zeros(n, dtype=dtype)
    e, ic = oracle.ic0_factorize(csr)
    assert e == 0
    M = A.getPreconditioner(P.IC0)
    np.testing.assert_array_equal(M.values(), ic)
    M.apply(rhs, x)
    np.testing.assert_array_equal(x, oracle.ic0_apply(csr, ic, rhs)[1])
    e, lu = oracle.ilu0_factorize(csr)
    assert e == 0
    M = A.getPreconditioner(P.ILU0)
    np.testing.assert_array_equal(M.values(), lu)
    M.apply(rhs, x)
    np.testing.assert_array_equal(x, oracle.ilu0_apply(csr, lu, rhs)[1])


def _band_lower_chain(n, width, dtype):
    """rows i hold columns i-width .. i+1: every row waits for its `width` predecessors -- a pure dependency chain with long rows"""
    offs = np.arange(-width, 2)
    cols = np.arange(n)[:, None] + offs[None, :]
    ok = (cols >= 0) & (cols < n)
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(ok.sum(axis=1), out=start[1:])
    pos = cols[ok].astype(np.int32)
    val = np.broadcast_to(np.where(offs == 0, 2.0 * width + 4.0, -1.0)[None, :], cols.shape)[ok].astype(dtype)
    return start, pos, val


@pytest.mark.parametrize("case", ["tridiagonal_1m", "band40_200k"])
def test_deep_chains_do_not_trip_the_escape_bound(smm, oracle, case):
    """the level analysis is one synchronisation-free launch whose escape bound must not depend on the depth of the DAG.
    A tridiagonal matrix of a million rows (a million levels) and a 40-wide band (200 000 levels, 42-entry rows): create, levels, apply
    bit-identical to the oracle's sequential sweeps."""
    dtype = np.float64
    P = smm.SolverPreconditioner
    n, width = (1_000_000, 1) if case == "tridiagonal_1m" else (200_000, 40)
    csr = _band_lower_chain(n, width, dtype)
    A = make(smm, csr)
    rhs = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    for kind in (P.SYMMETRIC_GAUS_SEIDEL, P.ILU0):
        M = A.getPreconditioner(kind)
        assert M.levels() == (n, n)  # both sweeps: one row per level
        x = np.zeros(n, dtype=dtype)
        assert M.apply(rhs, x) == 0
        if kind == P.ILU0:
            e, lu = oracle.ilu0_factorize(csr)
            assert e == 0
            np.testing.assert_array_equal(M.values(), lu)
            np.testing.assert_array_equal(x, oracle.ilu0_apply(csr, lu, rhs)[1])
        else:
            np.testing.assert_array_equal(x, oracle.sgs_apply(csr, rhs)[1])


def _smallest_shapes(dtype):
    """symmetric positive definite, so that every kind can be created: 1 x 1; 2 x 2 diagonal (no row has an off-diagonal entry); a 65-row
    tridiagonal matrix (every row its own level, one level more than a wavefront has lanes, first and last row with one neighbour)"""
    one = (np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([3.0], dtype=dtype))
    diag2 = (np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([3.0, 7.0], dtype=dtype))
    n = 65
    cols = np.arange(n)[:, None] + np.array([-1, 0, 1])[None, :]
    ok = (cols >= 0) & (cols < n)
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(ok.sum(axis=1), out=start[1:])
    lower = -(1.0 + 0.003 * np.arange(n))  # a(i, i - 1) = a(i - 1, i)
    vals = np.stack([lower, 4.0 + 0.01 * np.arange(n), np.roll(lower, -1)], axis=1)
    return {"1x1": one, "2x2_diagonal": diag2, "tridiagonal_65": (start, cols[ok].astype(np.int32), vals[ok].astype(dtype))}


@pytest.mark.parametrize("dtype", DTYPES)
def test_smallest_triangular_shapes(smm, oracle, dtype):
    """SGS / ILU0 / IC0 in every sweep mode and their multicolour forms on the smallest shapes a sweep can take: bit for bit the oracle's
    sequential sweeps (the multicolour kinds: on the restated permuted matrix, tests/multicolor_restatement.py); no rows: OK, nothing written"""
    import torch
    from device_views import address, assert_guards_intact, carve
    from multicolor_restatement import IC0, ILU0, SGS, make_apply

    from sparse_matrix_math_amd.host import SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD

    P = smm.SolverPreconditioner
    exact = {SGS: P.SYMMETRIC_GAUS_SEIDEL, ILU0: P.ILU0, IC0: P.IC0}
    multi = {SGS: P.MULTICOLOR_SGS, ILU0: P.MULTICOLOR_ILU0, IC0: P.MULTICOLOR_IC0}

    def bits(a):
        return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)

    def sequential(csr, base, rhs):
        if base == SGS:
            err, x = oracle.sgs_apply(csr, rhs)
        else:
            e, f = oracle.ilu0_factorize(csr) if base == ILU0 else oracle.ic0_factorize(csr)
            assert e == 0
            err, x = oracle.ilu0_apply(csr, f, rhs) if base == ILU0 else oracle.ic0_apply(csr, f, rhs)
        assert err == 0
        return x

    for name, csr in _smallest_shapes(dtype).items():
        n = len(csr[0]) - 1
        A = make(smm, csr)
        rhs = np.random.default_rng(21).uniform(-1, 1, n).astype(dtype)
        for base in (SGS, ILU0, IC0):
            want = sequential(csr, base, rhs)
            M = A.getPreconditioner(exact[base])
            assert M.levels() == ((n, n) if name == "tridiagonal_65" else (1, 1))
            for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD):
                M.set_sweep(mode)
                x = np.full(n, np.nan, dtype=dtype)
                M.apply(rhs, x)
                np.testing.assert_array_equal(bits(x), bits(want), err_msg=f"{name} {base} sweep mode {mode}")
            want = make_apply(oracle, csr, base)(rhs)
            x = np.full(n, np.nan, dtype=dtype)
            A.getPreconditioner(multi[base]).apply(rhs, x)
            np.testing.assert_array_equal(bits(x), bits(want), err_msg=f"{name} MULTICOLOR_{base}")
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    for kind in list(exact.values()) + list(multi.values()):
        M = E.getPreconditioner(kind)
        for mode in (SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD):
            M.set_sweep(mode)
            M.apply(np.zeros(0, dtype=dtype), np.zeros(0, dtype=dtype))
            d_r, d_x = carve(0, dtype, 0, device="cuda:0"), carve(0, dtype, 1, device="cuda:0")
            M.apply_dev(address(d_r), address(d_x))  # (a view of no elements has no address of its own)
            M.take_error()
            torch.cuda.synchronize()
            assert_guards_intact(d_r, "rhs")
            assert_guards_intact(d_x, "x")
