"""The zero start of the Krylov drivers (zeroStart, csrc/smm_solver_host.h): from x0 = 0 and a matrix of finite values BiCGStab,
ConjugateGradient and ConjugateGradientSquared copy b instead of launching the set-up SpMV r = b - A x0.  The claim is bit equality with
the launch, so every case runs twice on fresh handles -- SMM_HIP_ZERO_START=0 and the default -- and x, iterations, status and the
residual norm are compared without a tolerance; the SpMV launches of the two runs, counted by the library's own profile, differ by exactly
one where the start is zero and the values are finite, and not at all anywhere else.

rows = 4099 (no multiple of 4 or of 256: the tail of the 16-byte path and a partial last wave), 257 and 1; three offsets per side; 7
iterations at eps = 0; b random, so that the loop does not end in one step."""
import numpy as np
import pytest
import torch

from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
SOLVERS = ["bicgstab", "bicgstab_jacobi", "bicgstab_ilu0", "cg", "cgs"]
ITERS = 7
SWITCH = "SMM_HIP_ZERO_START"

_CASES = {}


def case(rows, dtype):
    """(csr, b) of the banded matrix with `rows` rows, made once"""
    key = (rows, np.dtype(dtype).name)
    if key not in _CASES:
        csr = gen.banded_random_spd(rows, k=3, dtype=dtype)
        b = np.random.default_rng(rows).uniform(0.5, 1.5, rows).astype(dtype)
        if rows > 1:
            b[rows // 2] = -0.0  # r = b must keep a negative zero
        _CASES[key] = (csr, b)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def loops_only(smm):
    """the single-launch solves have no set-up SpMV: the loops are what is under test"""
    cg, bi = host.cg_resident(0), host.bicgstab_resident(0)
    yield
    host.cg_resident(cg)
    host.bicgstab_resident(bi)


def run(smm, solver, A, b, x0):
    """one solve on host arrays: (x, iterations, status, residual norm, SpMV launches)"""
    M = None
    if solver == "bicgstab_jacobi":
        M = A.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    elif solver == "bicgstab_ilu0":
        M = A.getPreconditioner(smm.SolverPreconditioner.ILU0)
    x = x0.copy()
    info = {}
    host.profile_enable(True)
    host.profile_read(reset=True)
    try:
        if solver == "cg":
            st = smm.ConjugateGradient(A, b.copy(), x0.copy(), x, ITERS, 0.0, info=info)
        elif solver == "cgs":
            st = smm.ConjugateGradientSquared(A, b.copy(), x, ITERS, 0.0, info=info)
        else:
            st = smm.BiCGStab(A, b.copy(), x, ITERS, 0.0, M, info=info)
        _ms, launches = host.profile_read(reset=True)
    finally:
        host.profile_enable(False)
    res = info.get("resnorm", info.get("resnorm2"))
    return x, info["iterations"], int(st), np.asarray(res), launches


def both(smm, monkeypatch, solver, csr, b, x0, script=None):
    """[results with the switch off, results with the default]: a fresh handle each, `script(A)` yields after every edit of the values
    (None: one solve)"""
    out = []
    for off in (True, False):
        if off:
            monkeypatch.setenv(SWITCH, "0")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        rows = len(csr[0]) - 1
        A = smm.CSRMatrix(rows, rows, *csr)
        results = [run(smm, solver, A, b, x0)]
        if script:
            for _ in script(A):
                results.append(run(smm, solver, A, b, x0))
        A.close()
        out.append(results)
    return out


def assert_same(off, on, saved):
    """bit equality of what the caller receives (NaNs at the same places), and `saved` SpMV launches fewer"""
    for (x0, it0, st0, res0, n0), (x1, it1, st1, res1, n1), want in zip(off, on, saved):
        np.testing.assert_array_equal(x1, x0)
        np.testing.assert_array_equal(np.signbit(x1), np.signbit(x0))
        np.testing.assert_array_equal(res1, res0)
        assert (it1, st1) == (it0, st0)
        assert n0 - n1 == want, (n0, n1, want)
    assert len(off) == len(on) == len(saved)


def start(kind, rows, dtype):
    x0 = np.zeros(rows, dtype=dtype)
    if kind == "negzero":
        x0[:] = -0.0
    elif kind == "last":
        x0[-1] = 0.25
    elif kind == "nan":
        x0[rows // 3] = np.nan
    return x0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind,saved", [("zero", 1), ("negzero", 1), ("last", 0), ("nan", 0)])
def test_start_kinds(smm, monkeypatch, solver, dtype, kind, saved):
    csr, b = case(4099, dtype)
    off, on = both(smm, monkeypatch, solver, csr, b, start(kind, 4099, dtype))
    assert off[0][1] >= 1 and off[0][4] >= 2  # the loop ran, and through launchSpmv
    if kind != "nan":
        assert np.isfinite(off[0][0]).all() and off[0][1] == ITERS
    assert_same(off, on, [saved])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("rows", [1, 257])
def test_small_sizes(smm, monkeypatch, solver, dtype, rows):
    csr, b = case(rows, dtype)
    off, on = both(smm, monkeypatch, solver, csr, b, start("zero", rows, dtype))
    assert_same(off, on, [1])


def with_inf(csr, dtype):
    """one off-diagonal entry of the middle row made Inf"""
    start_, positions, values = csr
    row = (len(start_) - 1) // 2
    k = start_[row] if positions[start_[row]] != row else start_[row] + 1
    values = values.copy()
    values[k] = np.inf
    return (start_, positions, values), row, int(positions[k])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("solver", ["bicgstab", "bicgstab_jacobi", "cg", "cgs"])
def test_an_inf_among_the_values_keeps_the_spmv(smm, monkeypatch, solver, dtype):
    csr, b = case(4099, dtype)
    bad, _row, _col = with_inf(csr, dtype)
    off, on = both(smm, monkeypatch, solver, bad, b, start("zero", 4099, dtype))
    assert np.isnan(off[0][0]).any()  # 0 * Inf reached r
    np.testing.assert_array_equal(np.isnan(on[0][0]), np.isnan(off[0][0]))
    assert_same(off, on, [0])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("solver", ["bicgstab", "cg", "cgs"])
def test_value_edits_are_followed(smm, monkeypatch, solver, dtype):
    """finite (skip), an entry set to Inf through the editing API (no skip), set back (skip again)"""
    csr, b = case(4099, dtype)
    bad, row, col = with_inf(csr, dtype)
    k = int(np.flatnonzero(~np.isfinite(bad[2]))[0])
    original = csr[2][k]

    def script(A):
        assert A.updateEntry(row, col, np.inf)
        yield
        assert A.updateEntry(row, col, original)
        yield

    off, on = both(smm, monkeypatch, solver, csr, b, start("zero", 4099, dtype), script)
    assert np.isnan(off[1][0]).any() and np.isfinite(off[2][0]).all()
    np.testing.assert_array_equal(off[2][0], off[0][0])
    assert_same(off, on, [1, 0, 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("solver", ["bicgstab", "cg", "cgs"])
@pytest.mark.parametrize("kind,saved", [("zero", 1), ("last", 0)])
def test_unaligned_device_views(smm, monkeypatch, solver, dtype, kind, saved):
    """x (and b) as slices of larger device vectors that start one element past a 16-byte boundary: the one-element path of the zero test
    and of the copies"""
    rows = 4099
    csr, b = case(rows, dtype)
    t_dtype = torch.float32 if dtype == np.float32 else torch.float64
    results = []
    for off in (True, False):
        if off:
            monkeypatch.setenv(SWITCH, "0")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        A = smm.CSRMatrix(rows, rows, *csr)
        big_b = torch.full((rows + 8,), 7.0, dtype=t_dtype, device="cuda:0")
        big_x = torch.full((rows + 8,), 7.0, dtype=t_dtype, device="cuda:0")
        d_b, d_x = big_b[1:1 + rows], big_x[1:1 + rows]
        assert d_x.data_ptr() % 16 != 0
        d_b.copy_(torch.from_numpy(b))
        d_x.copy_(torch.from_numpy(start(kind, rows, dtype)))
        torch.cuda.synchronize()
        host.profile_enable(True)
        host.profile_read(reset=True)
        try:
            if solver == "cg":
                st, it, res = host.cg_dev(A, d_b, d_x, d_x, ITERS, 0.0)
            elif solver == "cgs":
                st, it, res = host.cgs_dev(A, d_b, d_x, ITERS, 0.0)
            else:
                st, it, res = host.bicgstab_dev(A, d_b, d_x, ITERS, 0.0)
            _ms, launches = host.profile_read(reset=True)
        finally:
            host.profile_enable(False)
        torch.cuda.synchronize()
        guard = big_x.cpu().numpy()
        assert (guard[0] == 7.0) and (guard[1 + rows:] == 7.0).all()  # nothing written outside the view
        results.append([(guard[1:1 + rows].copy(), it, int(st), np.asarray(res), launches)])
        A.close()
    assert np.isfinite(results[0][0][0]).all() and results[0][0][1] == ITERS
    assert_same(results[0], results[1], [saved])
