"""The device-pointer ABI with offset views and guard bands (tests/device_views.py).

Every array a `_dev` entry point receives here is a view INSIDE a larger buffer: at element alignment only (residue r: r elements past a
16-byte boundary) and with a band of known content on either side.  After each call the result is checked, the inputs still hold their
bits, and every guard of every array is intact -- the runs with all arrays at residue 0 included, where the guard check alone is the new
coverage.  The expected result of a case is the same call on a fresh handle whose arrays are whole, 256-byte-aligned tensors, forced to the
same kernel family and lanes (bit for bit), and the oracle / the numpy models of the tests of each feature."""
import numpy as np
import pytest
import torch
from conftest import kat_matrix
from device_views import address, assert_guards_intact, assert_unchanged, carve, carve_like, fit, snapshot
from test_assembly_cpu import assemble_model
from test_gpu_csr_update import apply_entries, batch, entry_index
from test_gpu_solvers import RTOL, bicgstab_sensitivity, close
from test_gpu_spmv import bound

from oracle.oracle import OP_ADD, OP_ASSIGN, OP_SUB, PRECOND_NONE
from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
VECTOR, STREAM, PATTERN = 1, 2, 3
MASKS, CODES, CONST = 1, 2, 3
TILE, SLOTS, SWEEP = "spmvPatternTileKernel", "spmvPatternSlotsKernel", "spmvPatternSweepKernel"
DEV = "cuda:0"

# which array sits how many elements past a 16-byte boundary (stated for 4-byte elements; 8-byte arrays fold 2 -> 0 and 3 -> 1)
ARRAYS = ("start", "positions", "values", "x", "lhs", "out")
R0 = dict.fromkeys(ARRAYS, 0)
ALL_DIFFERENT = dict(start=1, positions=2, values=3, x=3, lhs=1, out=2)
RESIDUES = {"R0": R0, **{f"{a}1": {**R0, a: 1} for a in ARRAYS}, "all-different": ALL_DIFFERENT}
MATRIX_RESIDUES = {"R0": R0, "all-different": ALL_DIFFERENT}


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def put(array, residue, fill=None):
    """a numpy array in a carved device view at `residue` (folded into the range of its type)"""
    return carve_like(array, fit(residue, array.dtype), fill=fill, device=DEV)


def whole(array):
    """a numpy array in a device allocation of its own"""
    t = torch.from_numpy(np.ascontiguousarray(array)).to(DEV)
    assert t.data_ptr() % 256 == 0
    return t


def get(t):
    return t.cpu().numpy()


def check_all(inputs, carved):
    """inputs: (name, view, snapshot) that must be unchanged; carved: (name, view) whose guards must be intact"""
    for name, view, saved in inputs:
        assert_unchanged(view, saved, name)
    for name, view in carved:
        assert_guards_intact(view, name)


# ---- matrices: the smallest that still reach each code path -------------------------------------------------------------------------
def ragged(dtype):
    """test_gpu_spmv.test_ragged_and_long_rows cut to 300 rows: leading and trailing empty rows, one 2049- and one 5000-entry row"""
    rng = np.random.default_rng(42)
    rows, cols = 300, 9000
    lens = rng.integers(0, 60, size=rows)
    lens[5] = 5000
    lens[150] = 2049
    lens[:3] = 0
    lens[-4:] = 0
    start = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens, out=start[1:])
    pos = np.concatenate([np.sort(rng.choice(cols, size=n, replace=False)) for n in lens]).astype(np.int32)
    return (start, pos, rng.uniform(-1, 1, start[-1]).astype(dtype)), cols


# The march kernels walk PLANES only when the far offset (a plane, nx * ny rows) is at least 4 * 256 * 8 = 8192 rows, and the kernel that
# reads values[] and the three-window kernel of the 27-point form need at least 8 / 2 such planes (planMarch, masksMarchApplies in
# csrc/smm_spmv_march.hip).  A smaller grid is served in one-plane mode -- every offset near -- by spmvPatternConstMarchKernel, and with
# values[] read by the wave kernel.  96 x 88 x 8 is the smallest grid of whole 16-byte pieces per plane that reaches all three.
PLANES_GRID = (96, 88, 8)
_MATRICES = {}


def matrix(name, dtype):
    """(csr, cols, x, lhs), made once"""
    key = (name, np.dtype(dtype).name)
    if key not in _MATRICES:
        cols = None
        if name == "masks":  # row masks; 46 waves and 57 rows; the number of entries is no multiple of 4
            csr = gen.banded_random_spd(3001, 30, 0x5EED + 3001, 2000, dtype=dtype)
            assert len(csr[0]) - 1 == 3001 and 3001 % 64 and len(csr[1]) % 4
        elif name == "const":
            csr = gen.poisson2d(33, 31, dtype=dtype)
        elif name == "codes":
            csr = gen.banded_random_spd(6000, 32, 0x5EED, 2500, dtype=dtype)
        elif name == "ragged":
            csr, cols = ragged(dtype)
        elif name == "convdiff":
            csr = gen.convdiff3d_varying(14, dtype=dtype)
        elif name == "stencil7":
            csr = gen.stencil3d(24, 20, 18, 6.0, -1.25, -0.75, dtype=dtype)
        elif name == "stencil27":
            csr = gen.stencil3d_wide(24, 20, 18, 27, dtype=dtype)
        elif name == "stencil7-planes":
            csr = gen.stencil3d(*PLANES_GRID, 6.0, -1.25, -0.75, dtype=dtype)
        elif name == "stencil27-planes":
            csr = gen.stencil3d_wide(*PLANES_GRID, 27, dtype=dtype)
        else:
            assert name == "kat"
            csr, cols = kat_matrix(dtype), 4
        rows = len(csr[0]) - 1
        cols = rows if cols is None else cols
        rng = np.random.default_rng(len(csr[1]))
        _MATRICES[key] = (csr, cols, rng.uniform(-1, 1, cols).astype(dtype), rng.uniform(-1, 1, rows).astype(dtype))
    return _MATRICES[key]


ENCODING = {"masks": MASKS, "const": CONST, "codes": CODES, "ragged": CODES, "kat": MASKS, "convdiff": MASKS}
# (matrix, family) pairs whose smm_hip_csr_set_kernel is refused.  By smm_hip.h the PATTERN family refuses a matrix only when its entries
# use more than 65536 distinct column offsets: the widest matrix here (ragged, 300 x 9000) can hold 9299 at most, so nothing is refused --
# and whatever is observed must equal this list.
EXPECTED_REFUSALS = []


def carved_csr(csr, res):
    """(start, positions, values) in carved views; guards: start -> nnz, positions -> a valid column, values -> NaN"""
    start, pos, val = csr
    return put(start, res["start"], fill=len(pos)), put(pos, res["positions"], fill=0), put(val, res["values"])


def handle(smm, arrays, rows, cols, dtype):
    return smm.CSRMatrix.from_device(rows, cols, arrays[0], arrays[1], arrays[2], dtype)


def carved_handle(smm, name, dtype, res):
    csr, cols, _, _ = matrix(name, dtype)
    arrays = carved_csr(csr, res)
    saved = [snapshot(a) for a in arrays]
    A = handle(smm, arrays, len(csr[0]) - 1, cols, dtype)

    def check():
        check_all(zip(("start", "positions", "values"), arrays, saved), zip(("start", "positions", "values"), arrays))

    return A, arrays, check


_ALIGNED = {}


def aligned_handle(smm, name, dtype):
    """one handle per matrix over whole allocations: the aligned run of every case"""
    key = (name, np.dtype(dtype).name)
    if key not in _ALIGNED:
        csr, cols, _, _ = matrix(name, dtype)
        _ALIGNED[key] = handle(smm, [whole(a) for a in csr], len(csr[0]) - 1, cols, dtype)
    return _ALIGNED[key]


# (label, family, lanes, pattern_slots mode or None)
SPMV_CONFIGS = [("VECTOR/2", VECTOR, 2, None), ("STREAM/1", STREAM, 1, None), ("STREAM/4", STREAM, 4, None)] + [
    (f"PATTERN/{lanes} slots {mode}", PATTERN, lanes, mode) for lanes in (1, 2) for mode in (0, 1, 3)]
SPMV_CALLS = [("assign", OP_ASSIGN, False), ("add", OP_ADD, False), ("sub", OP_SUB, False), ("add in place", OP_ADD, True), ("sub in place", OP_SUB, True)]


def configure(A, family, lanes, mode):
    """True when the family took the matrix"""
    try:
        A.set_kernel(family, lanes)
    except _lib.SmmHipError:
        return False
    if mode is not None:
        A.pattern_slots(mode)
    return True


def spmv_call(A, op, inplace, x, lhs, out):
    """one spmv_dev; returns the tensor that holds the result"""
    if inplace:
        A.spmv_dev(op, lhs, x, lhs, stream())
        return lhs
    A.spmv_dev(op, lhs if op != OP_ASSIGN else None, x, out, stream())
    return out


_SPMV_ALIGNED = {}


def spmv_aligned(smm, name, dtype, config):
    """call label -> result of the aligned run at this configuration (None when the family refuses the matrix), and the kernel's name"""
    key = (name, np.dtype(dtype).name, config[0])
    if key not in _SPMV_ALIGNED:
        csr, cols, x, lhs = matrix(name, dtype)
        A = aligned_handle(smm, name, dtype)
        if not configure(A, *config[1:]):
            _SPMV_ALIGNED[key] = None
        else:
            res = {}
            for label, op, inplace in SPMV_CALLS:
                out = torch.full((A.rows,), 77.0, dtype=torch.from_numpy(x).dtype, device=DEV)
                res[label] = get(spmv_call(A, op, inplace, whole(x), whole(lhs), out))
                sync()
            _SPMV_ALIGNED[key] = (res, A.kernel_desc()[0], A.pattern_info()[0] if config[1] == PATTERN else None)
    return _SPMV_ALIGNED[key]


_ORACLE = {}


def spmv_oracle(oracle, name, dtype, op):
    key = (name, np.dtype(dtype).name, op)
    if key not in _ORACLE:
        csr, _, x, lhs = matrix(name, dtype)
        _ORACLE[key] = oracle.spmv(csr, op, lhs if op != OP_ASSIGN else None, x)
    return _ORACLE[key]


def check_spmv(smm, oracle, name, dtype, res, configs=SPMV_CONFIGS, names=None):
    csr, cols, x, lhs = matrix(name, dtype)
    A, arrays, check_matrix = carved_handle(smm, name, dtype, res)
    longest = int(np.diff(csr[0]).max())
    refused = []
    for config in configs:
        want = spmv_aligned(smm, name, dtype, config)
        took = configure(A, *config[1:])
        assert took == (want is not None), (name, config[0])
        if not took:
            refused.append((name, config[1]))
            continue
        want, kernel, encoding = want
        if names is not None:
            assert kernel == names[config[0]], (config[0], kernel)
        if encoding is not None:
            assert encoding == ENCODING[name], (name, encoding)
        for label, op, inplace in SPMV_CALLS:
            dx, dl = put(x, res["x"]), put(lhs, res["lhs"] if not inplace else res["out"])
            dout = put(np.full(A.rows, 77, dtype=dtype), res["out"])  # the sentinel
            sx, sl = snapshot(dx), snapshot(dl)
            got = get(spmv_call(A, op, inplace, dx, dl, dout))
            sync()
            what = f"{name} {config[0]} {label}"
            np.testing.assert_array_equal(got, want[label], err_msg=what)
            ref = spmv_oracle(oracle, name, dtype, op)
            if config[2] == 1 and longest <= 1021:  # one lane per row, no over-long row: the reference's order of additions
                np.testing.assert_array_equal(got, ref, err_msg=what + " (oracle)")
            else:
                assert np.all(np.abs(got.astype(np.float64) - ref) <= bound(csr, x, dtype, lhs if op != OP_ASSIGN else None)), what
            inputs = [("x", dx, sx)] + ([] if inplace else [("lhs", dl, sl)])
            if inplace:
                np.testing.assert_array_equal(get(dout), 77, err_msg=what)  # not an argument of the call
            check_all(inputs, [("x", dx), ("lhs", dl), ("out", dout)])
            check_matrix()
        assert A.kernel_desc()[0] == kernel, (name, config[0], A.kernel_desc()[0], kernel)
    assert sorted(set(refused)) == sorted(r for r in EXPECTED_REFUSALS if r[0] == name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", list(RESIDUES))
@pytest.mark.parametrize("name", ["kat", "masks", "const", "codes", "ragged"])
def test_spmv(smm, oracle, name, res, dtype):
    names = None
    if name == "masks":  # the three forms of the PATTERN family at two lanes per row (tile, slots, sweep at the shipped R)
        names = {c[0]: spmv_aligned(smm, name, dtype, c)[1] for c in SPMV_CONFIGS}
        names.update({"PATTERN/2 slots 0": TILE, "PATTERN/2 slots 1": SLOTS, "PATTERN/2 slots 3": SWEEP})
    check_spmv(smm, oracle, name, dtype, RESIDUES[res], names=names)


def test_nothing_else_is_refused(smm):
    """the list of refusals holds for every matrix of this file, the ones the other tests drive through one family only included"""
    seen = []
    for dtype in DTYPES:
        for name in ("kat", "masks", "const", "codes", "ragged", "convdiff", "stencil7", "stencil27", "stencil7-planes", "stencil27-planes"):
            A = aligned_handle(smm, name, dtype)
            for family in (VECTOR, STREAM, PATTERN):
                if not configure(A, family, 1, None):
                    seen.append((name, family))
    assert sorted(set(seen)) == sorted(EXPECTED_REFUSALS)


@pytest.fixture()
def march_on_small_grids(smm):
    host.set_march_min_rows(1, 1)  # matrices analysed from here on
    yield
    host.set_march_min_rows(-1, -1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", list(RESIDUES))
@pytest.mark.parametrize("name,allow_const,kernel", [
    # 24 x 20 x 18: one-plane mode (a plane of 480 rows is below the 8192 a march along planes needs)
    ("stencil7", True, "spmvPatternConstMarchKernel"), ("stencil7", False, "spmvPatternWaveKernel"), ("stencil27", True, "spmvPatternConstMarchKernel"),
    # 96 x 88 x 8: the march along planes -- constant diagonals, values read, and the three windows of the 27-point form
    ("stencil7-planes", True, "spmvPatternConstMarchKernel"), ("stencil7-planes", False, "spmvPatternMasksMarchKernel"),
    ("stencil27-planes", True, "spmvPatternConstMarch3Kernel")])
def test_spmv_march(smm, oracle, march_on_small_grids, name, allow_const, kernel, res, dtype):
    """the 2.5-D kernels on a 24 x 20 x 18 grid (one-plane mode) and on the smallest grid that marches along planes: every call bit for bit
    the oracle's and the aligned run's"""
    csr, cols, x, lhs = matrix(name, dtype)
    res = RESIDUES[res]
    A, arrays, check_matrix = carved_handle(smm, name, dtype, res)
    F = handle(smm, [whole(a) for a in csr], A.rows, cols, dtype)  # analysed under this test's threshold
    for M in (A, F):
        M.set_kernel(PATTERN, 1)
        M.pattern_allow_const(allow_const)
        assert M.kernel_desc()[0] == kernel, M.kernel_desc()
    for label, op, inplace in SPMV_CALLS:
        dx, dl = put(x, res["x"]), put(lhs, res["lhs"] if not inplace else res["out"])
        dout = put(np.full(A.rows, 77, dtype=dtype), res["out"])
        sx, sl = snapshot(dx), snapshot(dl)
        got = get(spmv_call(A, op, inplace, dx, dl, dout))
        want = get(spmv_call(F, op, inplace, whole(x), whole(lhs), torch.full_like(whole(lhs), 77.0)))
        sync()
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {label}")
        np.testing.assert_array_equal(got, spmv_oracle(oracle, name, dtype, op), err_msg=f"{name} {label} (oracle)")
        check_all([("x", dx, sx)] + ([] if inplace else [("lhs", dl, sl)]), [("x", dx), ("lhs", dl), ("out", dout)])
        check_matrix()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", ["R0", "values1", "out1", "all-different"])
@pytest.mark.parametrize("config", [c for c in SPMV_CONFIGS if c[0] in ("VECTOR/2", "STREAM/1", "STREAM/4", "PATTERN/2 slots 0", "PATTERN/2 slots 3")],
                         ids=lambda c: c[0])
def test_spmv_fused_dots(smm, config, res, dtype):
    """spmv_fused_dev with and without the in-launch finish: out bit for bit the aligned run's, the partial sums and the finishing buffer
    carved and guarded, the totals within the tolerance test_gpu_pattern_sweep uses between two kernels"""
    name = "masks"
    csr, cols, x, w1 = matrix(name, dtype)
    res = RESIDUES[res]
    A, arrays, check_matrix = carved_handle(smm, name, dtype, res)
    F = aligned_handle(smm, name, dtype)
    assert configure(A, *config[1:]) and configure(F, *config[1:])
    P, off = host.partials_count(), host.finish_totals_offset()
    tol = 1e-4 if dtype == np.float32 else 1e-11
    for mode in (1, 2):
        cnt = 2 if mode == 2 else 1
        for finish in (False, True):
            runs = []
            for M, place in ((F, whole), (A, None)):
                if place is None:
                    dx, dw = put(x, res["x"]), put(w1, res["lhs"])
                    dout = put(np.full(A.rows, 77, dtype=dtype), res["out"])
                    dpart = put(np.zeros(host.finish_len() if finish else 2 * P, dtype=dtype), res["lhs"])
                else:
                    dx, dw, dout = whole(x), whole(w1), whole(np.full(A.rows, 77, dtype=dtype))
                    dpart = whole(np.zeros(host.finish_len() if finish else 2 * P, dtype=dtype))
                sx, sw = snapshot(dx), snapshot(dw)
                M.spmv_fused_dev(OP_ASSIGN, None, dx, dout, mode, dw, dpart, stream(), finish=finish)
                sync()
                parts = get(dpart).astype(np.float64)
                totals = parts[off:off + cnt] if finish else parts.reshape(2, P).sum(axis=1)[:cnt]
                runs.append((get(dout), totals))
                if place is None:
                    check_all([("x", dx, sx), ("w1", dw, sw)], [("x", dx), ("w1", dw), ("out", dout), ("partials", dpart)])
                    check_matrix()
            np.testing.assert_array_equal(runs[1][0], runs[0][0], err_msg=f"{config[0]} mode {mode} finish {finish}")
            np.testing.assert_allclose(runs[1][1], runs[0][1], rtol=tol, err_msg=f"{config[0]} mode {mode} finish {finish}")


# ---- SpMM ---------------------------------------------------------------------------------------------------------------------------
_SPMM_ALIGNED = {}


def blocks(name, dtype, k):
    csr, cols, _, _ = matrix(name, dtype)
    rng = np.random.default_rng(100 + k)
    return rng.uniform(-1, 1, (cols, k)).astype(dtype), rng.uniform(-1, 1, (len(csr[0]) - 1, k)).astype(dtype)


def spmm_aligned(smm, name, dtype, k):
    key = (name, np.dtype(dtype).name, k)
    if key not in _SPMM_ALIGNED:
        csr, cols, _, _ = matrix(name, dtype)
        A = handle(smm, [whole(a) for a in csr], len(csr[0]) - 1, cols, dtype)  # (a fresh one: no SpMV of another test has cut its tile table)
        X, L = blocks(name, dtype, k)
        res = {}
        for op in (OP_ASSIGN, OP_ADD, OP_SUB):
            out = whole(np.full(L.shape, 77, dtype=dtype))
            A.spmm_dev(op, k, whole(L) if op != OP_ASSIGN else None, whole(X), out, stream())
            sync()
            res[op] = get(out)
        _SPMM_ALIGNED[key] = res
    return _SPMM_ALIGNED[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_res", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 2)], ids=lambda r: "x%d-lhs%d-out%d" % r)
@pytest.mark.parametrize("matrix_res", list(MATRIX_RESIDUES))
@pytest.mark.parametrize("name", ["masks", "ragged"])
def test_spmm(smm, oracle, name, matrix_res, block_res, dtype):
    """spmm_dev at k = 1, 3, 4, 8 with X, Lhs and Out carved: every column bit for bit the aligned run's, in place equals out of place"""
    csr, cols, _, _ = matrix(name, dtype)
    A, arrays, check_matrix = carved_handle(smm, name, dtype, MATRIX_RESIDUES[matrix_res])
    rx, rl, ro = block_res
    for k in (1, 3, 4, 8):
        X, L = blocks(name, dtype, k)
        want = spmm_aligned(smm, name, dtype, k)
        for op in (OP_ASSIGN, OP_ADD, OP_SUB):
            dX, dL, dO = put(X, rx), put(L, rl), put(np.full(L.shape, 77, dtype=dtype), ro)
            sX, sL = snapshot(dX), snapshot(dL)
            A.spmm_dev(op, k, dL if op != OP_ASSIGN else None, dX, dO, stream())
            sync()
            np.testing.assert_array_equal(get(dO), want[op], err_msg=f"{name} k {k} op {op}")
            check_all([("X", dX, sX), ("Lhs", dL, sL)], [("X", dX), ("Lhs", dL), ("Out", dO)])
            if op != OP_ASSIGN:  # in place: Out is Lhs
                dI = put(L, ro)
                A.spmm_dev(op, k, dI, dX, dI, stream())
                sync()
                np.testing.assert_array_equal(get(dI), want[op], err_msg=f"{name} k {k} op {op} in place")
                check_all([("X", dX, sX)], [("X", dX), ("Out", dI)])
            check_matrix()
        if k == 3 and int(np.diff(csr[0]).max()) <= 1021:  # (one column against the oracle: the aligned run is not its own reference)
            ref = oracle.spmv(csr, OP_SUB, np.ascontiguousarray(L[:, 1]), np.ascontiguousarray(X[:, 1]))
            assert np.all(np.abs(want[OP_SUB][:, 1].astype(np.float64) - ref) <= bound(csr, np.ascontiguousarray(X[:, 1]), dtype, np.ascontiguousarray(L[:, 1])))


# ---- BLAS-1 -------------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 3, 4, 5, 1023, 1025)


def ptr(view):
    return address(view)  # (torch reports no address for an empty view)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ra,rb,rr", [(0, 0, 0), (1, 1, 0), (1, 0, 0), (0, 1, 1), (2, 3, 1), (3, 3, 3), (0, 2, 2)])
def test_dot(smm, ra, rb, rr, dtype):
    """dot_dev with a and b at equal and at different residues, the one-element result carved and guarded as well"""
    eps = np.finfo(dtype).eps
    for n in LENGTHS:
        rng = np.random.default_rng(n)
        a, b = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
        da, db = put(a, ra), put(b, rb)
        sa, sb = snapshot(da), snapshot(db)
        got = []
        for _ in range(2):
            dr = put(np.full(1, 77, dtype=dtype), rr)
            host.dot_dev(n, ptr(da), ptr(db), dr, dtype, stream())
            sync()
            got.append(get(dr)[0])
            check_all([("a", da, sa), ("b", db, sb)], [("a", da), ("b", db), ("result", dr)])
        exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
        tol = 8 * eps * float(np.abs(a.astype(np.float64) * b).sum()) * max(1.0, np.log2(max(n, 2)))  # test_gpu_property.test_dot_any_length
        assert abs(float(got[0]) - exact) <= tol + 1e-300, (n, got[0], exact)
        assert got[0].tobytes() == got[1].tobytes(), n  # bitwise reproducible call to call
    # a . a on one view
    a = np.random.default_rng(9).uniform(-1, 1, 1025).astype(dtype)
    da, dr = put(a, ra), put(np.full(1, 77, dtype=dtype), rr)
    host.dot_dev(1025, da, da, dr, dtype, stream())
    sync()
    exact = float(np.dot(a.astype(np.float64), a.astype(np.float64)))
    assert abs(float(get(dr)[0]) - exact) <= 8 * eps * exact * np.log2(1025)
    check_all([], [("a", da), ("result", dr)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rx,ry,ro", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 1, 2), (2, 2, 3)])
def test_axpy(smm, rx, ry, ro, dtype):
    """axpy_dev: out = a * x + y in two roundings like numpy, out of place and with out aliasing y or x"""
    alpha = 0.625
    for n in LENGTHS:
        rng = np.random.default_rng(n + 50)
        x, y = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, n).astype(dtype)
        want = dtype(alpha) * x + y
        dx, dy, do = put(x, rx), put(y, ry), put(np.full(n, 77, dtype=dtype), ro)
        sx, sy = snapshot(dx), snapshot(dy)
        host.axpy_dev(n, alpha, ptr(dx), ptr(dy), ptr(do), dtype, stream())
        sync()
        np.testing.assert_array_equal(get(do), want, err_msg=f"n {n}")
        check_all([("x", dx, sx), ("y", dy, sy)], [("x", dx), ("y", dy), ("out", do)])
        host.axpy_dev(n, alpha, ptr(dx), ptr(dy), ptr(dy), dtype, stream())  # out is y
        sync()
        np.testing.assert_array_equal(get(dy), want, err_msg=f"n {n} out = y")
        check_all([("x", dx, sx)], [("x", dx), ("y", dy)])
        dy2 = put(y, ry)
        host.axpy_dev(n, alpha, ptr(dx), ptr(dy2), ptr(dx), dtype, stream())  # out is x
        sync()
        np.testing.assert_array_equal(get(dx), want, err_msg=f"n {n} out = x")
        check_all([("y", dy2, sy)], [("x", dx), ("y", dy2)])


# ---- solvers ------------------------------------------------------------------------------------------------------------------------
VECTOR_RESIDUES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 2)]  # b, x0, x


def rhs(oracle, name, dtype):
    csr, _, _, _ = matrix(name, dtype)
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, len(csr[0]) - 1).astype(dtype)
    return oracle.spmv(csr, OP_ASSIGN, None, x_true)


_SENS = {}


def bicgstab_allowed(oracle, name, dtype, b, it, ref):
    key = (name, np.dtype(dtype).name, it, b.tobytes()[:64])
    if key not in _SENS:
        _SENS[key] = bicgstab_sensitivity(oracle, matrix(name, dtype)[0], b, it, PRECOND_NONE, None)
    return max(RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))), 4 * _SENS[key])


_SOLVE_REF = {}


def solve_oracle(oracle, kind, name, dtype, b, it):
    key = (kind, name, np.dtype(dtype).name, it, b.tobytes()[:64])
    if key not in _SOLVE_REF:
        csr = matrix(name, dtype)[0]
        zero = np.zeros(len(b), dtype=dtype)
        _SOLVE_REF[key] = oracle.cg(csr, b, zero, it, 0.0)[:3] if kind == "cg" else oracle.bicgstab(csr, b, zero, it, 1e-30)[:3]
    return _SOLVE_REF[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vec_res", VECTOR_RESIDUES, ids=lambda r: "b%d-x0%d-x%d" % r)
@pytest.mark.parametrize("matrix_res", list(MATRIX_RESIDUES))
@pytest.mark.parametrize("name", ["const", "masks"])
def test_cg(smm, oracle, name, matrix_res, vec_res, dtype):
    A, arrays, check_matrix = carved_handle(smm, name, dtype, MATRIX_RESIDUES[matrix_res])
    F = aligned_handle(smm, name, dtype)
    F.set_kernel(0, 0)
    b = rhs(oracle, name, dtype)
    zero = np.zeros(A.rows, dtype=dtype)
    for it in (1, 3, 10):
        db, dx0, dx = put(b, vec_res[0]), put(zero, vec_res[1]), put(np.full(A.rows, 123, dtype=dtype), vec_res[2])
        sb, sx0 = snapshot(db), snapshot(dx0)
        got = host.cg_dev(A, db, dx0, dx, it, 0.0, None, stream())
        fx = whole(np.full(A.rows, 123, dtype=dtype))
        want = host.cg_dev(F, whole(b), whole(zero), fx, it, 0.0, None, stream())
        sync()
        st_o, x_o, it_o = solve_oracle(oracle, "cg", name, dtype, b, it)
        assert int(got[0]) == int(want[0]) == st_o == 2 and got[1] == want[1] == it_o == it
        assert close(get(dx), x_o.astype(np.float64), dtype), (name, it)
        check_all([("b", db, sb), ("x0", dx0, sx0)], [("b", db), ("x0", dx0), ("x", dx)])
        check_matrix()
    # x is x0, as the reference's tests call it
    db, dx = put(b, vec_res[0]), put(zero, vec_res[2])
    got = host.cg_dev(A, db, dx, dx, 3, 0.0, None, stream())
    sync()
    assert int(got[0]) == 2 and got[1] == 3 and close(get(dx), solve_oracle(oracle, "cg", name, dtype, b, 3)[1].astype(np.float64), dtype)
    check_all([], [("b", db), ("x", dx)])
    check_matrix()


@pytest.fixture()
def resident_modes(smm):
    before = host.bicgstab_resident(-1)
    yield
    host.bicgstab_resident(before)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [host.CG_RESIDENT_OFF, host.CG_RESIDENT_REQUIRE], ids=["loop", "single-launch"])
@pytest.mark.parametrize("vec_res", [(0, 0), (1, 0), (0, 1), (3, 2)], ids=lambda r: "b%d-x%d" % r)
@pytest.mark.parametrize("matrix_res", list(MATRIX_RESIDUES))
def test_bicgstab(smm, oracle, resident_modes, matrix_res, vec_res, mode, dtype):
    """bicgstab_dev as the loop of launches and as the single launch (PATTERN family, convdiff3d_varying(14))"""
    name = "convdiff"
    A, arrays, check_matrix = carved_handle(smm, name, dtype, MATRIX_RESIDUES[matrix_res])
    csr = matrix(name, dtype)[0]
    F = handle(smm, [whole(a) for a in csr], A.rows, A.rows, dtype)
    for M in (A, F):
        M.set_kernel(PATTERN, 1)
    host.bicgstab_resident(mode)
    b = rhs(oracle, name, dtype)
    zero = np.zeros(A.rows, dtype=dtype)
    for it in (1, 3, 10):
        db, dx = put(b, vec_res[0]), put(zero, vec_res[1])
        sb = snapshot(db)
        got = host.bicgstab_dev(A, db, dx, it, 1e-30, None, stream())
        want = host.bicgstab_dev(F, whole(b), whole(zero), it, 1e-30, None, stream())
        sync()
        st_o, x_o, it_o = solve_oracle(oracle, "bicgstab", name, dtype, b, it)
        assert int(got[0]) == int(want[0]) == st_o == 0 and got[1] == want[1] == it_o == it
        x_o = x_o.astype(np.float64)
        err = float(np.max(np.abs(get(dx).astype(np.float64) - x_o)))
        assert err <= bicgstab_allowed(oracle, name, dtype, b, it, x_o), (it, err)
        check_all([("b", db, sb)], [("b", db), ("x", dx)])
        check_matrix()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vec_res", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 2)], ids=lambda r: "b%d-x0%d-x%d" % r)
@pytest.mark.parametrize("matrix_res", list(MATRIX_RESIDUES))
@pytest.mark.parametrize("k", [3, 4])
def test_batched_solvers(smm, oracle, k, matrix_res, vec_res, dtype):
    """bicgstab_batch_dev (convdiff) and cg_batch_dev (const) with the blocks carved: every column against the oracle's solve of it"""
    for solver, name in (("bicgstab", "convdiff"), ("cg", "const")):
        A, arrays, check_matrix = carved_handle(smm, name, dtype, MATRIX_RESIDUES[matrix_res])
        F = aligned_handle(smm, name, dtype)
        F.set_kernel(0, 0)
        rows = A.rows
        base = rhs(oracle, name, dtype)
        B = np.stack([base * dtype(s) for s in (1.0, 0.5, -2.0, 0.25)[:k]], axis=1).astype(dtype)
        for it in (1, 3, 10):
            dB, dX0 = put(B, vec_res[0]), put(np.zeros((rows, k), dtype=dtype), vec_res[1])
            dX = put(np.full((rows, k), 123, dtype=dtype), vec_res[2])
            sB, sX0 = snapshot(dB), snapshot(dX0)
            fX = whole(np.zeros((rows, k), dtype=dtype))
            if solver == "bicgstab":
                got = host.bicgstab_batch_dev(A, k, dB, dX0, it, 1e-30, None, stream())  # X0 holds the guesses and receives the results
                want = host.bicgstab_batch_dev(F, k, whole(B), fX, it, 1e-30, None, stream())
                result, inputs, status = dX0, [("B", dB, sB)], 0
            else:
                got = host.cg_batch_dev(A, k, dB, dX0, dX, it, 0.0, stream())
                want = host.cg_batch_dev(F, k, whole(B), whole(np.zeros((rows, k), dtype=dtype)), fX, it, 0.0, stream())
                result, inputs, status = dX, [("B", dB, sB), ("X0", dX0, sX0)], 2
            sync()
            assert [int(s) for s in got[0]] == [int(s) for s in want[0]] == [status] * k
            assert list(got[1]) == list(want[1]) == [it] * k
            X = get(result)
            for j in range(k):
                b = np.ascontiguousarray(B[:, j])
                st_o, x_o, it_o = solve_oracle(oracle, solver, name, dtype, b, it)
                assert st_o == status and it_o == it
                x_o = x_o.astype(np.float64)
                if solver == "cg":
                    assert close(X[:, j], x_o, dtype), (k, it, j)
                else:
                    err = float(np.max(np.abs(X[:, j].astype(np.float64) - x_o)))
                    assert err <= bicgstab_allowed(oracle, name, dtype, b, it, x_o), (k, it, j, err)
            check_all(inputs, [("B", dB), ("X0", dX0), ("X", dX)])
            check_matrix()


# ---- preconditioners ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vec_res", [(0, 0), (1, 0), (0, 1), (3, 2)], ids=lambda r: "rhs%d-x%d" % r)
@pytest.mark.parametrize("kind", ["JACOBI", "SYMMETRIC_GAUS_SEIDEL", "ILU0", "IC0", "BLOCK_ILU0", "BLOCK_SGS"])
def test_preconditioners(smm, kind, vec_res, dtype):
    """apply_dev (and apply_spmv_dev of the BLOCK_ kinds) of a preconditioner of a matrix made from carved arrays, rhs and x carved: the
    aligned run's bits"""
    name = "const"
    P = smm.SolverPreconditioner
    _, _, _, r = matrix(name, dtype)
    for matrix_res in MATRIX_RESIDUES.values():
        A, arrays, check_matrix = carved_handle(smm, name, dtype, matrix_res)
        F = aligned_handle(smm, name, dtype)
        M, N = A.getPreconditioner(P[kind]), F.getPreconditioner(P[kind])
        calls = ["apply_dev"] + (["apply_spmv_dev"] if kind.startswith("BLOCK_") else [])
        for call in calls:
            dr, dx = put(r, vec_res[0]), put(np.full(A.rows, 77, dtype=dtype), vec_res[1])
            sr = snapshot(dr)
            fx = whole(np.full(A.rows, 77, dtype=dtype))
            getattr(M, call)(dr, dx, stream())
            getattr(N, call)(whole(r), fx, stream())
            M.take_error(stream())
            N.take_error(stream())
            got = get(dx)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(got, get(fx), err_msg=f"{kind} {call}")
            check_all([("rhs", dr, sr)], [("rhs", dr), ("x", dx)])
            check_matrix()
        M.close()
        N.close()


# ---- edits on borrowed arrays -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("values_res,other_res", [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2)])
def test_edits_on_borrowed_arrays(smm, oracle, values_res, other_res, dtype):
    """scale / axpy / zero / update_entries_dev / set_values_dev / values_changed on a from_device handle whose values are a view at
    element alignment (the one-element path of the update kernels).  After each edit the CALLER's array holds the numpy model of
    test_gpu_csr_update.py, the guards are intact, and the SpMV is that of a fresh aligned handle made from the edited arrays."""
    name = "masks"
    csr, cols, x, _ = matrix(name, dtype)
    n = len(csr[0]) - 1
    rng = np.random.default_rng(21)
    res = {**R0, "values": values_res}
    A, (d_start, d_pos, d_val), _ = carved_handle(smm, name, dtype, res)
    other = rng.uniform(-1, 1, csr[2].size).astype(dtype)
    o_arrays = carved_csr((csr[0], csr[1], other), {**R0, "values": other_res})
    B = handle(smm, o_arrays, n, n, dtype)
    s_other = snapshot(o_arrays[2])
    s_pat = [snapshot(d_start), snapshot(d_pos)]
    dx = whole(x)
    model = csr[2].copy()

    def check(what):
        sync()
        np.testing.assert_array_equal(get(d_val), model, err_msg=what)
        check_all([("start", d_start, s_pat[0]), ("positions", d_pos, s_pat[1]), ("other", o_arrays[2], s_other)],
                  [("start", d_start), ("positions", d_pos), ("values", d_val), ("other", o_arrays[2])])
        F = handle(smm, [whole(csr[0]), whole(csr[1]), whole(model)], n, n, dtype)
        for family, lanes, mode in ((STREAM, 1, None), (PATTERN, 2, 3)):
            assert configure(A, family, lanes, mode) and configure(F, family, lanes, mode)
            ya, yf = torch.full_like(dx, 77.0), torch.full_like(dx, 77.0)
            A.spmv_dev(OP_ASSIGN, None, dx, ya, stream())
            F.spmv_dev(OP_ASSIGN, None, dx, yf, stream())
            sync()
            np.testing.assert_array_equal(get(ya), get(yf), err_msg=f"{what} {family}/{lanes}")
            if lanes == 1:
                np.testing.assert_array_equal(get(ya), oracle.spmv((csr[0], csr[1], model), OP_ASSIGN, None, x), err_msg=what)
        assert A.kernel_desc()[0] == SWEEP or not model.any()  # (all zeros: constant diagonals)
        F.close()

    check("as created")
    A.scale(1.7, stream())
    model = model * dtype(1.7)
    check("scale")
    A.axpy(0.25, B, stream())
    model = model + dtype(0.25) * other
    check("axpy")
    rr, cc, bv = batch(csr, rng, dtype)
    for add in (False, True):
        d_rr, d_cc, d_bv = put(rr, 1), put(cc, 2), put(bv, 3)
        d_found = put(np.full(len(rr), 9, dtype=np.uint8), 1)
        saved = [snapshot(d_rr), snapshot(d_cc), snapshot(d_bv)]
        A.update_entries_dev(len(rr), d_rr, d_cc, d_bv, add, d_found, stream())
        model = apply_entries((csr[0], csr[1], model), rr, cc, bv, add)
        check(f"update_entries add={add}")
        found = np.array([entry_index(csr, int(r), int(c)) >= 0 for r, c in zip(rr, cc)])
        np.testing.assert_array_equal(get(d_found).astype(bool), found)
        check_all(zip(("rows", "cols", "vals"), (d_rr, d_cc, d_bv), saved), [("rows", d_rr), ("cols", d_cc), ("vals", d_bv), ("found", d_found)])
    newv = rng.uniform(-1, 1, model.size).astype(dtype)
    d_new = put(newv, other_res)
    s_new = snapshot(d_new)
    A.set_values_dev(d_new, stream())
    model = newv.copy()
    check("set_values_dev")
    check_all([("source", d_new, s_new)], [("source", d_new)])
    mine = rng.uniform(-1, 1, model.size).astype(dtype)
    d_val.copy_(torch.from_numpy(mine))  # the caller writes its own array
    A.values_changed(stream())
    model = mine.copy()
    check("values_changed")
    A.zero(stream())
    model = np.zeros_like(model)
    check("zero")


# ---- assembly -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rr,rc,rv", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)])
def test_assembly(smm, rr, rc, rv, dtype):
    """AssemblyPlan.from_device on carved triplet indices, assemble_dev / refill_dev (SET and ADD) from carved values: the arrays of the
    numpy model of test_assembly_cpu.py"""
    csr, cols, _, _ = matrix("masks", dtype)
    rows = len(csr[0]) - 1
    rng = np.random.default_rng(31)
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(csr[0]))
    extra = rng.integers(0, len(r), 997)  # repeated pairs: they add up in list order
    ri, ci = np.concatenate([r, r[extra]]), np.concatenate([csr[1], csr[1][extra]])
    order = rng.permutation(len(ri))
    ri, ci = ri[order].astype(np.int32), ci[order].astype(np.int32)
    v1, v2 = rng.uniform(-1, 1, len(ri)).astype(dtype), rng.uniform(-1, 1, len(ri)).astype(dtype)
    assert len(ri) % 4  # no whole number of 16-byte pieces
    d_r, d_c = put(ri, rr, fill=0), put(ci, rc, fill=0)
    d_v1, d_v2 = put(v1, rv), put(v2, rv)
    saved = [snapshot(t) for t in (d_r, d_c, d_v1, d_v2)]
    plan = smm.AssemblyPlan.from_device(rows, cols, len(ri), d_r, d_c, stream())
    m_start, m_pos, m_val, first, longest = assemble_model(rows, cols, ri, ci, v1)
    assert plan.nnz == len(m_pos) and plan.longest_run == longest
    start, pos = plan.pattern()
    np.testing.assert_array_equal(start, m_start)
    np.testing.assert_array_equal(pos, m_pos)
    A = plan.assemble_dev(d_v1, dtype, stream())
    sync()
    np.testing.assert_array_equal(A.get_values(), m_val)
    assert A.first_active_start == first
    plan.refill_dev(A, d_v2, False, stream())
    sync()
    m2 = assemble_model(rows, cols, ri, ci, v2)[2]
    np.testing.assert_array_equal(A.get_values(), m2)
    plan.refill_dev(A, d_v1, True, stream())
    sync()
    want = m2 + m_val  # ADD: values[k] + assembled[k], one rounding
    np.testing.assert_array_equal(A.get_values(), want)
    check_all(zip(("rows", "cols", "values", "values 2"), (d_r, d_c, d_v1, d_v2), saved), zip(("rows", "cols", "values", "values 2"), (d_r, d_c, d_v1, d_v2)))
    plan.close()


# ---- generators ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res", ["R0", "start1", "positions1", "values1", "all-different"])
def test_generators(smm, res, dtype):
    """the device generators write start[], positions[] and values[] into carved arrays: the host generators' contents, not one element
    before or after"""
    res = RESIDUES[res]
    n, k, seed, mo = 3001, 30, 0x5EED + 3001, 2000
    banded = gen.banded_random_spd(n, k, seed, mo, dtype=dtype)
    begin, end = 500, 1777  # a row range that ends inside the matrix
    lo, hi = int(banded[0][begin]), int(banded[0][end])
    assert host.gen_banded_row_start(n, k, seed, mo, begin) == lo and host.gen_banded_row_start(n, k, seed, mo, end) == hi
    cases = [
        ("poisson2d", gen.poisson2d(33, 31, dtype=dtype), lambda s, p, v: host.gen_poisson2d_dev(33, 31, s, p, v, dtype, stream())),
        ("stencil3d", gen.stencil3d(12, 10, 9, 6.0, -1.3, -0.7, dtype=dtype), lambda s, p, v: host.gen_stencil3d_dev(12, 10, 9, 6.0, -1.3, -0.7, s, p, v, dtype, stream())),
        ("banded", banded, lambda s, p, v: host.gen_banded_dev(n, k, seed, mo, s, p, v, dtype, stream())),
        ("banded rows", ((banded[0][begin:end + 1] - lo).astype(np.int32), banded[1][lo:hi], banded[2][lo:hi]),
         lambda s, p, v: host.gen_banded_rows_dev(n, k, seed, mo, 1.0, begin, end, s, p, v, dtype, stream())),
    ]
    for name, want, call in cases:
        nnz = len(want[1])
        d_start = carve(len(want[0]), np.int32, fit(res["start"], np.int32), fill=nnz, device=DEV)
        d_pos = carve(nnz, np.int32, fit(res["positions"], np.int32), fill=0, device=DEV)
        d_val = carve(nnz, dtype, fit(res["values"], dtype), device=DEV)
        for t in (d_start, d_pos, d_val):
            t.fill_(-5)  # the sentinel; the guards keep a valid row end / column / NaN
        call(d_start, d_pos, d_val)
        sync()
        for what, w, g in zip(("start", "positions", "values"), want, (d_start, d_pos, d_val)):
            np.testing.assert_array_equal(get(g), w, err_msg=f"{name} {what}")
            assert_guards_intact(g, f"{name} {what}")
