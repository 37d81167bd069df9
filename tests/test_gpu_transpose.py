"""The device transpose (csrc/smm_transpose.hip) through the C ABI: smm_hip_csr_transpose_create / _refresh_* and
smm_hip_csr_is_symmetric.  The reference throughout is the host transpose by a stable argsort (tests/bicg_restatement.py); every
comparison is assert_array_equal on start[], positions[] and the value BITS (viewed as unsigned integers)."""
import numpy as np
import pytest
import torch
from bicg_restatement import transpose as host_transpose
from conftest import kat_matrix
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from test_gpu_spmv import CONFIGS, bound
from test_oracle import gen_matrices

from oracle.oracle import OP_ADD, OP_ASSIGN, OP_SUB
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
PATTERN = 3
MASKS, CONST = 1, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def column0_hit_by_every_row(dtype):
    """300 x 64: every row holds column 0 (a row of the transpose longer than a wavefront) and up to 5 further columns"""
    rng = np.random.default_rng(5)
    rows, cols = 300, 64
    lens = rng.integers(0, 6, size=rows)
    start = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens + 1, out=start[1:])
    pos = np.concatenate([np.concatenate([[0], np.sort(rng.choice(np.arange(1, cols), size=n, replace=False))]) for n in lens]).astype(np.int32)
    return (start, pos, rng.uniform(-1, 1, start[-1]).astype(dtype)), cols


def shapes(dtype):
    """name -> (csr, cols)"""
    m = gen_matrices(dtype)
    special = gen.random_rows(40, 40, 1, 6, seed=9, dtype=dtype)
    special[2][0] = -0.0
    bits(special[2])[1] = 0x7FC12345 if dtype == np.float32 else 0x7FF8000000ABCDEF  # a quiet NaN with a payload
    bits(special[2])[2] = 0xFFA00001 if dtype == np.float32 else 0xFFF4000000000001  # a signalling one, sign set
    return {
        "kat_5x4": (kat_matrix(dtype), 4),
        "ragged_300": (m["ragged_300"], 300),
        "rect_257x130": (gen.random_rows(257, 130, 0, 40, seed=3, dtype=dtype, empty_every=11), 130),
        "col0_300x64": column0_hit_by_every_row(dtype),
        "convdiff3d_12": (m["convdiff3d_12"], 12 ** 3),
        "no_entries_7x5": ((np.zeros(8, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)), 5),
        "rows0_0x6": ((np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)), 6),
        "cols0_6x0": ((np.zeros(7, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)), 0),
        "negative_zero_and_nans": (special, 40),
    }


def make(smm, csr, cols):
    return smm.CSRMatrix(len(csr[0]) - 1, cols, *csr)


def arrays(M):
    start, pos = M.get_pattern()
    return start, pos, M.get_values()


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what} start")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what} positions")
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg=f"{what} value bits")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_transpose_equals_the_stable_argsort(smm, dtype):
    for name, (csr, cols) in shapes(dtype).items():
        rows = len(csr[0]) - 1
        want = host_transpose(csr, cols)
        A = make(smm, csr, cols)
        T = A.transpose()
        assert (T.rows, T.cols, T.nnz, T.dtype) == (cols, rows, A.nnz, np.dtype(dtype)), name
        assert_same(arrays(T), want, name)
        F = make(smm, want, rows)  # what smm_hip_csr_create_* reports for the same three arrays
        assert T.first_active_start == F.first_active_start, name
        assert T.get_kernel() == F.get_kernel(), name
        assert_same(arrays(T.transpose()), (csr[0], csr[1][:A.nnz], csr[2][:A.nnz]), name + " twice")
        A.close()  # the transpose does not depend on its source's lifetime
        assert_same(arrays(T), want, name + " after the source is gone")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["kat_5x4", "ragged_300", "rect_257x130", "col0_300x64", "convdiff3d_12"])
def test_spmv_on_the_built_transpose(smm, oracle, dtype, name):
    """rMult / rMultAdd / rMultSub on the built handle against oracle.spmv on the host transpose, under every family set_kernel accepts
    for the matrix: the oracle's bits with one lane per row and on AUTO's choice for these short rows, the re-ordering bound otherwise"""
    csr, cols = shapes(dtype)[name]
    rows = len(csr[0]) - 1
    t_csr = host_transpose(csr, cols)
    T = make(smm, csr, cols).transpose()
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, rows).astype(dtype)
    lhs = rng.uniform(-1, 1, cols).astype(dtype)
    want = {op: oracle.spmv(t_csr, op, lhs if op else None, x) for op in (OP_ASSIGN, OP_ADD, OP_SUB)}
    ran = 0
    for family, lanes in CONFIGS + [(PATTERN, 1), (0, 0)]:
        try:
            T.set_kernel(family, lanes)
        except smm.SmmHipError:
            assert family == PATTERN, (family, lanes)  # (a matrix without a pattern is refused; the CSR families never are)
            continue
        ran += 1
        for op, ref in want.items():
            out = np.zeros(cols, dtype=dtype)
            {OP_ASSIGN: lambda: T.rMult(x, out), OP_ADD: lambda: T.rMultAdd(lhs, x, out), OP_SUB: lambda: T.rMultSub(lhs, x, out)}[op]()
            if lanes == 1:
                np.testing.assert_array_equal(bits(out), bits(ref), err_msg=f"{name} family {family} op {op}")
            else:
                assert np.all(np.abs(out.astype(np.float64) - ref) <= bound(t_csr, x, dtype, lhs if op else None)), (name, family, lanes, op)
    assert ran >= len(CONFIGS) + 1


def test_auto_adopts_the_pattern_family_for_a_large_transpose(smm, oracle):
    """just over 2^20 stored entries, fewer than 64 per row: left on AUTO, the transpose is analysed and moved to the PATTERN family by
    the first solver that plans 16 passes or more with it -- here BiCG, which runs it as `at` and leaves after its first pass (eps =
    1e30) --, exactly as a handle made by smm_hip_csr_create_* from the same arrays is"""
    dtype = np.float32
    csr = gen.banded_random_spd(22000, k=49, seed=0x5EED, max_offset=1 << 12, dtype=dtype)
    n = len(csr[0]) - 1
    assert len(csr[1]) > 1 << 20 and len(csr[1]) <= 64 * n
    # the matrix is symmetric; make the transpose differ from it in its values
    csr[2][:] = (csr[2] * np.linspace(0.5, 1.5, len(csr[2]))).astype(dtype)
    want = host_transpose(csr)
    A = make(smm, csr, n)
    T = A.transpose()
    F = make(smm, want, n)  # the same arrays through smm_hip_csr_create_*
    assert_same(arrays(T), want)
    b = gen.row_sums(csr[0], csr[2])
    for at in (T, F):
        info = {}
        smm.BiCG(A, b.copy(), np.zeros(n, dtype=dtype), 16, 1e30, at=at, info=info)
        assert info["iterations"] <= 1
    family, lanes = T.get_kernel()
    encoding, offsets = T.pattern_info()
    print("AUTO ->", family, lanes, T.kernel_desc()[0], "encoding", encoding, "offsets", offsets)
    assert family == PATTERN and encoding != 0
    assert F.get_kernel() == (family, lanes) and F.pattern_info() == (encoding, offsets)
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(dtype)
    out, out_f = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    T.rMult(x, out)
    F.rMult(x, out_f)
    np.testing.assert_array_equal(bits(out), bits(out_f))
    ref = oracle.spmv(want, OP_ASSIGN, None, x)
    if lanes == 1:
        np.testing.assert_array_equal(bits(out), bits(ref))
    else:
        assert np.all(np.abs(out.astype(np.float64) - ref) <= bound(want, x, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_refresh_follows_every_kind_of_edit(smm, dtype):
    csr = gen_matrices(dtype)["ragged_300"]
    A = make(smm, csr, 300)
    T = A.transpose()
    x = np.ones(300, dtype=dtype)
    out = np.zeros(300, dtype=dtype)
    T.rMult(x, out)  # (the first SpMV cuts the tile table)
    tile, pat = T.tile_info(), T.pattern_info()
    rng = np.random.default_rng(3)
    row_of = np.repeat(np.arange(300), np.diff(csr[0]))
    pick = rng.integers(0, len(csr[1]), size=12)
    pick[3] = pick[7] = pick[0]  # the same entry three times
    edits = (
        ("scale", lambda: A.scale(1.75)),
        ("update_entries with duplicates", lambda: A.update_entries(row_of[pick], csr[1][pick], rng.uniform(-1, 1, 12).astype(dtype), add=True)),
        ("set_values", lambda: A.set_values(rng.uniform(-2, 2, len(csr[1])).astype(dtype))),
    )
    for name, edit in edits:
        before = T.get_values()
        edit()
        np.testing.assert_array_equal(bits(T.get_values()), bits(before), err_msg=name)  # nothing reaches the transpose by itself
        T.transpose_refresh(A)
        fresh = A.transpose()
        assert_same(arrays(T), arrays(fresh), name)
        assert_same(arrays(T), host_transpose((csr[0], csr[1], A.get_values())), name + " (host)")
        assert T.tile_info() == tile and T.pattern_info() == pat, name
    # another handle over the same pattern is accepted too (one device pass, once), and a second time from the cached verdict
    B = make(smm, (csr[0], csr[1], rng.uniform(-1, 1, len(csr[1])).astype(dtype)), 300)
    for _ in range(2):
        T.transpose_refresh(B)
        assert_same(arrays(T), host_transpose((csr[0], csr[1], B.get_values())), "another handle")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_refresh_and_the_constant_diagonals(smm, oracle, dtype):
    """poisson2d_32 forced to PATTERN is CONST.  A refresh after a scale keeps (re-verifies) it; after one changed entry the transpose
    drops to MASKS; the SpMV has the oracle's bits each time"""
    csr = gen_matrices(dtype)["poisson2d_32"]
    n = len(csr[0]) - 1
    A = make(smm, csr, n)
    T = A.transpose()
    T.set_kernel(PATTERN, 1)
    assert T.pattern_info()[0] == CONST
    x = np.random.default_rng(4).uniform(-1, 1, n).astype(dtype)

    def check(what):
        out = np.zeros(n, dtype=dtype)
        T.rMult(x, out)
        ref = oracle.spmv(host_transpose((csr[0], csr[1], A.get_values())), OP_ASSIGN, None, x)
        np.testing.assert_array_equal(bits(out), bits(ref), err_msg=what)

    check("as built")
    A.scale(0.5)
    T.transpose_refresh(A)
    assert T.pattern_info()[0] == CONST and T.get_kernel()[0] == PATTERN
    check("after a scale")
    assert A.updateEntry(5, 6, 0.125)
    T.transpose_refresh(A)
    assert T.pattern_info()[0] == MASKS and T.get_kernel()[0] == PATTERN
    check("after one changed entry")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_rejected_refresh_changes_nothing(smm, dtype):
    other_dtype = np.float64 if dtype == np.float32 else np.float32
    csr = gen_matrices(dtype)["ragged_300"]
    A = make(smm, csr, 300)
    T = A.transpose()
    before = T.get_values()
    plain = make(smm, host_transpose(csr), 300)  # the right arrays, but not made by transpose()
    plain_before = plain.get_values()
    moved = csr[1].copy()  # another pattern with equal rows, cols and nnz: one entry moved to a free column of its row
    row = int(np.argmax(np.diff(csr[0]) > 0))
    k = csr[0][row + 1] - 1
    moved[k] = 299 if moved[k] != 299 else 298
    assert moved[k] not in csr[1][csr[0][row]:k]
    if k > csr[0][row]:
        assert moved[k] > moved[k - 1]
    cases = (
        ("not made by transpose", plain, A),
        ("the other dtype", T, make(smm, (csr[0], csr[1], csr[2].astype(other_dtype)), 300)),
        ("another pattern with equal nnz", T, make(smm, (csr[0], moved, csr[2]), 300)),
        ("another shape", T, make(smm, kat_matrix(dtype), 4)),
    )
    for name, at, src in cases:
        for _ in range(2):  # (the second time from the cached verdict)
            with pytest.raises(smm.SmmHipError) as e:
                at.transpose_refresh(src)
            assert e.value.code == INVALID, name
    np.testing.assert_array_equal(bits(T.get_values()), bits(before))
    np.testing.assert_array_equal(bits(plain.get_values()), bits(plain_before))
    T.transpose_refresh(A)  # and the right pair still works
    assert_same(arrays(T), host_transpose(csr))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_is_symmetric(smm, dtype):
    m = gen_matrices(dtype)
    n = 32 * 32
    assert make(smm, m["poisson2d_32"], n).isSymmetric() == (True, True)
    assert make(smm, m["convdiff3d_12"], 12 ** 3).isSymmetric() == (True, False)
    assert make(smm, m["ragged_300"], 300).isSymmetric() == (False, False)
    assert make(smm, gen.random_rows(257, 130, 0, 40, seed=3, dtype=dtype, empty_every=11), 130).isSymmetric() == (False, False)
    A = make(smm, m["poisson2d_32"], n)
    assert A.updateEntry(5, 6, -1.5)
    assert A.isSymmetric() == (True, False)
    assert A.updateEntry(6, 5, -1.5)
    assert A.isSymmetric() == (True, True)
    assert A.updateEntry(7, 7, np.nan)  # a NaN on the diagonal is its own mirror image and still not equal
    assert A.isSymmetric() == (True, False)
    csr = m["poisson2d_32"]
    signed = csr[2].copy()  # -0.0 equals +0.0
    k56 = csr[0][5] + int(np.flatnonzero(csr[1][csr[0][5]:csr[0][6]] == 6)[0])
    k65 = csr[0][6] + int(np.flatnonzero(csr[1][csr[0][6]:csr[0][7]] == 5)[0])
    signed[k56], signed[k65] = 0.0, -0.0
    assert make(smm, (csr[0], csr[1], signed), n).isSymmetric() == (True, True)
    assert make(smm, (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)), 0).isSymmetric() == (True, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_bad_matrices_are_refused_not_faulted(smm, dtype):
    """a column outside [0, cols) and a start[] that does not ascend, in caller-owned device arrays: SMM_HIP_ERR_INVALID from the
    device flag (nothing is addressed with the bad index)"""
    csr = kat_matrix(dtype)
    for what, start, pos in (("column == cols", csr[0], np.where(np.arange(10) == 4, 4, csr[1]).astype(np.int32)),
                             ("negative column", csr[0], np.where(np.arange(10) == 7, -3, csr[1]).astype(np.int32)),
                             ("start[] descends", np.array([0, 5, 2, 7, 10, 10], dtype=np.int32), csr[1])):
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (start, pos, csr[2])]
        torch.cuda.synchronize()
        A = smm.CSRMatrix.from_device(5, 4, d[0], d[1], d[2], dtype)
        with pytest.raises(smm.SmmHipError) as e:
            A.transpose(torch.cuda.current_stream().cuda_stream)
        assert e.value.code == INVALID, what


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_from_device_offset_views(smm, dtype):
    """the conventions of tests/device_views.py: the three arrays of a from_device matrix are views at element alignment inside
    larger buffers; the transpose is right, the source keeps its bits and every guard band is intact"""
    csr = gen.random_rows(257, 130, 0, 40, seed=3, dtype=dtype, empty_every=11)
    nnz = int(csr[0][-1])
    d_start = carve_like(csr[0], fit(1, np.int32), fill=nnz, device="cuda:0")
    d_pos = carve_like(csr[1], fit(2, np.int32), fill=0, device="cuda:0")
    d_val = carve_like(csr[2], fit(3, dtype), device="cuda:0")
    saved = [snapshot(t) for t in (d_start, d_pos, d_val)]
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(257, 130, d_start, d_pos, d_val, dtype)
    s = torch.cuda.Stream()
    T = A.transpose(s.cuda_stream)
    torch.cuda.synchronize()
    assert_same(arrays(T), host_transpose(csr, 130))
    d_val.mul_(2)  # the caller edits its own values, then refreshes on its stream
    torch.cuda.synchronize()
    A.values_changed(s.cuda_stream)
    T.transpose_refresh(A, s.cuda_stream)
    torch.cuda.synchronize()
    assert_same(arrays(T), host_transpose((csr[0], csr[1], csr[2] * 2), 130))
    for name, t, snap in zip(("start", "positions"), (d_start, d_pos), saved):
        assert_unchanged(t, snap, name)
    for name, t in zip(("start", "positions", "values"), (d_start, d_pos, d_val)):
        assert_guards_intact(t, name)
