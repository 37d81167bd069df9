"""tests/compose_restatement.py against dense NumPy on every case of tests/compose_cases.py, in both dtypes: structure exactly, values
exactly (every rounding of the restatement is a single product, which dense NumPy repeats bit for bit in the same order).  That makes the
restatement the yardstick of tests/test_gpu_compose.py.  No GPU."""
import compose_cases as cases
import numpy as np
import pytest
from compose_restatement import Invalid, bmat, dense, diagonal, scale_rows_cols, stored, submatrix

DTYPES = [np.float32, np.float64]


def check_triple(csr, shape):
    start, pos, val = csr
    assert start.dtype == np.int32 and pos.dtype == np.int32 and len(start) == shape[0] + 1 and start[0] == 0 and start[-1] == len(pos) == len(val)
    assert np.all(np.diff(start) >= 0) and (len(pos) == 0 or (pos.min() >= 0 and pos.max() < shape[1]))
    for i in range(shape[0]):
        assert np.all(np.diff(pos[start[i]:start[i + 1]]) > 0), f"row {i}: columns do not ascend strictly"


def table_of(case):
    blocks = [[None if k is None else case["mats"][k][0] for k in row] for row in case["table"]]
    shapes = [[None if k is None else case["mats"][k][1] for k in row] for row in case["table"]]
    return blocks, shapes


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.BLOCK_CASES))
def test_bmat_against_np_block(name, dtype):
    case = cases.BLOCK_CASES[name](dtype)
    for key, (csr, shape) in case["mats"].items():
        check_triple(csr, shape)
    for key, of in case["transposed"].items():
        np.testing.assert_array_equal(dense(*case["mats"][key]), dense(*case["mats"][of]).T)
    blocks, shapes = table_of(case)
    got, shape = bmat(blocks, shapes, dtype, case["coef"], case["row_sizes"], case["col_sizes"])
    check_triple(got, shape)
    p, q = len(blocks), len(blocks[0])
    h = [max([shapes[i][j][0] for j in range(q) if shapes[i][j]] + [(case["row_sizes"] or [None] * p)[i] or 0]) for i in range(p)]
    w = [max([shapes[i][j][1] for i in range(p) if shapes[i][j]] + [(case["col_sizes"] or [None] * q)[j] or 0]) for j in range(q)]
    coef = np.ones((p, q), dtype=dtype) if case["coef"] is None else np.asarray(case["coef"], dtype=dtype).reshape(p, q)
    want = np.block([[np.zeros((h[i], w[j]), dtype=dtype) if blocks[i][j] is None else coef[i, j] * dense(blocks[i][j], shapes[i][j]) for j in range(q)] for i in range(p)])
    mask = np.block([[np.zeros((h[i], w[j]), dtype=bool) if blocks[i][j] is None else stored(blocks[i][j], shapes[i][j]) for j in range(q)] for i in range(p)])
    assert want.dtype == np.dtype(dtype) and shape == want.shape
    np.testing.assert_array_equal(stored(got, shape), mask)
    np.testing.assert_array_equal(dense(got, shape), want)
    assert got[2].dtype == np.dtype(dtype) and len(got[1]) == int(mask.sum())


def test_block_cases_cover_what_they_claim():
    c = cases.BLOCK_CASES["leading_empty_rows"](np.float64)
    got, _ = bmat(*table_of(c), np.float64)
    assert got[0][4] == 0 and got[0][5] > 0
    for name, lanes in (("segments_waves", 64), ("segments_four_lanes", 4), ("segments_eight_lanes", 8)):
        start = cases.BLOCK_CASES[name](np.float64)["mats"]["S"][0][0]
        assert tuple(np.diff(start)[:6]) == cases.SEGMENT_LENGTHS
        mean, L = int(start[-1]) // (len(start) - 1), 1
        while 4 * L < mean:
            L *= 2
        assert L == lanes, (name, mean, L)
    assert set(np.asarray(cases.BLOCK_CASES["three_by_three"](np.float64)["coef"], dtype=float)) == set(map(float, cases.COEFS))


def test_bmat_refusals():
    c = cases.BLOCK_CASES["kkt"](np.float64)
    H, B = c["mats"]["H"], c["mats"]["B"]
    with pytest.raises(Invalid):
        bmat([[H[0], B[0]]], [[H[1], B[1]]], np.float64)  # heights 144 and 20 in one block row
    with pytest.raises(Invalid):
        bmat([[H[0]], [B[0]], [None]], [[H[1]], [B[1]], [None]], np.float64)  # a block row with no size
    with pytest.raises(Invalid):
        bmat([[H[0]]], [[H[1]]], np.float32)  # dtype
    with pytest.raises(Invalid):
        bmat([[H[0]]], [[H[1]]], np.float64, row_sizes=[10])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.SUB_CASES))
def test_submatrix_against_fancy_indexing(name, dtype):
    source, rows, cols = cases.SUB_CASES[name]
    csr, shape = cases.SOURCES[source](dtype)
    check_triple(csr, shape)
    got, out_shape, src = submatrix(csr, shape, rows, cols)
    check_triple(got, out_shape)
    r = np.arange(shape[0]) if rows is None else rows
    c = np.arange(shape[1]) if cols is None else cols
    np.testing.assert_array_equal(dense(got, out_shape), dense(csr, shape)[r][:, c])
    np.testing.assert_array_equal(stored(got, out_shape), stored(csr, shape)[r][:, c])
    np.testing.assert_array_equal(got[2].view(np.uint8), csr[2][src].view(np.uint8))  # the map carries a value edit over
    if name == "columns_without_entries":
        assert len(got[1]) == 0 and len(csr[1]) > 0


@pytest.mark.parametrize("name", sorted(cases.RANGE_CASES))
def test_ranges_are_index_lists(name):
    source, r0, r1, c0, c1 = cases.RANGE_CASES[name]
    csr, shape = cases.SOURCES[source](np.float64)
    got, out_shape, _ = submatrix(csr, shape, np.arange(r0, r1), np.arange(c0, c1))
    np.testing.assert_array_equal(dense(got, out_shape), dense(csr, shape)[r0:r1, c0:c1])
    np.testing.assert_array_equal(stored(got, out_shape), stored(csr, shape)[r0:r1, c0:c1])


def test_submatrix_refusals_name_the_first_position():
    csr, shape = cases.SOURCES["ragged"](np.float64)
    with pytest.raises(Invalid, match=r"rows_idx\[2\]"):
        submatrix(csr, shape, [0, 5, 131, -1], None)
    with pytest.raises(Invalid, match=r"cols_idx\[3\]"):
        submatrix(csr, shape, None, [0, 5, 9, 9, 4])
    with pytest.raises(Invalid, match=r"cols_idx\[1\]"):
        submatrix(csr, shape, None, [0, 97])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.SOURCES))
def test_diagonal_and_scaling_against_dense(name, dtype):
    csr, shape = cases.SOURCES[name](dtype)
    A, S = dense(csr, shape), stored(csr, shape)
    d, missing = diagonal(csr, shape)
    np.testing.assert_array_equal(d, np.diag(A))
    assert d.dtype == np.dtype(dtype) and missing == min(shape) - int(np.diag(S).sum())
    r, c = cases.vectors(shape, dtype)
    for rr, cc in ((r, c), (r, None), (None, c), (None, None)):
        want = A
        if rr is not None:
            want = rr[:, None] * want
        if cc is not None:
            want = want * cc[None, :]
        got = scale_rows_cols(csr, rr, cc)
        assert want.dtype == np.dtype(dtype) and got.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(dense((csr[0], csr[1], got), shape), want)
    np.testing.assert_array_equal(scale_rows_cols(csr).view(np.uint8), csr[2].view(np.uint8))
    if name == "ragged":
        assert 0 < missing < min(shape)  # a matrix with missing diagonal entries
    if name == "laplacian":
        assert missing == 0


def test_end_to_end_blocks_give_a_nonsingular_kkt_matrix():
    H, B = cases.e2e_blocks()
    Bd = dense(B, (20, 144))
    assert np.linalg.matrix_rank(Bd) == 20
    Hd = dense(H, (144, 144))
    assert np.all(np.linalg.eigvalsh(Hd) > 0)
    K, shape = bmat([[H, cases.transpose(B, (20, 144))], [B, None]], [[(144, 144), (144, 20)], [(20, 144), None]], np.float64)
    Kd = dense(K, shape)
    np.testing.assert_array_equal(Kd, np.block([[Hd, Bd.T], [Bd, np.zeros((20, 20))]]))
    assert np.linalg.matrix_rank(Kd) == 164
