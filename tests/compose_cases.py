"""Cases shared by the compose tests (a helper, not a test): block tables, submatrix selections, matrices for diagonal and scaling.  Every
matrix is a CSR triple (start, positions, values) with strictly ascending columns per row, from fixed seeds.

Where the sizes come from (csrc/smm_compose.hip): the fill of a block gives a slot L lanes per row, L = the power of two next to a quarter
of the slot's MEAN row length; groups of L < 64 lanes copy at most 8 L entries of a segment themselves and leave the rest to the whole
wavefront; L >= 64 are whole wavefronts, L > 256 spans workgroups.  The submatrix walks a selected row with L <= 64 lanes, L from the
SOURCE's mean row length."""
import numpy as np

from sparse_matrix_math_amd import generators as gen

SEGMENT_LENGTHS = (63, 64, 65, 255, 256, 257)
COEFS = (1, -1, 0.5, 0)
E2E_SEED = 3  # gen.random_rows(20, 144, 3, 9, seed=E2E_SEED) has rank 20 (asserted in tests/test_compose_cpu.py)


def from_rows(rows, dtype, rng):
    start = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=start[1:])
    pos = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    val = rng.uniform(-1, 1, len(pos)).astype(dtype)
    if len(val) > 3:
        val[1], val[2] = -0.0, 0.0  # a signed zero and a stored zero travel as bits
    return start, pos, val


def rows_of_lengths(lengths, cols, dtype, seed):
    rng = np.random.default_rng(seed)
    return from_rows([np.sort(rng.choice(cols, size=n, replace=False)) for n in lengths], dtype, rng)


def empty(rows, dtype):
    return np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)


def transpose(csr, shape):
    """the transpose as the library builds it: row j holds column j's entries, source rows ascending"""
    start, pos, val = csr
    rows = np.repeat(np.arange(shape[0]), np.diff(start))
    order = np.argsort(pos, kind="stable")
    t_start = np.zeros(shape[1] + 1, dtype=np.int32)
    np.cumsum(np.bincount(pos, minlength=shape[1]), out=t_start[1:])
    return t_start, rows[order].astype(np.int32), val[order].copy()


def e2e_blocks(dtype=np.float64):
    """H = poisson2d(12) and the full-rank 20 x 144 constraint block of the end-to-end test"""
    return gen.poisson2d(12, dtype=dtype), gen.random_rows(20, 144, 3, 9, seed=E2E_SEED, dtype=dtype)


# ---- block tables: name -> builder(dtype) -> {"mats": {key: (triple, (rows, cols))}, "table": [[key or None]], "coef", "row_sizes",
# "col_sizes", "transposed": {key: the key it is the transpose of}} ----
def _case(mats, table, coef=None, row_sizes=None, col_sizes=None, transposed=None):
    return {"mats": mats, "table": table, "coef": coef, "row_sizes": row_sizes, "col_sizes": col_sizes, "transposed": transposed or {}}


def one_by_one(dtype):
    return _case({"H": (gen.poisson2d(12, dtype=dtype), (144, 144))}, [["H"]])


def kkt(dtype):
    """[[H, Bt], [B, None]]: B 20 x 144 with every fifth row empty"""
    B = gen.random_rows(20, 144, 1, 9, seed=11, dtype=dtype, empty_every=5)
    mats = {"H": (gen.poisson2d(12, dtype=dtype), (144, 144)), "B": (B, (20, 144)), "Bt": (transpose(B, (20, 144)), (144, 20))}
    return _case(mats, [["H", "Bt"], ["B", None]], transposed={"Bt": "B"})


def kkt_coefs(dtype):
    c = kkt(dtype)
    c["coef"] = [1, -1, 0.5, 0]
    return c


def three_by_three(dtype):
    """the same handle A in two slots, every coefficient of COEFS"""
    mats = {"A": (gen.random_rows(30, 30, 0, 8, seed=21, dtype=dtype, empty_every=7), (30, 30)),
            "C": (gen.random_rows(30, 17, 0, 5, seed=22, dtype=dtype), (30, 17)),
            "D": (gen.random_rows(11, 30, 1, 30, seed=23, dtype=dtype), (11, 30))}
    return _case(mats, [["A", None, "C"], [None, "A", "C"], ["D", "D", None]], coef=[1, 0, -1, 0, 0.5, 0, -1, 1, 0])


def null_block_row(dtype):
    """a block row (and a block column) of NULLs alone, sized by row_sizes / col_sizes"""
    mats = {"A": (gen.random_rows(9, 13, 0, 6, seed=31, dtype=dtype), (9, 13)), "B": (gen.random_rows(4, 13, 1, 4, seed=32, dtype=dtype), (4, 13))}
    return _case(mats, [["A", None], [None, None], ["B", None]], row_sizes=[None, 5, None], col_sizes=[13, 3])


def degenerate_blocks(dtype):
    """blocks with 0 rows, 0 columns and 0 entries beside an ordinary one"""
    mats = {"norows": (empty(0, dtype), (0, 10)), "noentries": (empty(6, dtype), (6, 10)), "nocols": (empty(6, dtype), (6, 0)),
            "R": (gen.random_rows(5, 10, 1, 6, seed=41, dtype=dtype), (5, 10))}
    return _case(mats, [["norows", None], ["noentries", "nocols"], ["R", None]])


def leading_empty_rows(dtype):
    """first_active_start > 0 in the result"""
    mats = {"E": (empty(4, dtype), (4, 10)), "R": (gen.random_rows(5, 10, 1, 6, seed=42, dtype=dtype), (5, 10))}
    return _case(mats, [["E"], ["R"]])


def _segments(n_short, dtype, seed):
    lengths = list(SEGMENT_LENGTHS) + [2] * n_short
    return rows_of_lengths(lengths, 300, dtype, seed), (len(lengths), 300)


def segments_waves(dtype):
    """rows of 63 .. 257 entries alone in their block (mean 160: L = 64) beside a block of short rows, in both orders"""
    S = _segments(0, dtype, 51)
    P = (gen.random_rows(6, 20, 0, 5, seed=52, dtype=dtype), (6, 20))
    return _case({"S": S, "P": P}, [["S", "P", "S"]], coef=[1, 1, -1])


def segments_four_lanes(dtype):
    """the same six rows among 60 rows of 2 entries (mean 16: L = 4, a group's own share is 32 entries, the rest goes to the wavefront)"""
    S = _segments(60, dtype, 53)
    P = (gen.random_rows(66, 20, 0, 5, seed=54, dtype=dtype), (66, 20))
    return _case({"S": S, "P": P}, [["P", "S"]], coef=[0.5, 1])


def segments_eight_lanes(dtype):
    """... among 46 such rows (mean 20: L = 8, own share 64: rows of 63 and 64 stay with the group, 65 leaves one entry to the wavefront)"""
    S = _segments(46, dtype, 55)
    return _case({"S": S}, [["S"], ["S"]], coef=[1, 0.5])


def dense_row(dtype):
    """one fully dense 1 x 3000 row (L = 1024: four workgroups on one row) below and beside ordinary rows"""
    rng = np.random.default_rng(61)
    D = (from_rows([np.arange(3000)], dtype, rng), (1, 3000))
    P = (gen.random_rows(50, 3000, 0, 9, seed=62, dtype=dtype, empty_every=6), (50, 3000))
    Q = (gen.random_rows(1, 10, 3, 3, seed=63, dtype=dtype), (1, 10))
    return _case({"D": D, "P": P, "Q": Q, "Q50": (gen.random_rows(50, 10, 0, 4, seed=64, dtype=dtype), (50, 10))}, [["P", "Q50"], ["D", "Q"]], coef=[1, 1, -1, 1])


BLOCK_CASES = {"one_by_one": one_by_one, "kkt": kkt, "kkt_coefs": kkt_coefs, "three_by_three": three_by_three, "null_block_row": null_block_row,
               "degenerate_blocks": degenerate_blocks, "leading_empty_rows": leading_empty_rows, "segments_waves": segments_waves,
               "segments_four_lanes": segments_four_lanes, "segments_eight_lanes": segments_eight_lanes, "dense_row": dense_row}


# ---- sources for submatrix, diagonal and scaling: name -> builder(dtype) -> (triple, (rows, cols)) ----
def ragged(dtype):
    """131 x 97 (two wavefronts of rows plus 3), rows of 0 .. 12 entries, every ninth empty: mean 5, two lanes per row"""
    return gen.random_rows(131, 97, 0, 12, seed=71, dtype=dtype, empty_every=9), (131, 97)


def wide(dtype):
    return gen.random_rows(97, 131, 0, 12, seed=72, dtype=dtype, empty_every=8), (97, 131)


def long_rows(dtype):
    """9 x 700 with rows of 300 .. 600 entries: a whole wavefront per row"""
    return gen.random_rows(9, 700, 300, 600, seed=73, dtype=dtype), (9, 700)


def even_columns(dtype):
    """40 x 120 with entries on even columns only: the odd columns meet no stored entry"""
    start, pos, val = gen.random_rows(40, 60, 0, 20, seed=74, dtype=dtype, empty_every=6)
    return (start, (2 * pos).astype(np.int32), val), (40, 120)


def laplacian(dtype):
    return gen.poisson2d(12, dtype=dtype), (144, 144)


SOURCES = {"ragged": ragged, "wide": wide, "long_rows": long_rows, "even_columns": even_columns, "laplacian": laplacian}

_I = lambda *v: np.asarray(v, dtype=np.int32)  # noqa: E731

# name -> (source, rows, cols): None = all; ("range", lo, hi) = the range form
SUB_CASES = {
    "everything": ("ragged", None, None),
    "nothing": ("ragged", _I(), _I()),
    "no_rows": ("ragged", _I(), None),
    "no_cols": ("ragged", None, _I()),
    "one_row_one_col": ("ragged", _I(64), _I(40)),
    "columns_without_entries": ("even_columns", None, np.arange(1, 120, 2, dtype=np.int32)),
    "reversed_rows": ("ragged", np.arange(130, -1, -1, dtype=np.int32), np.arange(3, 97, 2, dtype=np.int32)),
    "repeated_rows": ("ragged", _I(5, 5, 64, 0, 130, 5, 64, 64), np.arange(0, 97, 3, dtype=np.int32)),
    "free_dofs": ("laplacian", np.setdiff1d(np.arange(144), np.arange(0, 144, 12)).astype(np.int32), np.setdiff1d(np.arange(144), np.arange(0, 144, 12)).astype(np.int32)),
    "wide_source": ("wide", np.arange(10, 90, dtype=np.int32), np.arange(20, 131, dtype=np.int32)),
    "long_rows_some": ("long_rows", _I(8, 0, 3, 3), np.arange(100, 650, dtype=np.int32)),
    "long_rows_all_columns": ("long_rows", _I(2, 7), None),
}
# (source, r0, r1, c0, c1): the range form must equal the index form on the same ranges
RANGE_CASES = {"block_11": ("ragged", 0, 70, 0, 50), "inner": ("ragged", 17, 101, 30, 97), "long": ("long_rows", 2, 9, 64, 577), "empty_range": ("ragged", 40, 40, 5, 5),
               "whole": ("wide", 0, 97, 0, 131)}


def vectors(shape, dtype, seed=81):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, shape[0]).astype(dtype), rng.uniform(-2.0, 2.0, shape[1]).astype(dtype)
