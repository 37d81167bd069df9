"""The named matrices of the BLOCKS family's tests: scalar patterns (one entry per block) that gen.block_expand turns into b x b-blocked
CSR matrices, and the single mutations that break the fit rule (tests/blocks_restatement.py).  Everything is made once and cached."""
import numpy as np

from sparse_matrix_math_amd import generators as gen

_CACHE = {}


def _pattern(name, full_blocks=0):
    """(start, positions, block columns) of the scalar pattern"""
    if name == "tiny":  # 7 block rows: fewer rows than one wavefront
        s, p, _ = gen.random_rows(7, 7, 1, 4, seed=11)
        return s, p, 7
    if name == "wave":  # 64 block rows plus one
        s, p, _ = gen.random_rows(65, 65, 1, 6, seed=12)
        return s, p, 65
    if name == "tiles":  # 1 to 9 blocks per block row, every 7th block row empty: several tiles
        s, p, _ = gen.random_rows(3000, 3000, 1, 9, seed=13, empty_every=7)
        return s, p, 3000
    if name == "wide":
        s, p, _ = gen.random_rows(50, 90, 1, 8, seed=14)
        return s, p, 90
    if name == "tall":
        s, p, _ = gen.random_rows(90, 50, 1, 8, seed=15)
        return s, p, 50
    if name == "corners":  # every block row holds a block in block column 0 and one in the last
        n = 33
        return np.arange(0, 2 * n + 1, 2, dtype=np.int32), np.tile(np.array([0, n - 1], dtype=np.int32), n), n
    if name == "empty":  # the only block row is empty
        return np.zeros(2, dtype=np.int32), np.zeros(0, dtype=np.int32), 5
    if name == "base":  # what the mutations start from: every block row has at least two blocks, none in the last two block columns
        s, p, _ = gen.random_rows(40, 38, 2, 6, seed=16)
        return s, p, 40
    if name == "six":  # expanded with b = 6; the first block sits in an odd block column, so groups of four cannot be aligned
        s, p, _ = gen.random_rows(10, 9, 1, 4, seed=17)
        p = p.copy()
        p[s[0]:s[1]] = np.array([1, 3, 5, 7], dtype=np.int32)[: s[1] - s[0]]
        return s, p, 10
    if name in ("full", "overfull"):  # one block row of full_blocks (+ 1) blocks in a matrix of 3 block rows
        nb = full_blocks + (1 if name == "overfull" else 0)
        start = np.array([0, 1, 1 + nb, 2 + nb], dtype=np.int32)
        pos = np.concatenate([[2], np.arange(nb), [nb + 1]]).astype(np.int32)
        return start, pos, nb + 2
    raise KeyError(name)


BIT_SHAPES = ["tiny", "wave", "tiles", "wide", "tall", "corners", "empty"]


def blocked(name, b, dtype=np.float64, full_blocks=0):
    """(csr, rows, cols) of pattern `name` expanded with b x b blocks ("six": 6 x 6, whatever b)"""
    key = (name, b, np.dtype(dtype).name, full_blocks)
    if key not in _CACHE:
        s, p, ncols = _pattern(name, full_blocks)
        e = 6 if name == "six" else b
        csr = gen.block_expand(s, p, e, seed=100 + b, dtype=dtype)
        _CACHE[key] = (csr, (len(s) - 1) * e, ncols * e)
    return _CACHE[key]


MUTATIONS = ["column_shifted", "row_shortened", "block_misaligned", "second_row_other_block", "rows_not_multiple", "cols_not_multiple"]


def mutated(kind, b, dtype=np.float64):
    """(csr, rows, cols): the "base" matrix with ONE change that breaks the rule at block size b.  The columns of every row stay ascending
    and inside the matrix."""
    (start, pos, val), rows, cols = blocked("base", b, dtype)
    start, pos, val = start.copy(), pos.copy(), val.copy()
    R = 5  # the block row that is changed (at least two blocks, last block column <= 37 of 40)
    r = R * b
    ln = start[r + 1] - start[r]
    if kind == "column_shifted":  # the last column of one row moved right by one
        pos[start[r + 1] - 1] += 1
    elif kind == "row_shortened":  # the second row of the block row loses its last entry
        k = start[r + 2] - 1
        pos, val = np.delete(pos, k), np.delete(val, k)
        start[r + 2:] -= 1
    elif kind == "block_misaligned":  # the last block of the block row starts at c + 1, in all b rows
        for i in range(b):
            pos[start[r + i + 1] - b:start[r + i + 1]] += 1
    elif kind == "second_row_other_block":  # the second row's last block is the next block column's
        pos[start[r + 2] - b:start[r + 2]] += b
    elif kind == "rows_not_multiple":  # one more (empty) row
        start = np.append(start, start[-1]).astype(np.int32)
        rows += 1
    elif kind == "cols_not_multiple":
        cols += 1
    else:
        raise KeyError(kind)
    assert ln >= 2 * b and pos.max() < cols
    return (start, pos, val), rows, cols
