"""The named matrices of the reverse Cuthill-McKee tests, built from generators.py and numpy only, and their restated orderings (made
once, shared by tests/test_rcm_cpu.py and tests/test_gpu_rcm.py).  A helper, not a test."""
import numpy as np
from rcm_restatement import rcm_levels

from sparse_matrix_math_amd import generators as gen

NAMES = ("poisson2d_32_shuffled", "convdiff3d_12_shuffled", "poisson3d_20_shuffled", "random_500", "bidiagonal_300", "star_2000", "tree_40x40_shuffled",
         "three_components", "dense70_in_200", "diagonal_100000", "empty", "one")
GRIDS = {"poisson2d_32_shuffled": 32, "convdiff3d_12_shuffled": 144, "poisson3d_20_shuffled": 400}  # the bandwidth of the natural numbering

_CACHE = {}


def shuffle_of(n):
    return np.random.default_rng(7).permutation(n)


def permute(csr, perm):
    """B = P A Pᵀ, b(i, j) = a(perm[i], perm[j]), columns ascending inside each row (tests/multicolor_restatement.py's, vectorised)"""
    start, pos, val = csr
    n = len(start) - 1
    inv = np.empty(n, dtype=np.int64)
    inv[np.asarray(perm, dtype=np.int64)] = np.arange(n)
    rows = inv[np.repeat(np.arange(n), np.diff(start))]
    cols = inv[pos[:start[-1]]]
    order = np.lexsort((cols, rows))
    bstart = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=bstart[1:])
    return bstart, cols[order].astype(np.int32), val[:start[-1]][order]


def from_edges(n, edges, dtype, diagonal=True):
    """the matrix that stores `edges` as given (one-sided unless both directions are listed) and, with `diagonal`, every (i, i)"""
    pairs = list(edges) + ([(i, i) for i in range(n)] if diagonal else [])
    rows = np.array([p[0] for p in pairs], dtype=np.int64).reshape(-1)
    cols = np.array([p[1] for p in pairs], dtype=np.int64).reshape(-1)
    order = np.lexsort((cols, rows))
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=start[1:])
    vals = (1.0 + 0.25 * ((rows[order] * 7 + cols[order] * 3) % 5)).astype(dtype)
    vals[rows[order] == cols[order]] = 64.0
    return start, cols[order].astype(np.int32), vals


def block_diagonal(parts, dtype):
    start, pos, val, base = [np.zeros(1, dtype=np.int64)], [], [], 0
    for s, p, v in parts:
        start.append(np.asarray(s[1:], dtype=np.int64) + start[-1][-1])
        pos.append(np.asarray(p, dtype=np.int64) + base)
        val.append(np.asarray(v, dtype=dtype))
        base += len(s) - 1
    return np.concatenate(start).astype(np.int32), np.concatenate(pos).astype(np.int32), np.concatenate(val)


def dense_block(dtype, n=200, first=40, size=70):
    """the identity with a dense, symmetric size x size block at rows first .. first + size (the multicolour tests' dense70_in_200): all
    degrees inside the block tie and the index decides"""
    rng = np.random.default_rng(11)
    dense = np.eye(n)
    blk = rng.uniform(-1, 1, (size, size))
    blk = (blk + blk.T) / 2
    blk[np.arange(size), np.arange(size)] = size + 1.0
    dense[first:first + size, first:first + size] = blk
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum((dense != 0).sum(axis=1), out=start[1:])
    return start, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(dtype)


def _build(name, dtype):
    if name.endswith("_shuffled") and name != "tree_40x40_shuffled":
        csr = {"poisson2d_32_shuffled": lambda: gen.poisson2d(32, dtype=dtype), "convdiff3d_12_shuffled": lambda: gen.convdiff3d(12, 0.3, dtype=dtype),
               "poisson3d_20_shuffled": lambda: gen.poisson3d(20, dtype=dtype)}[name]()
        return permute(csr, shuffle_of(len(csr[0]) - 1))
    if name == "random_500":  # not symmetric: the in-neighbours matter
        return gen.random_rows(500, 500, 1, 9, seed=3, dtype=dtype)
    if name == "bidiagonal_300":  # a path stored one-sided: 300 levels, the root moves to an end
        return from_edges(300, [(i, i + 1) for i in range(299)], dtype)
    if name == "star_2000":  # row 0 holds all columns: one long row, one level of 1999 under one parent
        return from_edges(2000, [(0, j) for j in range(1, 2000)], dtype)
    if name == "tree_40x40_shuffled":  # a root, 40 children, 40 children each: level 2 has 1600 vertices under 40 parents
        edges = [(0, 1 + c) for c in range(40)] + [(1 + c, 41 + 40 * c + g) for c in range(40) for g in range(40)]
        csr = from_edges(1641, edges + [(j, i) for i, j in edges], dtype)
        return permute(csr, shuffle_of(1641))
    if name == "three_components":  # a grid, a path of 7 and 10 isolated rows, shuffled together
        path = from_edges(7, [(i, i + 1) for i in range(6)] + [(i + 1, i) for i in range(6)], dtype)
        csr = block_diagonal([gen.poisson2d(5, dtype=dtype), path, from_edges(10, [], dtype)], dtype)
        return permute(csr, shuffle_of(42))
    if name == "dense70_in_200":
        return dense_block(dtype)
    if name == "diagonal_100000":
        n = 100000
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0, dtype=dtype)
    if name == "empty":
        return np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)
    if name == "one":
        return np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([2.5], dtype=dtype)
    raise KeyError(name)


def rcm_case(name, dtype=np.float64):
    """the matrix of that name, made once per dtype"""
    key = (name, np.dtype(dtype).name)
    if key not in _CACHE:
        _CACHE[key] = tuple(np.ascontiguousarray(a) for a in _build(name, dtype))
    return _CACHE[key]


def restated(name, reverse=True):
    """(perm, info) of the restatement's level form, made once"""
    key = ("rcm", name, bool(reverse))
    if key not in _CACHE:
        _CACHE[key] = rcm_levels(rcm_case(name), reverse)
    return _CACHE[key]
