"""Matrices for the multigrid set-up beyond grid stencils (a helper, not a test): irregular and one-way graphs, rows without a strong
neighbour, coarsening that stalls, row lengths from 1 to 513 on one level.  Every builder is deterministic, NumPy only, and returns a CSR
triple (start, positions, values) with sorted distinct columns and a diagonal of magnitude >= 1e-5 in every row; at most 2000 rows and
20 000 entries.  What each case must reach in the restatement is asserted by tests/test_amg_cases_cpu.py."""
import numpy as np

NAMES = ("graph_sym_1500", "graph_directed_1500", "bidiag_upper_1200", "bidiag_lower_1200", "chain_1200_c64", "hubs_900", "hubs_1500", "ragged_rows_1200")
REFUSED = ("hubs_1500",)  # the restatement raises AmgRefused, the library reports SMM_HIP_ERR_PRECOND


def from_entries(n, rows, cols, vals, dtype):
    """distinct (row, column) pairs in any order -> CSR triple, columns ascending inside a row"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    key = rows * n + cols
    order = np.argsort(key, kind="stable")
    assert len(np.unique(key)) == len(key), "an entry is stored twice"
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=start[1:])
    return start, cols[order].astype(np.int32), np.asarray(vals, dtype=np.float64)[order].astype(dtype)


def graph_edges(n=1500, seed=7, weak=0.5, hollow_every=97):
    """(i, j, w): each row i draws one or two targets j != i; an unordered pair is kept once, in the direction it was first drawn;
    w uniform in [0.5, 1.5), a fraction `weak` of them scaled by 1e-3; `stored` is False for every edge at a row that is a multiple of
    hollow_every: those rows lose their off-diagonal entries (and the entries towards them) but every diagonal keeps the whole sum"""
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.arange(n), np.flatnonzero(rng.random(n) < 0.5)])
    dst = (src + 1 + rng.integers(0, n - 1, len(src))) % n  # never i itself
    _, first = np.unique(np.minimum(src, dst) * n + np.maximum(src, dst), return_index=True)
    first.sort()
    src, dst = src[first], dst[first]
    w = rng.uniform(0.5, 1.5, len(src))
    w = np.where(rng.random(len(src)) < weak, w * 1e-3, w)
    return src, dst, w, (src % hollow_every != 0) & (dst % hollow_every != 0)


def graph_sym(dtype, n=1500):
    """the weighted graph Laplacian of graph_edges plus 0.05 I: both (i, j) and (j, i) stored.  The case stops at three levels
    (max_levels = 3): a row whose edges are all weak is a singleton aggregate with a diagonal near 0.05, which the Galerkin product
    multiplies by about 0.1 per level, so at level 3 it is below the 1e-5 the set-up accepts and the restatement refuses the matrix;
    and the nearly dense products of level 2 alone take the restatement ten seconds."""
    i, j, w, stored = graph_edges(n)
    d = np.bincount(i, weights=w, minlength=n) + np.bincount(j, weights=w, minlength=n) + 0.05
    i, j, w = i[stored], j[stored], w[stored]
    idx = np.arange(n)
    return from_entries(n, np.concatenate([i, j, idx]), np.concatenate([j, i, idx]), np.concatenate([-w, -w, d]), dtype)


def graph_directed(dtype, n=1500):
    """the same edges with (i, j) stored alone; the diagonal is the row sum + half the column sum + 0.05"""
    i, j, w, stored = graph_edges(n)
    d = np.bincount(i, weights=w, minlength=n) + 0.5 * np.bincount(j, weights=w, minlength=n) + 0.05
    i, j, w = i[stored], j[stored], w[stored]
    idx = np.arange(n)
    return from_entries(n, np.concatenate([i, idx]), np.concatenate([j, idx]), np.concatenate([-w, d]), dtype)


def bidiagonal(dtype, n=1200, upper=True):
    """2 on the diagonal, -1 on the first super-diagonal (upper) or sub-diagonal"""
    idx = np.arange(n)
    a, b = (idx[:-1], idx[1:]) if upper else (idx[1:], idx[:-1])
    return from_entries(n, np.concatenate([idx, a]), np.concatenate([idx, b]), np.concatenate([np.full(n, 2.0), np.full(n - 1, -1.0)]), dtype)


def chain(dtype, n=1200):
    """tridiagonal (-1, 2.05, -1)"""
    idx = np.arange(n)
    return from_entries(n, np.concatenate([idx, idx[:-1], idx[1:]]), np.concatenate([idx, idx[1:], idx[:-1]]),
                        np.concatenate([np.full(n, 2.05), np.full(2 * (n - 1), -1.0)]), dtype)


def hubs(dtype, n):
    """three hub rows (0, n / 3, 2 n / 3), each joined by -1 both ways to the n / 3 - 1 rows that follow it; a leaf's diagonal is 1.05,
    a hub's is 2 (n / 3 - 1): 1 < theta^2 * 1.05 * 2 (n / 3 - 1) at theta = 0.08 from n = 225 on, so every entry is weak at level 0.
    (The name counts rows: 900 rows are 3 hubs of 299 leaves each, 1500 rows 3 hubs of 499.)"""
    assert n % 3 == 0
    per = n // 3
    idx = np.arange(n)
    leaf = idx[idx % per != 0]
    hub = (leaf // per) * per
    d = np.where(idx % per == 0, 2.0 * (per - 1), 1.05)
    return from_entries(n, np.concatenate([idx, leaf, hub]), np.concatenate([idx, hub, leaf]), np.concatenate([d, np.full(2 * len(leaf), -1.0)]), dtype)


RAGGED_HUBS = (512, 256, 32, 32, 32, 32)  # off-diagonal entries of the six long rows


def ragged_rows(dtype, n=1200, seed=11):
    """Rows of 1, 2, 3, 33, 257 and 513 entries, symmetric pattern, strictly diagonally dominant (d_i = 1 + sum |a_ij|), every value a
    dyadic fraction (the same matrix in float and double), the row numbers shuffled so that the lengths interleave:
      6 hubs with 512, 256 and 4 x 32 leaves; a hub entry is -1/64 (weak at theta = 0.08) except towards three of its leaves, where it is -1
      96 leaves joined to two hubs (3 entries), 400 leaves joined to one hub and, by -1, to a leaf of another hub (3 entries),
      304 leaves joined to one hub (2 entries), 24 rows with the diagonal alone,
      37 chains of 10 rows joined by -1 (ends 2 entries, inner rows 3)
    A hub's row of A P names the aggregates of its leaves' neighbours, so the row of the 513-entry hub -- and, through it, the row of each
    of its leaves -- is longer than 512 entries in A P and in A_1, the 33-entry hubs' rows fall between 33 and 512, the rest below 33."""
    deg = RAGGED_HUBS
    first_leaf = len(deg)
    weak, tie = -1.0 / 64, -1.0
    ei, ej, ev = [], [], []
    free = [list(range(d)) for d in deg]  # link slots of each hub still to hand out
    leaf = first_leaf

    def join(a, b, v):
        ei.extend((a, b))
        ej.extend((b, a))
        ev.extend((v, v))

    for t in range(96):  # two hubs
        for h in (0 if t < 64 else 1, 2 + t % 4):
            free[h].pop()
            join(leaf, h, weak)
        leaf += 1
    for _ in range(200):  # one hub each, joined in pairs across hubs 0 and 1
        for h in (0, 1):
            free[h].pop()
            join(leaf, h, weak)
            leaf += 1
        join(leaf - 2, leaf - 1, tie)
    for h in range(len(deg)):  # one hub: the first three strongly
        for k in range(len(free[h])):
            join(leaf, h, tie if k < 3 else weak)
            leaf += 1
    assert leaf == first_leaf + 800
    leaf += 24  # the diagonal alone
    while leaf + 10 <= n:
        for k in range(9):
            join(leaf + k, leaf + k + 1, tie)
        leaf += 10
    assert leaf == n
    ei, ej, ev = np.array(ei), np.array(ej), np.array(ev)
    d = 1.0 + np.bincount(ei, weights=np.abs(ev), minlength=n)
    perm = np.random.default_rng(seed).permutation(n)
    idx = np.arange(n)
    return from_entries(n, perm[np.concatenate([ei, idx])], perm[np.concatenate([ej, idx])], np.concatenate([ev, d]), dtype)


def case(name, dtype=np.float64):
    """(csr, keyword arguments of the hierarchy)"""
    if name == "graph_sym_1500":
        return graph_sym(dtype), {"max_levels": 3}
    if name == "graph_directed_1500":
        return graph_directed(dtype), {}
    if name == "bidiag_upper_1200":
        return bidiagonal(dtype, upper=True), {}
    if name == "bidiag_lower_1200":
        return bidiagonal(dtype, upper=False), {}
    if name == "chain_1200_c64":
        return chain(dtype), {"coarse_rows": 64}
    if name == "hubs_900":
        return hubs(dtype, 900), {}
    if name == "hubs_1500":
        return hubs(dtype, 1500), {}
    assert name == "ragged_rows_1200", name
    return ragged_rows(dtype), {}
