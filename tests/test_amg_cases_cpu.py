"""The matrices of tests/amg_cases.py in the CPU restatement of the multigrid set-up (tests/amg_restatement.py), without a GPU: each case
reaches the path it was built for -- a strength relation that is not symmetric, rows without a strong neighbour, singleton aggregates
beside large ones, a stall, a refusal, a threshold that changes the strong set between levels, rows of A P and A_1 in three bins of the
numeric product -- so that tests/test_gpu_amg_graphs.py cannot pass on matrices that have drifted away from those paths.

Phase 2 and the left-over numbering.  A row leaves the undecided state of the root selection only as a root or because a root's key
reached it within two hops along stored strong entries; phase 1 assigns the rows one such hop from a root and the first phase-2 pass the
rows two hops from one.  Hence passes <= 1 and left == 0 on every level of a fresh set-up, asserted here for every case: the second
phase-2 pass and the left-over numbering are not reachable from it, and no case here is a counter-example.

What the restatement gives (fp32 and fp64 alike; strong = strong entries / stored entries of level 0; aggregate sizes of level 0):
  graph_sym_1500       rows 1500 / 661 / 370 (max_levels = 3)   strong 0.390   aggregates 1 .. 9
  graph_directed_1500  rows 1500 / 935 / 489 / 402 (level 3 stalls)   strong 0.311   aggregates 1 .. 9
  bidiag_upper_1200    rows 1200 / 573 / 139   strong 1199 / 2399   aggregates 1 .. 3
  bidiag_lower_1200    rows 1200 / 568 / 139   strong 1199 / 2399   aggregates 1 .. 3
  chain_1200_c64       rows 1200 / 329 / 89 / 33   strong 0.666   aggregates 2 .. 5; theta_2 = theta / 4 adds 140 strong entries at level 2
  hubs_900             rows 900 (level 0 stalls)   strong 0   n_c = n
  hubs_1500            refused: the coarsest level would have 1500 rows
  ragged_rows_1200     rows 1200 / 726 (level 1 stalls)   strong 0.272   aggregates 1 .. 5; rows of A P 1 .. 524, of A_1 1 .. 570"""
import numpy as np
import pytest
from amg_cases import NAMES, REFUSED, case
from amg_restatement import AmgRefused, hierarchy, row_of, strength

DTYPES = [np.float32, np.float64]
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731
NUM_UP = (32, 512)  # the cuts of the numeric product's bins that one level can straddle (NUM_UP in csrc/smm_spgemm.hip)

_REF = {}


def levels_of(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _REF:
        csr, kw = case(name, dtype)
        _REF[key] = (csr, kw, hierarchy(csr, **kw))
    return _REF[key]


def rows_of(levels):
    return [len(v["A"][0]) - 1 for v in levels]


def strong_pairs(csr, strong):
    return set(zip(row_of(csr[0])[strong].tolist(), np.asarray(csr[1])[strong].tolist()))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_builders_keep_their_word(name, dtype):
    """sorted distinct columns, a diagonal of magnitude >= 1e-5 in every row, at most 2000 rows and 20 000 entries, the same matrix twice"""
    (start, pos, val), kw = case(name, dtype)
    again = case(name, dtype)[0]
    n = len(start) - 1
    assert val.dtype == np.dtype(dtype) and start.dtype == pos.dtype == np.int32
    assert n <= 2000 and start[0] == 0 and start[-1] == len(pos) == len(val) <= 20000
    rows = row_of(start)
    key = rows * n + pos
    assert (np.diff(key) > 0).all() and pos.min() >= 0 and pos.max() < n
    on = pos == rows
    assert on.sum() == n and (np.abs(val[on]) >= 1e-5).all()
    for a, b in zip((start, pos, val), again):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", [n for n in NAMES if n not in REFUSED])
def test_invariants_on_every_level(name, dtype):
    """passes <= 1 and left == 0; no empty aggregate; no empty row or column of P (no empty row of R); a stored diagonal in every row
    of A_next"""
    csr, _, levels = levels_of(name, dtype)
    sizes = rows_of(levels)
    print(name, np.dtype(dtype).name, "rows", sizes, "nnz", [len(v["A"][1]) for v in levels], "strong / stored", [round(float(v["strong"].mean()), 3) for v in levels if "strong" in v],
          "aggregate sizes", [(int(np.bincount(v["agg"]).min()), int(np.bincount(v["agg"]).max())) for v in levels if "agg" in v],
          "rounds", [v.get("rounds") for v in levels], "passes", [v.get("passes") for v in levels], "left", [v.get("left") for v in levels])
    assert sizes[-1] <= 1024
    for l, lv in enumerate(levels):
        if "passes" in lv:  # a level whose aggregates were formed, the stalled ones included
            assert lv["passes"] <= 1 and lv["left"] == 0, (l, lv["passes"], lv["left"])
        if "P" not in lv:
            assert l == len(levels) - 1
            continue
        n, n_c = sizes[l], lv["n_c"]
        assert n_c == sizes[l + 1] and 10 * n_c < 9 * n
        np.testing.assert_array_equal(np.unique(lv["agg"]), np.arange(n_c))
        P, R, A_next = lv["P"], lv["R"], levels[l + 1]["A"]
        assert len(P[0]) - 1 == n and (np.diff(P[0]) > 0).all()
        assert (np.bincount(P[1], minlength=n_c) > 0).all()
        assert len(R[0]) - 1 == n_c and (np.diff(R[0]) > 0).all()
        on = np.zeros(n_c, dtype=bool)
        on[row_of(A_next[0])[A_next[1] == row_of(A_next[0])]] = True
        assert on.all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_graph_sym_reaches_singletons_beside_large_aggregates(dtype):
    csr, _, levels = levels_of("graph_sym_1500", dtype)
    lv = levels[0]
    assert 0.2 < lv["strong"].mean() < 0.6
    sizes = np.bincount(lv["agg"])
    assert sizes.min() == 1 and sizes.max() >= 8
    assert len(levels) >= 2
    hollow = np.arange(0, 1500, 97)
    assert (np.diff(csr[0])[hollow] == 1).all()  # rows with the diagonal alone
    assert (lv["state"][hollow] == 2).all() and (sizes[lv["agg"][hollow]] == 1).all()  # singleton roots
    assert strong_pairs(csr, lv["strong"]) == {(j, i) for i, j in strong_pairs(csr, lv["strong"])}


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_graph_directed_has_a_one_way_strength_relation(dtype):
    csr, _, levels = levels_of("graph_directed_1500", dtype)
    pairs = strong_pairs(csr, levels[0]["strong"])
    one_way = [p for p in pairs if (p[1], p[0]) not in pairs]
    print("strong entries", len(pairs), "without the opposite one", len(one_way))
    assert pairs and len(one_way) == len(pairs)  # (j, i) is never stored
    assert len(levels) >= 2
    empty = np.flatnonzero(np.diff(csr[0]) == 1)  # rows that store no edge are roots of their own, whoever points at them
    assert len(empty) and (levels[0]["state"][empty] == 2).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_bidiagonal_direction_matters(dtype):
    """every off-diagonal entry is strong: 1199 of 2399 stored entries, one half next to the last (or first) row's lone diagonal"""
    aggs = []
    for name in ("bidiag_upper_1200", "bidiag_lower_1200"):
        csr, _, levels = levels_of(name, dtype)
        strong = levels[0]["strong"]
        assert 2 * int(strong.sum()) == len(strong) - 1 and round(float(strong.mean()), 3) == 0.5
        assert (strong == (csr[1] != row_of(csr[0]))).all()
        aggs.append(levels[0]["agg"])
    assert len(aggs[0]) == len(aggs[1]) and (aggs[0] != aggs[1]).any()
    assert aggs[0].max() != aggs[1].max()  # 573 aggregates against 568


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_chain_threshold_changes_the_strong_set_below_level_0(dtype):
    _, kw, levels = levels_of("chain_1200_c64", dtype)
    assert kw == {"coarse_rows": 64} and len(levels) >= 3
    changed = {}
    for l, lv in enumerate(levels):
        if l >= 1 and "strong" in lv:
            changed[l] = int((strength(lv["A"], lv["diag"], 0.08) != lv["strong"]).sum())
    print("entries whose strength differs from what theta_0 gives, per level", changed)
    assert any(changed.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_hubs_stall_and_refusal(dtype):
    csr, _, levels = levels_of("hubs_900", dtype)
    assert len(levels) == 1 and "P" not in levels[0] and "agg" not in levels[0]
    lv = levels[0]
    assert lv["strong"].sum() == 0 and (lv["state"] == 2).all() and lv["rounds"] == 1
    assert sorted(set(np.diff(csr[0]).tolist())) == [2, 300]
    big, kw = case("hubs_1500", dtype)
    assert strength(big, np.abs(big[2][big[1] == row_of(big[0])]), 0.08).sum() == 0
    with pytest.raises(AmgRefused, match="1500"):
        hierarchy(big, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_ragged_rows_straddle_the_product_bins(dtype):
    csr, _, levels = levels_of("ragged_rows_1200", dtype)
    assert sorted(set(np.diff(csr[0]).tolist())) == [1, 2, 3, 33, 257, 513]
    pairs = set(zip(row_of(csr[0]).tolist(), csr[1].tolist()))
    assert pairs == {(j, i) for i, j in pairs}
    start, pos, val = csr
    a = np.abs(val.astype(np.float64))
    on = pos == row_of(start)
    off_sum = np.bincount(row_of(start)[~on], weights=a[~on], minlength=1200)
    assert (a[on] > off_sum).all()
    assert len(levels) >= 2
    for what, m in (("A P", levels[0]["AP"]), ("A_1", levels[1]["A"])):
        lens = np.diff(m[0])
        counts = [int((lens <= NUM_UP[0]).sum()), int(((lens > NUM_UP[0]) & (lens <= NUM_UP[1])).sum()), int((lens > NUM_UP[1]).sum())]
        print(what, "rows of at most 32 /", "33 .. 512 /", "more than 512 entries:", counts, "longest", int(lens.max()))
        assert all(counts), (what, counts)
    for hub in np.flatnonzero(np.diff(start) >= 33):  # the long rows: many weak entries and a few strong ones
        s = levels[0]["strong"][start[hub]:start[hub + 1]]
        assert 0 < s.sum() <= 3
