"""tests/stream_cases.py on the CPU: the restated cut agrees with a row-by-row walk, and every named case of tests/test_gpu_stream_edges.py
holds -- under every geometry it is run with -- the edge it is named after, with at least 60 % of its rows in staged tiles so that the
one-lane-per-row fallback of the kernels cannot carry the GPU test."""
import numpy as np
import pytest
import stream_cases as sc
from stream_cases import LONG_ROW, STAGED, TAIL

CAP = sc.CAP_NNZ
CHUNK = sc.TILES_PER_CHUNK * CAP
# every geometry the GPU tests run at SMM_HIP_STREAM_NV=1: the default kernel of each lane count, the TILE kernel forced (variant 1) and the
# pipelined kernel forced (variant 0)
GEOMETRIES = sorted({sc.expected_geometry(lanes, variant, 1, np.float32) for lanes in sc.LANES for variant in (None, 0, 1)})
# the larger tiles of the SMM_HIP_STREAM_NV sweep (cases built for 1021 entries, cut at another capacity)
NV_GEOMETRIES = sorted({sc.expected_geometry(lanes, None, nv, dt) for lanes, nvs in ((1, range(2, 5)), (2, range(2, 8))) for nv in nvs
                        for dt in (np.float32, np.float64)})


def starts(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


def cut(lens, geometry):
    cap_nnz, max_rows, kernel = geometry
    start = starts(lens)
    tiles = sc.cut_rows(start, cap_nnz, max_rows)
    return start, tiles, sc.classify(tiles, int(start[-1]), cap_nnz + 3, kernel)


def walk_cut(start, cap_nnz, max_rows):
    """the same cut, row by row and without a binary search"""
    rows, nnz = len(start) - 1, int(start[-1])
    n_chunks = nnz // (sc.TILES_PER_CHUNK * cap_nnz) + 1
    tiles = []
    for c in range(n_chunks):
        first = [next((r for r in range(rows) if start[r] >= t * sc.TILES_PER_CHUNK * cap_nnz), rows) for t in (c, c + 1)]
        r, r_end = first[0], rows if c == n_chunks - 1 else first[1]
        while r < r_end:
            tiles.append((r, int(start[r])))
            e = r + 1
            while e < min(r_end, r + max_rows) and start[e + 1] - start[r] <= cap_nnz:
                e += 1
            r = e
    return tiles + [(rows, nnz)]


def general_checks(lens, geometry, floor=0.6):
    cap_nnz, max_rows, _ = geometry
    start, tiles, classes = cut(lens, geometry)
    rows = len(lens)
    # every row exactly once, in order
    assert tiles[0] == (0, 0) and tiles[-1] == (rows, int(start[-1]))
    assert all(a[0] < b[0] for a, b in zip(tiles[:-1], tiles[1:]))
    assert all(n0 == start[r] for r, n0 in tiles)
    for (r0, n0), (r1, n1), cls in zip(tiles[:-1], tiles[1:], classes):
        assert r1 - r0 <= max_rows
        assert n1 - n0 <= cap_nnz or r1 - r0 == 1
        assert (cls == LONG_ROW) == (n1 - n0 > cap_nnz)
    staged = sc.staged_rows(tiles, classes, rows)
    assert staged.sum() >= floor * rows, (geometry, staged.sum(), rows)
    return start, tiles, classes


def test_the_geometries_are_the_ones_the_issue_names():
    assert sc.expected_geometry(1, None, 1, np.float64) == (1021, 256, 0)
    assert sc.expected_geometry(2, None, 1, np.float32) == (1021, 128, 1)
    assert sc.expected_geometry(4, None, 1, np.float64) == (1021, 64, 1)
    assert [sc.expected_geometry(lanes, None, 1, np.float32)[1:] for lanes in (8, 16, 32, 64)] == [(32, 0), (16, 0), (8, 0), (4, 0)]
    assert sc.expected_geometry(1, 1, 1, np.float32) == (1021, 256, 1) and sc.expected_geometry(2, 0, 1, np.float32) == (1021, 128, 0)
    # the TILE kernel's capacity is clipped to CAP_MAX and rounded up to whole 16-byte pieces; the pipelined kernel's to NVMAX passes
    assert sc.expected_geometry(2, None, 7, np.float32)[0] == 6556 - 3 and sc.expected_geometry(2, None, 7, np.float64)[0] == 4364 - 3
    assert sc.expected_geometry(2, None, 4, np.float64)[0] == 4096 - 3 and sc.expected_geometry(2, None, 6, np.float32)[0] == 6144 - 3
    assert sc.expected_geometry(1, None, 9, np.float32)[0] == 4096 - 3 and sc.expected_geometry(1, None, 3, np.float64)[0] == 2048 - 3
    assert len(GEOMETRIES) == 10


def test_builder_gives_distinct_ascending_columns_and_is_deterministic():
    lens = [0, 5, 0, 4096, 1, 2049, 0]
    a = sc.csr_from_row_lengths(lens, 4096, np.float64, seed=3)
    b = sc.csr_from_row_lengths(lens, 4096, np.float32, seed=3)
    start, pos, val = a
    assert start.dtype == np.int32 and pos.dtype == np.int32 and val.dtype == np.float64 and b[2].dtype == np.float32
    np.testing.assert_array_equal(np.diff(start), lens)
    np.testing.assert_array_equal(pos, b[1])
    np.testing.assert_array_equal(val.astype(np.float32), b[2])
    for r in range(len(lens)):
        row = pos[start[r]:start[r + 1]]
        assert np.all(np.diff(row) > 0) and (row.size == 0 or (row[0] >= 0 and row[-1] < 4096))
    assert np.all(np.abs(val) < 1) and val.min() < -0.99 and val.max() > 0.99
    assert not np.array_equal(pos, sc.csr_from_row_lengths(lens, 4096, np.float64, seed=4)[1])


def test_restated_cut_agrees_with_a_row_by_row_walk():
    rng = np.random.default_rng(5)
    cases = [rng.integers(0, 9, 300).tolist(), [0] * 40, [7], [0, 0, 50, 0], [10] * 64, [3] * 7 + [41] + [0] * 9 + [3] * 30]
    for lens in cases:
        for cap_nnz, max_rows, per_chunk in ((13, 4, 2), (40, 8, 1), (10, 3, 64), (5, 256, 3)):
            start = starts(lens)
            assert sc.cut_rows(start, cap_nnz, max_rows, per_chunk) == \
                walk_cut_with(start, cap_nnz, max_rows, per_chunk), (lens[:8], cap_nnz, max_rows, per_chunk)
    for geometry in (GEOMETRIES[0], GEOMETRIES[-1]):
        for lens in (sc.edges(*geometry), sc.seams("odd")):
            assert sc.cut_rows(starts(lens), *geometry[:2]) == walk_cut(starts(lens), *geometry[:2])


def walk_cut_with(start, cap_nnz, max_rows, per_chunk):
    old = sc.TILES_PER_CHUNK
    sc.TILES_PER_CHUNK = per_chunk  # (walk_cut reads it; cut_rows takes it as an argument)
    try:
        return walk_cut(start, cap_nnz, max_rows)
    finally:
        sc.TILES_PER_CHUNK = old


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_edges_holds_every_tile_edge(geometry):
    cap_nnz, max_rows, kernel = geometry
    lens = sc.edges(*geometry)
    start, tiles, classes = general_checks(lens, geometry)
    nnz = int(start[-1])
    assert lens[:3] == [0, 0, 0] and lens[3] > 0 and lens[-4:] == [0, 0, 0, 0] and lens[-5] > 0
    assert len(sc.chunk_bounds(start, cap_nnz)) == 1
    size = [b[1] - a[1] for a, b in zip(tiles[:-1], tiles[1:])]
    nrows = [b[0] - a[0] for a, b in zip(tiles[:-1], tiles[1:])]
    # consecutive staged tiles at each alignment of the aligned start
    assert [t[1] % 4 for t in tiles[:4]] == [0, 1, 2, 3] and classes[:4] == [STAGED] * 4 and min(nrows[:4]) >= 1
    # a tile of exactly cap_nnz entries and one of one fewer, each of several rows (for 4 rows per tile: of 3)
    for want in (cap_nnz, cap_nnz - 1):
        assert any(s == want and n > 1 and c == STAGED for s, n, c in zip(size, nrows, classes)), want
    # single rows where staged turns into direct
    single = {s: c for s, n, c in zip(size, nrows, classes) if n == 1 and s >= cap_nnz}
    assert single == {cap_nnz: STAGED, cap_nnz + 1: LONG_ROW, cap_nnz + 3: LONG_ROW, 2 * cap_nnz + 7: LONG_ROW}
    # more than max_rows empty rows in a run: a staged tile with n1 == n0
    run = max(len(z) for z in "".join("0" if n == 0 else "x" for n in lens).split("x"))
    assert run == max_rows + 5
    assert any(s == 0 and n == max_rows and c == STAGED for s, n, c in zip(size, nrows, classes))
    # the last staged tile starts exactly at stageLimit, the next one 4 further: direct
    limit = sc.stage_limit(nnz, cap_nnz + 3, kernel)
    last = max(i for i, c in enumerate(classes) if c == STAGED)
    assert tiles[last][1] & ~3 == limit and size[last] == 4
    assert tiles[last + 1][1] & ~3 == limit + 4 and classes[last + 1] == TAIL and size[last + 1] >= cap_nnz - 2
    assert all(c != STAGED for c in classes[last + 1:])
    assert set(classes) == {STAGED, LONG_ROW, TAIL}


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_edges_of_one_kernel_is_a_fair_case_for_the_other(geometry):
    """the pipelined kernel's `edges` also runs on the TILE kernel (the comparison of the two kernels row by row)"""
    other = (geometry[0], geometry[1], 1 - geometry[2])
    _, _, classes = general_checks(sc.edges(*other), geometry)
    assert set(classes) == {STAGED, LONG_ROW, TAIL}


@pytest.mark.parametrize("pad", ["multiple", "odd"])
def test_seams_holds_every_seam_edge(pad):
    lens = sc.seams(pad)
    start = starts(lens)
    nnz = int(start[-1])
    assert 3 * CHUNK <= nnz <= 200_000 and nnz > 2 * CHUNK
    bounds = sc.chunk_bounds(start, CAP)
    assert len(bounds) == 4
    # one row straddles the first seam and covers all of chunk 1: no row starts there, the chunk holds no tile
    long_row = int(np.argmax(lens))
    assert start[long_row] < CHUNK < start[long_row + 1] and lens[long_row] >= CHUNK
    assert start[long_row + 1] == 2 * CHUNK
    assert bounds[0] == (0, long_row + 1) and bounds[1] == (long_row + 1, long_row + 1)
    # empty rows exactly on the second seam: a row start falls on it
    r2 = bounds[2][0]
    assert start[r2] == 2 * CHUNK and lens[r2:r2 + 5] == [0] * 5 and lens[r2 + 5] > 0
    if pad == "multiple":
        assert nnz % CHUNK == 0 and bounds[3] == (len(lens), len(lens))  # the last chunk is empty
    else:
        assert nnz % 4 == 1
        r3 = bounds[3][0]
        assert start[r3 - 1] < 3 * CHUNK < start[r3] and lens[r3 - 1] == 24 and r3 < len(lens)  # a short row straddles the third seam
    for geometry in GEOMETRIES + NV_GEOMETRIES:
        _, tiles, classes = general_checks(lens, geometry)
        assert set(classes) == {STAGED, LONG_ROW, TAIL}
        # no tile crosses a seam
        firsts = {t[0] for t in tiles}
        assert all(b[0] in firsts for b in sc.chunk_bounds(start, geometry[0]))


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("tiles", [3, 11])
def test_few_has_that_many_tiles_all_but_the_last_staged(geometry, tiles):
    _, cut_tiles, classes = general_checks(sc.few(geometry[0], geometry[1], tiles), geometry)
    assert len(cut_tiles) - 1 == tiles
    assert classes == [STAGED] * (tiles - 1) + [LONG_ROW]


@pytest.mark.parametrize("lanes,variant", [(2, None), (4, None), (1, 1), (2, 0), (4, 0), (1, None)])
def test_batch_pieces_end_on_and_past_a_batch_boundary(lanes, variant):
    geometry = sc.expected_geometry(lanes, variant, 1, np.float32)
    lens = sc.batch(lanes)
    _, tiles, classes = general_checks(lens, geometry)
    staged = sc.staged_rows(tiles, classes, len(lens))
    sections = sc.batch_sections(lanes)
    assert [s[0] for s in sections] == list(sc.BATCH_P) and sum(s[2] for s in sections) == len(lens)
    piece_lengths = set()
    for p, first, n, longer in sections:
        section = lens[first:first + n]
        assert section.count(p * lanes) == n - 1 and lens[longer] == p * lanes + 1 and staged[longer]
        assert staged[first:first + n].sum() - 1 >= 8  # uniform rows of this length in staged tiles
        piecelen = -(-(p * lanes + 1) // lanes)
        pieces = [min(piecelen, max(0, p * lanes + 1 - q * piecelen)) for q in range(lanes)]
        assert sum(pieces) == p * lanes + 1 and (lanes == 1 or len(set(pieces)) > 1)
        piece_lengths |= {p} | set(pieces)
    for g in (4, 13, 16):  # pieces that end exactly on a batch boundary, and one past it
        assert any(n % g == 0 for n in piece_lengths) and any(n % g == 1 for n in piece_lengths)
    assert STAGED in classes and TAIL in classes


@pytest.mark.parametrize("geometry", NV_GEOMETRIES)
def test_the_cases_of_the_capacity_sweep_stay_mostly_staged(geometry):
    """SMM_HIP_STREAM_NV above 1: `edges` (built for 1021 entries) cut into larger tiles"""
    max_rows_1021 = geometry[1]
    general_checks(sc.edges(CAP, max_rows_1021, geometry[2]), geometry)


def test_tile_batch_follows_the_middle_row():
    start = starts([26] * 9)
    assert sc.tile_batch(start, 2) == 13 and sc.tile_batch(start, 1) == 13 and sc.tile_batch(start, 4) == 7
    assert sc.tile_batch(starts([51] * 9), 2) == 13 and sc.tile_batch(starts([3] * 9), 1) == 4
    assert sc.tile_batch(start, 2, forced=2) == 4 and sc.tile_batch(start, 2, forced=99) == 16 and sc.tile_batch(start, 2, forced=9) == 9
