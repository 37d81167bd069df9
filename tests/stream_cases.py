"""The cases of tests/test_gpu_stream_edges.py and a CPU restatement of how csrc/smm_spmv.hip cuts a matrix into row tiles and which path of
spmvStreamKernel / spmvTileKernel a tile then takes.  A helper, not a test; it needs no GPU, so tests/test_stream_cases_cpu.py can assert
that every case really holds the edge it is named after.

Words: `cap` is the capacity the kernels are launched with (streamCap); `cap_nnz = cap - 3` is the most entries a tile may hold (a tile is
staged from its 16-byte aligned start a0 = n0 & ~3, up to 3 entries before its first one); `max_rows` the most rows; `kernel` is 0 for the
pipelined spmvStreamKernel and 1 for spmvTileKernel.  A geometry is (cap_nnz, max_rows, kernel).

The named cases are lists of row lengths sized for cap_nnz = 1021, what SMM_HIP_STREAM_NV=1 gives both kernels:

  edges(cap_nnz, max_rows, kernel)  one super-chunk.  In order: 3 empty rows and four full tiles whose sizes are 1 (mod 4), so that they start
          at n0 % 4 = 0, 1, 2, 3; a tile of exactly cap_nnz entries and one of cap_nnz - 1; single rows of cap_nnz (staged), cap_nnz + 1,
          cap_nnz + 3 and 2 cap_nnz + 7 entries (direct) with full tiles between them; max_rows + 5 empty rows behind the last of those (an
          over-long row stands alone, so the run opens a tile of its own: n1 == n0); twenty full tiles; then a tile of one 4-entry row placed
          so that its a0 is exactly the kernel's stageLimit, a row of cap_nnz - 2 entries (a0 == stageLimit + 4: direct), a last short row and
          4 empty rows.  Rows are as long as max_rows needs for a tile to fill by entries, not by rows: 24 entries for 64 rows and more.
  seams(pad)  four super-chunks of 64 * 1021 entries.  Rows of 16 .. 32 entries up to 4 667 entries before the first seam; ONE row of 70 011
          entries from there to exactly the second seam -- it straddles the first seam and no row starts in chunk 1, which so holds no tile
          (a row that covers a chunk has to start before the chunk's first seam, so it is also the row that straddles it); 5 empty rows that
          start exactly on the second seam; short rows again.  pad "multiple": nnz == 3 * 64 * 1021, the last chunk is empty; pad "odd": a
          24-entry row straddles the third seam, a few more rows follow and nnz % 4 == 1.
  few(cap_nnz, max_rows, tiles)  tiles - 1 full tiles and one over-long row (so that every tile before it is staged): 3 tiles for a grid of 3
          workgroups, 11 for the round-robin deal with SMM_HIP_XCD_CHUNK_TILES.
  batch(lanes, cap_nnz)  for p in 3, 4, 13, 16, 17 a section of rows of exactly p * lanes entries -- every piece p entries, ending on a batch
          boundary for the batch sizes that divide p and one or more past it for the others -- with one row of p * lanes + 1 in each section,
          whose pieces differ in length (piecelen rounds up to p + 1, which leaves p + 2 - lanes entries to the last piece)."""
import bisect

import numpy as np

from oracle.oracle import OP_ADD, OP_ASSIGN, OP_SUB

STREAM = 2  # SMM_SPMV_STREAM
TPB = 256
WAVE = 64
TILES_PER_CHUNK = 64
PIECE = 4 * TPB  # entries per staging pass
CAP_NNZ = PIECE - 3  # with SMM_HIP_STREAM_NV=1, both kernels
LANES = (1, 2, 4, 8, 16, 32, 64)
BATCH_P = (3, 4, 13, 16, 17)
STAGED, LONG_ROW, TAIL = "staged", "direct-long-row", "direct-tail"


def csr_from_row_lengths(lens, cols, dtype, seed):
    """(start, positions, values): row i has lens[i] distinct ascending columns below `cols`, values uniform in (-1, 1); the same arrays for the
    same seed whatever the dtype (the values are drawn in float64 and rounded)"""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.min(initial=0) >= 0 and lens.max(initial=0) <= cols
    start = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=start[1:])
    nnz = int(start[-1])
    rng = np.random.default_rng(seed)
    rowof = np.repeat(np.arange(len(lens)), lens)
    room = cols // np.maximum(lens, 1)  # a row of n entries takes strides of 1 .. cols // n: its last column stays below cols
    stride = 1 + np.floor(rng.random(nnz) * room[rowof]).astype(np.int64)
    upto = np.concatenate(([0], np.cumsum(stride)))
    positions = (upto[1:] - upto[start[:-1]][rowof] - 1).astype(np.int32)
    values = rng.uniform(-1, 1, nnz).astype(dtype)
    return start, positions, values


# ---- the cut (tileCutKernel / cutRows) ----------------------------------------------------------------------------------------------
def chunk_bounds(start, cap_nnz, tiles_per_chunk=TILES_PER_CHUNK):
    """[(first row, end row)] of every super-chunk: the seams are at firstRowAtOrAfter(c * chunkNnz), nChunks = nnz // chunkNnz + 1"""
    start = [int(v) for v in start]
    rows = len(start) - 1
    chunk_nnz = tiles_per_chunk * cap_nnz
    n_chunks = start[rows] // chunk_nnz + 1
    first = [bisect.bisect_left(start, c * chunk_nnz, 0, rows) for c in range(n_chunks)]  # smallest r in [0, rows] with start[r] >= target
    return [(first[c], rows if c == n_chunks - 1 else first[c + 1]) for c in range(n_chunks)]


def cut_rows(start, cap_nnz, max_rows, tiles_per_chunk=TILES_PER_CHUNK):
    """tileCutKernel in plain Python: [(row, start[row])] per tile and the closing sentinel (rows, nnz).  Inside a super-chunk the cut is greedy:
    a tile runs to the largest e in (r, min(rEnd, r + max_rows)] with start[e] - start[r] <= cap_nnz, at least r + 1 (an over-long row stands
    alone)."""
    start = [int(v) for v in start]
    rows = len(start) - 1
    tiles = []
    for r, r_end in chunk_bounds(start, cap_nnz, tiles_per_chunk):
        while r < r_end:
            base = start[r]
            tiles.append((r, base))
            hi = min(r_end, r + max_rows)
            e = bisect.bisect_right(start, base + cap_nnz, r + 1, hi + 1) - 1  # the last e in [r + 1, hi] with start[e] <= base + cap_nnz, or r
            r = max(e, r + 1)
    tiles.append((rows, start[rows]))
    return tiles


def stage_limit(nnz, cap, kernel):
    """the largest aligned start a staged tile may have: its 16-byte pieces then stay inside the arrays"""
    return (nnz & ~3) - (cap + 4 if kernel else cap)


def classify(tiles, nnz, cap, kernel):
    """per tile STAGED, LONG_ROW or TAIL by the kernels' own conditions (`cap` is the launch capacity, cap_nnz + 3):
    direct = n1 - n0 > cap - 3 || a0 > stageLimit, stageLimit = (nnz & ~3) - cap (pipelined) / - (cap + 4) (TILE).
    (A direct tile of ONE row is summed by wavefront 0 whichever of the two conditions made it direct; TAIL here names the condition.)"""
    limit = stage_limit(nnz, cap, kernel)
    out = []
    for (_, n0), (_, n1) in zip(tiles[:-1], tiles[1:]):
        if n1 - n0 > cap - 3:
            out.append(LONG_ROW)
        elif (n0 & ~3) > limit:
            out.append(TAIL)
        else:
            out.append(STAGED)
    return out


def staged_rows(tiles, classes, rows):
    """mask of the rows that sit in staged tiles"""
    mask = np.zeros(rows, dtype=bool)
    for (r0, _), (r1, _), cls in zip(tiles[:-1], tiles[1:], classes):
        mask[r0:r1] = cls == STAGED
    return mask


# ---- what the host side chooses (useTileKernel, streamCap, tileRows, tileBatch) -------------------------------------------------------
def use_tile_kernel(lanes, variant=None):
    """variant: SMM_HIP_STREAM_VARIANT (None: unset)"""
    if variant == 0:
        return False
    if variant == 1:
        return lanes in (1, 2, 4)
    return lanes in (2, 4)


def expected_geometry(lanes, variant, nv, dtype):
    """(cap_nnz, max_rows, tile_kernel) with SMM_HIP_STREAM_NV=nv"""
    size = np.dtype(dtype).itemsize
    if use_tile_kernel(lanes, variant):
        cap_max = ((160 * 1024) // 3 - 2048) // (size + 4) - 16  # TileCfg::CAP_MAX: 6554 (fp32) / 4364 (fp64)
        cap = (max(256, min(nv * PIECE, cap_max)) + 3) & ~3
        return cap - 3, 64 * (TPB // WAVE // lanes), 1
    nv_max = 4 if size == 4 else 2  # StreamCfg::NVMAX
    return max(1, min(nv, nv_max)) * PIECE - 3, TPB // min(lanes, WAVE), 0


def tile_batch(start, lanes, forced=None):
    """G of spmvTileKernel<T, L, G>: the middle row's pieces in the fewest evenly filled batches, or SMM_HIP_TILE_BATCH; within 4 .. 16"""
    rows = len(start) - 1
    mid = int(start[rows // 2 + 1] - start[rows // 2])
    length = mid if mid > 0 else int(start[rows]) / rows
    p = max(1, int(np.ceil(length / lanes)))
    nb = (p + 15) // 16
    g = forced if forced is not None else (p + nb - 1) // nb
    return max(4, min(16, g))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def base_len(cap_nnz, max_rows):
    """a row length at which a tile fills by entries before it reaches max_rows rows"""
    return max(24, cap_nnz // max_rows + 8)


def _split(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


class _Rows:
    """row lengths, appended tile by tile: a `full` tile holds cap_nnz - 7 .. cap_nnz entries, so no row that follows it fits into it"""

    def __init__(self, cap_nnz, max_rows, seed):
        self.cap, self.max_rows = cap_nnz, max_rows
        self.per_tile = cap_nnz // base_len(cap_nnz, max_rows)  # rows of a full tile; below max_rows
        assert 1 <= self.per_tile < max_rows
        self.rng = np.random.default_rng(seed)
        self.lens = []

    @property
    def nnz(self):
        return sum(self.lens)

    def full(self, total=None, lead=0):
        """one tile: `lead` empty rows (already appended by the caller or appended here) and rows that hold `total` entries"""
        total = int(self.rng.integers(self.cap - 7, self.cap + 1)) if total is None else total
        assert self.cap - 7 <= total <= self.cap and lead < self.max_rows
        self.lens += [0] * lead + _split(total, min(self.per_tile, self.max_rows - lead))

    def row(self, n):
        self.lens.append(n)

    def aligned(self, residue, lo=3):
        """a full tile's size in [cap - lo, cap] after which the next tile starts at n0 % 4 == residue"""
        return next(t for t in range(self.cap, self.cap - lo - 1, -1) if (self.nnz + t) % 4 == residue)


def edges(cap_nnz=CAP_NNZ, max_rows=TPB, kernel=0):
    r = _Rows(cap_nnz, max_rows, 100 * max_rows + kernel)
    for i in range(4):  # tiles that start at n0 % 4 == 0, 1, 2, 3
        r.full(r.aligned((i + 1) % 4, lo=7), lead=3 if i == 0 else 0)
    r.full(cap_nnz)
    r.full(cap_nnz - 1)
    r.row(cap_nnz)  # staged: the longest row that is
    for long_row in (cap_nnz + 1, cap_nnz + 3, 2 * cap_nnz + 7):
        r.full()
        r.row(long_row)
    empties = max_rows + 5  # behind an over-long row: the first max_rows of them are a tile with n1 == n0
    r.lens += [0] * (empties - empties % max_rows)
    r.full(lead=empties % max_rows)
    for _ in range(20):
        r.full()
    r.full(r.aligned(0))  # >= cap_nnz - 3 entries: the 4-entry row below does not fit in
    x = r.nnz  # x % 4 == 0: the aligned start of the next tile
    last = 6 if kernel else 2
    r.lens += [4, cap_nnz - 2, last, 0, 0, 0, 0]
    # nnz & ~3 == x + cap (pipelined, nnz == x + cap + 1) or x + cap + 4 (TILE, nnz == x + cap + 5): a0 == stageLimit for the 4-entry tile
    assert stage_limit(r.nnz, cap_nnz + 3, kernel) == x
    assert r.nnz < TILES_PER_CHUNK * cap_nnz  # one super-chunk: the greedy cut alone decides
    return r.lens


def _fill(lens, total, rng, lo=16, hi=32):
    """rows of lo .. hi entries that hold exactly `total`"""
    left = total
    while left >= 2 * hi:
        n = int(rng.integers(lo, hi + 1))
        lens.append(n)
        left -= n
    if left:
        lens += [n for n in (left // 2, left - left // 2) if n]


def seams(pad, cap_nnz=CAP_NNZ):
    chunk = TILES_PER_CHUNK * cap_nnz
    over = chunk // 14  # 4 667: the long row starts this far before the first seam
    rng = np.random.default_rng(7)
    lens = []
    _fill(lens, chunk - over, rng)
    lens.append(chunk + over)  # ends exactly on the second seam
    lens += [0] * 5
    if pad == "multiple":
        _fill(lens, chunk, rng)
        assert sum(lens) == 3 * chunk
    else:
        assert pad == "odd"
        _fill(lens, chunk - 10, rng)
        lens.append(24)  # straddles the third seam
        _fill(lens, 300, rng)
        lens.append(17 + (1 - (sum(lens) + 17)) % 4)
        assert sum(lens) % 4 == 1
    return lens


def few(cap_nnz=CAP_NNZ, max_rows=TPB, tiles=3):
    r = _Rows(cap_nnz, max_rows, 300 * max_rows + tiles)
    for _ in range(tiles - 1):
        r.full()
    r.row(cap_nnz + 9)  # the last `cap` entries of the arrays are never staged: they are this row's
    return r.lens


def batch_sections(lanes, cap_nnz=CAP_NNZ):
    """[(p, first row, rows, the row that is one entry longer)] of batch(lanes)"""
    sections, first = [], 0
    for p in BATCH_P:  # (the longest rows last: the fewest rows in the tail that is not staged)
        n = -(-5 * cap_nnz // (2 * p * lanes))  # two and a half tiles' worth of entries
        sections.append((p, first, n, first + n // 3))
        first += n
    return sections


def batch(lanes, cap_nnz=CAP_NNZ):
    lens = []
    for p, _, n, longer in batch_sections(lanes, cap_nnz):
        lens += [p * lanes] * n
        lens[longer] += 1
    return lens


def columns(lens):
    """columns of a case: twice its longest row, at least 4096"""
    return max(4096, 2 * int(max(lens)))


_PROBLEMS = {}


def problem(name, dtype, geometry=None, lanes=None, tiles=3):
    """{"csr", "rows", "cols", "x", "lhs"} of a named case, built once per (case, geometry, dtype) and never changed.  name: "edges" / "few" (take
    a geometry), "seams-multiple" / "seams-odd", "batch" (takes lanes)"""
    dtype = np.dtype(dtype)
    geometry = geometry if name in ("edges", "few") else None  # (the other cases are the same matrix under every geometry)
    key = (name, dtype.name, geometry, lanes if name == "batch" else None, tiles if name == "few" else None)
    if key not in _PROBLEMS:
        if name == "edges":
            lens = edges(*geometry)
        elif name == "few":
            lens = few(geometry[0], geometry[1], tiles)
        elif name == "batch":
            lens = batch(lanes)
        else:
            lens = seams(name.split("-")[1])
        cols = columns(lens)
        csr = csr_from_row_lengths(lens, cols, dtype, seed=len(lens))
        rng = np.random.default_rng(11)
        _PROBLEMS[key] = {"csr": csr, "rows": len(lens), "cols": cols, "x": rng.uniform(-1, 1, cols).astype(dtype),
                          "lhs": rng.uniform(-1, 1, len(lens)).astype(dtype)}
    return _PROBLEMS[key]


OPS = (("rMult", OP_ASSIGN), ("rMultAdd", OP_ADD), ("rMultSub", OP_SUB))


def run_ops(A, prob, after_first=None):
    """{name: out} of rMult / rMultAdd / rMultSub and rMultSub in place ("rMultSub-inplace") on a CSRMatrix handle; after_first() is called
    behind the first SpMV, the one that cuts the tile table"""
    x, lhs = prob["x"], prob["lhs"]
    outs = {}
    for name, op in OPS:
        out = np.full(prob["rows"], 7, dtype=x.dtype)
        if op == OP_ASSIGN:
            A.rMult(x, out)
            if after_first:
                after_first()
        else:
            getattr(A, name)(lhs, x, out)
        outs[name] = out
    inpl = lhs.copy()
    A.rMultSub(inpl, x, inpl)
    outs["rMultSub-inplace"] = inpl
    return outs


def references(oracle, prob):
    """the oracle's outputs for run_ops, computed once per problem"""
    if "refs" not in prob:
        refs = {name: oracle.spmv(prob["csr"], op, prob["lhs"] if op else None, prob["x"]) for name, op in OPS}
        refs["rMultSub-inplace"] = refs["rMultSub"]
        prob["refs"] = refs
    return prob["refs"]


def mismatches(outs, refs, prob, lanes, bound):
    """the outputs that miss the project's SpMV rule (tests/test_gpu_spmv.py): bit-identical to the oracle at one lane per row, else
    |out - ref| <= bound(csr, x, dtype, lhs) row by row.  `bound` is test_gpu_spmv.bound; returns one line per miss"""
    missed = []
    for name, out in outs.items():
        ref = refs[name]
        if lanes == 1:
            bad = np.flatnonzero(out != ref)
            if bad.size:
                missed.append(f"{name}: {bad.size} rows differ from the oracle, the first is row {int(bad[0])}: {out[bad[0]]!r} != {ref[bad[0]]!r}")
            continue
        err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
        bnd = bound(prob["csr"], prob["x"], prob["x"].dtype, None if name == "rMult" else prob["lhs"])
        bad = np.flatnonzero(~(err <= bnd))
        if bad.size:
            worst = int(bad[np.argmax(err[bad] - bnd[bad])])
            missed.append(f"{name}: {bad.size} rows beyond the bound, the worst is row {worst}: |{out[worst]!r} - {ref[worst]!r}| > {bnd[worst]:.3e}")
    return missed
