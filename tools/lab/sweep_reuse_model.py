#!/usr/bin/env python3
"""r09 model (CPU only): how often one XCD fetches a 128-byte line of x during one PATTERN SpMV of the benchmark matrix, by an LRU of the
XCD's L2 over the x lines alone (the value stream is read once with nt loads and is left out, as in DESIGN_HISTORY section K item 5).

  (a) the row-major front (tile and slots kernels): the XCD walks its eighth of the rows once, a 64-row wave touching the lines of
      x[wave + off[e]] for every offset e before the next wave starts;
  (b) the super-block sweep (sweep kernel): the XCD's 32 workgroups hold B = 32 x 4 x R x 64 rows open and step through the offsets; step e
      of workgroup g touches x[rows of g + off[e]].  `drift` (in steps) spreads the workgroups over that many steps, either evenly
      (workgroup g runs step e at time e + drift * g / 31: neighbours stay close) or at random (a seeded uniform share each: neighbours
      can be a whole drift apart, the adverse case).  --wgs-per-cu adds the rows for that many workgroups per CU (B grows with it).

The LRU capacity is the one free number (the L2 has 4 MB; the value stream passes through it as well, so less than that holds x): the
table is printed for every capacity in --l2-mb.  Measured for (a): 31-32 fetches per line (r08 counters: 1.3 GB / 40 MB).  The closed form
for (b) at zero drift is 1 + sum(min(gap, B)) / B over the gaps between neighbouring offsets.

  python tools/lab/sweep_reuse_model.py [--rows 10000000] [--l2-mb 2,3,4] [--wgs-per-cu 3] > profiles/r09/sweep_reuse_model.txt"""
import argparse
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from sparse_matrix_math_amd.generators import band_offsets

LINE_ROWS = 32  # fp32: 128-byte lines


class Lru:
    def __init__(self, lines):
        self.cap, self.d, self.misses = lines, OrderedDict(), 0

    def touch(self, first, last):
        d = self.d
        for line in range(first, last + 1):
            if line in d:
                d.move_to_end(line)
            else:
                self.misses += 1
                d[line] = None
                if len(d) > self.cap:
                    d.popitem(last=False)


def all_offsets(rows, k, seed, max_offset):
    o = band_offsets(rows, k, seed, max_offset)
    return np.concatenate([-o[::-1], [0], o]).astype(np.int64)


def front(offs, begin, end, cap_lines):
    """fetches per x line of a row-major walk over one XCD's rows [begin, end), from a cold L2: misses over the lines of x[begin..end)"""
    lru = Lru(cap_lines)
    for row in range(begin, end, 64):
        for off in offs:
            lru.touch((row + off) // LINE_ROWS, (row + off + 63) // LINE_ROWS)
    return lru.misses / ((end - begin) / LINE_ROWS)


def sweep(offs, begin, blocks, rows_open, drift, cap_lines, wgs=32, random_phase=False):
    """fetches per x line of `blocks` consecutive super-blocks from row `begin`; counted without the first block"""
    wg_rows = 4 * rows_open * 64
    block_rows = wgs * wg_rows
    phase = np.random.default_rng(7).uniform(0, 1, wgs) if random_phase else np.arange(wgs) / max(1, wgs - 1)
    lru = Lru(cap_lines)
    after_first = 0
    for b in range(blocks):
        if b == 1:
            after_first = lru.misses
        events = sorted((e + drift * phase[g], g, e) for g in range(wgs) for e in range(len(offs)))
        for _, g, e in events:
            r0 = begin + b * block_rows + g * wg_rows + int(offs[e])
            lru.touch(r0 // LINE_ROWS, (r0 + wg_rows - 1) // LINE_ROWS)
    return (lru.misses - after_first) / ((blocks - 1) * block_rows / LINE_ROWS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0x5EED)
    ap.add_argument("--max-offset", type=int, default=1 << 20)
    ap.add_argument("--l2-mb", default="2,3,4")
    ap.add_argument("--wgs-per-cu", type=int, default=3, help="also print R = 8 / 16 / 32 at this many workgroups per CU (shipped: R = 16 at 3)")
    args = ap.parse_args()
    offs = all_offsets(args.rows, args.k, args.seed, args.max_offset)
    gaps = np.diff(offs)
    begin = args.rows // 2 // 64 * 64  # an XCD whose eighth lies in the interior of the matrix: every diagonal present
    print(f"rows {args.rows}, {len(offs)} offsets within +-{args.max_offset}: gaps {gaps.min()}..{gaps.max()}, mean {gaps.mean():.0f}")
    for mb in (float(v) for v in args.l2_mb.split(",")):
        table(args, offs, gaps, begin, mb)


def table(args, offs, gaps, begin, mb):
    cap = int(mb * (1 << 20) / 128)
    reach = cap * 128 // (4 * len(offs))
    print(f"---- LRU of {mb} MB = {cap} lines of x ----")
    print(f"(a) row-major front: {front(offs, begin, begin + args.rows // 8 // 64 * 64, cap):.1f} fetches per line of x "
          f"(1 + the gaps above {reach} rows: {1 + int((gaps > reach).sum())})")
    print("(b) super-block sweep, fetches per line of x (x bytes per launch at 40 MB per fetch of every line); drift in steps,")
    print("    'even': workgroup g of n runs drift * g / (n - 1) behind; 'rand': every workgroup a seeded uniform share of the drift")
    drifts = ((0, False), (1, False), (4, False), (0.5, True), (1, True), (2, True), (4, True))
    print(f"{'R':>3s} {'wg/CU':>5s} {'B rows':>8s} {'closed form':>12s}" + "".join(f"{('rand ' if rnd else 'even ') + str(d):>12s}" for d, rnd in drifts))
    for r, per_cu in [(8, 1), (16, 1), (32, 1), (64, 1)] + [(r, args.wgs_per_cu) for r in (8, 16, 32) if args.wgs_per_cu != 1]:
        wgs = 32 * per_cu
        block = wgs * 4 * r * 64
        closed = 1 + np.minimum(gaps, block).sum() / block
        cells = []
        for drift, rnd in drifts:
            f = sweep(offs, begin, 3, r, drift, cap, wgs, rnd)
            cells.append(f"{f:6.1f} {f * args.rows * 4 / 1e9:4.2f}G")
        print(f"{r:3d} {per_cu:5d} {block:8d} {closed:6.1f} {closed * args.rows * 4 / 1e9:4.2f}G" + "".join(f"{c:>12s}" for c in cells), flush=True)


if __name__ == "__main__":
    main()
