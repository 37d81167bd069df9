#!/usr/bin/env python3
"""What the LONGROWS SpMV family (SMM_SPMV_LONGROWS: rows past split_len cut into segments that the whole device sums) buys -- or costs --
on one MI355X against STREAM at AUTO's lane count, which is what the library ran for such a matrix before the family existed.  Both
families run on the SAME handle; matrices are built on the device with torch.  Cases (fp64):
  a  arrow / KKT shape: the 7-point stencil of a 161^3 grid (4.17 M rows) plus 4 dense rows and their columns;
  b  the transpose handle of tools/lsqr_timing.py's tall matrix [I; Dx; Dy; Dz] of a 160^3 grid with one dense column added to A: the
     last row of the transpose holds 16.3 M entries;
  c  20000 ragged rows of 1 .. 2000 entries (about 20 M), split_len at its maximum so that NO row is split: the family's overhead on a
     matrix it has nothing to do for, against STREAM at one lane per row (the same arithmetic) and at AUTO's lanes;
  d  case a again at segment_len 256, 512, 1024 and 2048.
Cases b and c are STAND-INS built on the device: b restates the construction of tools/lsqr_timing.py's tall_on_device with the extra column
(the tool is not imported), c draws its columns one per stratum of 524 instead of calling generators.random_rows (a host loop over rows,
too slow for 20 M entries); the row lengths and the shapes are the ones named.
Per case and family: ms per SpMV -- the MEDIAN of --reps readings, each the mean of --inner launches between two HIP events after 3
warm-up launches --, the bytes smm_hip_csr_kernel_desc prices THAT launch with, and the TB/s the two give.
    python tools/longrows_timing.py [--reps 7] [--inner 10] [--cases abcd] [--out FILE]
The driver starts one child process per case under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 240  # seconds per child


def arrow_on_device(n, dense, td, dev):
    """the 7-point stencil of an n^3 grid bordered by `dense` dense rows and columns: (rows, start, positions, values)"""
    import torch

    N = n**3
    i = torch.arange(N, dtype=torch.int64, device=dev)
    ix, iy, iz = i % n, (i // n) % n, i // (n * n)
    cand = [(i - n * n, iz > 0, -1.0), (i - n, iy > 0, -1.0), (i - 1, ix > 0, -1.0), (i, torch.ones_like(i, dtype=torch.bool), 6.0 + dense),
            (i + 1, ix < n - 1, -1.0), (i + n, iy < n - 1, -1.0), (i + n * n, iz < n - 1, -1.0)]
    cand += [(torch.full_like(i, N + k), torch.ones_like(i, dtype=torch.bool), 0.25) for k in range(dense)]
    cols = torch.stack([c for c, _, _ in cand], dim=1)
    valid = torch.stack([m for _, m, _ in cand], dim=1)
    vals = torch.tensor([v for _, _, v in cand], dtype=td, device=dev)[None, :].expand(N, len(cand))
    lens = torch.cat([valid.sum(dim=1), torch.full((dense,), N + dense, dtype=torch.int64, device=dev)])
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    border = torch.arange(N + dense, dtype=torch.int64, device=dev).repeat(dense)
    bval = torch.full((dense * (N + dense),), 0.25, dtype=td, device=dev)
    for k in range(dense):
        bval[k * (N + dense) + N + k] = float(N)  # the diagonal of a dense row
    return N + dense, start.to(torch.int32), torch.cat([cols[valid], border]).to(torch.int32), torch.cat([vals[valid], bval])


def tall_with_dense_column(n, td, dev):
    """tools/lsqr_timing.py's [I; Dx; Dy; Dz] with one more column that every row holds: (rows, cols, start, positions, values)"""
    import torch

    cols = n**3
    idx = torch.arange(cols, dtype=torch.int64, device=dev)
    last = torch.full_like(idx, cols)
    pos = [torch.stack([idx, last], dim=1).reshape(-1)]
    val = [torch.tensor([1.0, 0.5], dtype=td, device=dev).repeat(cols)]
    pairs = 0
    for stride in (1, n, n * n):
        sel = idx[(idx // stride) % n < n - 1]
        pos.append(torch.stack([sel, sel + stride, torch.full_like(sel, cols)], dim=1).reshape(-1))
        val.append(torch.tensor([-1.0, 1.0, 0.5], dtype=td, device=dev).repeat(len(sel)))
        pairs += len(sel)
    start = torch.cat([2 * torch.arange(cols + 1, dtype=torch.int64, device=dev), 2 * cols + 3 * torch.arange(1, pairs + 1, dtype=torch.int64, device=dev)])
    return cols + pairs, cols + 1, start.to(torch.int32), torch.cat(pos).to(torch.int32), torch.cat(val)


def ragged_on_device(rows, max_len, td, dev, g):
    """rows of 1 .. max_len entries on strictly ascending random columns (one per stratum of 524 columns): (cols, start, positions, values)"""
    import torch

    width = 524
    lens = torch.randint(1, max_len + 1, (rows,), generator=g, device=dev, dtype=torch.int64)
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    nnz = int(start[-1])
    row = torch.repeat_interleave(torch.arange(rows, device=dev), lens)
    k = torch.arange(nnz, device=dev, dtype=torch.int64) - start[row]
    pos = k * width + torch.randint(0, width, (nnz,), generator=g, device=dev, dtype=torch.int64)
    val = torch.rand(nnz, generator=g, device=dev, dtype=torch.float64).to(td) * 2 - 1
    return max_len * width, start.to(torch.int32), pos.to(torch.int32), val


def child(label, reps, inner):
    import torch

    import sparse_matrix_math_amd as smm

    dtype, td = np.dtype("float64"), torch.float64
    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(2025)
    keep = None
    if label in ("a", "d"):
        rows, d_start, d_pos, d_val = arrow_on_device(161, 4, td, dev)
        cols = rows
        A = smm.CSRMatrix.from_device(rows, cols, d_start, d_pos, d_val, dtype)
        what = "7-point stencil of 161^3 + 4 dense rows and columns"
    elif label == "b":
        r0, c0, d_start, d_pos, d_val = tall_with_dense_column(160, td, dev)
        keep = smm.CSRMatrix.from_device(r0, c0, d_start, d_pos, d_val, dtype)
        A = keep.transpose(stream)
        rows, cols = c0, r0
        what = "transpose of [I; Dx; Dy; Dz] of 160^3 with a dense column"
    else:
        rows = 20000
        cols, d_start, d_pos, d_val = ragged_on_device(rows, 2000, td, dev, g)
        A = smm.CSRMatrix.from_device(rows, cols, d_start, d_pos, d_val, dtype)
        what = "ragged rows of 1 .. 2000 entries, none split"
    torch.cuda.synchronize()
    A.set_kernel(smm.SPMV_AUTO)
    auto = A.get_kernel()
    assert auto[0] == smm.SPMV_STREAM, auto
    x = torch.rand(cols, generator=g, device=dev, dtype=torch.float64).to(td)
    y = torch.empty(rows, dtype=td, device=dev)
    print(f"case {label}: {what}: {rows} x {cols}, nnz {A.nnz}, {dtype.name}; AUTO runs STREAM at {auto[1]} lanes per row")

    def spmv_ms():
        for _ in range(3):
            A.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)
        readings = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                A.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)
            e1.record()
            torch.cuda.synchronize()
            readings.append(e0.elapsed_time(e1) / inner)
        return float(np.median(readings)), min(readings), max(readings)

    def measure(tag):
        name, nbytes = A.kernel_desc()
        med, lo_ms, hi_ms = spmv_ms()
        print(f"  spmv {tag:28s} {name:18s} {med:9.4f} ms (min {lo_ms:.4f} max {hi_ms:.4f}, median of {reps} x {inner})  bytes {nbytes}  {nbytes / med / 1e9:6.3f} TB/s")
        return med, y.clone()

    A.set_kernel(smm.SPMV_STREAM, auto[1])
    t_stream, y_stream = measure(f"STREAM {auto[1]} lanes (AUTO)")
    scale = float(y_stream.abs().max())
    if label == "c":
        A.set_kernel(smm.SPMV_STREAM, 1)
        t_one, y_one = measure("STREAM 1 lane")
        A.longrows_configure(2045, 0)
        A.set_kernel(smm.SPMV_LONGROWS)
        t_long, y_long = measure("LONGROWS split 2045")
        assert A.longrows_info()[2] == 0 and bool((y_long == y_one).all())
        print(f"  STREAM(1 lane) / LONGROWS {t_one / t_long:.3f}   STREAM(AUTO) / LONGROWS {t_stream / t_long:.3f}   (no row split: the bits of STREAM at one lane)")
        return
    for seg in ((0,) if label != "d" else (256, 512, 1024, 2048)):
        A.longrows_configure(0, seg)
        A.set_kernel(smm.SPMV_LONGROWS)
        S, G, nlong, nseg = A.longrows_info()
        t_long, y_long = measure(f"LONGROWS split {S} segment {G}")
        print(f"  long rows {nlong} segments {nseg}   STREAM(AUTO) / LONGROWS {t_stream / t_long:.3f}   max |y_L - y_S| / max|y| {float((y_long - y_stream).abs().max()) / scale:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.inner)
        return 0
    text = []
    for label in args.cases:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", label, "--reps", str(args.reps), "--inner", str(args.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        text.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"case {label} ended with status {r.returncode}: stopping")
            return 1
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/longrows_timing.py --reps %d --inner %d   (one MI355X)\n" % (args.reps, args.inner))
            f.write("".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
