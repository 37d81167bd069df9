#!/usr/bin/env python3
"""What the BLOCKS SpMV family (SMM_SPMV_BLOCKS: one column index per dense b x b block) buys -- or costs -- on one MI355X against
STREAM at AUTO's lane count, which is what the library ran for such a matrix before the family existed.  Both families run on the SAME
handle.  Cases: b = 3 in fp64 and fp32, b = 2 and b = 4 in fp64; 27 blocks per block row on sorted distinct random block columns (the law
of generators.random_rows, one column per stratum of the block columns so that 10^5 block rows can be drawn in one vectorised step on the
device; the block of the diagonal is always present), at sizes whose CSR arrays exceed the 256 MB Infinity Cache.  Per case and family:
ms per SpMV -- the MEDIAN of --reps readings, each the mean of --inner launches between two HIP events after 3 warm-up launches --, the
bytes smm_hip_csr_kernel_desc prices THAT kernel's launch with, and the TB/s the two give.  The b = 3 fp64 case also runs one BiCGStab
of a fixed 50 iterations (eps 1e-30, b = A 1, x0 = 0) under both families: ms per solve, median of --reps.
    python tools/blocks_timing.py [--reps 7] [--inner 10] [--out FILE]
The driver starts one child process per case under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PER_ROW = 27
# (label, b, dtype, block rows): nnz (s + 4) bytes of CSR arrays = 350 / 291 / 285 / 311 MB
CASES = [("b3_fp64", 3, "float64", 27 * 4444), ("b3_fp32", 3, "float32", 27 * 5556), ("b2_fp64", 2, "float64", 27 * 8149), ("b4_fp64", 4, "float64", 27 * 2223)]
LIMIT = 240  # seconds per child


def child(label, reps, inner):
    import torch

    import sparse_matrix_math_amd as smm

    _, b, dname, nbr = next(c for c in CASES if c[0] == label)
    dtype = np.dtype(dname)
    td = torch.float64 if dname == "float64" else torch.float32
    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(2024 + b)
    # block columns: stratum j of a block row -- block columns [j W, (j + 1) W), W = nbr / 27 -- holds one uniformly drawn column; the
    # stratum of R holds R itself
    assert nbr % PER_ROW == 0
    W = nbr // PER_ROW
    j = torch.arange(PER_ROW, device=dev, dtype=torch.int64)[None, :]
    u = torch.rand((nbr, PER_ROW), generator=g, device=dev, dtype=torch.float64)
    bc = j * W + torch.clamp((u * W).floor().to(torch.int64), max=W - 1)
    R = torch.arange(nbr, device=dev, dtype=torch.int64)
    own = R // W
    bc[R, own] = R
    assert bool((bc[:, 1:] > bc[:, :-1]).all())
    rows = nbr * b
    len_row = PER_ROW * b
    pos = (bc[:, None, :, None] * b + torch.arange(b, device=dev)[None, None, None, :]).expand(nbr, b, PER_ROW, b).reshape(rows, len_row)
    val = (torch.rand((rows, len_row), generator=g, device=dev, dtype=torch.float64) * 2 - 1)
    diag_at = (own[:, None] * b + torch.arange(b, device=dev)[None, :]).reshape(rows)  # entry of column r in row r
    r_all = torch.arange(rows, device=dev)
    assert bool((pos[r_all, diag_at] == r_all).all())
    val[r_all, diag_at] = 0.0
    val[r_all, diag_at] = val.abs().sum(dim=1) + 1.0  # diagonally dominant: BiCGStab can run on it
    d_start = (torch.arange(rows + 1, device=dev, dtype=torch.int64) * len_row).to(torch.int32)
    d_pos = pos.reshape(-1).to(torch.int32).contiguous()
    d_val = val.reshape(-1).to(td).contiguous()
    del pos, val, u, bc
    torch.cuda.synchronize()
    nnz = rows * len_row
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    A.set_kernel(smm.SPMV_AUTO)
    auto = A.get_kernel()
    assert auto[0] == smm.SPMV_STREAM, auto
    assert A.find_blocks(0) == b, A.blocks_info()
    x = torch.rand(rows, generator=g, device=dev, dtype=torch.float64).to(td)
    y = torch.empty(rows, dtype=td, device=dev)
    ones = torch.ones(rows, dtype=td, device=dev)
    rhs = torch.empty(rows, dtype=td, device=dev)
    print(f"case {label}: b {b} {dname} block rows {nbr} rows {rows} nnz {nnz} CSR arrays {nnz * (dtype.itemsize + 4) / 1e6:.0f} MB; AUTO runs STREAM at {auto[1]} lanes per row")

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

    results, outs = {}, {}
    for family in ("STREAM", "BLOCKS"):
        if family == "STREAM":
            A.set_kernel(smm.SPMV_STREAM, auto[1])
        else:
            A.set_kernel(smm.SPMV_BLOCKS)
        name, nbytes = A.kernel_desc()
        med, lo_ms, hi_ms = spmv_ms()
        outs[family] = y.clone()
        results[family] = med
        print(f"  spmv {family:6s} {name:18s} lanes {A.get_kernel()[1]}  {med:8.4f} ms (min {lo_ms:.4f} max {hi_ms:.4f}, median of {reps} x {inner})  "
              f"bytes {nbytes}  {nbytes / med / 1e9:6.3f} TB/s")
    scale = float(outs["STREAM"].abs().max())
    print(f"  spmv BLOCKS / STREAM time ratio {results['BLOCKS'] / results['STREAM']:.3f}  (STREAM / BLOCKS {results['STREAM'] / results['BLOCKS']:.3f}); "
          f"max |y_B - y_S| / max|y| {float((outs['BLOCKS'] - outs['STREAM']).abs().max()) / scale:.2e} (STREAM at {auto[1]} lanes sums a row in pieces)")
    if label == "b3_fp64":
        A.spmv_dev(smm.OP_ASSIGN, None, ones, rhs, stream)
        torch.cuda.synchronize()
        solve = {}
        for family in ("STREAM", "BLOCKS"):
            if family == "STREAM":
                A.set_kernel(smm.SPMV_STREAM, auto[1])
            else:
                A.set_kernel(smm.SPMV_BLOCKS)
            readings = []
            for rep in range(reps + 1):
                sol = torch.zeros(rows, dtype=td, device=dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st, it, _ = smm.bicgstab_dev(A, rhs, sol, 50, 1e-30, None, stream)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    readings.append(e0.elapsed_time(e1))
            solve[family] = float(np.median(readings))
            print(f"  bicgstab {family:6s} status {int(st)} iterations {it}  {solve[family]:8.3f} ms per solve (median of {reps})  max|x - 1| {float((sol - 1).abs().max()):.2e}")
        print(f"  bicgstab BLOCKS / STREAM time ratio {solve['BLOCKS'] / solve['STREAM']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.inner)
        return 0
    text = []
    for label, *_ in CASES:
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
            f.write("tools/blocks_timing.py --reps %d --inner %d   (one MI355X)\n" % (args.reps, args.inner))
            f.write("".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
