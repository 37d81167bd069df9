#!/usr/bin/env python3
"""What the device transpose costs on one MI355X: smm_hip_csr_transpose_create and smm_hip_csr_transpose_refresh_* on the benchmark's
banded matrix (gen_banded_dev, 25 offsets per side, 1 M rows, fp32) and on the 108^3 convection-diffusion stencil in fp64.  After a
warm-up, HIP events around 5 synchronised calls of each; reported: the median [min .. max] in ms, and for the refresh the effective
bandwidth of its nnz (2 s + 4) bytes against the 8 TB/s peak.
    python tools/transpose_timing.py [--reps 5] [--only banded|convdiff] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"banded": 240, "convdiff": 240}  # seconds per child
PEAK = 8.0e12


def fmt(t):
    return f"{np.median(t):8.3f} [{t.min():7.3f} .. {t.max():7.3f}]"


def matrix(kind):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "banded":
        dtype, td = np.float32, torch.float32
        rows, kk, seed, maxoff = 1_000_000, 25, 0x5EED, 1 << 20
        nnz = host.gen_banded_nnz(rows, kk, seed, maxoff)
    else:
        dtype, td = np.float64, torch.float64
        nx = 108
        rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    keep = (torch.empty(rows + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev))
    if kind == "banded":
        host.gen_banded_dev(rows, kk, seed, maxoff, *keep, dtype, stream)
    else:
        host.gen_stencil3d_dev(nx, nx, nx, 6.0, -1.3, -0.7, *keep, dtype, stream)
    torch.cuda.synchronize()
    return smm.CSRMatrix.from_device(rows, rows, *keep, dtype), rows, nnz, dtype, td, stream


def timed(fn, reps):
    import torch

    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.array(out)


def child(kind, reps):
    A, rows, nnz, dtype, _, stream = matrix(kind)
    s = np.dtype(dtype).itemsize
    T = A.transpose(stream)  # warm-up: the code object, the allocator's blocks
    T.transpose_refresh(A, stream)
    made = []
    t_create = timed(lambda: made.append(A.transpose(stream)), reps)
    t_refresh = timed(lambda: T.transpose_refresh(A, stream), reps)
    nbytes = nnz * (2 * s + 4)
    print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}")
    print(f"   transpose_create  {fmt(t_create)} ms")
    print(f"   transpose_refresh {fmt(t_refresh)} ms = {nbytes / (1e-3 * np.median(t_refresh)) / 1e12:6.3f} TB/s over nnz (2 s + 4) = {nbytes / 1e6:.1f} MB "
          f"({100 * nbytes / (1e-3 * np.median(t_refresh)) / PEAK:.1f} % of 8 TB/s)")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["banded", "convdiff"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{kind}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
