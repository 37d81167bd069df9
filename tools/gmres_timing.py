#!/usr/bin/env python3
"""What an Arnoldi step of GMRES(30) costs on one MI355X, next to the SpMV of the same handle, and how close the two Gram-Schmidt
kernels come to the memory system's 8 TB/s.  Workloads:
  * banded    the benchmark's banded generator (gen_banded_dev, 25 offsets per side) at 1 M rows, fp32;
  * convdiff  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7), fp64.
b = A 1, x0 = 0, eps = 0, restart 30.  A step at j is timed as the difference of two single-cycle solves, one of j + 1 and one of j
steps (medians of --reps interleaved rounds, each solve between two HIP events): the set-up, the cycle end and the residual cancel.
The kernels: smm_hip_multi_dot_dev / smm_hip_multi_axpy_dev on a basis of k = j + 1 columns of n elements, --inner launches between two
events; bytes counted as the algorithm needs them, (k + 1) n s for the products (V and w once) and (k + 2) n s for the update (V, w in,
w out).
    python tools/gmres_timing.py [--reps 7] [--inner 20] [--only banded|convdiff] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"banded": 240, "convdiff": 240}  # seconds per child
RESTART = 30
JS = (0, 15, 29)
PEAK = 8.0e12  # bytes per second


def child(kind, reps, inner):
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
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    if kind == "banded":
        host.gen_banded_dev(rows, kk, seed, maxoff, d_start, d_pos, d_val, dtype, stream)
    else:
        host.gen_stencil3d_dev(nx, nx, nx, 6.0, -1.3, -0.7, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    ones = torch.ones(rows, dtype=td, device=dev)
    b = torch.empty(rows, dtype=td, device=dev)
    A.spmv_dev(smm.OP_ASSIGN, None, ones, b, stream)
    x = torch.zeros(rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    def solve(steps):
        x.zero_()
        done = host.gmres_dev(A, b, x, steps, 0.0, RESTART, None, stream)[1]
        assert done == steps, (done, steps)

    solve(RESTART)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    counts = sorted({j + d for j in JS for d in (0, 1)})
    t = {c: [] for c in counts}
    for _ in range(reps):
        for c in counts:
            t[c].append(timed(lambda: solve(c)))
    med = {c: float(np.median(v)) for c, v in t.items()}
    y = torch.empty(rows, dtype=td, device=dev)
    spmv = float(np.median([timed(lambda: [A.spmv_dev(smm.OP_ASSIGN, None, b, y, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}: {1e3 * spmv:.2f} us per launch; "
          f"GMRES({RESTART}), {reps} rounds")
    for j in JS:
        print(f"   step at j = {j:2d}: {1e3 * (med[j + 1] - med[j]):8.2f} us  (solves of {j + 1} and {j} steps: {med[j + 1]:.3f} and {med[j]:.3f} ms)")
    size = np.dtype(dtype).itemsize
    ld = (rows + 63) // 64 * 64
    V = torch.rand((max(JS) + 1, ld), dtype=td, device=dev) - 0.5
    w = torch.rand(rows, dtype=td, device=dev)
    out = torch.empty(max(JS) + 1, dtype=td, device=dev)
    coef = torch.full((max(JS) + 1,), 1e-3, dtype=td, device=dev)
    for j in JS:
        k = j + 1
        dot = float(np.median([timed(lambda: [host.multi_dot_dev(rows, k, V, ld, w, out, dtype, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
        axpy = float(np.median([timed(lambda: [host.multi_axpy_dev(rows, k, V, ld, coef, w, y, dtype, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
        bd, ba = (k + 1) * rows * size, (k + 2) * rows * size
        print(f"   k = {k:2d}: multi_dot (with its finish launch) {1e3 * dot:8.2f} us = {bd / (dot * 1e-3) / PEAK:5.1%} of 8 TB/s; "
              f"multi_axpy {1e3 * axpy:8.2f} us = {ba / (axpy * 1e-3) / PEAK:5.1%}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["banded", "convdiff"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps), "--inner", str(args.inner)]
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
