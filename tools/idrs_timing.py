#!/usr/bin/env python3
"""What a step of IDR(s) costs on one MI355X, next to the SpMV of the same handle, and create plus solve against BiCGStab and GMRES(30).
Workloads, both fp64, b = A 1, x0 = 0:
  * convdiff  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7);
  * laplace   the 256^3 7-point Laplacian (diag 6, off-diagonals -1).
A step is timed as the difference of two fixed-step solves (eps = 0), one of c + 1 and one of c steps, at c inside the first cycle, on
its dimension-reduction step and in the second cycle (medians of --reps interleaved rounds, each solve between two HIP events): the
set-up, the shadow space and the read-back cancel.  Create plus solve: the handle made from device arrays, then one solve to --eps with
maxIterations = -1, between two host clock readings around a device synchronise, for IDR(s) at s = 1, 4, 8, BiCGStab and GMRES(30);
the status, the iteration count of each method (SpMVs for IDR(s) and GMRES, passes of two SpMVs for BiCGStab) and max|x - 1| beside it.
    python tools/idrs_timing.py [--reps 7] [--inner 20] [--eps 1e-8] [--only convdiff|laplace] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"convdiff": 300, "laplace": 420}  # seconds per child
S_VALUES = (1, 4, 8)


def child(kind, reps, inner, eps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype, td = np.float64, torch.float64
    nx, lo, hi = (108, -1.3, -0.7) if kind == "convdiff" else (256, -1.0, -1.0)
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(nx, nx, nx, 6.0, lo, hi, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()

    def create():
        return smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)

    A = create()
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

    def fixed(s, steps):
        x.zero_()
        done = host.idrs_dev(A, b, x, steps, 0.0, s, None, None, 0, 0, stream)[1]
        assert done == steps, (done, steps)

    fixed(4, 10)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    y = torch.empty(rows, dtype=td, device=dev)
    spmv = float(np.median([timed(lambda: [A.spmv_dev(smm.OP_ASSIGN, None, b, y, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}: {1e3 * spmv:.2f} us per launch; {reps} rounds")
    for s in S_VALUES:
        at = {"inner step k = 0": 0, f"inner step k = {s - 1}": s - 1, "reduction step": s, "second cycle, k = 0": s + 1}
        counts = sorted({c + d for c in at.values() for d in (0, 1)})
        t = {c: [] for c in counts}
        for _ in range(reps):
            for c in counts:
                t[c].append(timed(lambda: fixed(s, c)))
        med = {c: float(np.median(v)) for c, v in t.items()}
        for name, c in at.items():
            print(f"   IDR({s}) {name:22s}: {1e3 * (med[c + 1] - med[c]):8.2f} us  (solves of {c + 1} and {c} steps: {med[c + 1]:.3f} and {med[c]:.3f} ms)")

    def whole(name, solve):
        t = []
        for _ in range(max(3, reps // 2)):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            H = create()
            st, it, _ = solve(H)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        err = float((x - 1).abs().max())
        print(f"   create + solve to {eps:g}: {name:10s} {float(np.median(t)):9.2f} ms  status {int(st)}  iterations {it:5d}  max|x - 1| {err:.2e}")

    for s in S_VALUES:
        whole(f"IDR({s})", lambda H, s=s: host.idrs_dev(H, b, x, -1, eps, s, None, None, 0, 0, stream))
    whole("BiCGStab", lambda H: host.bicgstab_dev(H, b, x, -1, eps, None, stream))
    whole("GMRES(30)", lambda H: host.gmres_dev(H, b, x, -1, eps, 30, None, stream))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner, args.eps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["convdiff", "laplace"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps), "--inner", str(args.inner),
               "--eps", repr(args.eps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{kind}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
