#!/usr/bin/env python3
"""What a step of MINRES costs on one MI355X, next to the SpMV of the same handle, and create plus solve against GMRES(30) and BiCGStab
on a shifted Laplacian -- a symmetric indefinite matrix, where ConjugateGradient does not apply.
Workloads, both fp64, b = A 1, x0 = 0: the 7-point Laplacian minus sigma I, generated on the device as a stencil with diagonal 6 - sigma:
  * small   108^3, sigma = 0.05;
  * large   256^3, sigma = 0.01.
A step is timed as the difference of two fixed-step solves (eps = 0) of c + 1 and c steps (medians of --reps interleaved rounds, each
solve between two HIP events): the set-up and the read-back cancel.  Create plus solve: the handle made from device arrays, then one solve
to --eps with maxIterations = --maxit, between two host clock readings around a device synchronise, for MINRES, GMRES(30) and BiCGStab;
one line per run with the status, the iteration count (SpMVs for MINRES and GMRES, passes of two SpMVs for BiCGStab) and max|x - 1|.
    python tools/minres_timing.py [--reps 7] [--inner 20] [--eps 1e-8] [--maxit 20000] [--only small|large] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"small": 300, "large": 420}  # seconds per child
SHAPES = {"small": (108, 0.05), "large": (256, 0.01)}


def child(kind, reps, inner, eps, maxit):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype, td = np.float64, torch.float64
    nx, sigma = SHAPES[kind]
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(nx, nx, nx, 6.0 - sigma, -1.0, -1.0, d_start, d_pos, d_val, dtype, stream)
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

    def fixed(steps):
        x.zero_()
        done = host.minres_dev(A, b, x, steps, 0.0, None, stream)[1]
        assert done == steps, (done, steps)

    fixed(20)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    y = torch.empty(rows, dtype=td, device=dev)
    spmv = float(np.median([timed(lambda: [A.spmv_dev(smm.OP_ASSIGN, None, b, y, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    print(f"== {kind}: rows {rows}, nnz {nnz}, sigma {sigma}, {np.dtype(dtype).name}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}: {1e3 * spmv:.2f} us per launch; "
          f"{reps} rounds")
    counts = (20, 21, 40, 41)
    t = {c: [] for c in counts}
    for _ in range(reps):
        for c in counts:
            t[c].append(timed(lambda: fixed(c)))
    med = {c: float(np.median(v)) for c, v in t.items()}
    for c in (20, 40):
        print(f"   MINRES step {c:3d}: {1e3 * (med[c + 1] - med[c]):8.2f} us  (solves of {c + 1} and {c} steps: {med[c + 1]:.3f} and {med[c]:.3f} ms)")

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
        print(f"   create + solve to {eps:g}: {name:10s} {float(np.median(t)):9.2f} ms  status {int(st)}  iterations {it:6d}  max|x - 1| {err:.2e}")

    whole("MINRES", lambda H: host.minres_dev(H, b, x, maxit, eps, None, stream))
    whole("GMRES(30)", lambda H: host.gmres_dev(H, b, x, maxit, eps, 30, None, stream))
    whole("BiCGStab", lambda H: host.bicgstab_dev(H, b, x, maxit, eps, None, stream))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner, args.eps, args.maxit)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["small", "large"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps), "--inner", str(args.inner),
               "--eps", repr(args.eps), "--maxit", str(args.maxit)]
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
