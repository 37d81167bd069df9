#!/usr/bin/env python3
"""What the multicolour preconditioners (SMM_PRECOND_MULTICOLOR_*) buy -- or cost -- on one MI355X, against the exact triangular kinds,
the block kind, AMG and the unpreconditioned loops, all in ONE run.  Workloads, fp64, b = A 1, x0 = 0, eps 1e-8:
  * bicgstab  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7): BiCGStab with none, SGS, ILU0, BLOCK_ILU0,
              MULTICOLOR_SGS and MULTICOLOR_ILU0;
  * cg        the 256^3 7-point Laplacian: ConjugateGradient with none, IC0, MULTICOLOR_IC0 and AMG.
Per leg: the levels of a sweep (ncolors for the multicolour kinds), set-up ms (wall clock around the create call, the device drained
before and after), us per apply (--inner applies between two HIP events, median of --reps), iterations, ms per solve (median of --reps
solves, each between two events, after one warm-up solve) and create + solve ms.  The exact kinds' kernels are untouched by the
multicolour work, so their figures of the same run are the baseline.
    python tools/multicolor_timing.py [--reps 3] [--inner 10] [--only bicgstab|cg] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bicgstab": 300, "cg": 540}  # seconds per child
KINDS = {"bicgstab": (None, "SYMMETRIC_GAUS_SEIDEL", "ILU0", "BLOCK_ILU0", "MULTICOLOR_SGS", "MULTICOLOR_ILU0"), "cg": (None, "IC0", "MULTICOLOR_IC0", "AMG")}
EPS = 1e-8


def child(kind, reps, inner):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype, td = np.float64, torch.float64
    nx = 108 if kind == "bicgstab" else 256
    lo, hi = (-1.3, -0.7) if kind == "bicgstab" else (-1.0, -1.0)
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(nx, nx, nx, 6.0, lo, hi, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    ones = torch.ones(rows, dtype=td, device=dev)
    b = torch.empty(rows, dtype=td, device=dev)
    A.spmv_dev(smm.OP_ASSIGN, None, ones, b, stream)
    x = torch.zeros(rows, dtype=td, device=dev)
    zero = torch.zeros(rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def solve(M):
        x.zero_()
        if kind == "bicgstab":
            return host.bicgstab_dev(A, b, x, -1, EPS, M, stream)
        return host.cg_dev(A, b, zero, x, -1, EPS, M, stream)

    def leg(name):
        import time

        M, create_ms, levels = None, 0.0, 0
        if name is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = A.getPreconditioner(name)
            torch.cuda.synchronize()
            create_ms = 1e3 * (time.perf_counter() - t0)
            levels = M.amg_info()["levels"] if name == "AMG" else max(M.levels())
        solve(M)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
        runs = [timed(lambda: solve(M)) for _ in range(reps)]
        ms = float(np.median([r[0] for r in runs]))
        st, it = int(runs[-1][1][0]), int(runs[-1][1][1])
        err = float((x - 1).abs().max())
        ap = 0.0
        if M is not None:
            y = torch.empty(rows, dtype=td, device=dev)
            M.apply_dev(b, y, stream)
            ap = float(np.median([timed(lambda: [M.apply_dev(b, y, stream) for _ in range(inner)])[0] for _ in range(reps)])) / inner
            M.take_error(stream)
            M.close()
        print(f"   {name or 'none':<22s} levels {levels:4d}  set-up {create_ms:9.1f} ms  apply {1e3 * ap:9.2f} us  status {st} iterations {it:5d}  solve {ms:9.3f} ms  "
              f"create + solve {create_ms + ms:9.1f} ms  max|x - 1| {err:.2e}", flush=True)

    print(f"== {kind}: {nx}^3 = {rows} rows, nnz {nnz}, float64, eps {EPS}")
    for name in KINDS[kind]:
        leg(name)
    print(f"   SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner)
    report = []
    status = 0
    for kind in [args.only] if args.only else ["bicgstab", "cg"]:
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
