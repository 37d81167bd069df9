#!/usr/bin/env python3
"""What mixed-precision iterative refinement (smm_hip_refine_f64) buys -- or costs -- on one MI355X against the fp64 solve it replaces.
Workloads, fp64, b = A 1, x0 = 0, eps 1e-8:
  * lap256  the 256^3 7-point Laplacian: ConjugateGradient, without a preconditioner and with the default AMG;
  * lap512  the 512^3 7-point Laplacian: ConjugateGradient without a preconditioner;
  * cd108   the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7): BiCGStab without a preconditioner and with
            JACOBI.
Per workload and preconditioner: the existing fp64 solve (the baseline: the parent commit's code), then IterativeRefinement with a KEPT
fp32 matrix (and the fp32 preconditioner made for it) at innerEps 1e-2 and 1e-4.  Per leg: status, iterations (fp64: the solver's; refined:
outer / inner), ms per solve (median of --reps solves, each between two HIP events, after one warm-up solve that pays the PATTERN
analysis and the code objects) and the true ||b - A x|| of the result, recomputed in fp64 by an SpMV.  The conversion (astype) and the
preconditioner's create are timed once, by wall clock with the device drained, and are not part of a solve's time.
    python tools/refine_timing.py [--reps 3] [--only lap256|lap512|cd108] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"lap256": 300, "lap512": 540, "cd108": 240}  # seconds per child
EPS = 1e-8


def child(kind, reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    td = torch.float64
    nx = {"lap256": 256, "lap512": 512, "cd108": 108}[kind]
    lo, hi = (-1.3, -0.7) if kind == "cd108" else (-1.0, -1.0)
    inner = "BICGSTAB" if kind == "cd108" else "CG"
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(nx, nx, nx, 6.0, lo, hi, d_start, d_pos, d_val, np.float64, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, np.float64)
    b = torch.empty(rows, dtype=td, device=dev)
    A.spmv_dev(smm.OP_ASSIGN, None, torch.ones(rows, dtype=td, device=dev), b, stream)
    x = torch.zeros(rows, dtype=td, device=dev)
    zero = torch.zeros(rows, dtype=td, device=dev)
    r = torch.empty(rows, dtype=td, device=dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def residual():
        A.spmv_dev(smm.OP_SUB, b, x, r, stream)
        torch.cuda.synchronize()
        return float(torch.linalg.vector_norm(r))

    def leg(name, solve):
        def run():
            x.zero_()
            return solve()

        run()  # the warm-up
        runs = [timed(run) for _ in range(reps)]
        ms = float(np.median([t for t, _ in runs]))
        out = runs[-1][1]
        its = f"iterations {int(out[1]):6d}" if len(out) == 3 else f"outer {int(out[1]):2d} inner {int(out[2]):6d}"
        print(f"   {name:<34s} status {int(out[0])} {its:<28s} {ms:10.3f} ms per solve  true residual {residual():.3e}  max|x - 1| {float((x - 1).abs().max()):.2e}", flush=True)

    print(f"== {kind}: {nx}^3 = {rows} rows, nnz {nnz}, eps {EPS}, inner solver {inner}")
    ms, A32 = wall(lambda: A.astype(np.float32))
    print(f"   astype(float32) {ms:9.2f} ms (the pattern copied, {nnz} values converted)", flush=True)
    for pname in ["none"] + ({"lap256": ["AMG"], "cd108": ["JACOBI"]}.get(kind, [])):
        M = M32 = None
        if pname != "none":
            ms, M = wall(lambda: A.getPreconditioner(pname))
            ms32, M32 = wall(lambda: A32.getPreconditioner(pname))
            print(f"   {pname} create: fp64 {ms:9.1f} ms, fp32 {ms32:9.1f} ms", flush=True)
        if inner == "CG":
            leg(f"fp64 CG, {pname}", lambda: host.cg_dev(A, b, zero, x, -1, EPS, M, stream))
        else:
            leg(f"fp64 BiCGStab, {pname}", lambda: host.bicgstab_dev(A, b, x, -1, EPS, M, stream))
        for inner_eps in (1e-2, 1e-4):
            leg(f"refined, {pname}, innerEps {inner_eps:g}", lambda: host.refine_dev(A, b, x, EPS, inner=inner, a32=A32, M=M32, innerEps=inner_eps, stream=stream))
        print(f"   SpMV kernels: fp64 {A.kernel_desc()[0]} {A.get_kernel()}, fp32 {A32.kernel_desc()[0]} {A32.get_kernel()}", flush=True)
        for P in (M, M32):
            if P is not None:
                P.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    report = []
    status = 0
    for kind in [args.only] if args.only else ["cd108", "lap256", "lap512"]:
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        report.append(r.stdout)
        if args.out:
            with open(args.out, "w") as f:
                f.write("".join(report))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{kind}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    return status


if __name__ == "__main__":
    sys.exit(main())
