#!/usr/bin/env python3
"""What the multigrid preconditioner (SMM_PRECOND_AMG) buys -- or costs -- on one MI355X, against the unpreconditioned loops.  Workloads,
fp64, b = A 1, x0 = 0, eps 1e-8:
  * bicgstab  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7): BiCGStab without a preconditioner -- as
              the launch-per-kernel loop (smm_hip_bicgstab_resident(OFF)) and as a user gets it (AUTO: the single-launch kernel where
              it applies) -- and with the default AMG;
  * cg        the 256^3 7-point Laplacian: ConjugateGradient without a preconditioner and with the default AMG.
Per leg: iterations, ms per solve (median of --reps solves, each between two HIP events, after one warm-up solve), and for AMG the create
time (wall clock around the call, the device drained before and after), the levels and us per apply (--inner applies between two events).
--parent-lib FILE adds the unpreconditioned legs on another build of the library (the parent commit's libsmm_hip.so), each in a
process of its own, in the same session.
    python tools/amg_timing.py [--reps 5] [--inner 20] [--only bicgstab|cg] [--parent-lib FILE] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bicgstab": 240, "cg": 420}  # seconds per child
EPS = 1e-8


def child(kind, reps, inner, baseline_only):
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

    def leg(name, M):
        solve(M)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
        runs = [timed(lambda: solve(M)) for _ in range(reps)]
        ms = float(np.median([r[0] for r in runs]))
        st, it = int(runs[-1][1][0]), int(runs[-1][1][1])
        err = float((x - 1).abs().max())
        line = f"   {name:<28s} status {st} iterations {it:5d}  {ms:9.3f} ms per solve  {1e3 * ms / max(it, 1):8.2f} us per iteration  max|x - 1| {err:.2e}"
        if M is not None:
            y = torch.empty(rows, dtype=td, device=dev)
            M.apply_dev(b, y, stream)
            ap = float(np.median([timed(lambda: [M.apply_dev(b, y, stream) for _ in range(inner)])[0] for _ in range(reps)])) / inner
            line += f"  {1e3 * ap:8.2f} us per apply"
        print(line, flush=True)

    tag = os.environ.get("SMM_HIP_LIBRARY", "this build")
    print(f"== {kind}: {nx}^3 = {rows} rows, nnz {nnz}, float64, eps {EPS}, library: {tag}")
    if kind == "bicgstab":
        previous = host.bicgstab_resident(0)
        leg("none (resident OFF)", None)
        host.bicgstab_resident(1)
        leg("none (resident AUTO)", None)
        host.bicgstab_resident(previous)
    else:
        leg("none", None)
    print(f"   SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}")
    if baseline_only:
        return 0
    import time

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M = A.getPreconditioner("AMG")
    torch.cuda.synchronize()
    create_ms = 1e3 * (time.perf_counter() - t0)
    info = M.amg_info()
    print(f"   amg create {create_ms:9.1f} ms  levels {info['levels']}  rows {info['rows']}  operator complexity {info['operator_complexity']:.3f}", flush=True)
    leg("amg (defaults)", M)
    t0 = time.perf_counter()
    M.amg_refresh()
    torch.cuda.synchronize()
    print(f"   amg refresh {1e3 * (time.perf_counter() - t0):8.1f} ms", flush=True)
    M.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner, args.baseline_only)
    report = []
    status = 0
    legs = [(kind, None) for kind in ([args.only] if args.only else ["bicgstab", "cg"])]
    if args.parent_lib:
        legs = [leg for kind, _ in legs for leg in ((kind, args.parent_lib), (kind, None))]
    for kind, lib in legs:
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps), "--inner", str(args.inner)]
        env = dict(os.environ)
        if lib:
            cmd.append("--baseline-only")
            env["SMM_HIP_LIBRARY"] = os.path.abspath(lib)
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
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
