#!/usr/bin/env python3
"""What a ConjugateGradientSquared pass costs on one MI355X, against a pass of the plain BiCGStab loop (smm_hip_bicgstab_resident(OFF))
on the same matrix: both run two SpMVs per pass; CGS's two update kernels move 11 n vector elements, BiCGStab's three 14 n.  Workloads:
  * banded    the benchmark's banded generator (gen_banded_dev, 25 offsets per side) at 1 M rows, fp32;
  * convdiff  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7), fp64.
b = A 1, x0 = 0, --passes (200) fixed passes (eps = 0).  Neither loop has a breakdown test and a NaN residual leaves both, so a probe
run first finds how many passes each really executes and the timed runs plan no more than that: every timed pass is a real one.  Per
workload a warm-up, then --reps rounds with the two solvers interleaved, each solve between two HIP events; reported: ms per solve as
median [min .. max] and microseconds per pass.
    python tools/cgs_timing.py [--passes 200] [--reps 7] [--only banded|convdiff] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails.  For the time of each of
the four launches of a pass, run one child under the profiler:  rocprofv3 --kernel-trace --stats -- python tools/cgs_timing.py --child banded"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"banded": 240, "convdiff": 240}  # seconds per child


def fmt(t):
    return f"{np.median(t):8.3f} [{t.min():7.3f} .. {t.max():7.3f}]"


def child(kind, passes, reps):
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
    before = host.bicgstab_resident(host.CG_RESIDENT_OFF)
    try:
        def cgs(n):
            x.zero_()
            return host.cgs_dev(A, b, x, n, 0.0, stream)[1]

        def bicgstab(n):
            x.zero_()
            return host.bicgstab_dev(A, b, x, n, 0.0, None, stream)[1]

        legs = {"cgs": cgs, "bicgstab": bicgstab}
        ran = {name: fn(passes) for name, fn in legs.items()}  # (also the warm-up: the PATTERN analysis, the tile tables, the code objects)
        plan = min(passes, min(ran.values()))
        print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}; of {passes} planned passes "
              f"cgs ran {ran['cgs']}, bicgstab {ran['bicgstab']}; timing {plan} passes, {reps} interleaved rounds")
        if plan < 1:
            return 1
        times = {name: [] for name in legs}
        for _ in range(reps):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                done = fn(plan)
                e1.record()
                torch.cuda.synchronize()
                assert done == plan, (name, done, plan)
                times[name].append(e0.elapsed_time(e1))
        t = {name: np.array(v) for name, v in times.items()}
        for name in legs:
            print(f"   {name:9s} {fmt(t[name])} ms per solve = {1e3 * np.median(t[name]) / plan:8.2f} us per pass")
        print(f"   cgs / bicgstab = {np.median(t['cgs']) / np.median(t['bicgstab']):.3f}")
    finally:
        host.bicgstab_resident(before)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.passes, args.reps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["banded", "convdiff"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--passes", str(args.passes), "--reps", str(args.reps)]
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
