#!/usr/bin/env python3
"""What a BiCG pass costs on one MI355X, against a pass of the plain BiCGStab loop (smm_hip_bicgstab_resident(OFF)) on the same matrix
in the same run: both run two SpMVs per pass (BiCG one with A and one with the built transpose); BiCG's update and direction kernels
move 15 n vector elements, BiCGStab's three update kernels 14 n.  Workloads as tools/cgs_timing.py:
  * banded    the benchmark's banded generator (gen_banded_dev, 25 offsets per side) at 1 M rows, fp32;
  * convdiff  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7), fp64.
b = A 1, x0 = 0, --passes (200) fixed passes (eps = 0).  A probe run first finds how many passes each loop really executes (a NaN
residual leaves both) and the timed runs plan no more than that.  Per workload a warm-up, then --reps (5) rounds with the two solvers
interleaved, each solve between two HIP events; reported: ms per solve as median [min .. max] and microseconds per pass.
    python tools/bicg_timing.py [--passes 200] [--reps 5] [--only banded|convdiff] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = {"banded": 240, "convdiff": 240}  # seconds per child


def fmt(t):
    return f"{np.median(t):8.3f} [{t.min():7.3f} .. {t.max():7.3f}]"


def child(kind, passes, reps):
    import torch
    from transpose_timing import matrix

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    A, rows, nnz, dtype, td, stream = matrix(kind)
    dev = torch.device("cuda:0")
    T = A.transpose(stream)
    ones = torch.ones(rows, dtype=td, device=dev)
    b = torch.empty(rows, dtype=td, device=dev)
    A.spmv_dev(smm.OP_ASSIGN, None, ones, b, stream)
    x = torch.zeros(rows, dtype=td, device=dev)
    before = host.bicgstab_resident(host.CG_RESIDENT_OFF)
    try:
        def bicg(n):
            x.zero_()
            return host.bicg_dev(A, b, x, n, 0.0, at=T, stream=stream)[1]

        def bicgstab(n):
            x.zero_()
            return host.bicgstab_dev(A, b, x, n, 0.0, None, stream)[1]

        legs = {"bicg": bicg, "bicgstab": bicgstab}
        ran = {name: fn(passes) for name, fn in legs.items()}  # (also the warm-up: the PATTERN analysis, the tile tables, the code objects)
        plan = min(passes, min(ran.values()))
        print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}; SpMV kernel of A {A.kernel_desc()[0]} {A.get_kernel()}, of At {T.kernel_desc()[0]} "
              f"{T.get_kernel()}; of {passes} planned passes bicg ran {ran['bicg']}, bicgstab {ran['bicgstab']}; timing {plan} passes, {reps} interleaved rounds")
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
        print(f"   bicg / bicgstab = {np.median(t['bicg']) / np.median(t['bicgstab']):.3f}")
    finally:
        host.bicgstab_resident(before)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
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
