#!/usr/bin/env python3
"""What the iterated triangular sweeps (SMM_PRECOND_JSWEEP_SGS / _ILU0 / _IC0) buy -- or cost -- on one MI355X, against the exact kinds,
the other preconditioners and the unpreconditioned loops, every leg in one run.  Workloads, fp64, b = A 1, x0 = 0, eps 1e-8:
  * bicgstab  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7): first the APPLY alone -- JSWEEP_ILU0 at
              1 / 1, 2 / 2, 3 / 3 and 4 / 4 steps (set on one handle) beside the byte model of a step, exact ILU0, BLOCK_ILU0,
              MULTICOLOR_ILU0 and one SpMV of the same matrix --, then BiCGStab with none, BLOCK_ILU0, exact ILU0, JSWEEP_ILU0 at 2 / 2 and
              3 / 3 and JSWEEP_SGS at 3 / 3;
  * cg        the 256^3 7-point Laplacian: ConjugateGradient with none, MULTICOLOR_IC0, AMG and JSWEEP_IC0 at 2 / 2 and 3 / 3.
The byte model of one step: nnz_tri (4 + sizeof T) for its triangle, 4 rows of row pointers, and the vectors -- own, the diagonal, the
result and the previous iterate once each, sizeof T per row.  An apply of s / s steps is 2 s steps (SGS / IC0: one element-wise pass more).
Per leg: set-up ms (wall clock around the create, the device drained before and after), us per apply (--inner applies between two HIP
events; median of --reps and the smallest and largest), iterations and ms per solve (median, smallest, largest of --reps solves after
one warm-up solve), and create + solve.
    python tools/jsweep_timing.py [--reps 5] [--inner 20] [--only bicgstab|cg] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bicgstab": 300, "cg": 540}  # seconds per child
EPS = 1e-8
LEGS = {"bicgstab": [("none", None), ("BLOCK_ILU0", None), ("ILU0", None), ("JSWEEP_ILU0", 2), ("JSWEEP_ILU0", 3), ("JSWEEP_SGS", 3)],
        "cg": [("none", None), ("MULTICOLOR_IC0", None), ("AMG", None), ("JSWEEP_IC0", 2), ("JSWEEP_IC0", 3)]}


def spread(ms):
    return f"{float(np.median(ms)):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"


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
    y = torch.empty(rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def solve(M):
        x.zero_()
        if kind == "bicgstab":
            return host.bicgstab_dev(A, b, x, -1, EPS, M, stream)
        return host.cg_dev(A, b, zero, x, -1, EPS, M, stream)

    def per_call_us(fn):
        """us per call: `inner` calls between two events, `reps` times"""
        fn()
        return [1e3 * timed(lambda: [fn() for _ in range(inner)])[0] / inner for _ in range(reps)]

    def make(name, sweeps):
        return A.getPreconditioner(name, sweeps=sweeps) if sweeps else A.getPreconditioner(name)

    size = np.dtype(dtype).itemsize
    tri = (nnz - rows) // 2  # the stencil's pattern is symmetric: either triangle
    step_bytes = tri * (4 + size) + 4 * rows + 4 * size * rows
    print(f"== {kind}: {nx}^3 = {rows} rows, nnz {nnz}, float64, eps {EPS}")
    print(f"   byte model of one step: {tri} entries x {4 + size} + {rows} x (4 + 4 x {size}) = {step_bytes / 1e6:.1f} MB")
    if kind == "bicgstab":
        print("-- the apply alone")
        us = per_call_us(lambda: A.spmv_dev(smm.OP_ASSIGN, None, b, y, stream))
        spmv_bytes = nnz * (4 + size) + 4 * rows + 2 * size * rows
        print(f"   {'one SpMV':<22s} {spread(us)} us   ({spmv_bytes / 1e6:.1f} MB as CSR: {spmv_bytes / np.median(us) / 1e3:7.1f} GB/s; the handle's own kernel may read less)")
        M = make("JSWEEP_ILU0", 3)
        lv = M.jsweep_info()
        for s in (1, 2, 3, 4):
            M.jsweep_set_sweeps(s, s)
            us = per_call_us(lambda: M.apply_dev(b, y, stream))
            med = float(np.median(us))
            print(f"   {f'JSWEEP_ILU0 {s} / {s}':<22s} {spread(us)} us   {2 * s} steps, model {2 * s * step_bytes / 1e6:7.1f} MB = {2 * s * step_bytes / med / 1e3:7.1f} GB/s,"
                  f" {med / (2 * s):7.1f} us per step")
        M.close()
        for name in ("ILU0", "BLOCK_ILU0", "MULTICOLOR_ILU0"):
            M = make(name, None)
            us = per_call_us(lambda: M.apply_dev(b, y, stream))
            print(f"   {name:<22s} {spread(us)} us   levels {M.levels()}")
            M.close()
        print(f"   (levels of the exact sweeps: {lv['levels_lower']} + {lv['levels_upper']})")
        print("-- create + solve")
    for name, sweeps in LEGS[kind]:
        M, create_ms = None, 0.0
        if name != "none":
            create_ms, M = wall(lambda: make(name, sweeps))
        solve(M)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
        runs = [timed(lambda: solve(M)) for _ in range(reps)]
        ms = [r[0] for r in runs]
        st, it = int(runs[-1][1][0]), int(runs[-1][1][1])
        err = float((x - 1).abs().max())
        ap = ""
        if M is not None:
            ap = f"apply {spread(per_call_us(lambda: M.apply_dev(b, y, stream)))} us  "
        label = name + (f" {sweeps} / {sweeps}" if sweeps else "")
        print(f"   {label:<18s} status {st} set-up {create_ms:9.1f} ms  {ap}iterations {it:5d}  solve {spread(ms)} ms  create + solve {create_ms + float(np.median(ms)):9.1f} ms"
              f"  max|x - 1| {err:.2e}", flush=True)
        if M is not None:
            M.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
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
