#!/usr/bin/env python3
"""What the sparse sum C = alpha A + beta B (csrc/smm_add.hip) costs on one MI355X, against the only device route there was before it: the
assembly of the concatenated, scaled triplet list.  Workloads, fp64 and fp32:
  * transpose  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7) plus its transpose;
  * diagonal   the 256^3 7-point Laplacian plus a diagonal matrix.
Per leg: ms (median of --reps calls after one warm-up call, wall time around calls that synchronise), the bytes the header's formulas
give -- create: (nnz_a + nnz_b) 4 symbolic + (nnz_a + nnz_b)(s + 4) fill read, nnz_c (s + 4) written; into: (nnz_a + nnz_b)(s + 4) read,
nnz_c s written -- and what fraction of the copy rate of 6.3 TB/s that is.  The comparison legs: AssemblyPlan.from_device + assemble_dev
(the sort of the list and the gather-and-sum pass), and refill_dev alone.
    python tools/add_timing.py [--reps 7] [--only transpose|diagonal] [--out FILE]
The driver starts one child process per workload and dtype under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"transpose": 240, "diagonal": 420}  # seconds per child
COPY_RATE = 6.3e12  # bytes per second: what a float4 copy reaches on this memory system


def child(kind, dtype_name, reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype = np.dtype(dtype_name).type
    td = torch.float64 if dtype == np.float64 else torch.float32
    s = np.dtype(dtype).itemsize
    nx = 108 if kind == "transpose" else 256
    lo, hi = (-1.3, -0.7) if kind == "transpose" else (-1.0, -1.0)
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    a_dev = [torch.empty(rows + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev)]
    host.gen_stencil3d_dev(nx, nx, nx, 6.0, lo, hi, *a_dev, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, *a_dev, dtype)
    if kind == "transpose":
        B = A.transpose()
        start, pos = B.get_pattern()
        b_dev = [torch.from_numpy(start).to(dev), torch.from_numpy(pos).to(dev), torch.from_numpy(B.get_values()).to(dev)]
        alpha, beta = 1.0, 1.0
    else:
        b_dev = [torch.arange(rows + 1, dtype=torch.int32, device=dev), torch.arange(rows, dtype=torch.int32, device=dev),
                 torch.linspace(0.5, 1.5, rows, dtype=td, device=dev)]
        B = smm.CSRMatrix.from_device(rows, rows, *b_dev, dtype)
        alpha, beta = 1.0, 0.01
    torch.cuda.synchronize()

    def timed(fn):
        fn()  # the warm-up: code objects, the operand check (kept in the handles), the allocator's blocks
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            del out
        return float(np.median(ms)), float(min(ms))

    C = A.add(B, alpha, beta, stream)
    nnz_a, nnz_b, nnz_c = A.nnz, B.nnz, C.nnz
    print(f"== {kind}: {nx}^3 = {rows} rows, {dtype_name}, nnz a {nnz_a} b {nnz_b} c {nnz_c}", flush=True)

    def report(name, ms, best, bytes_moved=None):
        line = f"   {name:<34s} {ms:9.3f} ms (best {best:9.3f})"
        if bytes_moved:
            line += f"  {bytes_moved / 1e9:7.3f} GB by the formulas  {bytes_moved / (ms * 1e-3) / COPY_RATE:5.2f} of the copy rate"
        print(line, flush=True)

    create_bytes = (nnz_a + nnz_b) * 4 + (nnz_a + nnz_b) * (s + 4) + nnz_c * (s + 4)
    into_bytes = (nnz_a + nnz_b) * (s + 4) + nnz_c * s
    report("add (create)", *timed(lambda: A.add(B, alpha, beta, stream)), create_bytes)
    report("add_into", *timed(lambda: C.add_into(A, B, alpha, beta, stream)), into_bytes)

    # the route there was before: the triplets of a scaled by alpha, then those of b scaled by beta, assembled
    def row_index(start_t):
        return torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), (start_t[1:] - start_t[:-1]).to(torch.int64))

    r = torch.cat([row_index(a_dev[0]), row_index(b_dev[0])])
    c = torch.cat([a_dev[1], b_dev[1]])
    v = torch.cat([a_dev[2] * alpha, b_dev[2] * beta])
    torch.cuda.synchronize()
    n = int(r.numel())

    def plan_and_assemble():
        plan = smm.AssemblyPlan.from_device(rows, rows, n, r, c, stream)
        return plan, plan.assemble_dev(v, dtype, stream)

    report("assembly: plan + csr_create", *timed(plan_and_assemble))
    plan, T = plan_and_assemble()
    report("assembly: refill alone", *timed(lambda: plan.refill_dev(T, v, stream=stream)))
    same = T.nnz == nnz_c and bool(np.array_equal(T.get_values().view(np.uint8), A.add(B, alpha, beta, stream).get_values().view(np.uint8)))
    print(f"   the two routes agree bit for bit: {same}", flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.dtype, args.reps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["transpose", "diagonal"]):
        for dtype in ("float64", "float32"):
            cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--dtype", dtype, "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            report.append(r.stdout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                print(f"{kind} {dtype}: exit status {r.returncode}; stopping here")
                report.append(f"{kind} {dtype}: exit status {r.returncode}\n")
                status = r.returncode
                break
        if status:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
