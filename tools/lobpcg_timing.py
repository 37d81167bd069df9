#!/usr/bin/env python3
"""What lobpcg costs against eigsh on one MI355X: the 4 smallest eigenpairs of the 7-point Laplacian on a 128^3 and a 256^3 grid, fp64,
tol 1e-8: lobpcg with AMG, with JSWEEP_IC0 and without a preconditioner, and eigsh (ncv = 20).  The set-up of a preconditioner is timed
apart from the solve.  Every solve is capped (--max-iterations, --max-restarts) and reports what it reached: a solve that ends at its cap
is printed as such, not judged.  Then the two block kernels alone at m = l = 24, n = 2^24, fp64 and fp32, against their byte models:
multi_gram reads (m + l) n elements (m n in the symmetric case), multi_block_axpy reads m n + l n and writes l n.
Medians of --reps rounds, each call between two HIP events.
    python tools/lobpcg_timing.py [--reps 3] [--grids 128,256] [--out FILE]
The driver starts one child process per part under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 540  # seconds per child
K, NCV, TOL = 4, 20, 1e-8


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out  # ms


def solves(grid, reps, max_iterations, max_restarts):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype = np.dtype(np.float64)
    rows, nnz = grid**3, host.gen_stencil3d_nnz(grid, grid, grid)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=torch.float64, device=dev)
    host.gen_stencil3d_dev(grid, grid, grid, 6.0, -1.0, -1.0, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    d_w = torch.zeros(K, dtype=torch.float64, device=dev)
    d_X = torch.zeros(K * rows, dtype=torch.float64, device=dev)
    exact = np.sort([6 - 2 * sum(np.cos(np.pi * np.array(ijk) / (grid + 1))) for ijk in ((1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2))])
    host.lobpcg_dev(A, K, "SA", d_w, d_X, rows, tol=TOL, max_iterations=2, seed=1, stream=stream)  # the warm-up: the analysis, the code objects
    print(f"== {grid}^3 fp64: rows {rows}, nnz {nnz}, k {K}, tol {TOL}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}; {reps} rounds")
    for label, kind in (("AMG", "AMG"), ("JSWEEP_IC0", "JSWEEP_IC0"), ("none", None)):
        M, setup = None, 0.0
        if kind:
            t0 = time.perf_counter()
            M = A.getPreconditioner(kind)
            torch.cuda.synchronize()
            setup = (time.perf_counter() - t0) * 1e3
        ms, info = [], None
        for _ in range(reps):
            t, info = timed(torch, lambda: host.lobpcg_dev(A, K, "SA", d_w, d_X, rows, M=M, tol=TOL, max_iterations=max_iterations, seed=1, stream=stream))
            ms.append(t)
        err = float(np.max(np.abs(d_w.cpu().numpy() - exact)))
        print(f"   lobpcg {label:10s}: set-up {setup:9.1f} ms; solve {float(np.median(ms)):10.1f} ms, {info.iterations} iterations, {info.matvecs} SpMVs, "
              f"{info.applies} applies, status {info.status.name}, nconv {info.nconv}, max|theta - lambda| {err:.2e}")
    ms, info = [], None
    for _ in range(reps):
        t, info = timed(torch, lambda: host.eigsh_dev(A, K, "SA", d_w, d_X, rows, ncv=NCV, tol=TOL, max_restarts=max_restarts, seed=1, stream=stream))
        ms.append(t)
    err = float(np.max(np.abs(d_w.cpu().numpy() - exact)))
    print(f"   eigsh  ncv {NCV:6d}: solve {float(np.median(ms)):10.1f} ms, {info.restarts} restarts, {info.matvecs} SpMVs, status {info.status.name}, nconv {info.nconv}, "
          f"max|theta - lambda| {err:.2e}")
    return 0


def kernels(reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, m = 1 << 24, 24
    for dtype, td in ((np.dtype(np.float64), torch.float64), (np.dtype(np.float32), torch.float32)):
        V = torch.randn(m * n, dtype=td, device=dev)
        W = torch.randn(m * n, dtype=td, device=dev)
        G = torch.zeros(m * m, dtype=td, device=dev)
        H = torch.randn(m * m, dtype=td, device=dev) * 1e-3
        runs = (("multi_gram V^T W", lambda: host.multi_gram_dev(n, m, m, V, n, W, n, G, m, dtype, stream), 2 * m * n),
                ("multi_gram V^T V", lambda: host.multi_gram_dev(n, m, m, V, n, V, n, G, m, dtype, stream), m * n),
                ("multi_block_axpy", lambda: host.multi_block_axpy_dev(n, m, m, V, n, H, m, W, n, dtype, stream), 3 * m * n))
        print(f"== the block kernels, {dtype.name}, m = l = {m}, n = 2^24")
        for label, fn, elements in runs:
            fn()
            torch.cuda.synchronize()
            ms = float(np.median([timed(torch, fn)[0] for _ in range(reps)]))
            moved = elements * dtype.itemsize
            print(f"   {label}: {ms:9.3f} ms, {moved / ms / 1e9:.2f} TB/s of the {moved / 1e6:.0f} MB of its byte model")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grids", default="128,256")
    ap.add_argument("--max-iterations", type=int, default=300)
    ap.add_argument("--max-restarts", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child == "kernels":
        return kernels(args.reps)
    if args.child:
        return solves(int(args.child), args.reps, args.max_iterations, args.max_restarts)
    report = []
    status = 0
    for part in ["kernels"] + args.grids.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", part, "--reps", str(args.reps), "--max-iterations",
               str(args.max_iterations), "--max-restarts", str(args.max_restarts)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{part}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
