#!/usr/bin/env python3
"""What a cycle and a restart of eigsh cost on one MI355X: the 7-point Laplacian on a 256^3 grid generated on the device, k = 4,
ncv = 20, LARGEST and SMALLEST, fp64 and fp32.
A solve with max_restarts = r runs the first cycle (ncv steps) and r further cycles of ncv - l steps, each behind one restart (the host's
Ritz step, the compression kernel, one column copy); with --tol far below what r restarts can reach none of them converges, so the
difference of the solves with r + 1 and r restarts is one restart plus one later cycle, and the solve with r = 0 is the first cycle plus
the set-up and the read-back.  The compression kernel alone is timed through multi_rotate_dev on a basis of the same shape.  Medians of
--reps interleaved rounds, each solve between two HIP events.  The eigenvalues reached and their estimates are printed, not judged: the
small end of this spectrum converges slowly, as with any plain Lanczos.
    python tools/eigsh_timing.py [--reps 5] [--grid 256] [--out FILE]
The driver starts one child process per dtype under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 420  # seconds per child
K, NCV = 4, 20


def child(name, reps, grid):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype = np.dtype(name)
    td = torch.float64 if dtype == np.float64 else torch.float32
    rows, nnz = grid**3, host.gen_stencil3d_nnz(grid, grid, grid)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(grid, grid, grid, 6.0, -1.0, -1.0, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    d_w = torch.zeros(K, dtype=td, device=dev)
    d_X = torch.zeros(K * rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def solve(which, restarts):
        return host.eigsh_dev(A, K, which, d_w, d_X, rows, ncv=NCV, tol=1e-30, max_restarts=restarts, seed=1, stream=stream)

    solve("LA", 1)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    print(f"== {dtype.name}: rows {rows}, nnz {nnz}, k {K}, ncv {NCV}; SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}; {reps} rounds")
    l = K + (NCV - K) // 2
    for which in ("LA", "SA"):
        counts = (0, 4, 5)
        t = {c: [] for c in counts}
        for _ in range(reps):
            for c in counts:
                ms, info = timed(lambda: solve(which, c))
                assert info.restarts == c and info.matvecs == NCV + c * (NCV - l), info
                t[c].append(ms)
        med = {c: float(np.median(v)) for c, v in t.items()}
        print(f"   {which}: first cycle of {NCV} steps with set-up and read-back {med[0]:9.3f} ms; one restart + a cycle of {NCV - l} steps {med[5] - med[4]:9.3f} ms "
              f"(solves of 5 and 4 restarts: {med[5]:.3f} and {med[4]:.3f} ms)")
        info = solve(which, 5)
        print(f"       after 5 restarts: w {d_w.cpu().numpy()} estimates {info.residuals} nconv {info.nconv}")
    ld = (rows + 63) // 64 * 64
    V = torch.randn(NCV * ld, dtype=td, device=dev)
    Y = np.linalg.qr(np.random.default_rng(0).standard_normal((NCV, NCV)))[0][:, :l].astype(dtype)
    ms = float(np.median([timed(lambda: host.multi_rotate_dev(rows, NCV, l, V, ld, Y, dtype, stream))[0] for _ in range(reps)]))
    moved = rows * (NCV + l) * dtype.itemsize
    print(f"   multi_rotate {NCV} -> {l} columns: {ms:9.3f} ms, {moved / ms / 1e9:.2f} TB/s of the {moved / 1e6:.0f} MB it must move (the staging of Y and the "
          f"synchronise included)")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--child", choices=["float64", "float32"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.grid)
    report = []
    status = 0
    for name in ("float64", "float32"):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--grid", str(args.grid)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{name}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
