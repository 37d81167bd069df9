#!/usr/bin/env python3
"""What a Golub-Kahan step of svds costs on one MI355X, next to one SpMV on `a` plus one on `at` from the same handles -- the floor a
step cannot beat -- and the cycle's byte model at the measured rate.
Workload, fp64 and fp32: LSQR's large tall matrix (tools/lsqr_timing.py: [I; Dx; Dy; Dz] of an n^3 grid, built on the device), its
transpose kept, k = 4, ncv = 20, no vectors asked for, the hash start vector.
Two figures, medians of --reps rounds, each solve between two HIP events:
  the first cycle     a solve with max_restarts = 0 is ONE cycle of 20 steps (j = 0 .. 19) with its allocations, its one read-back and
                      the small SVD on the host; its time / 20 is the mean step with all of that included
  the restart cycle   the difference of the solves with max_restarts = 1 and 0: the compression of both bases and the 8 steps
                      j = 12 .. 19, whose Gram-Schmidt passes are the longest of the cycle; allocation and set-up cancel
The byte model of step j: the two SpMVs (values, positions and start once each, the input vector once, the
output once) plus (4 j + 8) rows + (4 (j + 1) + 8) cols vector elements of the two orthogonalisations and scalings.
    python tools/svds_timing.py [--n 160] [--reps 5] [--inner 20] [--only f64|f32] [--out FILE]
The driver starts one child process per dtype under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300  # seconds per child
DTYPES = {"f64": np.float64, "f32": np.float32}
K, NCV = 4, 20


def child(kind, n, reps, inner):
    import torch
    from lsqr_timing import tall_on_device

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype = DTYPES[kind]
    td = torch.float64 if dtype == np.float64 else torch.float32
    size = np.dtype(dtype).itemsize
    rows, cols, d_start, d_pos, d_val = tall_on_device(n, td, dev)
    nnz = int(d_pos.numel())
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, cols, d_start, d_pos, d_val, dtype)
    At = A.transpose(stream)
    d_s = torch.zeros(K, dtype=td, device=dev)
    x = torch.ones(cols, dtype=td, device=dev)
    b = torch.ones(rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    seen = {}

    def solve(restarts):
        info = host.svds_dev(A, K, d_s, None, 0, None, 0, ncv=NCV, tol=1e-30, max_restarts=restarts, at=At, stream=stream)
        l = K + (NCV - K) // 2
        assert info.restarts == restarts and info.matvecs == 2 * (NCV + restarts * (NCV - l)), info
        seen[restarts] = float(d_s[0])

    solve(1)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    q = torch.empty(rows, dtype=td, device=dev)
    t = torch.empty(cols, dtype=td, device=dev)
    spmv_a = float(np.median([timed(lambda: [A.spmv_dev(smm.OP_ASSIGN, None, x, q, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    spmv_at = float(np.median([timed(lambda: [At.spmv_dev(smm.OP_ASSIGN, None, b, t, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    print(f"== {kind}: [I; Dx; Dy; Dz] of a {n}^3 grid: {rows} x {cols}, nnz {nnz}, {np.dtype(dtype).name}, k {K}, ncv {NCV}; {reps} rounds")
    print(f"   SpMV on a : {A.kernel_desc()[0]} {A.get_kernel()}: {1e3 * spmv_a:8.2f} us per launch")
    print(f"   SpMV on at: {At.kernel_desc()[0]} {At.get_kernel()}: {1e3 * spmv_at:8.2f} us per launch")
    floor = spmv_a + spmv_at
    took = {0: [], 1: []}
    for _ in range(reps):
        for r in (0, 1):
            took[r].append(timed(lambda: solve(r)))
    med = {r: float(np.median(v)) for r, v in took.items()}
    spmv_bytes = 2 * (nnz * (size + 4) + (rows + cols + 2) * 4) + 2 * (rows + cols) * size
    gs = lambda j: ((4 * j + 8) * rows + (4 * (j + 1) + 8) * cols) * size  # noqa: E731
    l = K + (NCV - K) // 2
    first = sum(spmv_bytes + gs(j) for j in range(NCV))
    again = sum(spmv_bytes + gs(j) for j in range(l, NCV)) + ((NCV + l) * rows + (NCV + l + 2) * cols) * size  # + the compression: m read, l written (+ v_m moved)
    print(f"   byte model of step j: the two SpMVs {spmv_bytes / 1e6:.1f} MB + Gram-Schmidt twice and the scaling on both sides {gs(0) / 1e6:.1f} MB (j = 0) .. "
          f"{gs(NCV - 1) / 1e6:.1f} MB (j = {NCV - 1})")
    step = med[0] / NCV
    print(f"   first cycle  ({NCV} steps, allocation, read-back and host SVD included): {med[0]:9.3f} ms = {1e3 * step:8.2f} us per step = {step / floor:5.2f} x the two "
          f"SpMVs ({1e3 * floor:.2f} us); the model's bytes at that time: {first / (med[0] * 1e-3) / 1e12:.2f} TB/s")
    extra = med[1] - med[0]
    step = extra / (NCV - l)
    print(f"   restart cycle (compression + steps {l} .. {NCV - 1}):                       {extra:9.3f} ms = {1e3 * step:8.2f} us per step = {step / floor:5.2f} x the two "
          f"SpMVs; the model's bytes at that time: {again / (extra * 1e-3) / 1e12:.2f} TB/s")
    print(f"   sigma_0 estimate after 0 / 1 restarts: {seen[0]:.6f} / {seen[1]:.6f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=sorted(DTYPES))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(DTYPES))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.n, args.reps, args.inner)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["f64", "f32"]):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(args.n), "--reps", str(args.reps), "--inner",
               str(args.inner)]
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
