#!/usr/bin/env python3
"""What the device sparse product costs on one MI355X: smm_hip_csr_multiply_create and smm_hip_csr_multiply_into_* for
    poisson2d    A A of the 1000 x 1000 5-point Laplacian, fp64 (13 entries per row of the product)
    stencil3d    A A of the 108^3 7-point convection-diffusion stencil, fp64 (25 entries per row)
    ata          At A of the banded generator's matrix (gen_banded_dev, 8 offsets per side, 200 000 rows, fp32), At from transpose()
    longrow      3 rows against 3000 rows of 40 entries: one row of the product with 120 000 entries, fp64 (the global-memory path)
After a warm-up, HIP events around 5 synchronised calls of each; reported: the median [min .. max] in ms, the scalar products (sum of
ub_i) and the entries of the product.
    python tools/spgemm_timing.py [--reps 5] [--only NAME] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"poisson2d": 240, "stencil3d": 240, "ata": 240, "longrow": 120}  # seconds per child
ORDER = ["poisson2d", "stencil3d", "ata", "longrow"]


def fmt(t):
    return f"{np.median(t):8.3f} [{t.min():7.3f} .. {t.max():7.3f}]"


def factors(kind):
    """(A, B, dtype, what has to stay alive)"""
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "longrow":
        dtype = np.float64
        rng = np.random.default_rng(47)
        a_start = np.array([0, 3000, 3000, 3005], dtype=np.int32)
        a_pos = np.concatenate([np.arange(3000), [4, 700, 701, 1999, 2999]]).astype(np.int32)
        b_start = (40 * np.arange(3001)).astype(np.int32)
        b_pos = np.arange(120000, dtype=np.int32)
        A = smm.CSRMatrix(3, 3000, a_start, a_pos, rng.uniform(-1, 1, len(a_pos)))
        B = smm.CSRMatrix(3000, 120000, b_start, b_pos, rng.uniform(-1, 1, len(b_pos)))
        return A, B, dtype, None
    if kind == "ata":
        dtype, td = np.float32, torch.float32
        rows, kk, seed, maxoff = 200_000, 8, 0x5EED, 1 << 12
        nnz = host.gen_banded_nnz(rows, kk, seed, maxoff)
    elif kind == "poisson2d":
        dtype, td = np.float64, torch.float64
        nx = 1000
        rows, nnz = nx * nx, host.gen_poisson2d_nnz(nx, nx)
    else:
        dtype, td = np.float64, torch.float64
        nx = 108
        rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    keep = (torch.empty(rows + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev))
    if kind == "ata":
        host.gen_banded_dev(rows, kk, seed, maxoff, *keep, dtype, stream)
    elif kind == "poisson2d":
        host.gen_poisson2d_dev(nx, nx, *keep, dtype, stream)
    else:
        host.gen_stencil3d_dev(nx, nx, nx, 6.0, -1.3, -0.7, *keep, dtype, stream)
    torch.cuda.synchronize()
    B = smm.CSRMatrix.from_device(rows, rows, *keep, dtype)
    A = B.transpose(stream) if kind == "ata" else B
    return A, B, dtype, keep


def timed(fn, reps):
    import torch

    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.array(out)


def child(kind, reps):
    import torch

    A, B, dtype, keep = factors(kind)
    stream = torch.cuda.current_stream().cuda_stream
    C = A.multiply(B, stream)  # warm-up: the code object, the allocator's blocks
    C.multiply_into(A, B, stream)
    made = []
    t_create = timed(lambda: made.append(A.multiply(B, stream)), reps)
    t_into = timed(lambda: C.multiply_into(A, B, stream), reps)
    a_start, a_pos = A.get_pattern()
    b_start, _ = B.get_pattern()
    products = int(np.diff(b_start.astype(np.int64))[a_pos].sum())
    s = np.dtype(dtype).itemsize
    moved = A.nnz * (s + 4) + products * (s + 4) + C.nnz * (s + 4)
    print(f"== {kind}: A {A.rows} x {A.cols} nnz {A.nnz}, B {B.rows} x {B.cols} nnz {B.nnz}, {np.dtype(dtype).name}; products {products}, nnz(C) {C.nnz}")
    print(f"   multiply_create {fmt(t_create)} ms")
    print(f"   multiply_into   {fmt(t_into)} ms = {moved / (1e-3 * np.median(t_into)) / 1e12:6.3f} TB/s over A once + products (s + 4) + nnz(C) (s + 4) = {moved / 1e6:.1f} MB")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ORDER):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps)]
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
