#!/usr/bin/env python3
"""What a step of LSQR costs on one MI355X, next to one SpMV on `a` plus one on `at` from the same handles -- the floor a step cannot
beat -- and the step's byte model at the measured rate.
Workload, fp64 and fp32, b seeded uniform, x0 = 0: the tall matrix [I; Dx; Dy; Dz] of an n^3 grid (the identity over the forward
differences along the three axes), built on the device with torch: n^3 columns, n^3 + 3 n^2 (n - 1) rows, one or two entries per row; its
transpose is kept (CSRMatrix.transpose), so the solve builds none.  n = 160: 16.3 M rows, 4.1 M columns, 28.5 M entries -- the matrix
(342 MB of values and positions in fp64) and the five work vectors leave the 256 MB Infinity Cache.
A step is timed as the difference of two fixed-step solves (eps = 0) of c + 1 and c steps (medians of --reps interleaved rounds, each
solve between two HIP events): the set-up and the read-back cancel.  The byte model of a step: the two SpMVs
(values, positions and start once each, the input vector once, the output once) plus 3 m + 9 n vector elements of the three update kernels.
    python tools/lsqr_timing.py [--n 160] [--reps 7] [--inner 20] [--damp 0] [--only f64|f32] [--out FILE]
The driver starts one child process per dtype under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 300  # seconds per child
DTYPES = {"f64": np.float64, "f32": np.float32}


def tall_on_device(n, td, dev):
    """(rows, cols, start, positions, values) of [I; Dx; Dy; Dz] in device memory"""
    import torch

    cols = n**3
    idx = torch.arange(cols, dtype=torch.int64, device=dev)
    pos = [idx]
    val = [torch.ones(cols, dtype=td, device=dev)]
    pairs = 0
    for stride in (1, n, n * n):
        sel = idx[(idx // stride) % n < n - 1]
        pos.append(torch.stack([sel, sel + stride], dim=1).reshape(-1))
        val.append(torch.tensor([-1.0, 1.0], dtype=td, device=dev).repeat(len(sel)))
        pairs += len(sel)
    rows = cols + pairs
    start = torch.cat([torch.arange(cols + 1, dtype=torch.int64, device=dev), cols + 2 * torch.arange(1, pairs + 1, dtype=torch.int64, device=dev)])
    return rows, cols, start.to(torch.int32), torch.cat(pos).to(torch.int32), torch.cat(val)


def child(kind, n, reps, inner, damp):
    import torch

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
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    b = torch.rand(rows, dtype=td, device=dev, generator=gen) * 2 - 1
    x = torch.zeros(cols, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    def fixed(steps):
        x.zero_()
        done = host.lsqr_dev(A, b, x, steps, 0.0, damp, At, stream)[1]
        assert done == steps, (done, steps)

    fixed(20)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
    q = torch.empty(rows, dtype=td, device=dev)
    t = torch.empty(cols, dtype=td, device=dev)
    spmv_a = float(np.median([timed(lambda: [A.spmv_dev(smm.OP_ASSIGN, None, x, q, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    spmv_at = float(np.median([timed(lambda: [At.spmv_dev(smm.OP_ASSIGN, None, b, t, stream) for _ in range(inner)]) for _ in range(reps)])) / inner
    print(f"== {kind}: [I; Dx; Dy; Dz] of a {n}^3 grid: {rows} x {cols}, nnz {nnz}, {np.dtype(dtype).name}, damp {damp:g}; {reps} rounds")
    print(f"   SpMV on a : {A.kernel_desc()[0]} {A.get_kernel()}: {1e3 * spmv_a:8.2f} us per launch")
    print(f"   SpMV on at: {At.kernel_desc()[0]} {At.get_kernel()}: {1e3 * spmv_at:8.2f} us per launch")
    floor = spmv_a + spmv_at
    counts = (20, 21, 40, 41)
    took = {c: [] for c in counts}
    for _ in range(reps):
        for c in counts:
            took[c].append(timed(lambda: fixed(c)))
    med = {c: float(np.median(v)) for c, v in took.items()}
    spmv_bytes = 2 * (nnz * (size + 4) + (rows + cols + 2) * 4) + 2 * (rows + cols) * size
    update_bytes = (3 * rows + 9 * cols) * size
    print(f"   byte model of a step: the two SpMVs {spmv_bytes / 1e6:.1f} MB + the three update kernels (3 m + 9 n elements) {update_bytes / 1e6:.1f} MB")
    for c in (20, 40):
        step = med[c + 1] - med[c]
        print(f"   LSQR step {c:3d}: {1e3 * step:8.2f} us  = {step / floor:5.2f} x the two SpMVs ({1e3 * floor:.2f} us); the model's bytes at that time: "
              f"{(spmv_bytes + update_bytes) / (step * 1e-3) / 1e12:.2f} TB/s  (solves of {c + 1} and {c} steps: {med[c + 1]:.3f} and {med[c]:.3f} ms)")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--damp", type=float, default=0.0)
    ap.add_argument("--only", choices=sorted(DTYPES))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(DTYPES))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.n, args.reps, args.inner, args.damp)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["f64", "f32"]):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", kind, "--n", str(args.n), "--reps", str(args.reps), "--inner",
               str(args.inner), "--damp", repr(args.damp)]
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
