#!/usr/bin/env python3
"""What several right-hand sides at once buy: smm_hip_spmm_dev for k = 2, 4, 8 against k consecutive smm_hip_spmv_dev launches of the
family AUTO picks and of STREAM, and one BiCGStabBatch iteration (k = 4, 20 fixed iterations) against 4 x the single loop.  Workloads:
  * bench    the benchmark matrix (gen_banded_dev, 10 M rows, 25 offsets per side, fp32);
  * stencil  the 512^3 7-point stencil in fp64.
One process per workload; per k a warm-up, then --reps (>= 20) rounds with the legs interleaved A / B / C / A / B / C so that a clock
change hits all of them; every leg of a round sits between two HIP events on one stream.  Reported: median [min .. max] in ms, the ratio
to k x AUTO, and the SpMM's fraction of the 8 TB/s peak on its own bytes nnz (4 + s) + rows (4 + 2 k s).
    python tools/spmm_timing.py [--reps 20] [--only bench|stencil] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails; the report goes to stdout
and to --out."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bench": 420, "stencil": 540}  # seconds per child
PEAK = 8.0e12


def fmt(t):
    return f"{np.median(t):8.3f} [{t.min():7.3f} .. {t.max():7.3f}]"


def interleaved(legs, reps, warmup=3):
    """legs: name -> callable that enqueues the leg on the current stream; returns name -> ms per round"""
    import torch

    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(reps):
        marks = []
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in marks:
            times[name].append(e0.elapsed_time(e1))
    return {name: np.array(t) for name, t in times.items()}


def child(kind, reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "bench":
        dtype, td = np.float32, torch.float32
        rows, kk, seed, maxoff = 10_000_000, 25, 0x5EED, 1 << 20
        nnz = host.gen_banded_nnz(rows, kk, seed, maxoff)
    else:
        dtype, td = np.float64, torch.float64
        nx = 512
        rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    if kind == "bench":
        host.gen_banded_dev(rows, kk, seed, maxoff, d_start, d_pos, d_val, dtype, stream)
    else:
        host.gen_stencil3d_dev(nx, nx, nx, 6.0, -1.3, -0.7, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    s = np.dtype(dtype).itemsize
    # three handles on the same arrays: AUTO's choice, STREAM, and an untouched one for the SpMM (it reads the CSR arrays only)
    A_auto = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    A_stream = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    A_stream.set_kernel(smm.SPMV_STREAM, 0)
    A_mm = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    g = torch.Generator(device=dev).manual_seed(7)
    print(f"== {kind}: rows {rows}, nnz {nnz}, {np.dtype(dtype).name}, {reps} interleaved rounds per k; ms as median [min .. max]")
    first = True
    for k in (2, 4, 8):
        X = torch.rand((rows, k), dtype=td, device=dev, generator=g) - 0.5
        Out = torch.empty((rows, k), dtype=td, device=dev)
        xs = [X[:, j].contiguous() for j in range(k)]
        ys = [torch.empty(rows, dtype=td, device=dev) for _ in range(k)]

        def spmm():
            A_mm.spmm_dev(smm.OP_ASSIGN, k, None, X, Out, stream)

        def spmv_auto():
            for x, y in zip(xs, ys):
                A_auto.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)

        def spmv_stream():
            for x, y in zip(xs, ys):
                A_stream.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)

        t = interleaved({"spmm": spmm, "auto": spmv_auto, "stream": spmv_stream}, reps)
        if first:
            print(f"   AUTO runs {A_auto.kernel_desc()[0]} {A_auto.get_kernel()}, STREAM runs {A_stream.kernel_desc()[0]} {A_stream.get_kernel()}, "
                  f"SpMM tile table {A_mm.tile_info()[:3]}")
            first = False
        # the same numbers from both routes (the SpMM keeps one lane per row; the SpMV legs may split rows)
        worst = max(float((Out[:, j] - ys[j]).abs().max()) for j in range(k))
        own = nnz * (4 + s) + rows * (4 + 2 * k * s)
        ms = float(np.median(t["spmm"]))
        print(f"   k = {k}: spmm      {fmt(t['spmm'])}   = {ms / np.median(t['auto']):.3f} x (k AUTO launches), {ms / np.median(t['stream']):.3f} x (k STREAM launches); "
              f"{own / 1e9:.2f} GB -> {own / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * own / (ms * 1e-3) / PEAK:.0f} % of peak")
        print(f"          k x AUTO   {fmt(t['auto'])}   ({np.median(t['auto']) / k:.3f} per launch)")
        print(f"          k x STREAM {fmt(t['stream'])}   ({np.median(t['stream']) / k:.3f} per launch)    max |spmm - spmv| = {worst:.2e}")
        del X, Out, xs, ys
    # one BiCGStab iteration: the batch of 4 against 4 single solves, 20 fixed iterations (eps = 0)
    k, its = 4, 20
    B = torch.rand((rows, k), dtype=td, device=dev, generator=g) + 0.5
    bs = [B[:, j].contiguous() for j in range(k)]
    Xb = torch.zeros((rows, k), dtype=td, device=dev)
    x1 = torch.zeros(rows, dtype=td, device=dev)
    counts = {}

    def batch():
        Xb.zero_()
        counts["batch"] = host.bicgstab_batch_dev(A_mm, k, B, Xb, its, 0.0, None, stream)[1]

    def singles():
        for b in bs:
            x1.zero_()
            counts["single"] = host.bicgstab_dev(A_auto, b, x1, its, 0.0, None, stream)[1]

    t = interleaved({"batch": batch, "single": singles}, max(5, reps // 4), warmup=1)
    assert list(counts["batch"]) == [its] * k and counts["single"] == its, counts
    print(f"   BiCGStab, {its} iterations: batch of {k} {fmt(t['batch'])} = {np.median(t['batch']) / its:.3f} per iteration; "
          f"{k} single solves {fmt(t['single'])} = {np.median(t['single']) / its:.3f} per iteration of all {k}; ratio {np.median(t['batch']) / np.median(t['single']):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        child(args.child, max(20, args.reps))
        return 0
    report = []
    for kind in ([args.only] if args.only else ["bench", "stencil"]):
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"{kind}: exit status {r.returncode}; stopping here")
            if args.out:
                open(args.out, "w").write("".join(report))
            return r.returncode
    if args.out:
        open(args.out, "w").write("".join(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
