#!/usr/bin/env python3
"""What reverse Cuthill-McKee (smm_hip_csr_rcm) costs and what it buys an SpMV on one MI355X.  Two matrices, each in fp64 and fp32: the
7-point Laplacian of a 160^3 grid (4.1 M rows) and a mesh of dense 3 x 3 blocks (generators.block_expand on the 40^3 grid's pattern,
192 000 rows).  Each is taken in its natural numbering, shuffled by numpy.random.default_rng(7).permutation(rows) (A.permute), and the
shuffled matrix reordered by A.rcm() + A.permute().  Recorded: the wall time of rcm and of permute (both synchronise), the ordering's
components / levels / bandwidths, and per matrix -- natural under AUTO, shuffled under AUTO, reordered under AUTO and under PATTERN --
the kernel and bytes smm_hip_csr_kernel_desc names, ms per SpMV (the MEDIAN of --reps readings, each the mean of --inner launches between
two HIP events after 3 warm-up launches) and the TB/s the two give.
    python tools/rcm_timing.py [--reps 7] [--inner 10] [--out FILE]
The driver starts one child process per case under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("poisson3d_160_fp64", "grid", "float64"), ("poisson3d_160_fp32", "grid", "float32"), ("blocks3_40_fp64", "mesh", "float64"),
         ("blocks3_40_fp32", "mesh", "float32")]
LIMIT = 300  # seconds per child


def child(label, reps, inner):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import _lib
    from sparse_matrix_math_amd import generators as gen

    _, kind, dname = next(c for c in CASES if c[0] == label)
    dtype = np.dtype(dname)
    td = torch.float64 if dname == "float64" else torch.float32
    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "grid":
        csr = gen.poisson3d(160, dtype=dtype)
    else:
        s, p, _ = gen.poisson3d(40, dtype=dtype)
        csr = gen.block_expand(s, p, 3, seed=4, dtype=dtype, diag_dominant=True)
    rows = len(csr[0]) - 1
    natural = smm.CSRMatrix(rows, rows, *csr)
    shuffle = np.random.default_rng(7).permutation(rows).astype(np.int32)
    shuffled = natural.permute(shuffle)
    t0 = time.perf_counter()
    perm, info = shuffled.rcm()
    t_rcm = time.perf_counter() - t0
    t0 = time.perf_counter()
    ordered = shuffled.permute(perm)
    smm.synchronize()
    t_permute = time.perf_counter() - t0
    print(f"case {label}: rows {rows} nnz {natural.nnz}; natural bandwidth / offsets {natural.bandwidth()}, shuffled {shuffled.bandwidth()}, after RCM {ordered.bandwidth()}")
    print(f"  rcm {t_rcm * 1e3:9.2f} ms  permute {t_permute * 1e3:8.2f} ms  {info}")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    x = torch.rand(rows, generator=g, device=dev, dtype=torch.float64).to(td)
    y = torch.empty(rows, dtype=td, device=dev)

    def spmv_ms(A):
        for _ in range(3):
            A.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)
        readings = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                A.spmv_dev(smm.OP_ASSIGN, None, x, y, stream)
            e1.record()
            torch.cuda.synchronize()
            readings.append(e0.elapsed_time(e1) / inner)
        return float(np.median(readings)), min(readings), max(readings)

    for what, A, family in (("natural", natural, "AUTO"), ("shuffled", shuffled, "AUTO"), ("after RCM", ordered, "AUTO"), ("after RCM", ordered, "PATTERN")):
        try:
            A.set_kernel(smm.SPMV_PATTERN if family == "PATTERN" else smm.SPMV_AUTO)
        except _lib.SmmHipError as e:
            print(f"  spmv {what:9s} {family:7s} refused: {e}")
            continue
        name, nbytes = A.kernel_desc()
        med, lo_ms, hi_ms = spmv_ms(A)
        print(f"  spmv {what:9s} {family:7s} {name:26s} family {A.get_kernel()[0]} lanes {A.get_kernel()[1]} encoding {A.pattern_info()}  {med:8.4f} ms "
              f"(min {lo_ms:.4f} max {hi_ms:.4f}, median of {reps} x {inner})  bytes {nbytes}  {nbytes / med / 1e9:6.3f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.inner)
        return 0
    text = []
    for label, *_ in CASES:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", label, "--reps", str(args.reps), "--inner", str(args.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        text.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"case {label} ended with status {r.returncode}: stopping")
            return 1
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/rcm_timing.py --reps %d --inner %d   (one MI355X)\n" % (args.reps, args.inner))
            f.write("".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
