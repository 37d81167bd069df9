#!/usr/bin/env python3
"""r09 lab: the PATTERN tile, slots and sweep kernels (R = 8 / 16 / 32 waves held open) on one device-generated banded matrix, the same
handle and the same x: launch time by device events (best of 5 x 20 launches) and the outputs compared bit for bit with the tile kernel's.
  python tools/lab/sweep_kernel_timing.py --rows 10000000 --max-offset 1048576 [--dtype f64] [--lanes 4] [--reps 1]
SMM_HIP_PATTERN_SWEEP_WGS=1..8 in the environment: workgroups of the sweep kernel per CU (default 3, or as many as fit)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import sparse_matrix_math_amd as smm
from sparse_matrix_math_amd import host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--max-offset", type=int, default=1 << 20)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="tile,slots,sweep8,sweep16,sweep32,auto")
    args = ap.parse_args()
    smm.init(0)
    dev = torch.device("cuda:0")
    npd = np.float32 if args.dtype == "f32" else np.float64
    td = torch.float32 if args.dtype == "f32" else torch.float64
    s0 = torch.cuda.current_stream().cuda_stream
    n = args.rows
    nnz = host.gen_banded_nnz(n, args.k, 0x5EED, args.max_offset)
    ds = torch.empty(n + 1, dtype=torch.int32, device=dev)
    dp = torch.empty(nnz, dtype=torch.int32, device=dev)
    dv = torch.empty(nnz, dtype=td, device=dev)
    host.gen_banded_dev(n, args.k, 0x5EED, args.max_offset, ds, dp, dv, npd, s0)
    torch.cuda.synchronize()
    x = torch.rand(n, dtype=td, device=dev, generator=torch.Generator(device=dev).manual_seed(11)) - 0.5
    A = smm.CSRMatrix.from_device(n, n, ds, dp, dv, npd)
    A.set_kernel(3, args.lanes)
    print(f"rows {n} offsets per side {args.k} below {args.max_offset} {args.dtype} lanes {args.lanes}: {nnz} entries; "
          f"SMM_HIP_PATTERN_SWEEP_WGS={os.environ.get('SMM_HIP_PATTERN_SWEEP_WGS', 'unset (3)')}", flush=True)
    want = None
    for cfg in args.configs.split(","):
        host.set_pattern_sweep_rows(int(cfg[5:]) if cfg.startswith("sweep") else 0)
        A.pattern_slots({"tile": 0, "slots": 1, "auto": 2}.get(cfg, 3))
        y = torch.zeros(n, dtype=td, device=dev)
        for _ in range(5):
            A.spmv_dev(0, None, x, y, s0)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                A.spmv_dev(0, None, x, y, s0)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 50.0)
        if want is None:
            want = y.clone()
        name, nbytes = A.kernel_desc()
        same = "same bits as the first" if torch.equal(y, want) else "BITS DIFFER"
        print(f"  {cfg:8s} {name:24s} {best:8.1f} us per launch, {nbytes / best / 1e6:5.2f} TB/s on its own {nbytes / 1e9:.3f} GB; {same}", flush=True)


if __name__ == "__main__":
    main()
