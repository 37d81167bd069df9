#!/usr/bin/env python3
"""The PATTERN sweep kernel against the tile kernel on device-generated banded matrices, in a process of its own, so that the variables
read once per process can be set by the caller (tests/test_gpu_pattern_sweep.py):

  SMM_HIP_PATTERN_SWEEP_WGS=1 python tools/lab/sweep_blocks_check.py --dtype f32 --rows-open 8,16,32 --rows 2097152,2300017
      one workgroup per CU: an XCD group's super-block is 32 x 4 x R waves whatever the registers of the variant
  SMM_HIP_PATTERN_SLOTS=3 python tools/lab/sweep_blocks_check.py --env-mode --rows 16001
      the handle's mode is left at -1: the variable alone must select the sweep kernel

Prints one "ok" line per case with the super-block geometry an XCD group of a 256-CU grid gets; exits non-zero on any difference."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import sparse_matrix_math_amd as smm
from sparse_matrix_math_amd import host

SWEEP, TILE = "spmvPatternSweepKernel", "spmvPatternTileKernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--rows-open", default="16")
    ap.add_argument("--rows", default="2097152,2300017")
    ap.add_argument("--max-offset", type=int, default=1 << 18)
    ap.add_argument("--env-mode", action="store_true", help="never call pattern_slots for the sweep handle: SMM_HIP_PATTERN_SLOTS decides")
    args = ap.parse_args()
    smm.init(0)
    dev = torch.device("cuda:0")
    npd = np.float32 if args.dtype == "f32" else np.float64
    td = torch.float32 if args.dtype == "f32" else torch.float64
    s0 = torch.cuda.current_stream().cuda_stream
    for n in (int(v) for v in args.rows.split(",")):
        maxoff = min(args.max_offset, n // 4)
        nnz = host.gen_banded_nnz(n, 25, 0x5EED, maxoff)
        ds = torch.empty(n + 1, dtype=torch.int32, device=dev)
        dp = torch.empty(nnz, dtype=torch.int32, device=dev)
        dv = torch.empty(nnz, dtype=td, device=dev)
        host.gen_banded_dev(n, 25, 0x5EED, maxoff, ds, dp, dv, npd, s0)
        torch.cuda.synchronize()
        x = torch.rand(n, dtype=td, device=dev, generator=torch.Generator(device=dev).manual_seed(11)) - 0.5
        lhs = torch.rand(n, dtype=td, device=dev, generator=torch.Generator(device=dev).manual_seed(12))
        T = smm.CSRMatrix.from_device(n, n, ds, dp, dv, npd)
        T.set_kernel(3, 2)
        T.pattern_slots(0)
        want = {}
        for op in (0, 1):
            want[op] = torch.zeros(n, dtype=td, device=dev)
            T.spmv_dev(op, lhs if op else None, x, want[op], s0)
        torch.cuda.synchronize()
        assert T.kernel_desc()[0] == TILE, T.kernel_desc()
        assert float(want[0].abs().max()) > 0
        for r in (int(v) for v in args.rows_open.split(",")):
            host.set_pattern_sweep_rows(r)
            S = smm.CSRMatrix.from_device(n, n, ds, dp, dv, npd)
            S.set_kernel(3, 2)
            if not args.env_mode:
                S.pattern_slots(3)
            for op in (0, 1):
                y = torch.zeros(n, dtype=td, device=dev)
                S.spmv_dev(op, lhs if op else None, x, y, s0)
                torch.cuda.synchronize()
                if not torch.equal(y, want[op]):
                    print(f"BITS DIFFER rows {n} R {r} op {op}")
                    return 1
            name = S.kernel_desc()[0]
            if name != SWEEP:
                print(f"rows {n} R {r}: {name} ran, not {SWEEP}")
                return 1
            print(f"ok rows {n} {args.dtype} R {r} {name} SMM_HIP_PATTERN_SLOTS={os.environ.get('SMM_HIP_PATTERN_SLOTS', 'unset')} "
                  f"SMM_HIP_PATTERN_SWEEP_WGS={os.environ.get('SMM_HIP_PATTERN_SWEEP_WGS', 'unset')}", flush=True)
            del S
        del T, ds, dp, dv
    print("sweep blocks check: ALL OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
