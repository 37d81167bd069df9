"""The STREAM family under SMM_HIP_STREAM_VARIANT, a once-per-process switch: tests/test_gpu_stream_edges.py starts this script as a fresh child
with the switch in its environment (one child at a time) and asserts on the one line `STREAM_VARIANT_WORKER {json}` it prints.

  variant 1  spmvTileKernel<T, 1, G>, which no other setting launches: cases edges, batch and seams at one lane per row, both dtypes,
             SMM_HIP_TILE_BATCH 4 .. 16; rMult / rMultAdd / rMultSub (and rMultSub in place) bit-identical to the oracle, tile_info() equal
             to the restated cut with tile_kernel == 1.
  variant 0  spmvStreamKernel<T, 2> and <T, 4> (pieces of a row inside one wave, met by shuffles), which no other setting launches: the
             same cases at 2 and 4 lanes; outputs within test_gpu_spmv.bound of the oracle, tile_kernel == 0, and -- given the TILE
             kernel's outputs for the same matrices in DEFAULTS.npz, keys "case/dtype/lanes/op" -- the rows of tiles that BOTH kernels
             stage bit-identical to them (both add the pieces of a row left to right).

usage: stream_variant_worker.py VARIANT [DEFAULTS.npz]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("edges", "batch", "seams-multiple", "seams-odd")
LANES = {0: (2, 4), 1: (1,)}


def main():
    variant = int(sys.argv[1])
    defaults = np.load(sys.argv[2]) if len(sys.argv) > 2 else None
    assert os.environ.get("SMM_HIP_STREAM_VARIANT") == str(variant)
    import stream_cases as sc
    from test_gpu_spmv import bound

    import sparse_matrix_math_amd as smm
    from oracle.oracle import Oracle

    smm.init(0)
    oracle = Oracle()
    os.environ["SMM_HIP_STREAM_NV"] = "1"
    failures, launched, checks, compared_rows = [], [], 0, 0
    for dtype in (np.float32, np.float64):
        dn = np.dtype(dtype).name
        for lanes in LANES[variant]:
            geometry = sc.expected_geometry(lanes, variant, 1, dtype)
            assert geometry[2] == variant
            for name in CASES:
                prob = sc.problem(name, dtype, geometry, lanes=lanes)
                refs = sc.references(oracle, prob)
                start = prob["csr"][0]
                tiles = sc.cut_rows(start, geometry[0], geometry[1])
                A = smm.CSRMatrix(prob["rows"], prob["cols"], *prob["csr"])
                A.set_kernel(sc.STREAM, lanes)
                for forced in (range(4, 17) if variant == 1 else (None,)):
                    tag = f"{name} {dn} lanes {lanes} batch {forced}"
                    if forced is not None:
                        os.environ["SMM_HIP_TILE_BATCH"] = str(forced)
                    outs = sc.run_ops(A, prob)
                    if A.get_kernel() != (sc.STREAM, lanes) or A.tile_info() != (len(tiles) - 1, *geometry):
                        failures.append(f"{tag}: kernel {A.get_kernel()}, tile_info {A.tile_info()}, restated {(len(tiles) - 1, *geometry)}")
                    failures += [f"{tag}: {m}" for m in sc.mismatches(outs, refs, prob, lanes, bound)]
                    checks += len(outs)
                    launched.append(["tile" if variant else "stream", dn, lanes, sc.tile_batch(start, lanes, forced) if variant else None])
                    if defaults is not None:
                        nnz = int(start[-1])
                        both = np.ones(prob["rows"], dtype=bool)
                        for kernel in (0, 1):
                            both &= sc.staged_rows(tiles, sc.classify(tiles, nnz, geometry[0] + 3, kernel), prob["rows"])
                        for op, out in outs.items():
                            want = defaults[f"{name}/{dn}/{lanes}/{op}"]
                            bad = np.flatnonzero(both & (out != want))
                            if bad.size:
                                failures.append(f"{tag}: {op}: {bad.size} staged rows differ from the TILE kernel's, the first is row {int(bad[0])}")
                            checks += 1
                        compared_rows += int(both.sum())
                os.environ.pop("SMM_HIP_TILE_BATCH", None)
    print("STREAM_VARIANT_WORKER " + json.dumps({"variant": variant, "checks": checks, "failures": failures[:40], "n_failures": len(failures),
                                                 "launched": launched, "compared_rows": compared_rows}), flush=True)


if __name__ == "__main__":
    main()
