#!/usr/bin/env python3
"""What editing a matrix's values costs on the device (smm_hip_csr_scale / axpy / zero / update_entries / set_values / values_changed),
against destroying and re-creating the handle.  Two matrices, both generated on the device:
  * the benchmark matrix (bench.py defaults: 10 M rows, 25 offsets per side, fp32; STREAM, no PATTERN analysis);
  * the 512^3 fp64 Laplacian (PATTERN, constant diagonals): also the CONST re-verification (values_changed).
Every figure: HIP events around the synchronised call, after a warm-up, median of --reps.  Bytes are the bytes the edit itself has to
move (values read + written, the batch, the masks the re-verification reads); GB/s = bytes / time.
    python tools/csr_update_timing.py [--reps 5] [--only bench|lap] [--trace]
--trace: one short sequence on the benchmark matrix for `rocprofv3 --kernel-trace --stats` (first SpMV, edits, the SpMV after each):
the trace shows which kernels each step launches."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparse_matrix_math_amd as smm  # noqa: E402
from sparse_matrix_math_amd import _lib, host  # noqa: E402
from sparse_matrix_math_amd._lib import check  # noqa: E402


def timed(fn, stream, reps):
    fn()  # warm-up (events on the current stream, which the calls use)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def wall(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def make(kind, dtype, dev, stream):
    td = torch.float32 if dtype == np.float32 else torch.float64
    if kind == "bench":
        n, k, seed, maxoff = 10_000_000, 25, 0x5EED, 1 << 20
        nnz = host.gen_banded_nnz(n, k, seed, maxoff)
        arrs = (torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev))
        host.gen_banded_dev(n, k, seed, maxoff, *arrs, dtype, stream, diag_shift=1.0)
    else:
        N = 512
        n = N ** 3
        nnz = host.gen_stencil3d_nnz(N, N, N)
        arrs = (torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev))
        host.gen_stencil3d_dev(N, N, N, 6.0, -1.0, -1.0, *arrs, dtype, stream)
    torch.cuda.synchronize()
    return n, nnz, arrs


def run(kind, reps, out):
    dtype = np.float32 if kind == "bench" else np.float64
    s = np.dtype(dtype).itemsize
    suf = "f32" if dtype == np.float32 else "f64"
    fn = lambda base: getattr(_lib.load(), f"{base}_{suf}")  # noqa: E731
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st = ctypes.c_void_p(stream)
    n, nnz, (ds, dp, dv) = make(kind, dtype, dev, stream)
    # A: a handle over its own copy of the values (the edits below change it); B: the generator's arrays (same pattern: the axpy partner)
    av = dv.clone()
    A = smm.CSRMatrix.from_device(n, n, ds, dp, av, dtype)
    B = smm.CSRMatrix.from_device(n, n, ds, dp, dv, dtype)
    x = torch.ones(n, dtype=av.dtype, device=dev)
    y = torch.empty_like(x)
    spmv = lambda M: M.spmv_dev(0, None, x, y, stream)  # noqa: E731
    t0 = time.perf_counter()
    spmv(A)  # first SpMV: analysis / tile table
    torch.cuda.synchronize()
    first_ms = 1e3 * (time.perf_counter() - t0)
    spmv_ms = timed(lambda: spmv(A), stream, reps)
    rows = []

    def row(name, ms, nbytes, note=""):
        gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 and nbytes else 0.0
        rows.append({"matrix": kind, "edit": name, "ms": round(ms, 4), "bytes": int(nbytes), "GB/s": round(gbs, 1), "note": note})
        print(f"{kind:5s} {name:34s} {ms:10.3f} ms {nbytes / 1e9:8.3f} GB {gbs:8.1f} GB/s  {note}", flush=True)

    row("SpMV (steady state)", spmv_ms, 0, f"first SpMV {first_ms:.2f} ms wall; encoding {A.pattern_info()}, kernel {A.kernel_desc()[0]}")
    alpha = 1.0000001
    row("scale", timed(lambda: check(fn("smm_hip_csr_scale")(A._h, alpha, st)), stream, reps), 2 * nnz * s)
    row("axpy (second handle)", timed(lambda: check(fn("smm_hip_csr_axpy")(A._h, 1e-7, B._h, st)), stream, reps), 3 * nnz * s)
    row("zero", timed(lambda: check(fn("smm_hip_csr_zero")(A._h, st)), stream, reps), nnz * s)
    row("set values (device)", timed(lambda: check(fn("smm_hip_csr_set_values_dev")(A._h, ctypes.c_void_p(dv.data_ptr()), st)), stream, reps), 2 * nnz * s)
    if kind == "bench":
        hv = dv.cpu().numpy()
        row("set values (host, pageable)", wall(lambda: A.set_values(hv), reps), nnz * s, "bound by the host link")
    m = 1_000_000
    g = np.random.default_rng(1)
    r = torch.from_numpy(g.integers(0, n, m).astype(np.int32)).to(dev)
    sh = ds.cpu().numpy() if kind == "bench" else None
    if kind == "bench":
        rh = r.cpu().numpy()
        k = sh[rh] + (g.integers(0, 1 << 30, m) % np.maximum(1, sh[rh + 1] - sh[rh]))
        c = dp[torch.from_numpy(k.astype(np.int64)).to(dev)]
    else:
        c = r.clone()  # the diagonal
    vals = torch.rand(m, dtype=av.dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    upd = lambda: check(fn("smm_hip_csr_update_entries_dev")(A._h, m, ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(c.data_ptr()),  # noqa: E731
                                                             ctypes.c_void_p(vals.data_ptr()), 1, None, st))
    if kind == "lap":
        # every entry edit of a CONST handle re-verifies; time the edit on a handle that stays MASKS afterwards, and the re-verification alone below
        check(fn("smm_hip_csr_set_values_dev")(A._h, ctypes.c_void_p(dv.data_ptr()), st))
    row("update entries (1 M, ADD)", timed(upd, stream, reps), m * (8 + s), f"encoding after: {A.pattern_info()}")
    if kind == "lap":
        C = smm.CSRMatrix.from_device(n, n, ds, dp, dv, dtype)
        C.set_kernel(3, 1)
        assert C.pattern_info()[0] == 3
        row("CONST re-verification (values_changed)", timed(lambda: check(fn("smm_hip_csr_values_changed")(C._h, st)), stream, reps), n * 12 + nnz * s,
            f"encoding after: {C.pattern_info()}")
        row("  scale of the CONST handle (k diagonals)", timed(lambda: check(fn("smm_hip_csr_scale")(C._h, 1.0, st)), stream, reps), 2 * nnz * s)
    # an edit + the next SpMV against destroy + create + first SpMV
    edit_spmv = timed(lambda: (check(fn("smm_hip_csr_scale")(A._h, alpha, st)), spmv(A)), stream, reps)
    row("scale + next SpMV", edit_spmv, 0)
    if kind == "bench":
        hs, hp = ds.cpu().numpy(), dp.cpu().numpy()

        def recreate():
            M = smm.CSRMatrix(n, n, hs, hp, hv)
            spmv(M)
            torch.cuda.synchronize()
            M.close()
        rc = wall(recreate, max(2, reps // 2))
        row("destroy + create (host arrays) + first SpMV", rc, (n + 1) * 4 + nnz * (4 + s), f"{rc / edit_spmv:.1f} x scale + SpMV")
    else:
        def recreate_dev():
            M = smm.CSRMatrix.from_device(n, n, ds, dp, av, dtype)
            M.set_kernel(3, 1)
            spmv(M)
            torch.cuda.synchronize()
            del M
        rc = wall(recreate_dev, max(2, reps // 2))
        row("destroy + create (device arrays) + PATTERN analysis + first SpMV", rc, 0, f"{rc / edit_spmv:.1f} x scale + SpMV")
    out.extend(rows)


def trace():
    """one pass for the profiler: first SpMV, then every edit followed by an SpMV (markers on stdout)"""
    dtype = np.float32
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, nnz, (ds, dp, dv) = make("bench", dtype, dev, stream)
    av = dv.clone()
    A = smm.CSRMatrix.from_device(n, n, ds, dp, av, dtype)
    B = smm.CSRMatrix.from_device(n, n, ds, dp, dv, dtype)
    x = torch.ones(n, dtype=av.dtype, device=dev)
    y = torch.empty_like(x)
    A.spmv_dev(0, None, x, y, stream)
    A.scale(0.5, stream)
    A.spmv_dev(0, None, x, y, stream)
    A.axpy(1.0, B, stream)
    A.spmv_dev(0, None, x, y, stream)
    r = torch.arange(0, n, 10, dtype=torch.int32, device=dev)
    A.update_entries_dev(r.numel(), r, r, torch.ones(r.numel(), dtype=av.dtype, device=dev), True, None, stream)
    A.spmv_dev(0, None, x, y, stream)
    A.zero(stream)
    A.spmv_dev(0, None, x, y, stream)
    torch.cuda.synchronize()
    print("trace sequence: spmv, scale, spmv, axpy, spmv, update_entries, spmv, zero, spmv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["bench", "lap"])
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    smm.init(0)
    if args.trace:
        trace()
        return
    out = []
    for kind in ("bench", "lap"):
        if args.only in (None, kind):
            run(kind, args.reps, out)
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
