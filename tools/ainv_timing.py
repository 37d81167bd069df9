#!/usr/bin/env python3
"""What the approximate-inverse preconditioners (SMM_PRECOND_FSAI / SMM_PRECOND_SPAI) buy -- or cost -- on one MI355X, against the
unpreconditioned loops and the other kinds, every leg in one run.  Workloads, fp64, b = A 1, x0 = 0, eps 1e-8:
  * cg        the 256^3 7-point Laplacian: ConjugateGradient with none, IC0, MULTICOLOR_IC0, AMG and FSAI at power 1, 2, 3;
  * bicgstab  the 108^3 7-point convection-diffusion stencil (diag 6, lower -1.3, upper -0.7): BiCGStab with none, BLOCK_ILU0,
              MULTICOLOR_ILU0, SPAI at power 1, 2 and FSAI at power 1 (the matrix is not symmetric: FSAI reads its lower triangle).
Per leg: set-up ms (wall clock around the create, the device drained before and after), us per apply (--inner applies between two HIP
events), iterations and ms per solve (median of --reps solves after one warm-up solve), and create + solve.  For FSAI / SPAI also the
refresh, the entries of G / M and THE SET-UP KERNEL ALONE: the library's set-up trace (SMM_HIP_TRACE_SETUP=1) times the one launch that
gathers and solves all row systems, from the drained stream to its 4-byte read-back, in the create and again in the refresh (the
smaller of the two is reported); rows per second and bytes gathered per second follow from it.  Bytes gathered are COUNTED from the
patterns, not estimated: for every entry (i, r) of G / M the stored entries of row r of the source (a, or a a^T) with a column <= r,
sizeof(T) + 4 bytes each, plus 4 bytes per entry of the pattern; counted on the host, so only for patterns of at most 2^27 entries.
    python tools/ainv_timing.py [--reps 5] [--inner 20] [--only bicgstab|cg] [--out FILE]
The driver starts one child process per workload under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bicgstab": 300, "cg": 540}  # seconds per child
EPS = 1e-8
LEGS = {"cg": [("none", None), ("IC0", None), ("MULTICOLOR_IC0", None), ("AMG", None), ("FSAI", 1), ("FSAI", 2), ("FSAI", 3)],
        "bicgstab": [("none", None), ("BLOCK_ILU0", None), ("MULTICOLOR_ILU0", None), ("SPAI", 1), ("SPAI", 2), ("FSAI", 1)]}


def child(kind, reps, inner):
    import tempfile

    trace = tempfile.TemporaryFile(mode="w+")
    os.dup2(trace.fileno(), 2)  # the library's set-up trace goes to stderr: keep it in a file this process reads back
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype, td = np.float64, torch.float64
    nx = 108 if kind == "bicgstab" else 256
    lo, hi = (-1.3, -0.7) if kind == "bicgstab" else (-1.0, -1.0)
    rows, nnz = nx**3, host.gen_stencil3d_nnz(nx, nx, nx)
    d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=td, device=dev)
    host.gen_stencil3d_dev(nx, nx, nx, 6.0, lo, hi, d_start, d_pos, d_val, dtype, stream)
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(rows, rows, d_start, d_pos, d_val, dtype)
    ones = torch.ones(rows, dtype=td, device=dev)
    b = torch.empty(rows, dtype=td, device=dev)
    A.spmv_dev(smm.OP_ASSIGN, None, ones, b, stream)
    x = torch.zeros(rows, dtype=td, device=dev)
    zero = torch.zeros(rows, dtype=td, device=dev)
    y = torch.empty(rows, dtype=td, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def solve(M):
        x.zero_()
        if kind == "bicgstab":
            return host.bicgstab_dev(A, b, x, -1, EPS, M, stream)
        return host.cg_dev(A, b, zero, x, -1, EPS, M, stream)

    def kernel_ms():
        """the 'ainv: solve kernel' lines the trace has written since the last call"""
        trace.seek(kernel_ms.read_to)  # (the descriptor is shared with stderr: reading to the end leaves it where the library appends)
        text = trace.read()
        kernel_ms.read_to = trace.tell()
        return [float(ln.split()[-2]) for ln in text.splitlines() if "ainv: solve kernel" in ln]

    kernel_ms.read_to = 0

    lower = {}  # per source: the stored entries of every row with a column <= the row

    def lower_lengths(which):
        if which not in lower:
            src, keep = A, None
            if which == "SPAI":
                keep = A.transpose()
                src = A.multiply(keep)
            st, ps = src.get_pattern()
            row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(st))
            lower[which] = np.bincount(row_of[ps <= row_of], minlength=rows)
            if keep is not None:
                src.close()
                keep.close()
        return lower[which]

    print(f"== {kind}: {nx}^3 = {rows} rows, nnz {nnz}, float64, eps {EPS}")
    kernel_ms()
    for name, power in LEGS[kind]:
        M, create_ms, extra = None, 0.0, ""
        if name != "none":
            try:
                create_ms, M = wall(lambda: A.getPreconditioner(name, power=power) if power else A.getPreconditioner(name))
            except smm.SmmHipError as e:  # a refused create is a result too (FSAI on a matrix whose lower triangle is not positive definite)
                print(f"   {name + (f' p={power}' if power else ''):<18s} create refused: {e}", flush=True)
                continue
        if power:
            info = M.ainv_info()
            refresh_ms, _ = wall(M.ainv_refresh)
            k_ms = min(kernel_ms())
            per_row = info["nnz"] / rows
            extra = (f"\n      entries {info['nnz']} ({per_row:.1f} per row, longest {info['max_row']})  refresh {refresh_ms:8.1f} ms"
                     f"  set-up kernel alone {k_ms:8.3f} ms = {rows / k_ms / 1e3:7.2f} M rows/s")
            if info["nnz"] <= 1 << 27:
                gp = M.ainv_matrix()[0].get_pattern()[1]
                gathered = int(lower_lengths(name)[gp].sum()) * (np.dtype(dtype).itemsize + 4) + 4 * info["nnz"]
                extra += f", {gathered / 1e6:9.1f} MB gathered = {gathered / k_ms / 1e6:7.1f} GB/s"
            else:
                extra += ", bytes not counted (pattern above 2^27 entries)"
        solve(M)  # the warm-up: the PATTERN analysis, the tile tables, the code objects
        runs = [timed(lambda: solve(M)) for _ in range(reps)]
        ms = float(np.median([r[0] for r in runs]))
        st, it = int(runs[-1][1][0]), int(runs[-1][1][1])
        err = float((x - 1).abs().max())
        ap = 0.0
        if M is not None:
            M.apply_dev(b, y, stream)
            ap = float(np.median([timed(lambda: [M.apply_dev(b, y, stream) for _ in range(inner)])[0] for _ in range(reps)])) / inner
        label = name + (f" p={power}" if power else "")
        print(f"   {label:<18s} status {st} set-up {create_ms:9.1f} ms  apply {1e3 * ap:9.1f} us  iterations {it:5d}  solve {ms:9.3f} ms  create + solve {create_ms + ms:9.1f} ms"
              f"  max|x - 1| {err:.2e}{extra}", flush=True)
        if M is not None:
            M.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        try:
            return child(args.child, args.reps, args.inner)
        except Exception:  # (stderr is the trace file by now)
            import traceback

            print(traceback.format_exc(), flush=True)
            return 1
    report = []
    status = 0
    for kind in [args.only] if args.only else ["bicgstab", "cg"]:
        cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps), "--inner", str(args.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SMM_HIP_TRACE_SETUP="1"))
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
