#!/usr/bin/env python3
"""What assembling a matrix from triplets costs on the device (smm_hip_assembly_*), against the route a time loop had before it:
smm_hip_csr_zero + smm_hip_csr_update_entries_dev(ADD) of the same batch, which sorts and searches on every call.  Two lists:
  * bench     the benchmark matrix (10 M rows, 25 offsets per side, fp32): one contribution per entry, 485 M triplets;
  * convdiff  the 108^3 convection-diffusion stencil (fp64) with 4 contributions per entry, 35 M triplets.
Per list: (a) plan creation, (b) assemble_dev, (c) refill_dev SET with the list in sorted (CSR) order and in shuffled order -- a plan
each --, (d) zero + update_entries_dev(ADD) of the same two lists.  HIP events around the call, after a warm-up; --reps repetitions (5),
reported as median [min .. max].  GB/s of (b) / (c) = the bytes of the numeric pass, n (s + 4) + (nnz + 1) 4 + nnz s (without repeated
pairs n (s + 4) + n s), over the median time.
    python tools/assembly_timing.py [--reps 5] [--only bench|convdiff] [--out FILE]
The driver starts one child process per list under its own `timeout` and stops at the first that fails; the report goes to stdout and
to --out."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"bench": 420, "convdiff": 240}  # seconds per child


def measure(fn, reps, wall=False):
    import torch

    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0) if wall else e0.elapsed_time(e1))
    return np.array(times)


def child(kind, reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import generators as gen
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "bench":
        dtype, td, contributions = np.float32, torch.float32, 1
        rows, k, seed, maxoff = 10_000_000, 25, 0x5EED, 1 << 20
        nnz = host.gen_banded_nnz(rows, k, seed, maxoff)
        d_start = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
        d_val = torch.empty(nnz, dtype=td, device=dev)
        host.gen_banded_dev(rows, k, seed, maxoff, d_start, d_pos, d_val, dtype, stream)
    else:
        dtype, td, contributions = np.float64, torch.float64, 4
        start, pos, val = gen.convdiff3d(108, dtype=dtype)
        rows, nnz = len(start) - 1, len(pos)
        d_start, d_pos, d_val = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (start, pos, val))
    s = np.dtype(dtype).itemsize
    counts = (d_start[1:] - d_start[:-1]).long()
    r = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), counts, output_size=nnz)
    g = torch.Generator(device=dev).manual_seed(11)
    # sorted list: CSR order, the contributions of an entry side by side, each the entry divided by their number (exact for 1 and 4)
    r_sorted = r.repeat_interleave(contributions)
    c_sorted = d_pos.repeat_interleave(contributions)
    v_sorted = (d_val / contributions).repeat_interleave(contributions)
    del r, counts
    n = r_sorted.numel()
    perm = torch.randperm(n, device=dev, generator=g)
    r_shuf, c_shuf, v_shuf = r_sorted[perm], c_sorted[perm], v_sorted[perm]
    del perm
    nbytes = n * (s + 4) + (0 if contributions == 1 else (nnz + 1) * 4) + nnz * s
    print(f"== {kind}: {rows} rows, {nnz} entries, {n} triplets ({contributions} per entry), {np.dtype(dtype).name}; numeric pass = {nbytes / 1e9:.3f} GB", flush=True)

    def line(name, t, nb=0, note=""):
        med = float(np.median(t))
        rate = f"{nb / (med * 1e-3) / 1e9:9.1f} GB/s" if nb else " " * 14
        print(f"{kind:8s} {name:46s} {med:10.3f} ms [{t.min():9.3f} .. {t.max():9.3f}] {rate}  {note}", flush=True)
        return med

    plans = {}

    def make_plan(key, rr, cc):
        old = plans.pop(key, None)
        if old is not None:
            old.close()
        plans[key] = smm.AssemblyPlan.from_device(rows, rows, n, rr, cc, stream)

    line("(a) plan creation, shuffled list (wall)", measure(lambda: make_plan("shuffled", r_shuf, c_shuf), reps, wall=True), 0, "sort + run heads + pattern; synchronises")
    line("(a) plan creation, sorted list (wall)", measure(lambda: make_plan("sorted", r_sorted, c_sorted), reps, wall=True))
    mats = {}

    def assemble(key, vv):
        old = mats.pop(key, None)
        if old is not None:
            old.close()
        mats[key] = plans[key].assemble_dev(vv, dtype, stream)

    line("(b) assemble_dev, shuffled list", measure(lambda: assemble("shuffled", v_shuf), reps), nbytes + (rows + 1 + nnz) * 8, "pattern copied + numeric pass")
    assemble("sorted", v_sorted)
    c_sorted_ms = line("(c) refill_dev SET, sorted list", measure(lambda: plans["sorted"].refill_dev(mats["sorted"], v_sorted, False, stream), reps), nbytes)
    c_shuf = measure(lambda: plans["shuffled"].refill_dev(mats["shuffled"], v_shuf, False, stream), reps)
    c_shuf_ms = line("(c) refill_dev SET, shuffled list", c_shuf, nbytes)
    line("    refill_dev ADD, shuffled list", measure(lambda: plans["shuffled"].refill_dev(mats["shuffled"], v_shuf, True, stream), reps), nbytes + nnz * s)
    A = mats["shuffled"]

    def old_route(rr, cc, vv):
        A.zero(stream)
        A.update_entries_dev(n, rr, cc, vv, True, None, stream)

    d_sorted = measure(lambda: old_route(r_sorted, c_sorted, v_sorted), reps)
    line("(d) zero + update_entries_dev(ADD), sorted list", d_sorted)
    d_shuf = measure(lambda: old_route(r_shuf, c_shuf, v_shuf), reps)
    line("(d) zero + update_entries_dev(ADD), shuffled list", d_shuf)
    for name, c_ms, d in (("sorted", c_sorted_ms, d_sorted), ("shuffled", c_shuf_ms, d_shuf)):
        spread = float(d.max() - d.min())
        gain = float(np.median(d)) - c_ms
        verdict = "faster than (d) by more than (d)'s spread" if gain > spread else "NOT faster than (d) beyond its spread"
        print(f"{kind:8s} {name}: (d) - (c) = {gain:.3f} ms, spread of (d) over {reps} repetitions = {spread:.3f} ms: (c) is {verdict}; (d) / (c) = {np.median(d) / c_ms:.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "assembly_timing.txt"))
    ap.add_argument("--child", choices=sorted(LIMITS))
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for kind in ("bench", "convdiff"):
            if args.only not in (None, kind):
                continue
            cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(args.reps)]
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for ln in p.stdout:
                sys.stdout.write(ln)
                sys.stdout.flush()
                out.write(ln)
                out.flush()
            p.wait()
            if p.returncode != 0:
                msg = f"{kind}: exit status {p.returncode}; stopping here\n"
                sys.stdout.write(msg)
                out.write(msg)
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
