#!/usr/bin/env python3
"""What near-null-space candidates buy the multigrid preconditioner on one MI355X.  Workload: generators.elasticity3d(n, n, n), Q1 bricks
clamped on one face, fp64, b = A 1, x0 = 0, ConjugateGradient to eps 1e-8, three legs:
  * none              no preconditioner;
  * amg (scalar)      getPreconditioner("AMG"): the hierarchy of the constant vector on the dof graph (candidates=None);
  * amg (6 modes)     getPreconditioner("AMG", candidates=rigid_body_modes(coords), dofs_per_node=3).
Per leg: iterations, ms per solve (median of --reps solves, each between two HIP events, after one warm-up solve); for the AMG legs the
create time (wall clock around the call, the device drained before and after), the levels, the columns dropped, the operator complexity
and us per apply (--inner applies between two events).
    python tools/amg_candidates_timing.py [--n 24 32] [--reps 5] [--inner 20] [--out FILE]
The driver starts one child process per size under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 300  # seconds per child
EPS = 1e-8


def child(n, reps, inner):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import generators as gen
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    start, pos, val, coords = gen.elasticity3d(n, n, n)
    rows = len(start) - 1
    B = gen.rigid_body_modes(coords)
    A = smm.CSRMatrix(rows, rows, start, pos, val)
    b = torch.from_numpy(gen.row_sums(start, val)).to(dev)
    x = torch.zeros(rows, dtype=torch.float64, device=dev)
    zero = torch.zeros(rows, dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out  # ms

    def solve(M):
        x.zero_()
        return host.cg_dev(A, b, zero, x, -1, EPS, M, stream)

    def leg(name, M):
        solve(M)  # the warm-up: the analysis of the matrix, the tile tables, the code objects
        runs = [timed(lambda: solve(M)) for _ in range(reps)]
        ms = float(np.median([r[0] for r in runs]))
        st, it = int(runs[-1][1][0]), int(runs[-1][1][1])
        err = float((x - 1).abs().max())
        line = f"   {name:<16s} status {st} iterations {it:5d}  {ms:9.3f} ms per solve  {1e3 * ms / max(it, 1):8.2f} us per iteration  max|x - 1| {err:.2e}"
        if M is not None:
            y = torch.empty(rows, dtype=torch.float64, device=dev)
            M.apply_dev(b, y, stream)
            ap = float(np.median([timed(lambda: [M.apply_dev(b, y, stream) for _ in range(inner)])[0] for _ in range(reps)])) / inner
            line += f"  {1e3 * ap:8.2f} us per apply"
        print(line, flush=True)

    def made(name, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M = A.getPreconditioner("AMG", **kw)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        info = M.amg_info()
        dropped = [M.amg_candidates(l)["dropped"] for l in range(info["levels"])] if kw else "-"
        print(f"   {name:<16s} create {ms:9.1f} ms  levels {info['levels']}  rows {info['rows']}  dropped {dropped}  operator complexity {info['operator_complexity']:.3f}",
              flush=True)
        return M

    print(f"== elasticity3d({n}, {n}, {n}): {rows} rows, nnz {len(pos)}, float64, eps {EPS}")
    leg("none", None)
    print(f"   SpMV kernel {A.kernel_desc()[0]} {A.get_kernel()}")
    try:
        M = made("amg (scalar)")
        leg("amg (scalar)", M)
        M.close()
    except smm.SmmHipError as e:  # (a coarsest level above 1024 rows is a refusal, not a failure of this tool)
        print(f"   amg (scalar)     refused: {e}", flush=True)
    M = made("amg (6 modes)", candidates=B, dofs_per_node=3)
    leg("amg (6 modes)", M)
    t0 = time.perf_counter()
    M.amg_refresh()
    torch.cuda.synchronize()
    print(f"   amg (6 modes)    refresh {1e3 * (time.perf_counter() - t0):8.1f} ms", flush=True)
    M.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[24, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--child", type=int)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.inner)
    report = []
    status = 0
    for n in args.n:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(args.reps), "--inner", str(args.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        report.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"n = {n}: exit status {r.returncode}; stopping here")
            status = r.returncode
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
