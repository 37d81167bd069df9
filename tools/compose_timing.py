#!/usr/bin/env python3
"""What composing and slicing (csrc/smm_compose.hip) cost on one MI355X, against the only device route there was before them: an
AssemblyPlan over the concatenated (renumbered) triplets plus its assembly.  fp64 and fp32:
  * kkt        K = [[H, Bt], [B, 0]] with H the 161^3 7-point Laplacian and B 3000 constraint rows of 4 .. 12 entries;
  * submatrix  the leading half of H's rows and columns (range form) and every second row and column (index form).
Per leg: ms (median of --reps calls after one warm-up call, wall time around calls that synchronise), the bytes of the byte model of
DESIGN.md section 3.29 -- create nnz (2 s + 8) plus the row pointers, refresh nnz 2 s -- and what fraction of the copy rate of 6.3 TB/s
that is; the ratio to the assembly route is printed last.
    python tools/compose_timing.py [--reps 7] [--only kkt|submatrix] [--out FILE]
The driver starts one child process per workload and dtype under its own `timeout` and stops at the first that fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kkt": 300, "submatrix": 300}  # seconds per child
COPY_RATE = 6.3e12  # bytes per second: what a float4 copy reaches on this memory system
NX, CONSTRAINTS = 161, 3000


def child(kind, dtype_name, reps):
    import torch

    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import generators as gen
    from sparse_matrix_math_amd import host

    smm.init(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dtype = np.dtype(dtype_name).type
    td = torch.float64 if dtype == np.float64 else torch.float32
    s = np.dtype(dtype).itemsize
    rows, nnz = NX**3, host.gen_stencil3d_nnz(NX, NX, NX)
    h_dev = [torch.empty(rows + 1, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=td, device=dev)]
    host.gen_stencil3d_dev(NX, NX, NX, 6.0, -1.0, -1.0, *h_dev, dtype, stream)
    torch.cuda.synchronize()
    H = smm.CSRMatrix.from_device(rows, rows, *h_dev, dtype)

    def timed(fn):
        fn()  # the warm-up: code objects, the operand check (kept in the handles), the allocator's blocks
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            del out
        return float(np.median(ms)), float(min(ms))

    def report(name, ms, best, bytes_moved=None):
        line = f"   {name:<36s} {ms:9.3f} ms (best {best:9.3f})"
        if bytes_moved:
            line += f"  {bytes_moved / 1e9:7.3f} GB by the model  {bytes_moved / (ms * 1e-3) / COPY_RATE:5.2f} of the copy rate"
        print(line, flush=True)
        return ms

    def row_index(start_t, n):
        return torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), (start_t[1:] - start_t[:-1]).to(torch.int64))

    def assembly_route(m, n, r, c, v):
        count = int(r.numel())

        def plan_and_assemble():
            plan = smm.AssemblyPlan.from_device(m, n, count, r, c, stream)
            return plan, plan.assemble_dev(v, dtype, stream)

        return plan_and_assemble

    def same_matrix(X, Y):
        return (X.rows, X.cols, X.nnz) == (Y.rows, Y.cols, Y.nnz) and all(np.array_equal(a, b) for a, b in zip(X.get_pattern(), Y.get_pattern())) and \
            bool(np.array_equal(X.get_values().view(np.uint8), Y.get_values().view(np.uint8)))

    ok = True
    if kind == "kkt":
        b = gen.random_rows(CONSTRAINTS, rows, 4, 12, seed=5, dtype=dtype)
        B = smm.CSRMatrix(CONSTRAINTS, rows, *b)
        Bt = B.transpose()
        table = [[H, Bt], [B, None]]
        K = smm.bmat(table, stream=stream)
        print(f"== kkt: H {NX}^3 = {rows} rows ({nnz} entries), B {CONSTRAINTS} x {rows} ({B.nnz} entries), {dtype_name}: K {K.rows} x {K.cols}, {K.nnz} entries", flush=True)
        ptr = 4 * (2 * (rows + Bt.rows) + B.rows + K.rows + 1)
        create = report("bmat (create)", *timed(lambda: smm.bmat(table, stream=stream)), K.nnz * (2 * s + 8) + ptr)
        report("block_refresh", *timed(lambda: K.block_refresh(table, stream=stream)), K.nnz * 2 * s + ptr)
        bt = [torch.from_numpy(a).to(dev) for a in (*Bt.get_pattern(), Bt.get_values())]
        bd = [torch.from_numpy(a).to(dev) for a in b]
        r = torch.cat([row_index(h_dev[0], rows), row_index(bt[0], rows), row_index(bd[0], CONSTRAINTS) + rows])
        c = torch.cat([h_dev[1], bt[1] + rows, bd[1]])
        v = torch.cat([h_dev[2], bt[2], bd[2]])
        torch.cuda.synchronize()
        route = assembly_route(K.rows, K.cols, r, c, v)
        before = report("assembly: plan + csr_create", *timed(route))
        ok = same_matrix(route()[1], K)
        print(f"   the two routes agree bit for bit: {ok}; bmat is {before / create:.1f} x faster than the assembly route", flush=True)
    else:
        half = rows // 2
        every_second = np.arange(0, rows, 2, dtype=np.int32)
        d_idx = torch.from_numpy(every_second).to(dev)
        R = H.submatrix(slice(0, half), slice(0, half), stream=stream)
        E = H.submatrix_dev(d_idx, len(every_second), d_idx, len(every_second), stream=stream)
        print(f"== submatrix: H {NX}^3 = {rows} rows ({nnz} entries), {dtype_name}: leading half {R.rows} rows, {R.nnz} entries; every second {E.rows} rows, {E.nnz} entries",
              flush=True)
        r_all = row_index(h_dev[0], rows)
        for name, S, make, keep, renum in (("range", R, lambda: H.submatrix(slice(0, half), slice(0, half), stream=stream), (r_all < half) & (h_dev[1] < half), lambda t: t),
                                           ("index", E, lambda: H.submatrix_dev(d_idx, len(every_second), d_idx, len(every_second), stream=stream),
                                            (r_all % 2 == 0) & (h_dev[1] % 2 == 0), lambda t: t // 2)):
            read = int(h_dev[0][S.rows if name == "range" else rows].item()) if name == "range" else nnz // 2
            model = 2 * read * 4 + read * s + S.nnz * (s + 8) + 4 * (3 * S.rows) + (4 * rows if name == "index" else 0)
            create = report(f"submatrix, {name} form (create)", *timed(make), model)
            report(f"submatrix_refresh, {name} form", *timed(lambda S=S: S.submatrix_refresh(H, stream=stream)), S.nnz * (2 * s + 4))
            r, c, v = renum(r_all[keep]).contiguous(), renum(h_dev[1][keep]).contiguous(), h_dev[2][keep].contiguous()
            torch.cuda.synchronize()
            route = assembly_route(S.rows, S.cols, r, c, v)
            before = report("assembly: plan + csr_create", *timed(route))
            same = same_matrix(route()[1], S)
            ok = ok and same
            print(f"   the two routes agree bit for bit: {same}; submatrix is {before / create:.1f} x faster than the assembly route", flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=sorted(LIMITS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(LIMITS))
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.dtype, args.reps)
    report = []
    status = 0
    for kind in ([args.only] if args.only else ["kkt", "submatrix"]):
        for dtype in ("float64", "float32"):
            cmd = ["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--child", kind, "--dtype", dtype, "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            report.append(r.stdout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                print(f"{kind} {dtype}: exit status {r.returncode}; stopping here")
                report.append(f"{kind} {dtype}: exit status {r.returncode}\n")
                status = r.returncode
                break
        if status:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main())
