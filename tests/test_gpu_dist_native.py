"""The native row-partitioned solvers (csrc/smm_dist.hip, behind smm_hip_dist_*) on ONE GPU.

RCCL cannot put two ranks on one device, so several ranks are run as threads of this process joined by a host-callback
communicator (smm_hip_comm_create_host): every byte of the halo exchanges and all-reduces really travels between the ranks, only
through host memory.  The RCCL code path itself is exercised with a real one-rank RCCL communicator (dlopen, ncclCommInitRank,
ncclAllReduce, grouped ncclSend / ncclRecv to itself) and, end to end, by bench.py's two-process gloo rehearsal.
Reference of every result: the single-process CPU oracle."""
import json
import os
import queue
import subprocess
import sys
import threading

import numpy as np
import pytest

from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu


class _Shared:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.mail = {}
        self.lock = threading.Lock()


def _host_comm(shared, rank):
    """smm_hip_comm over host callbacks: the ranks are threads of this process"""
    from sparse_matrix_math_amd.distributed import NativeComm

    def allreduce(a):
        shared.slots[rank] = a.copy()
        shared.barrier.wait()
        total = shared.slots[0].copy()
        for q in range(1, shared.world):
            total += shared.slots[q]
        shared.barrier.wait()
        a[:] = total

    def box(src, dst):
        with shared.lock:
            return shared.mail.setdefault((src, dst), queue.Queue())

    def sendrecv(sends, recvs):  # pairwise hand-off: a rank without neighbours never gets here, so no global barrier
        for peer, buf in sends:
            box(rank, peer).put(buf.copy())
        for peer, buf in recvs:
            buf[:] = box(peer, rank).get(timeout=120)

    return NativeComm.host(rank, shared.world, allreduce, sendrecv)


def _run_ranks(world, fn):
    """fn(rank, shared) -> result, run on `world` threads; an exception in one rank aborts the others' barriers"""
    shared = _Shared(world)
    out, errors = [None] * world, []

    def main(rank):
        try:
            import torch

            torch.cuda.set_device(0)
            out[rank] = fn(rank, shared)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            shared.barrier.abort()

    threads = [threading.Thread(target=main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return out


def _solve(smm, csr, b_full, world, dtype, max_it, eps, solver="bicgstab", precond=None, x0_full=None, families=None, chunks_seen=None, options_seen=None,
           own_streams=False, forms_seen=None, lanes=None, bounds=None):
    import torch

    from sparse_matrix_math_amd.distributed import NativeDistMatrix, partition_rows_by_nnz

    dev = torch.device("cuda:0")
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    start, pos, val = csr
    n = len(start) - 1
    bounds = bounds or partition_rows_by_nnz(lambda i: int(start[i]), n, world)

    def rank_main(rank, shared):
        lo, hi = bounds[rank], bounds[rank + 1]
        comm = _host_comm(shared, rank)
        comm.selftest()
        d_start = torch.from_numpy((start[lo:hi + 1] - start[lo]).astype(np.int32)).to(dev)
        d_pos = torch.from_numpy(pos[start[lo]:start[hi]].copy()).to(dev)
        d_val = torch.from_numpy(val[start[lo]:start[hi]].copy()).to(dev)
        A = NativeDistMatrix(comm, n, bounds, d_start, d_pos, d_val, dtype)
        assert A.n_local == hi - lo and A.nnz_loc + A.nnz_rem == int(start[hi] - start[lo])
        A.set_precond(precond)
        for blk, L in zip(A.local_blocks(), lanes or ()):
            blk.set_kernel(3, L)  # SMM_SPMV_PATTERN at L pieces per row, whatever the solvers' adoption would have decided
        b = torch.from_numpy(b_full[lo:hi].copy()).to(dev)
        x = torch.zeros(hi - lo, dtype=tdt, device=dev) if x0_full is None else torch.from_numpy(x0_full[lo:hi].copy()).to(dev)
        # y = A x through the distributed SpMV as well
        y = torch.empty(hi - lo, dtype=tdt, device=dev)
        # own_streams: every thread rank works on a stream of its own and nobody synchronises the DEVICE while a peer may be running: with the
        # peer-to-peer path kernels of one rank wait (bounded) for kernels of another, which must neither sit behind them on the shared default
        # stream nor be waited for by a device-wide synchronise of the rank they wait for (ranks in separate processes on separate GPUs -- the
        # real deployment -- cannot do that to each other)
        own = torch.cuda.Stream(device=dev) if own_streams else None
        stream = own.cuda_stream if own_streams else None
        if own_streams:
            torch.cuda.synchronize()
            shared.barrier.wait()
        A.spmv(0, None, b, y, stream)
        if solver == "cg":
            res = A.cg(b, x, x, max_it, eps, stream)
        else:
            res = A.bicgstab(b, x, max_it, eps, stream)
        if own_streams:
            own.synchronize()
            shared.barrier.wait()
        torch.cuda.synchronize()
        if families is not None:  # (kernel family, lanes, PATTERN encoding) of this rank's A_loc and A_rem after the solve
            families[rank] = tuple(blk.get_kernel() + blk.pattern_info()[:1] for blk in A.local_blocks()) + (A.local_blocks()[0].kernel_desc()[0],)
        if chunks_seen is not None:
            chunks_seen[rank] = A.halo_chunks
        if options_seen is not None:
            options_seen[rank] = dict(A.options)
        if forms_seen is not None:  # (rows listed as holding a remote entry, SpMVs over those rows only, SpMVs of cg() that formed the direction themselves)
            forms_seen[rank] = A.thin_remote() + (A.cg_fused(),)
        r = (res, lo, hi, x.cpu().numpy(), y.cpu().numpy(), A.halo_elements)
        A.close()
        comm.close()
        return r

    out = _run_ranks(world, rank_main)
    x, y = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for res, lo, hi, xs, ys, _ in out:
        x[lo:hi], y[lo:hi] = xs, ys
        assert res == out[0][0]  # every rank reports the same status / iterations / residual
    return out[0][0], x, y, sum(o[5] for o in out)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_native_bicgstab_matches_oracle(smm, oracle, world, dtype):
    cases = {
        "banded": gen.banded_random_spd(60000, k=12, seed=4, max_offset=9000, dtype=dtype),
        "convdiff": gen.convdiff3d(20, 0.3, dtype=dtype),
    }
    tol = 3e-4 if dtype == np.float32 else 1e-10
    for name, csr in cases.items():
        n = len(csr[0]) - 1
        x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
        b = oracle.spmv(csr, 0, None, x_true)
        for max_it in (1, 6):
            (status, iters, res), x, y, halo = _solve(smm, csr, b, world, dtype, max_it, 1e-30)
            st_ref, x_ref, it_ref, res_ref = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), max_it, 1e-30)
            assert status == st_ref == 0 and iters == it_ref == max_it, (name, world)
            assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref))), (name, world, max_it)
            assert abs(res - res_ref) <= 50 * tol * max(res_ref, 1e-30) + 1e-30
            assert (halo > 0) == (world > 1)
            y_ref = oracle.spmv(csr, 0, None, b)
            assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8
        if name == "convdiff":
            eps = 1e-3 if dtype == np.float32 else 1e-8
            (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, eps)
            assert status == 0 and res <= eps
            np.testing.assert_allclose(x, x_true, rtol=1e-3 if dtype == np.float32 else 1e-7)
    # maxIterations == 0: the body runs once and the status is MAX_ITERATIONS_REACHED (ref:2277-2282)
    csr = cases["convdiff"]
    n = len(csr[0]) - 1
    b = oracle.spmv(csr, 0, None, np.ones(n, dtype=dtype))
    (status, iters, _), _, _, _ = _solve(smm, csr, b, world, dtype, 0, 1e-30)
    assert (status, iters) == (2, 1)


@pytest.mark.parametrize("world,chunks", [(2, 2), (3, 4), (4, 3)])
def test_halo_in_pieces(smm, oracle, world, chunks, monkeypatch):
    """SMM_HIP_HALO_CHUNKS: the halo of every SpMV travels in `chunks` exchanges and A_rem is cut by columns into as many parts, part k
    starting when piece k has landed (csrc/smm_dist_matvec.hip, distMatvec).  Row sums are then ((loc + rem_0) + rem_1) + ...: within the bound
    the one-piece form is held to.  Both kernel families (the banded matrix's blocks stay on the CSR kernels at 6 iterations; the
    converged solves adopt PATTERN), BiCGStab with and without Jacobi (the division rides in the LAST part's epilogue), CG."""
    monkeypatch.setenv("SMM_HIP_HALO_CHUNKS", str(chunks))
    P = smm.SolverPreconditioner
    for dtype in (np.float32, np.float64):
        tol = 3e-4 if dtype == np.float32 else 1e-10
        csr = gen.banded_random_spd(60000, k=12, seed=4, max_offset=9000, dtype=dtype)
        n = len(csr[0]) - 1
        x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
        b = oracle.spmv(csr, 0, None, x_true)
        seen = {}
        (status, iters, res), x, y, halo = _solve(smm, csr, b, world, dtype, 6, 1e-30, chunks_seen=seen)
        assert set(seen.values()) == {chunks}, seen
        st_ref, x_ref, it_ref, res_ref = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 6, 1e-30)
        assert status == st_ref == 0 and iters == it_ref == 6 and halo > 0
        assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))
        y_ref = oracle.spmv(csr, 0, None, b)
        assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8
    dtype = np.float64
    # converged, >= 2^20 entries per block for the small worlds: the parts adopt the PATTERN family like A_loc does
    csr = gen.banded_random_spd(100_000, k=12, seed=4, max_offset=9000, dtype=dtype)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n)
    b = oracle.spmv(csr, 0, None, x_true)
    for precond in (None, P.JACOBI):
        (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, 1e-9, precond=precond)
        assert status == 0 and res <= 1e-9
        np.testing.assert_allclose(x, x_true, rtol=1e-8)
    csr = gen.stencil3d(40, 40, 40, dtype=dtype)
    n = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2]).astype(dtype)
    (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, 10, 0.0, solver="cg")
    st_ref, x_ref, it_ref, res_ref = oracle.cg(csr, b, np.zeros(n), 10, 0.0)
    assert (status, iters) == (st_ref, it_ref) == (2, 10)
    np.testing.assert_allclose(x, x_ref, rtol=1e-10, atol=1e-12)


def _upwind_matrix(n, far, dtype):
    """structurally NON-symmetric: row i holds the diagonal and the two upwind entries i - 1, i - far (lower triangular)"""
    rows = np.arange(n)
    cols = np.stack([rows - far, rows - 1, rows], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -0.5, 4.0]), cols.shape) * (1.0 + 0.25 * np.sin(0.37 * rows))[:, None]
    keep = cols >= 0
    start = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return start, cols[keep].astype(np.int32), vals[keep].astype(dtype)


@pytest.mark.parametrize("world,chunks", [(2, 1), (3, 2), (4, 4)])
def test_one_sided_halo(smm, oracle, world, chunks, monkeypatch):
    """An upwind (lower triangular) matrix: rank 0 RECEIVES nothing -- its A_rem is empty -- but sends to rank 1, the last rank sends
    nothing.  With the halo in pieces every rank must still run the K-exchange form (`chunks` is agreed collectively; r04 let a rank
    with an empty A_rem fall through to one full-count exchange while its peer posted K piece-sized receives: ADVICE r04), and the fused
    dot products of the rank without remote entries ride in its (empty) last part."""
    monkeypatch.setenv("SMM_HIP_HALO_CHUNKS", str(chunks))
    for dtype in (np.float32, np.float64):
        tol = 3e-4 if dtype == np.float32 else 1e-10
        csr = _upwind_matrix(30000, 700, dtype)
        n = len(csr[0]) - 1
        x_true = np.random.default_rng(5).uniform(0.5, 1.5, n).astype(dtype)
        b = oracle.spmv(csr, 0, None, x_true)
        seen = {}
        for precond in (None, smm.SolverPreconditioner.JACOBI):
            (status, iters, res), x, y, halo = _solve(smm, csr, b, world, dtype, 6, 1e-30, precond=precond, chunks_seen=seen)
            assert set(seen.values()) == {chunks}, seen
            if precond is None:
                st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 6, 1e-30)
            else:
                from oracle.oracle import PRECOND_JACOBI

                _, diag = oracle.jacobi_setup(csr)
                st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 6, 1e-30, PRECOND_JACOBI, diag)
            assert status == st_ref == 0 and iters == it_ref == 6
            assert halo == (world - 1) * 700  # every rank but the first receives the `far` rows above its own
            assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))
            y_ref = oracle.spmv(csr, 0, None, b)
            assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8


@pytest.mark.parametrize("world", [1, 2])
def test_native_loops_adopt_the_pattern_family(smm, oracle, world):
    """a solve with many iterations ahead lets both local blocks take the index-free family (>= 2^20 entries; adoptPatternForSolver):
    BiCGStab on a banded matrix (row masks + values), CG on a 3-D Laplacian (constant diagonals: no values[] read), to convergence"""
    dtype = np.float64
    csr = gen.banded_random_spd(100_000, k=12, seed=4, max_offset=9000, dtype=dtype)  # 2.5 M entries
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n)
    b = oracle.spmv(csr, 0, None, x_true)
    fam = {}
    (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, 1e-9, families=fam)
    assert status == 0 and res <= 1e-9
    np.testing.assert_allclose(x, x_true, rtol=1e-8)
    for rank in range(world):
        loc, rem = fam[rank][:2]
        assert loc[0] == 3 and loc[2] == 1, fam  # PATTERN, row masks
        assert world == 1 or rem[0] in (1, 2, 3)  # (A_rem is small: VECTOR / STREAM unless it reaches 2^20 entries)
    csr = gen.stencil3d(72, 72, 72, dtype=dtype)  # 2.6 M entries
    n = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2]).astype(dtype)
    fam = {}
    (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, 1e-9, solver="cg", families=fam)
    st_ref, x_ref, it_ref, _ = oracle.cg(csr, b, np.zeros(n), -1, 1e-9)
    assert status == st_ref == 0 and abs(iters - it_ref) <= 2
    np.testing.assert_allclose(x, np.ones(n), rtol=1e-6)
    for rank in range(world):
        assert fam[rank][0] == (3, 1, 3), fam  # PATTERN, one lane per row, constant diagonals


def test_native_cg_on_slabs_of_a_big_grid_uses_the_march_kernel(smm, oracle):
    """BASELINE config 4 in small: CG on a 3-D Laplacian split into two slabs of > 2^21 rows each.  The partition balances stored entries,
    so a slab starts and ends INSIDE a grid plane; its local block is still grid-shaped (offsets +-1, +-nx, +-nx ny) and must be served
    by the 2.5-D constant-diagonal kernel (partial first / last planes, the fused dot products finished in the launch), the few remote
    entries by the remote block.  x after 12 iterations against the single-process oracle."""
    dtype = np.float64
    csr = gen.stencil3d(160, 160, 172, dtype=dtype)  # 4.4 M rows
    n = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2]).astype(dtype)
    fam = {}
    (status, iters, res), x, y, halo = _solve(smm, csr, b, 2, dtype, 20, 0.0, solver="cg", families=fam)
    st_ref, x_ref, it_ref, res_ref = oracle.cg(csr, b, np.zeros(n), 20, 0.0)
    assert (status, iters) == (st_ref, it_ref) == (2, 20) and halo == 2 * 160 * 160
    np.testing.assert_allclose(x, x_ref, rtol=1e-10, atol=1e-12)
    np.testing.assert_array_equal(y, oracle.spmv(csr, 0, None, b))  # one lane per row everywhere: the reference's bits
    for rank in range(2):
        assert fam[rank][0] == (3, 1, 3), fam  # A_loc: PATTERN, one lane per row, constant diagonals
        assert fam[rank][2] == "spmvPatternConstMarchKernel", fam


@pytest.mark.parametrize("world", [1, 2, 4])
def test_native_cg_matches_oracle(smm, oracle, world):
    dtype = np.float64
    csr = gen.poisson2d(48, dtype=dtype)
    n = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2]).astype(dtype)
    for max_it in (1, 3, 10):
        (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, max_it, 0.0, solver="cg")
        st_ref, x_ref, it_ref, res_ref = oracle.cg(csr, b, np.zeros(n), max_it, 0.0)
        assert (status, iters) == (st_ref, it_ref) == (2, max_it)
        np.testing.assert_allclose(x, x_ref, rtol=1e-10, atol=1e-12)
        assert abs(res - res_ref) <= 1e-8 * res_ref
    (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, 1e-8, solver="cg")
    st_ref, x_ref, it_ref, _ = oracle.cg(csr, b, np.zeros(n), -1, 1e-8)
    assert status == st_ref == 0 and abs(iters - it_ref) <= 2
    np.testing.assert_allclose(x, np.ones(n), rtol=1e-6)
    # early exit leaves x untouched (ref:2342-2344)
    x0 = np.ones(n)
    (status, iters, _), x, _, _ = _solve(smm, csr, b, world, dtype, -1, 1e-6, solver="cg", x0_full=x0)
    assert (status, iters) == (0, 0)
    np.testing.assert_array_equal(x, x0)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_native_cg_deferred_x_is_bit_identical(smm, oracle, world):
    """distCgLazyP (csrc/smm_dist.hip): on vectors beyond the caches the row-partitioned CG keeps its last eight directions in a ring of
    halo-extended vectors and brings x up to date every eighth iteration, in the last planned one and in the launch that finds the
    iteration converged -- the reference's roundings in the reference's order (ref:2362-2366).  Forced on at a small size: iteration
    counts around the window of eight, convergence inside a window, an early exit, a start vector away from zero -- the eager loop's bits."""
    from sparse_matrix_math_amd import host

    dtype = np.float64
    csr = gen.poisson2d(48, dtype=dtype)
    n = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2]).astype(dtype)
    x0 = np.random.default_rng(11).uniform(-1, 1, n)
    try:
        for max_it, eps in [(k, 0.0) for k in (1, 2, 7, 8, 9, 15, 16, 17, 19)] + [(-1, 1e-8), (-1, 1e-3), (40, 1e-2), (-1, 1e3)]:
            got = {}
            for lazy in (True, False):
                host.set_cg_lazy_x_min_bytes(0 if lazy else 1 << 60)
                got[lazy] = _solve(smm, csr, b, world, dtype, max_it, eps, solver="cg", x0_full=x0)
            assert got[True][0] == got[False][0], (max_it, eps, got[True][0], got[False][0])
            np.testing.assert_array_equal(got[True][1], got[False][1], err_msg=f"max_it {max_it} eps {eps}")
        st_ref, x_ref, it_ref, _ = oracle.cg(csr, b, x0.copy(), 17, 0.0)
        host.set_cg_lazy_x_min_bytes(0)
        (status, iters, _), x, _, _ = _solve(smm, csr, b, world, dtype, 17, 0.0, solver="cg", x0_full=x0)
        assert (status, iters) == (st_ref, it_ref)
        np.testing.assert_allclose(x, x_ref, rtol=1e-10, atol=1e-12)
    finally:
        host.set_cg_lazy_x_min_bytes(-1)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_native_preconditioned(smm, oracle, world):
    """block-Jacobi by rank: one rank = the single-GPU preconditioned solver; Jacobi is the same preconditioner for any number of
    ranks; SGS / ILU0 and their block forms on several ranks are weaker preconditioners that must still converge and still help"""
    P = smm.SolverPreconditioner
    dtype = np.float64
    csr = gen.convdiff3d(16, 0.3, dtype=dtype)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(7).uniform(0.5, 1.5, n)
    b = oracle.spmv(csr, 0, None, x_true)
    A = smm.CSRMatrix(n, n, *csr)
    eps = 1e-9
    (_, it_none, _), _, _, _ = _solve(smm, csr, b, world, dtype, -1, eps)
    for kind in (P.JACOBI, P.ILU0, P.SYMMETRIC_GAUS_SEIDEL, P.BLOCK_ILU0, P.BLOCK_SGS):
        (status, iters, res), x, _, _ = _solve(smm, csr, b, world, dtype, -1, eps, precond=kind)
        assert status == 0 and res <= eps, (kind, world)
        np.testing.assert_allclose(x, x_true, rtol=1e-6, err_msg=f"{kind} world {world}")
        assert iters <= 2 * it_none, (kind, world, iters, it_none)
        if kind != P.JACOBI:
            assert iters < it_none, (kind, world, iters, it_none)
        if world == 1:
            xs = np.zeros(n)
            info = {}
            st = smm.BiCGStab(A, b.copy(), xs, -1, eps, A.getPreconditioner(kind), info=info)
            assert int(st) == 0 and abs(info["iterations"] - iters) <= 1
            np.testing.assert_allclose(x, xs, rtol=1e-7)


def test_native_rccl_single_rank(smm, oracle):
    """a real RCCL communicator (one rank): librccl found by dlopen, ncclCommInitRank from a unique id, the all-reduce and the grouped
    send / recv (to itself) of the self-test, and the loop with its all-reduces on the side stream"""
    import torch

    from sparse_matrix_math_amd import _lib
    from sparse_matrix_math_amd.distributed import NativeComm, NativeDistMatrix
    import ctypes

    lib = _lib.load()
    ident = ctypes.create_string_buffer(128)
    _lib.check(lib.smm_hip_comm_unique_id(ident))
    h = ctypes.c_void_p()
    _lib.check(lib.smm_hip_comm_create_rccl(0, 1, ident, ctypes.byref(h)))
    comm = NativeComm(h)
    assert comm.info() == {"rank": 0, "world": 1, "kind": "rccl", "rccl_ranks": 1}  # rccl_ranks: ncclCommCount
    comm.selftest()
    dev = torch.device("cuda:0")
    dtype = np.float32
    csr = gen.banded_random_spd(50000, 10, 77, 6000, dtype, 1.0)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
    b = oracle.spmv(csr, 0, None, x_true)
    tens = [torch.from_numpy(a).to(dev) for a in csr]
    A = NativeDistMatrix(comm, n, [0, n], tens[0], tens[1], tens[2], dtype)
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    status, iters, res = A.bicgstab(torch.from_numpy(b).to(dev), x, 5, 0.0)
    st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 5, 0.0)
    assert status == st_ref and iters == it_ref == 5
    assert float(np.max(np.abs(x.cpu().numpy() - x_ref))) <= 3e-4 * float(np.max(np.abs(x_ref)))
    A.close()
    comm.close()


def test_rccl_init_gives_up_when_a_peer_never_arrives():
    """failure containment: ncclCommInitRank for a world of 2 with only this rank present must not block for ever --
    after SMM_HIP_COMM_TIMEOUT_S the call returns SMM_HIP_ERR_COMM, and the process can leave with a status of its own (a fresh
    process here: the helper thread left behind in ncclCommInitRank dies with it)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import ctypes, os, sys, time\n"
        "sys.path.insert(0, %r)\n"
        "import sparse_matrix_math_amd as smm\n"
        "from sparse_matrix_math_amd import _lib\n"
        "smm.init(0)\n"
        "lib = _lib.load()\n"
        "ident = ctypes.create_string_buffer(128)\n"
        "_lib.check(lib.smm_hip_comm_unique_id(ident))\n"
        "h = ctypes.c_void_p()\n"
        "t0 = time.time()\n"
        "rc = lib.smm_hip_comm_create_rccl(0, 2, ident, ctypes.byref(h))\n"
        "print('RC', rc, 'SECONDS', round(time.time() - t0, 1), lib.smm_hip_last_error().decode(), flush=True)\n"
        "os._exit(7 if rc == -6 else 1)\n" % root)
    env = dict(os.environ, SMM_HIP_COMM_TIMEOUT_S="4", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 7, out.stdout + out.stderr[-2000:]
    assert "RC -6" in out.stdout and "ncclCommInitRank" in out.stdout
    seconds = float(out.stdout.split("SECONDS")[1].split()[0])
    assert 3.5 <= seconds <= 30


def test_partition_rows_by_nnz_native_matches_python(smm):
    import ctypes

    from sparse_matrix_math_amd import _lib
    from sparse_matrix_math_amd.distributed import partition_rows_by_nnz

    start = gen.banded_random_spd(30000, 6, 1, 4000, np.float32)[0]
    for world in (1, 2, 3, 8):
        out = (ctypes.c_int * (world + 1))()
        _lib.check(_lib.load().smm_hip_partition_rows_by_nnz(start.ctypes.data_as(ctypes.c_void_p), len(start) - 1, world, out))
        assert list(out) == partition_rows_by_nnz(lambda i: int(start[i]), len(start) - 1, world)


def _solve_forms(smm, csr, b_full, world, dtype, lanes, split, sums_lds=None, thin=None):
    """SpMV (three ops), BiCGStab with / without Jacobi and CG on thread ranks with both local blocks forced to the PATTERN family at `lanes` =
    (A_loc, A_rem) pieces per row; `split` = SMM_HIP_SPLIT_SPMV at create time.  Returns the assembled bytes and the counts of matvec forms."""
    import torch

    from sparse_matrix_math_amd.distributed import NativeDistMatrix, partition_rows_by_nnz

    dev = torch.device("cuda:0")
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    start, pos, val = csr
    n = len(start) - 1
    bounds = partition_rows_by_nnz(lambda i: int(start[i]), n, world)
    os.environ["SMM_HIP_SPLIT_SPMV"] = "1" if split else "0"
    if sums_lds is not None:
        os.environ["SMM_HIP_SPLIT_SUMS_LDS"] = str(sums_lds)  # 0: the local half's row sums travel through out[] (what many rows per workgroup get)
    if thin is not None:
        os.environ["SMM_HIP_THIN_REMOTE"] = "1" if thin else "0"  # (0: the general second launch also where few rows hold a remote entry)

    def rank_main(rank, shared):
        lo, hi = bounds[rank], bounds[rank + 1]
        comm = _host_comm(shared, rank)
        d_start = torch.from_numpy((start[lo:hi + 1] - start[lo]).astype(np.int32)).to(dev)
        d_pos = torch.from_numpy(pos[start[lo]:start[hi]].copy()).to(dev)
        d_val = torch.from_numpy(val[start[lo]:start[hi]].copy()).to(dev)
        A = NativeDistMatrix(comm, n, bounds, d_start, d_pos, d_val, dtype)
        for blk, L in zip(A.local_blocks(), lanes or ()):
            blk.set_kernel(3, L)  # SMM_SPMV_PATTERN: the analysis runs now, on the block's own arrays
        b = torch.from_numpy(b_full[lo:hi].copy()).to(dev)
        out = []
        for op in (0, 1, 2):  # assign / add / sub (ref:1458-1515), lhs = b
            y = torch.empty(hi - lo, dtype=tdt, device=dev)
            A.spmv(op, b if op else None, b, y)
            torch.cuda.synchronize()
            out.append(y.cpu().numpy())
        for solver, precond, max_it in (("bicgstab", None, 7), ("bicgstab", smm.SolverPreconditioner.JACOBI, 7), ("cg", None, 9)):
            A.set_precond(precond)
            x = torch.zeros(hi - lo, dtype=tdt, device=dev)
            res = A.cg(b, x, x, max_it, 1e-30) if solver == "cg" else A.bicgstab(b, x, max_it, 1e-30)
            torch.cuda.synchronize()
            out.append(x.cpu().numpy())
            out.append(np.array(res, dtype=np.float64))
        forms = A.matvec_forms() + A.thin_remote()
        A.set_precond(None)
        A.close()
        comm.close()
        return out, forms

    try:
        got = _run_ranks(world, rank_main)
    finally:
        os.environ.pop("SMM_HIP_SPLIT_SPMV", None)
        os.environ.pop("SMM_HIP_SPLIT_SUMS_LDS", None)
        os.environ.pop("SMM_HIP_THIN_REMOTE", None)
    pieces = [np.concatenate([g[0][i] for g in got]).tobytes() if got[0][0][i].shape != (3,) else got[0][0][i].tobytes() for i in range(len(got[0][0]))]
    return pieces, [g[1] for g in got]


@pytest.mark.parametrize("world,dtype,lanes", [(2, np.float32, (2, 1)), (3, np.float64, (2, 2)), (2, np.float64, (1, 1)), (3, np.float32, (4, 2)), (2, np.float32, (1, 4))])
def test_one_launch_spmv_is_the_two_launches_bit_for_bit(smm, oracle, world, dtype, lanes):
    """csrc/smm_spmv_split.hip (r06): the row-partitioned SpMV as ONE launch -- the local half of a workgroup's rows, the
    wait for the exchange's word, the remote half, out[] written once -- against the two launches (A_loc, then A_rem behind the exchange):
    every SpMV op, BiCGStab with and without the Jacobi division in the epilogue, CG, fp32 / fp64, every pairing of pieces per row the
    blocks can have -- the same bytes; and against the oracle within the piece forms' bound."""
    csr = gen.banded_random_spd(60000, k=12, seed=4, max_offset=9000, dtype=dtype)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
    b = oracle.spmv(csr, 0, None, x_true)
    one, forms_one = _solve_forms(smm, csr, b, world, dtype, lanes, split=True)
    two, forms_two = _solve_forms(smm, csr, b, world, dtype, lanes, split=False)
    assert all(f[0] > 0 and f[1] == 0 for f in forms_one), forms_one  # every SpMV with a halo ran as one launch ...
    assert all(f[0] == 0 and f[1] > 0 for f in forms_two), forms_two  # ... / as two
    # the SpMV itself: the same bytes, every op.  The solvers' dot products ride in the epilogue as per-WORKGROUP partial sums, and the two forms
    # deal the rows to workgroups differently: their scalars agree to rounding, x to the solvers' tolerance
    assert [a == b_ for a, b_ in zip(one[:3], two[:3])] == [True] * 3
    tol = 3e-4 if dtype == np.float32 else 1e-10
    for i in (3, 5, 7):
        xa, xb = np.frombuffer(one[i], dtype=dtype), np.frombuffer(two[i], dtype=dtype)
        assert float(np.max(np.abs(xa - xb))) <= tol * float(np.max(np.abs(xb))), i
        ra, rb = np.frombuffer(one[i + 1], dtype=np.float64), np.frombuffer(two[i + 1], dtype=np.float64)
        assert tuple(ra[:2]) == tuple(rb[:2]) and abs(ra[2] - rb[2]) <= 50 * tol * max(abs(rb[2]), 1e-30), (ra, rb)
    y = np.frombuffer(one[0], dtype=dtype)
    y_ref = oracle.spmv(csr, 0, None, b)
    assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8
    st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 7, 1e-30)
    x = np.frombuffer(one[3], dtype=dtype)
    assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))


def _ragged(csr, seed, drop=0.3):
    """the band with holes: every off-diagonal entry dropped with probability `drop`, a run of rows reduced to their diagonal, a run of rows
    that keep only entries LEFT of the diagonal and one that keeps only entries far to the RIGHT (rows without a local / without a remote
    part for some partition); diagonally dominant as before"""
    start, pos, val = csr
    n = len(start) - 1
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), np.diff(start))
    keep = (pos == rows) | (rng.random(len(pos)) >= drop)
    keep &= ~((rows >= n // 5) & (rows < n // 5 + 300) & (pos != rows))
    keep &= ~((rows >= n // 2) & (rows < n // 2 + 500) & (pos > rows))
    keep &= ~((rows >= n // 3) & (rows < n // 3 + 500) & (pos != rows) & (pos < rows + 2000))
    new_start = np.zeros(n + 1, dtype=np.int32)
    np.add.at(new_start, rows[keep] + 1, 1)
    return np.cumsum(new_start).astype(np.int32), pos[keep].copy(), val[keep].copy()


@pytest.mark.parametrize("world,dtype,lanes,seed", [(2, np.float32, (2, 1), 1), (3, np.float64, (1, 1), 2), (3, np.float32, (4, 2), 3), (2, np.float64, (2, 4), 4),
                                                    (4, np.float32, (1, 2), 5)])
def test_one_launch_spmv_on_ragged_matrices(smm, oracle, world, dtype, lanes, seed):
    """the one-launch SpMV on bands with HOLES: rows of every length, rows without a local or without a remote part, runs of diagonal-only rows
    (wavefronts whose rows differ take the general path beside wavefronts that take the uniform one), partial tiles at the end -- the two
    launches' bytes for every op, the oracle's numbers within the piece forms' bound"""
    csr = _ragged(gen.banded_random_spd(50000 + 137 * seed, k=14, seed=seed, max_offset=8000, dtype=dtype), seed)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
    b = oracle.spmv(csr, 0, None, x_true)
    one, forms_one = _solve_forms(smm, csr, b, world, dtype, lanes, split=True)
    two, forms_two = _solve_forms(smm, csr, b, world, dtype, lanes, split=False)
    assert all(f[0] > 0 and f[1] == 0 for f in forms_one), forms_one
    assert all(f[0] == 0 and f[1] > 0 for f in forms_two), forms_two
    assert [a == b_ for a, b_ in zip(one[:3], two[:3])] == [True] * 3
    # ... and with the local half's row sums travelling through out[] instead of LDS (the form many rows per workgroup get: few ranks of a big matrix)
    via_out, forms_out = _solve_forms(smm, csr, b, world, dtype, lanes, split=True, sums_lds=0)
    assert all(f[0] > 0 and f[1] == 0 for f in forms_out), forms_out
    assert via_out[:3] == one[:3] and via_out[3:] == one[3:]  # (the same rows in the same workgroups: the solves are the same bytes too)
    y_ref = oracle.spmv(csr, 0, None, b)
    for op, ref in ((0, y_ref), (1, b + y_ref), (2, b - y_ref)):
        y = np.frombuffer(one[op], dtype=dtype)
        assert float(np.max(np.abs(y - ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8, op
    tol = 3e-4 if dtype == np.float32 else 1e-10
    st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 7, 1e-30)
    x = np.frombuffer(one[3], dtype=dtype)
    assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))


@pytest.mark.parametrize("seed", list(range(10, 22)))
def test_one_launch_spmv_fuzz(smm, oracle, seed):
    """random bands with holes, random worlds (2-4), lanes pairings, dtypes and forms of the row sums (LDS / through out[]), among them matrices
    whose entries sit in the rows near one end (the chunked deal of the super tiles) and rows no rank shares: the one-launch SpMV's bytes are
    the two launches' for every op, and the oracle's numbers within the piece forms' bound"""
    rng = np.random.default_rng(seed)
    dtype = (np.float32, np.float64)[seed % 2]
    world = int(rng.integers(2, 5))
    lanes = ((1, 1), (2, 1), (1, 2), (2, 2), (4, 1), (4, 4), (2, 4))[int(rng.integers(0, 7))]
    n = int(rng.integers(30000, 90000))
    csr = _ragged(gen.banded_random_spd(n, k=int(rng.integers(3, 20)), seed=seed, max_offset=int(rng.integers(200, 12000)), dtype=dtype), seed,
                  drop=float(rng.uniform(0.0, 0.6)))
    if seed % 3 == 0:
        # everything beyond the diagonal dropped from the first 60 % of the rows: what is left of the off-diagonal entries sits near the end
        start, pos, val = csr
        rows = np.repeat(np.arange(n), np.diff(start))
        keep = (pos == rows) | (rows >= int(0.6 * n))
        new_start = np.zeros(n + 1, dtype=np.int32)
        np.add.at(new_start, rows[keep] + 1, 1)
        csr = (np.cumsum(new_start).astype(np.int32), pos[keep].copy(), val[keep].copy())
    b = np.random.default_rng(seed + 100).uniform(0.5, 1.5, n).astype(dtype)
    sums = None if seed % 2 else 0
    one, forms_one = _solve_forms(smm, csr, b, world, dtype, lanes, split=True, sums_lds=sums)
    two, forms_two = _solve_forms(smm, csr, b, world, dtype, lanes, split=False)
    # (a rank without a halo has nothing to count; long rows at one lane per row in fp64 do not fit the 64 KB a tile may stage: those pairs of
    # blocks keep the two launches -- by design, and then both runs are the same form)
    nnz_row = (csr[0][-1] / n)
    fits = all(256 // L * nnz_row * 1.25 + 3 <= 65536 // np.dtype(dtype).itemsize for L in lanes)
    if fits:
        assert sum(f[0] for f in forms_one) > 0 and all(f[1] == 0 for f in forms_one), forms_one
    assert all(f[0] == 0 or f[1] == 0 for f in forms_one), forms_one
    assert all(f[0] == 0 for f in forms_two), forms_two
    assert [a == b_ for a, b_ in zip(one[:3], two[:3])] == [True] * 3
    y_ref = oracle.spmv(csr, 0, None, b)
    y = np.frombuffer(one[0], dtype=dtype)
    assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8


@pytest.mark.parametrize("world,dtype,matrix", [(2, np.float64, "band"), (3, np.float32, "band"), (3, np.float64, "grid"), (2, np.float32, "grid"), (2, np.float32, "ragged"),
                                                (4, np.float64, "ragged"), (3, np.float64, "ragged7"), (2, np.float64, "ragged9"), (4, np.float32, "ragged11")])
def test_thin_remote_block(smm, oracle, world, dtype, matrix):
    """csrc/smm_dist_matvec.hip thinRemoteKernel (r06): when at most an eighth of a rank's rows hold a remote entry (a narrow band, the slabs of a
    grid) the second half of the row-partitioned SpMV runs over the listed rows only and the dot products ride in the local launch --
    against the general second launch (SMM_HIP_THIN_REMOTE=0): every SpMV op the same bytes; BiCGStab and CG the same iteration counts, x
    and residual to the solvers' tolerance (the dot products add the same terms in another order); and against the oracle."""
    if matrix == "grid":
        csr = gen.stencil3d(24, 24, 60, dtype=dtype)
    else:
        csr = gen.banded_random_spd(60000, k=10, seed=8, max_offset=1200, dtype=dtype)
        if matrix.startswith("ragged"):
            csr = _ragged(csr, int(matrix[6:] or 5))
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(5).uniform(0.5, 1.5, n).astype(dtype)
    b = oracle.spmv(csr, 0, None, x_true)
    lanes = None if matrix == "grid" else (1, 1)  # (the grid: whatever AUTO and the solvers' adoption choose -- seven entries per row are one lane)
    thin, forms_thin = _solve_forms(smm, csr, b, world, dtype, lanes, split=False, thin=True)
    wide, forms_wide = _solve_forms(smm, csr, b, world, dtype, lanes, split=False, thin=False)
    # rows listed, SpMVs run over them (a rank of the ragged band may hold too many rows with a remote entry: it keeps the general launch)
    assert sum(1 for f in forms_thin if f[2] > 0) >= world - 1 and all((f[2] > 0) == (f[3] > 0) and f[2] * 8 <= n for f in forms_thin), forms_thin
    assert all(f[2] == 0 and f[3] == 0 and f[1] > 0 for f in forms_wide), forms_wide
    assert [a == b_ for a, b_ in zip(thin[:3], wide[:3])] == [True] * 3
    tol = 3e-4 if dtype == np.float32 else 1e-10
    for i in (3, 5, 7):
        xa, xb = np.frombuffer(thin[i], dtype=dtype), np.frombuffer(wide[i], dtype=dtype)
        assert float(np.max(np.abs(xa - xb))) <= tol * float(np.max(np.abs(xb))), i
        ra, rb = np.frombuffer(thin[i + 1], dtype=np.float64), np.frombuffer(wide[i + 1], dtype=np.float64)
        assert tuple(ra[:2]) == tuple(rb[:2]) and abs(ra[2] - rb[2]) <= 50 * tol * max(abs(rb[2]), 1e-30), (ra, rb)
    y, y_ref = np.frombuffer(thin[0], dtype=dtype), oracle.spmv(csr, 0, None, b)  # (a row with both parts is two sums added: not the reference's one chain)
    assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref)))
    st_ref, x_ref, it_ref, _ = oracle.cg(csr, b, np.zeros(n, dtype=dtype), 9, 1e-30)
    x = np.frombuffer(thin[7], dtype=dtype)
    assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))


def test_cg_direction_formed_inside_the_spmv_across_ranks():
    """tests/dist_cg_fuse_check.py in a process of its own: the row-partitioned ConjugateGradient with p = beta p_old + r formed in the load
    phase of the local block's 2.5-D SpMV kernel -- r's halo travels, each rank forms the halo of p itself, the thin
    remote block follows -- against the deferred-x loop and the eager loop, bit for bit, 1 / 2 / 3 slabs, fp32 / fp64, and against the oracle"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "dist_cg_fuse_check.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "dist cg fuse check: ALL OK" in r.stdout and r.stdout.count("fused == deferred == eager") == 10


def test_peer_to_peer_is_refused_between_ranks_of_one_process(smm, oracle, monkeypatch):
    """Ranks that are THREADS of one process asking for the peer-to-peer transport stay with the communicator's collectives (r06): the
    transport makes kernels of one rank wait for kernels of another, and inside one process HIP gives no control over which hardware queue
    a stream's dispatches take -- a kernel trace of the r05 thread-rank test (GPU_MAX_HW_QUEUES=32) shows streams dispatched on more than
    one queue and the side streams of two live ranks on the same one (profiles/r06/p2p_thread_rank_queues.txt): the cause of the bounded
    waits that expired now and then in r05 (there the test skipped) and r06.  Every rank sees every rank's process id at set-up, so all
    vote alike.  The transport itself is tested where it is deployed: between processes (below)."""
    monkeypatch.setenv("SMM_HIP_P2P", "1")
    monkeypatch.setenv("SMM_HIP_P2P_RELAYS", "1")
    dtype = np.float32
    csr = gen.banded_random_spd(60000, k=12, seed=4, max_offset=9000, dtype=dtype)
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
    b = oracle.spmv(csr, 0, None, x_true)
    seen = {}
    (status, iters, res), x, y, halo = _solve(smm, csr, b, 3, dtype, 7, 1e-30, options_seen=seen, own_streams=True)
    assert len(seen) == 3 and all(o["p2p"] is False and o["relays"] == 0 for o in seen.values()), seen
    st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 7, 1e-30)
    assert status == st_ref and iters == it_ref == 7 and halo > 0
    assert float(np.max(np.abs(x - x_ref))) <= 3e-4 * float(np.max(np.abs(x_ref)))


def _run_worker_processes(world, matrix, dtype, env_extra, extra_args=()):
    """tests/p2p_proc_worker.py as `world` processes sharing the GPU (gloo for the set-up collectives); returns rank 0's report"""
    import socket

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "p2p_proc_worker.py"), matrix, np.dtype(dtype).name, *extra_args], cwd=root, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:  # (exactly the processes started here)
            if p.poll() is None:
                p.kill()
    for rank, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank}: " + se[-3000:]
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("P2P_WORKER ")]
    assert len(lines) == 1, outs[0][0][-2000:] + outs[0][1][-2000:]
    return json.loads(lines[0][len("P2P_WORKER "):])


def _check_worker_report(oracle, smm, rep, dtype):
    """the assembled results of the worker processes against the single-process oracle"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import p2p_proc_worker as w

    csr, bounds = w.build_matrix(rep["kind"], dtype, rep["world"])
    assert [int(v) for v in bounds] == rep["bounds"]
    n = len(csr[0]) - 1
    x_true = np.random.default_rng(3).uniform(0.5, 1.5, n).astype(dtype)
    import scipy.sparse as sp

    b = (sp.csr_matrix((csr[2].astype(np.float64), csr[1], csr[0]), shape=(n, n)) @ x_true.astype(np.float64)).astype(dtype)
    tol = 3e-4 if dtype == np.float32 else 1e-10
    if rep["kind"] == "grid" and dtype == np.float32:
        tol = 5e-3  # (the oracle adds 456 192 fp32 products one after the other: any blocked sum sits this far from it -- tests/dist_cg_fuse_check.py)
    y = np.frombuffer(bytes.fromhex(rep["results"]["y"]), dtype=dtype)
    y_ref = oracle.spmv(csr, 0, None, b)
    assert float(np.max(np.abs(y - y_ref))) <= 64 * np.finfo(dtype).eps * float(np.max(np.abs(y_ref))) * 8
    _, diag = oracle.jacobi_setup(csr)
    from oracle.oracle import PRECOND_JACOBI

    for name, ref in (("bicgstab7", lambda: oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 7, 1e-30)),
                      ("cg9", lambda: oracle.cg(csr, b, np.zeros(n, dtype=dtype), 9, 1e-30))):
        st_ref, x_ref, it_ref, _ = ref()
        got = rep["results"][name]
        x = np.frombuffer(bytes.fromhex(got["x"]), dtype=dtype)
        assert got["res"][0] == st_ref and got["res"][1] == it_ref, (name, got["res"], st_ref, it_ref)
        assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref))), name
    # Jacobi by rank IS the global Jacobi (a diagonal): the oracle's preconditioned template with the matrix's diagonal
    st_ref, x_ref, it_ref, _ = oracle.bicgstab(csr, b, np.zeros(n, dtype=dtype), 7, 1e-30, PRECOND_JACOBI, diag)
    got = rep["results"]["jacobi7"]
    x = np.frombuffer(bytes.fromhex(got["x"]), dtype=dtype)
    assert got["res"][0] == st_ref and got["res"][1] == it_ref
    assert float(np.max(np.abs(x - x_ref))) <= tol * float(np.max(np.abs(x_ref)))
    got = rep["results"]["bicgstab40"]
    x = np.frombuffer(bytes.fromhex(got["x"]), dtype=dtype)
    assert got["res"][0] == 0
    if rep["kind"] != "grid":  # (the grid's Laplacian is nowhere near converged after 40 iterations: the bands are diagonally dominant)
        np.testing.assert_allclose(x, x_true, rtol=2e-3 if dtype == np.float32 else 1e-4)


@pytest.mark.parametrize("world,relays,dtype", [(3, 1, np.float64), (4, 2, np.float32), (4, 1, np.float64)])
def test_peer_to_peer_relay_only_rank(smm, oracle, world, relays, dtype):
    """A rank WITHOUT a halo of its own in a world with relays (ADVICE r05 / VERDICT r05 item 2): the last rank's rows are a decoupled
    diagonal block -- it neither sends nor receives, yet planRelays picks it (ring distance alone) to relay the others' shares.  r05's
    distExchangeBegin returned early for such a rank: its forwards never ran and every solve expired.  Between processes (real IPC
    handles), stand-alone SpMVs back to back, BiCGStab with / without Jacobi, CG -- against the single-process oracle."""
    rep = _run_worker_processes(world, "decoupled", dtype, {"SMM_HIP_P2P": "1", "SMM_HIP_P2P_RELAYS": str(relays), "SMM_HIP_P2P_TIMEOUT_S": "20"})
    for rank, o in enumerate(rep["options"]):
        assert o["p2p"] is True and o["relays"] == relays, rep["options"]
        assert (o["halo_elements"] == 0) == (rank == world - 1), rep["options"]  # the last rank has no halo at all
    _check_worker_report(oracle, smm, rep, dtype)


@pytest.mark.parametrize("world,relays,dtype,transport", [(2, 0, np.float64, "p2p"), (3, 1, np.float32, "p2p"), (3, 0, np.float64, "hybrid")])
def test_slabs_of_a_grid_between_processes(smm, oracle, world, relays, dtype, transport):
    """BASELINE config 4's shape between PROCESSES: a 3-D grid cut into slabs of whole planes.  Every rank's local block runs on the 2.5-D
    constant-diagonal kernel, its remote block is THIN (the launch over the listed rows), and ConjugateGradient forms its next direction
    inside the SpMV -- the halo of r arrives through the peer-to-peer transport's push / land kernels (or the communicator's send / receive:
    the hybrid) and each rank forms the halo of p itself.  SpMV, BiCGStab with / without Jacobi, CG against the single-process oracle."""
    env = {"SMM_HIP_P2P_RELAYS": str(relays), "SMM_HIP_P2P_TIMEOUT_S": "20", "SMM_HIP_NT_OUT": "1", "SMM_HIP_MARCH_MIN_ROWS": "1"}
    if transport == "hybrid":
        env["SMM_HIP_P2P_HALO"] = "0"
    rep = _run_worker_processes(world, "grid", dtype, env)
    for o in rep["options"]:
        assert o["p2p_scalars"] is True and o["p2p"] is (transport == "p2p"), rep["options"]
        assert o["thin_remote"][0] > 0 and o["thin_remote"][1] > 0, rep["options"]  # rows listed; SpMVs ran over them
        assert o["cg_fused"] >= 8, rep["options"]                                    # CG's 9 iterations: every SpMV but the first formed p
    _check_worker_report(oracle, smm, rep, dtype)


@pytest.mark.parametrize("ranks,relays", [(2, 0), (3, 1), (4, 2)])
def test_peer_to_peer_between_processes(ranks, relays):
    """The same between PROCESSES: `python bench.py --gpus N` with the gloo rehearsal communicator and SMM_HIP_P2P=1 -- the ranks share the one
    GPU, every rank exports its block with hipIpcGetMemHandle and maps the others' with hipIpcOpenMemHandle (what ranks on separate GPUs do
    over xGMI), halos and scalars travel peer to peer; the line reports which options ran."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMM_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", SMM_HIP_P2P="1", SMM_HIP_P2P_RELAYS=str(relays), SMM_HIP_P2P_TIMEOUT_S="30")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--rows", "600000", "--max-offset", "65536", "--steps", "20",
           "--warmup", "10", "--iters-per-solve", "10", "--cpu-seconds", "0"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["dist_options"] == {"p2p": True, "p2p_scalars": True, "relays": relays, "halo_first": True, "direct_share": 4.0 / (relays + 4) if relays else 1.0}, line["dist_options"]
    assert line["n_gpus"] == ranks and line["value"] > 0 and line["max_rel_err_vs_x_true"] < 1e-3
    if ranks == 2:
        # two ranks: a + b in either order is the same sum, so the collectives' result must come out bit for bit (pure data movement)
        env2 = dict(env, SMM_HIP_P2P="0")
        out2 = subprocess.run(cmd, cwd=root, env=env2, capture_output=True, text=True, timeout=900)
        assert out2.returncode == 0, out2.stderr[-3000:]
        line2 = json.loads([ln for ln in out2.stdout.splitlines() if ln.startswith("{")][0])
        assert line2["dist_options"]["p2p"] is False
        assert line2["resnorm"] == line["resnorm"] and line2["max_rel_err_vs_x_true"] == line["max_rel_err_vs_x_true"], (line2["resnorm"], line["resnorm"])


@pytest.mark.parametrize("ranks", [2, 4])
def test_bench_self_launch_rehearsal(ranks):
    """`python bench.py --gpus N` exactly as the driver types it (no torch.distributed.run in front): bench.py starts its own N rank
    processes.  Here the ranks share the one GPU and SMM_BENCH_BACKEND=gloo carries the communicator's bytes through the host, so
    this checks function, not speed: per-rank generation, the device-side A_loc / A_rem split, the native loop with real
    inter-process exchanges and all-reduces, the max-over-ranks timing and the single JSON line of rank 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMM_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--rows", "600000", "--max-offset", "65536", "--steps", "20",
           "--warmup", "10", "--iters-per-solve", "10", "--cpu-seconds", "2", "--full"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == ranks and line["steps"] == 20 and line["scaling"] == "strong"
    assert line["unit"] == "iterations/s" and line["value"] > 0
    assert line["rehearsal_backend"] == "gloo"
    assert line["distributed"] == {"driver": "native", "comm": "host", "comm_ranks": ranks, "kernels_per_iteration": 8,
                                   "allreduces_per_iteration": 3, "halo_exchanges_per_iteration": 2}
    assert line["per_rank"]["halo_elements"] > 0
    assert line["max_rel_err_vs_x_true"] < 1e-3
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1
    # the N > 1 line carries the same objects as the one-GPU line: the per-rank roofline (A_loc + A_rem bytes over
    # their launch time), the CPU baseline of the WORKLOAD (rank 0 times it on the whole matrix) and the communicator's size as RCCL
    # reports it (0 here: the rehearsal's communicator is host callbacks over gloo, not RCCL)
    assert line["roofline"]["algorithmic_bytes_per_launch"] > 0 and line["roofline"]["avg_launch_ms"] > 0 and line["roofline"]["launches"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1 and line["cpu_baseline"]["kind"] in ("port", "reference")
    assert line["rccl_ranks"] == 0
    # `value` comes from a pass without timing events; the SpMV launch times and the exposed waits from a second pass of the same K
    # iterations behind it (r05: the events perturb the row-partitioned loop) -- the line says so and what the instrumented pass cost
    assert line["ms_per_step_instrumented"] > 0 and "second pass" in line["roofline"]["measured_in"]
    assert 40 <= line["roofline"]["launches"] <= 44  # (matvecs of the instrumented pass: two per iteration + one set-up matvec per solve of 10)
    # what a multi-GPU line that scales worse than hoped is read by first: the exchanges' share that A_loc did not cover (events on the
    # solver's and the communicator's stream; the rehearsal's host-staged exchanges run on the solver's own stream: no pairs, 0 ms)
    assert line["exposed_comm_ms"] >= 0 and line["exposed_comm"]["exchanges"] >= 0 and line["halo_chunks"] == 1
    # r06: between processes the peer-to-peer transport is the default (taken because every rank passed its create-time self-test; 2 and 4 ranks:
    # world - 4 <= 0 relays); SMM_HIP_P2P=0 would keep the collectives
    assert line["dist_options"] == {"p2p": True, "p2p_scalars": True, "relays": 0, "halo_first": True, "direct_share": 1.0}, line["dist_options"]
    assert "spmvTileKernel" in line["roofline"]["kernel"] or "spmvStreamKernel" in line["roofline"]["kernel"] or "Pattern" in line["roofline"]["kernel"]


@pytest.mark.parametrize("world,relays,dtype", [(2, 0, np.float32), (3, 1, np.float64)])
def test_one_launch_spmv_between_processes(smm, oracle, world, relays, dtype):
    """The one-launch SpMV behind the peer-to-peer transport between PROCESSES: the word a rank's SpMV kernel polls is raised behind ITS land
    kernel, which waits for pushes of other processes -- the kernel sits on the GPU with its local half done while they arrive.  Both local
    blocks forced to the row-mask encoding; SpMVs back to back, BiCGStab +- Jacobi, CG; against the oracle."""
    # (SMM_HIP_SPLIT_SPMV=2: ranks that share a GPU normally keep the two launches -- on a card that two full-size grids fill, the copy kernels the
    # grids wait for find no room; these matrices leave it half empty)
    rep = _run_worker_processes(world, "banded", dtype, {"SMM_HIP_P2P": "1", "SMM_HIP_P2P_RELAYS": str(relays), "SMM_HIP_P2P_TIMEOUT_S": "20", "SMM_HIP_SPLIT_SPMV": "2"},
                                extra_args=("pattern",))
    for o in rep["options"]:
        assert o["p2p"] is True and o["matvec_forms"][0] > 0 and o["matvec_forms"][1] == 0, rep["options"]
    _check_worker_report(oracle, smm, rep, dtype)


@pytest.mark.parametrize("world,relays,dtype", [(2, 0, np.float64), (3, 1, np.float32)])
def test_peer_to_peer_equals_the_collectives_between_processes(smm, oracle, world, relays, dtype):
    """Pure data movement and sums in a fixed order: the same row-partitioned SpMVs and solves through the peer-to-peer transport and through
    the communicator's collectives, between processes (real IPC handles).  Two ranks: a + b in either order is the same sum, so EVERY result
    is the same bytes.  Three ranks with a relay: the SpMV (no sum crosses ranks) is the same bytes, the solves agree to the solvers'
    tolerance (gloo's all-reduce adds in its own order, the slot reduction in rank order) -- and both match the oracle."""
    on = _run_worker_processes(world, "banded", dtype, {"SMM_HIP_P2P": "1", "SMM_HIP_P2P_RELAYS": str(relays), "SMM_HIP_P2P_TIMEOUT_S": "20"})
    off = _run_worker_processes(world, "banded", dtype, {"SMM_HIP_P2P": "0"})
    assert all(o["p2p"] is True and o["p2p_scalars"] is True and o["relays"] == relays for o in on["options"])
    assert not any(o["p2p"] or o["p2p_scalars"] for o in off["options"])
    assert on["results"]["y"] == off["results"]["y"]
    tol = 3e-4 if dtype == np.float32 else 1e-10
    for name in ("bicgstab7", "jacobi7", "cg9"):
        a, b_ = on["results"][name], off["results"][name]
        assert a["res"][:2] == b_["res"][:2]
        if world == 2:
            assert a == b_, name
        else:
            xa, xb = (np.frombuffer(bytes.fromhex(r["x"]), dtype=dtype) for r in (a, b_))
            assert float(np.max(np.abs(xa - xb))) <= tol * float(np.max(np.abs(xb))), name
    _check_worker_report(oracle, smm, on, dtype)


def test_hybrid_transport_between_processes(smm, oracle):
    """The hybrid (r06): the halo through the communicator's grouped send / receive, the scalars through the per-rank slots -- what every rank
    falls back to when the halo part of the create-time self-test fails somewhere (here: SMM_HIP_P2P_HALO=0 makes every rank vote so).
    Three processes, the default transport otherwise; against the oracle."""
    dtype = np.float64
    rep = _run_worker_processes(3, "banded", dtype, {"SMM_HIP_P2P_HALO": "0", "SMM_HIP_P2P_TIMEOUT_S": "20"})
    for o in rep["options"]:
        assert o["p2p"] is False and o["p2p_scalars"] is True and o["relays"] == 0, rep["options"]
    _check_worker_report(oracle, smm, rep, dtype)


def test_ranks_that_share_a_gpu_keep_the_two_launch_spmv(smm, oracle):
    """r06: the one-launch SpMV waits inside a grid that fills the chip but for a few workgroup slots; ranks of a rehearsal that share ONE card
    would take each other's spare slots and starve the copy kernels both are waiting for (seen with 2 x 2.5 M rows: both ranks' bounded waits
    expired).  The peer-to-peer set-up sees every rank's GPU and keeps the two launches when two ranks share one -- the transport itself stays."""
    dtype = np.float64
    rep = _run_worker_processes(2, "banded", dtype, {"SMM_HIP_P2P_TIMEOUT_S": "20"}, extra_args=("pattern",))
    for o in rep["options"]:
        assert o["p2p"] is True and o["matvec_forms"][0] == 0 and o["matvec_forms"][1] > 0, rep["options"]
    _check_worker_report(oracle, smm, rep, dtype)
