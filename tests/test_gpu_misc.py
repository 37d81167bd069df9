"""Smaller GPU checks: autotune keeps results right, set-up paths are ordered behind work the caller still has in flight on
its own stream, the fused-dot SpMV entry point, thread safety of independent solves."""
import ctypes
import threading

import numpy as np
import pytest

from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu


def test_autotune_and_kernel_selection(smm, oracle):
    csr = gen.banded_random_spd(40000, k=20, seed=9, max_offset=5000, dtype=np.float32)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    assert A.get_kernel()[0] == smm.SPMV_STREAM
    x = np.random.default_rng(0).uniform(-1, 1, n).astype(np.float32)
    ref = oracle.spmv(csr, 0, None, x)
    fam, lanes = A.autotune()
    assert fam in (smm.SPMV_VECTOR, smm.SPMV_STREAM) and lanes in (1, 2, 4, 8, 16, 32, 64)
    y = np.zeros(n, dtype=np.float32)
    A.rMult(x, y)
    np.testing.assert_allclose(y, ref, rtol=2e-5, atol=2e-5)
    A.set_kernel(smm.SPMV_AUTO, 0)
    assert A.get_kernel()[0] == smm.SPMV_STREAM


def test_setup_is_ordered_behind_the_callers_stream(smm):
    """the matrix is generated on torch's stream and handed over without a synchronise: csr_create_dev, the tile build and the
    preconditioner analysis must still see the finished arrays"""
    import torch

    from sparse_matrix_math_amd import host

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    N = 96
    n, nnz = N ** 3, host.gen_stencil3d_nnz(N, N, N)
    for _ in range(3):
        ds = torch.empty(n + 1, dtype=torch.int32, device=dev)
        dp = torch.empty(nnz, dtype=torch.int32, device=dev)
        dv = torch.empty(nnz, dtype=torch.float64, device=dev)
        big = torch.rand(64_000_000, device=dev)
        for _ in range(4):
            big = big * 1.0001 + 0.5  # keeps the stream busy ahead of the generator
        host.gen_stencil3d_dev(N, N, N, 6.0, -1.3, -0.7, ds, dp, dv, np.float64, stream)
        A = smm.CSRMatrix.from_device(n, n, ds, dp, dv, np.float64)
        assert A.nnz == nnz and A.first_active_start == 0
        M = A.getPreconditioner(smm.SolverPreconditioner.ILU0)
        assert M.levels() == (3 * N - 2, 3 * N - 2)
        ones = torch.ones(n, dtype=torch.float64, device=dev)
        y = torch.empty_like(ones)
        A.spmv_dev(0, None, ones, y, stream)
        torch.cuda.synchronize()
        assert abs(float(y.sum()) - (0.7 + 1.3) * 0.0 - float(y.sum())) == 0.0
        interior = y.view(N, N, N)[1:-1, 1:-1, 1:-1]
        assert float(interior.abs().max()) < 1e-12  # 6 - 3*1.3 - 3*0.7 == 0 in the interior


def test_auto_analysis_is_ordered_behind_the_callers_stream(smm):
    """the FIRST SpMV of an AUTO matrix of >= 2^25 entries runs the PATTERN analysis (sampling, mask build,
    verification of every entry, tile table) inside an asynchronous `_dev` entry point.  The handle is created through the raw C ABI
    (no query that would drain the device) while the generator of the arrays is still queued behind busy work on the caller's stream:
    everything the analysis reads must be ordered behind it.  Checked against a second, fully synchronised handle, bit for bit."""
    import torch

    from sparse_matrix_math_amd import _lib, host

    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, k, seed, max_off = 700_000, 25, 0x5EED, 1 << 16
    nnz = host.gen_banded_nnz(n, k, seed, max_off)
    assert nnz >= 1 << 25
    x = torch.rand(n, dtype=torch.float32, device=dev) - 0.5
    for _ in range(2):
        ds = torch.empty(n + 1, dtype=torch.int32, device=dev)
        dp = torch.empty(nnz, dtype=torch.int32, device=dev)
        dv = torch.empty(nnz, dtype=torch.float32, device=dev)
        y = torch.empty(n, dtype=torch.float32, device=dev)
        big = torch.rand(64_000_000, device=dev)
        for _ in range(4):
            big = big * 1.0001 + 0.5  # keeps the stream busy ahead of the generator
        host.gen_banded_dev(n, k, seed, max_off, ds, dp, dv, np.float32, stream)
        h = ctypes.c_void_p()
        _lib.check(lib.smm_hip_csr_create_dev_f32(n, n, host._dptr(ds), host._dptr(dp), host._dptr(dv), ctypes.byref(h)))
        _lib.check(lib.smm_hip_spmv_dev_f32(h, 0, None, host._dptr(x), host._dptr(y), host._dptr(stream)))  # AUTO: analysis + first launch
        torch.cuda.synchronize()
        fam, lanes = ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.smm_hip_csr_get_kernel(h, ctypes.byref(fam), ctypes.byref(lanes)))
        assert (fam.value, lanes.value) == (3, 2)  # PATTERN: the analysis saw the finished arrays and every entry verified
        B = smm.CSRMatrix.from_device(n, n, ds, dp, dv, np.float32)  # (drains the device)
        B.set_kernel(2, 2)  # STREAM at the same lanes: the same bits
        y2 = torch.empty_like(y)
        B.spmv_dev(0, None, x, y2, stream)
        torch.cuda.synchronize()
        body = (ds[1:] <= nnz - 8200).cpu().numpy()  # (the directly streamed last tiles differ in how a row is cut into lanes)
        assert body.sum() > n - 400
        np.testing.assert_array_equal(y.cpu().numpy()[body], y2.cpu().numpy()[body])
        np.testing.assert_allclose(y.cpu().numpy(), y2.cpu().numpy(), rtol=2e-5, atol=2e-5)
        B.close()
        _lib.check(lib.smm_hip_csr_destroy(h))
        del big


def test_automatic_pattern_attempt_never_fails_the_callers_work(smm, oracle):
    """the switch to the PATTERN family is an optional optimisation -- when its analysis cannot get its memory (8 bytes
    per row of masks, scratch of the sort ...) the caller's SpMV / solve must run on STREAM as if nothing had been tried, automatic
    attempts must not try again, and an explicit request later must (and succeed).  The allocation failure is injected
    (smm_hip_debug_fail_next_alloc)."""
    import torch

    from sparse_matrix_math_amd import _lib, host

    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    # (a) the first SpMV of a matrix of >= 2^25 entries
    n, k, seed, max_off = 700_000, 25, 0x5EED, 1 << 16
    nnz = host.gen_banded_nnz(n, k, seed, max_off)
    ds = torch.empty(n + 1, dtype=torch.int32, device=dev)
    dp = torch.empty(nnz, dtype=torch.int32, device=dev)
    dv = torch.empty(nnz, dtype=torch.float32, device=dev)
    host.gen_banded_dev(n, k, seed, max_off, ds, dp, dv, np.float32, stream)
    A = smm.CSRMatrix.from_device(n, n, ds, dp, dv, np.float32)
    x = torch.rand(n, dtype=torch.float32, device=dev) - 0.5
    y = torch.empty_like(x)
    _lib.check(lib.smm_hip_debug_fail_next_alloc(n * 8))  # the masks: 8 bytes per row
    A.spmv_dev(0, None, x, y, stream)  # must not raise
    torch.cuda.synchronize()
    assert A.get_kernel()[0] == 2 and A.pattern_info()[0] == 0  # stayed on STREAM
    y2 = torch.empty_like(x)
    A.spmv_dev(0, None, x, y2, stream)  # no second automatic attempt
    torch.cuda.synchronize()
    assert A.get_kernel()[0] == 2 and torch.equal(y, y2)
    A.set_kernel(3, 0)  # an explicit request tries again -- and the memory is there now
    assert A.get_kernel() == (3, 2) and A.pattern_info()[0] == 1
    A.spmv_dev(0, None, x, y2, stream)
    torch.cuda.synchronize()
    np.testing.assert_allclose(y2.cpu().numpy(), y.cpu().numpy(), rtol=2e-5, atol=2e-5)
    A.close()
    _lib.check(lib.smm_hip_debug_fail_next_alloc(0))
    # (b) a solver's own attempt (>= 2^20 entries): the solve runs on STREAM and gives the oracle's x
    csr = gen.convdiff3d(64, 0.3, dtype=np.float64)
    m = len(csr[0]) - 1
    b = gen.row_sums(csr[0], csr[2])
    B = smm.CSRMatrix(m, m, *csr)
    db = torch.from_numpy(b).to(dev)
    dx = torch.zeros(m, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    # (the device entry point: the analysis is the solve's FIRST allocation of that size -- the masks; its own vectors come after)
    _lib.check(lib.smm_hip_debug_fail_next_alloc(m * 8))
    status, iters, _res = host.bicgstab_dev(B, db, dx, 20, 0.0, None, stream)  # must not raise
    torch.cuda.synchronize()
    assert B.get_kernel()[0] == 2 and iters == 20
    x_ref = oracle.bicgstab(csr, b, np.zeros(m), 20, 0.0)[1]
    np.testing.assert_allclose(dx.cpu().numpy(), x_ref, rtol=0, atol=1e-7 * float(np.abs(x_ref).max()))
    B.close()
    _lib.check(lib.smm_hip_debug_fail_next_alloc(0))


def test_fused_dot_entry_point(smm, oracle):
    import torch

    from sparse_matrix_math_amd import _lib, host

    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lib.smm_hip_partials_count()
    for dtype, suf, td in ((np.float32, "f32", torch.float32), (np.float64, "f64", torch.float64)):
        csr = gen.banded_random_spd(30000, k=15, seed=2, max_offset=4000, dtype=dtype)
        n = len(csr[0]) - 1
        A = smm.CSRMatrix(n, n, *csr)
        rng = np.random.default_rng(1)
        x, w, lhs = (rng.uniform(-1, 1, n).astype(dtype) for _ in range(3))
        dx, dw, dl = (torch.from_numpy(a).to(dev) for a in (x, w, lhs))
        out = torch.empty(n, dtype=td, device=dev)
        parts = torch.full((2 * P,), 123.0, dtype=td, device=dev)
        fn = getattr(lib, f"smm_hip_spmv_fused_dev_{suf}")
        d = host._dptr
        for family, lanes in ((2, 0), (2, 1), (1, 8)):
            A.set_kernel(family, lanes)
            _lib.check(fn(A._h, 2, d(dl), d(dx), d(out), 2, d(dw), d(parts), stream))  # out = lhs - A x; out.out and out.w
            torch.cuda.synchronize()
            o = out.cpu().numpy().astype(np.float64)
            ref = oracle.spmv(csr, 2, lhs, x).astype(np.float64)
            np.testing.assert_allclose(o, ref, rtol=1e-4 if dtype == np.float32 else 1e-12, atol=1e-5 if dtype == np.float32 else 1e-13)
            p = parts.cpu().numpy().astype(np.float64)
            tol = 1e-4 if dtype == np.float32 else 1e-11
            assert abs(p[:P].sum() - np.dot(o, o)) <= tol * np.dot(o, o)
            assert abs(p[P:].sum() - np.dot(o, w)) <= tol * np.abs(o * w).sum()


def test_concurrent_host_api_solves(smm, oracle):
    """the reference's solvers are re-entrant on a const matrix: four threads solve on the same matrix, each with
    a right-hand side of its own (a vector shared by mistake then holds foreign data), and get the bits of the same solve made alone
    (tests/test_gpu_concurrent.py has the other solvers, the preconditioners and the overlap condition)"""
    csr = gen.poisson2d(40, dtype=np.float64)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    bs = [gen.row_sums(csr[0], csr[2]) + np.random.default_rng(i).uniform(-1, 1, n) for i in range(4)]
    x_refs = [oracle.cg(csr, b, np.zeros(n), -1, 1e-10)[1] for b in bs]

    def solve(i):
        x = np.zeros(n)
        st = smm.ConjugateGradient(A, bs[i], x, x, -1, 1e-10) if i % 2 == 0 else smm.BiCGStab(A, bs[i].copy(), x, -1, 1e-10)
        return int(st), x

    alone = [solve(i) for i in range(4)]
    results, errors = [None] * 4, []
    gate = threading.Barrier(4)

    def work(i):
        try:
            gate.wait()
            results[i] = solve(i)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for (st, x), x_ref, (st_alone, x_alone) in zip(results, x_refs, alone):
        assert st == 0 == st_alone
        np.testing.assert_allclose(x, x_ref, rtol=1e-7, atol=1e-9)
        np.testing.assert_array_equal(x.view(np.uint64), x_alone.view(np.uint64))


@pytest.mark.parametrize("kind", ["convdiff64_auto_adopts", "iid_auto_refuses"])
def test_concurrent_solves_while_auto_switches_the_kernel_family(smm, oracle, kind):
    """concurrent solves on one const matrix are safe (ref:2316-2324 take `const CSRMatrix<T>&`).  Above 2^20 stored
    entries the FIRST solve of an AUTO matrix runs the PATTERN analysis and switches the kernel family from inside the solve: four
    threads start their solves on a fresh matrix together -- one analyses (adoptMutex), the others wait and read the published
    family | lanes word -- and every one of them must get the oracle's answer.  Repeated for a matrix whose analysis says no (i.i.d.
    columns), which must stay on STREAM, quietly."""
    if kind == "convdiff64_auto_adopts":
        csr = gen.convdiff3d(64, 0.3, dtype=np.float64)  # 262 144 rows, 1.8 M entries
    else:
        rng = np.random.default_rng(3)
        n, width = 120_000, 9  # 1.08 M entries, i.i.d. columns + a dominant diagonal: no pattern
        cols = np.sort(rng.integers(0, n, (n, width - 1)), axis=1)
        rows_idx = np.arange(n)[:, None]
        cols = np.where(cols == rows_idx, (cols + 1) % n, cols)
        allc = np.sort(np.concatenate([cols, rows_idx], axis=1), axis=1)
        keep = np.ones_like(allc, dtype=bool)
        keep[:, 1:] = allc[:, 1:] != allc[:, :-1]
        lens = keep.sum(axis=1)
        start = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        pos = allc[keep].astype(np.int32)
        vals = rng.uniform(-1, 1, len(pos))
        rr = np.repeat(np.arange(n), lens)
        vals[pos == rr] = 6.0
        csr = (start, pos, vals)
    n = len(csr[0]) - 1
    assert csr[0][-1] >= 1 << 20
    b = gen.row_sums(csr[0], csr[2])
    x_ref_b = oracle.bicgstab(csr, b, np.zeros(n), 20, 0.0)[1]  # (the solvers adopt the family when >= 16 iterations are allowed)
    for attempt in range(3):  # a fresh handle each time: the switch happens once per matrix
        A = smm.CSRMatrix(n, n, *csr)
        results, errors = [None] * 4, []
        gate = threading.Barrier(4)

        def work(i):
            try:
                x = np.zeros(n)
                info = {}
                gate.wait()
                st = smm.BiCGStab(A, b.copy(), x, 20, 0.0, info=info)
                results[i] = (int(st), info["iterations"], x)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        fam, lanes = A.get_kernel()
        if kind == "convdiff64_auto_adopts":
            assert (fam, lanes) == (3, 1) and A.pattern_info()[0] == 3  # PATTERN, one lane per row, constant diagonals
        else:
            assert fam == 2 and A.pattern_info()[0] == 0  # refused quietly: STREAM
        for st, it, x in results:
            assert it == 20
            np.testing.assert_allclose(x, x_ref_b, rtol=0, atol=1e-7 * float(np.abs(x_ref_b).max()))
        A.close()


def test_handle_destroyed_behind_an_async_launch_does_not_corrupt_it(smm, oracle):
    """`_dev` entry points only enqueue, and destroy / __del__ hand buffers back to the caching allocator.  A block must not
    be reused while a queued kernel still reads it: the matrix (library-owned copy of the arrays) is destroyed right behind an SpMV
    that is still waiting in the stream, and a second matrix of the same size -- different values -- is created at once."""
    import torch

    from sparse_matrix_math_amd import host

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    csr1 = gen.banded_random_spd(300000, k=8, seed=1, max_offset=4000, dtype=np.float32)
    csr2 = (csr1[0], csr1[1], (csr1[2] * np.float32(-3.0)).astype(np.float32))
    n = len(csr1[0]) - 1
    x = np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32)
    want = oracle.spmv(csr1, 0, None, x)
    dx = torch.from_numpy(x).to(dev)
    for _ in range(3):
        y = torch.zeros(n, dtype=torch.float32, device=dev)
        A = smm.CSRMatrix(n, n, *csr1)  # host arrays: the library owns the device copy
        A.spmv_dev(0, None, dx, y, stream)  # builds the tile table, so that the next launches only enqueue
        torch.cuda.synchronize()
        big = torch.rand(96_000_000, device=dev)
        for _ in range(6):
            big = big * 1.0001 + 0.5  # ~100 ms of queued work ahead of the SpMV
        y.zero_()
        A.spmv_dev(0, None, dx, y, stream)
        A.close()  # frees values / positions / start / tiles while the SpMV above is still queued
        B = smm.CSRMatrix(n, n, *csr2)  # same sizes: the allocator would hand the same blocks out again
        torch.cuda.synchronize()
        np.testing.assert_allclose(y.cpu().numpy(), want, rtol=2e-5, atol=2e-5)
        y2 = torch.zeros(n, dtype=torch.float32, device=dev)
        B.spmv_dev(0, None, dx, y2, stream)
        torch.cuda.synchronize()
        np.testing.assert_allclose(y2.cpu().numpy(), -3.0 * want, rtol=2e-5, atol=6e-5)
        B.close()
        del big


def test_dot_on_two_streams_at_once(smm):
    """smm_hip_dot_dev keeps one partial-sum buffer per stream, so dots enqueued on different streams do not race"""
    import torch

    from sparse_matrix_math_amd import host

    dev = torch.device("cuda:0")
    n = 6_000_000
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    vecs = [torch.full((n,), float(k + 1), dtype=torch.float64, device=dev) for k in range(3)]
    outs = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    for rep in range(20):
        for k, st in enumerate(streams):
            host.dot_dev(n, vecs[k], vecs[k], outs[k], np.float64, st.cuda_stream)
    torch.cuda.synchronize()
    for k in range(3):
        assert float(outs[k]) == float(n) * (k + 1) ** 2


def test_sweeps_with_long_dependent_rows(smm, oracle):
    """a dense lower-triangular block makes every row depend on all earlier ones with hundreds of entries per row -- the
    case where waiting wavefronts poll far more often than the working one advances.  The sweeps must finish (escape bound scaled by
    the longest row, smm_hip_precond_take_error clean) and stay bit-identical to the sequential sweeps."""
    import torch

    P = smm.SolverPreconditioner
    rng = np.random.default_rng(11)
    nb, n = 700, 1500
    dense = np.zeros((n, n))
    blk = rng.uniform(-0.5, 0.5, (nb, nb)) / nb
    dense[:nb, :nb] = blk + blk.T  # symmetric dense block: lower AND upper sweeps are fully sequential over 700 rows
    for i in range(n):
        dense[i, i] = 4.0
        if i + 1 < n:
            dense[i, i + 1] = dense[i + 1, i] = -1.0
    start = np.zeros(n + 1, dtype=np.int32)
    pos, val = [], []
    for r in range(n):
        (c,) = np.nonzero(dense[r])
        pos.extend(c.tolist())
        val.extend(dense[r, c].tolist())
        start[r + 1] = len(pos)
    csr = (start, np.array(pos, dtype=np.int32), np.array(val, dtype=np.float64))
    A = smm.CSRMatrix(n, n, *csr)
    rhs = rng.uniform(-1, 1, n)
    dev = torch.device("cuda:0")
    for kind in (P.SYMMETRIC_GAUS_SEIDEL, P.ILU0):
        M = A.getPreconditioner(kind)
        assert max(M.levels()) >= nb
        if kind == P.ILU0:
            _, lu = oracle.ilu0_factorize(csr)
            err, want = oracle.ilu0_apply(csr, lu, rhs)
        else:
            err, want = oracle.sgs_apply(csr, rhs)
        assert err == 0
        x = np.zeros(n)
        assert M.apply(rhs, x) == 0
        np.testing.assert_array_equal(x, want)
        d_rhs, d_x = torch.from_numpy(rhs).to(dev), torch.zeros(n, dtype=torch.float64, device=dev)
        M.apply_dev(d_rhs, d_x, torch.cuda.current_stream().cuda_stream)
        M.take_error(torch.cuda.current_stream().cuda_stream)  # raises if a sweep tripped its bound
        np.testing.assert_array_equal(d_x.cpu().numpy(), want)


def test_an_allocation_never_waits_for_queued_work(smm):
    """csrc/smm_runtime.hip, r06: a freed block is reusable once the work queued before the free has ended (event epochs) -- and an allocation
    that finds its size still quarantined takes FRESH memory instead of waiting for those events.  r03-r05 polled them: with ranks as
    threads of one process and the peer-to-peer transport, a rank entering a solve waited in the allocator for an event recorded behind a
    peer's kernel that was itself waiting (on the device) for a kernel this rank had yet to enqueue.  Here: ~0.3 s of SpMVs
    are queued on a stream, a handle is destroyed behind them, and a handle of the same sizes is created at once: the create must return
    while the stream is still busy."""
    import time

    import torch

    from sparse_matrix_math_amd import host

    dev = torch.device("cuda:0")
    rows = 4_000_000
    nnz = host.gen_banded_nnz(rows, 25, 0x5EED, 1 << 18)
    own = torch.cuda.Stream(device=dev)
    st = own.cuda_stream
    ds = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    dp = torch.empty(nnz, dtype=torch.int32, device=dev)
    dv = torch.empty(nnz, dtype=torch.float32, device=dev)
    host.gen_banded_dev(rows, 25, 0x5EED, 1 << 18, ds, dp, dv, np.float32, st, diag_shift=1.0)
    big = smm.CSRMatrix.from_device(rows, rows, ds, dp, dv, np.float32)
    x = torch.rand(rows, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    small = gen.poisson2d(300, dtype=np.float64)
    n_small = len(small[0]) - 1
    for _ in range(3):
        big.spmv_dev(0, None, x, y, st)
    torch.cuda.synchronize()
    h1 = smm.CSRMatrix(n_small, n_small, *small)  # owns device copies of its three arrays
    t0 = time.perf_counter()
    for _ in range(1500):  # ~0.2 ms each: some tenths of a second of queued work behind which ...
        big.spmv_dev(0, None, x, y, st)
    enqueue_s = time.perf_counter() - t0
    h1.close()  # ... the handle's arrays are freed (quarantined: an event on the busy stream guards them)
    t1 = time.perf_counter()
    h2 = smm.CSRMatrix(n_small, n_small, *small)  # the same three sizes, at once
    create_s = time.perf_counter() - t1
    still_busy = not own.query()
    torch.cuda.synchronize()
    total_s = time.perf_counter() - t0
    assert still_busy, (enqueue_s, create_s, total_s)  # the queued work outlived the create ...
    assert create_s < 0.5 * (total_s - enqueue_s), (enqueue_s, create_s, total_s)  # ... which did not wait for it
    yv = np.zeros(n_small)
    h2.rMult(np.ones(n_small), yv)
    assert np.isfinite(yv).all()
    h2.close()
    big.close()
