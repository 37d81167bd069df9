"""lobpcg on the GPU (csrc/smm_solvers_lobpcg.hip) and its two block kernels (multi_gram, multi_block_axpy: csrc/smm_multiblock.h),
through the C ABI, the Python binding and the device-pointer form (the drop-in C++ header: tests/test_cpp_lobpcg.py).  The cases are those
of tests/lobpcg_cases.py; the reference is numpy.linalg.eigvalsh of the dense fp64 matrix.  Bounds, with lambda = eigvalsh,
|A| = max|lambda| and tol = 1e-10 (fp64) / 1e-4 (fp32):
  |theta_i - lambda_i| <= 10 tol |A|;  ||A x_i - theta_i x_i||_2 <= 10 tol |A| (formed in fp64 on the host);  residuals[i] <= tol |A|;
  max|X^T X - I| <= 4 ORTH_WORST eps, ORTH_WORST the worst ratio of the CPU restatement (tests/lobpcg_cases.py: 130 in fp64, 5.5 in fp32)
  and 4 the allowance for another summation order.  None of them is tuned to the code under test.
The solves pass maxIterations = 1000 and must report SUCCESS: the restatement needs at most 343 iterations on these cases."""
import ctypes

import lobpcg_cases as cases
import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, carve, fit
from lobpcg_restatement import block_axpy, start_block

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS, DIVERGED = 0, 1
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_DENSE = {}


def dense(name):
    if name not in _DENSE:
        _DENSE[name] = cases.dense(cases.matrix(name, np.float64))
        _DENSE[name].setflags(write=False)
    return _DENSE[name]


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def check_pairs(a64, want, norm_a, w, X, info, k, which, dtype, tol, orth_bound=True):
    """items 1 and 2 of the issue on one solve; prints every figure before it asserts"""
    eps = float(np.finfo(dtype).eps)
    w64, X64 = w.astype(np.float64), np.asarray(X, dtype=np.float64)
    err = float(np.max(np.abs(w64 - want)))
    res = float(np.max(np.linalg.norm(a64 @ X64 - X64 * w64, axis=0)))
    orth = float(np.max(np.abs(X64.T @ X64 - np.eye(k))))
    rn = float(np.max(info.residuals))
    print("status", int(info.status), "iterations", info.iterations, "matvecs", info.matvecs, "applies", info.applies, "nconv", info.nconv, "| err", err, "res", res,
          "bound", 10 * tol * norm_a, "| orth / eps", orth / eps, "bound", 4 * cases.ORTH_WORST[np.dtype(dtype)], "| rn", rn, "bound", tol * norm_a)
    assert int(info.status) == SUCCESS and info.nconv == k
    assert w.dtype == dtype and X.shape == (a64.shape[0], k)
    assert err <= 10 * tol * norm_a
    assert res <= 10 * tol * norm_a
    assert rn <= tol * norm_a
    assert info.iterations <= cases.MAX_ITERATIONS
    if orth_bound:
        assert orth <= 4 * cases.ORTH_WORST[np.dtype(dtype)] * eps
    if k > 1:
        order = np.diff(w64)
        assert np.all(order <= 0) if which == "LA" else np.all(order >= 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k", cases.combos(), ids=_ID)
def test_eigenpairs_order_counts_and_orthonormality(smm, name, which, k, dtype):
    """items 1 and 2.  Measured on an MI355X: the worst max|X^T X - I| / eps over the cases is 13 in fp64 (lap2d_33x29, LA, k = 6) and 6.6
    in fp32 (lap2d_33x29, LA, k = 8), against the bounds 520 and 22 -- the fp64 figure is below the restatement's 129 because the library
    accumulates the Jacobi rotations in long double."""
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    w, X, info = smm.lobpcg(A, k, which, tol=tol, max_iterations=cases.MAX_ITERATIONS)
    lam = cases.exact(name)
    check_pairs(dense(name), cases.wanted(lam, which, k), float(np.max(np.abs(lam))), w, X, info, k, which, dtype, tol)
    assert info.applies == 0 and k < info.matvecs <= k + k * info.iterations


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_multiple_eigenvalues_square_grid(smm, dtype):
    """the 16 x 16 five-point Laplacian, SA, k = 6: two double eigenvalues inside the block, a clean cut after the sixth"""
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.lap2d_16x16(dtype))
    a64 = cases.dense(cases.lap2d_16x16())
    lam = np.linalg.eigvalsh(a64)
    w, X, info = smm.lobpcg(A, 6, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS)
    check_pairs(a64, lam[:6], float(lam[-1]), w, X, info, 6, "SA", dtype, tol)


@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_multiple_eigenvalues_diagonal(smm, dtype, which):
    """diag(1 x 20, 2 x 20, 5 x 20), k = 3: three copies of one eigenvalue; X is zero outside the eigenspace's rows"""
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.triple_diagonal(dtype))
    a64 = cases.dense(cases.triple_diagonal())
    w, X, info = smm.lobpcg(A, 3, which, tol=tol, max_iterations=cases.MAX_ITERATIONS)
    value, outside = (5.0, slice(0, 40)) if which == "LA" else (1.0, slice(20, 60))
    check_pairs(a64, np.full(3, value), 5.0, w, X, info, 3, which, dtype, tol)
    assert float(np.max(np.abs(X[outside].astype(np.float64)))) <= 100 * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_edges(smm, dtype):
    tol = cases.TOL[np.dtype(dtype)]
    # the identity: every start block is an invariant subspace -- converged at iteration 0.  At the cases' tol, not at tol = eps: the
    # residual of an exactly invariant block is the normalisation's rounding, (1 - theta) x with |1 - theta| a few eps, which passes a test
    # against eps only by luck (the restatement in fp32: 3.5 eps).
    A = make(smm, cases.diagonal(np.ones(50), dtype))
    w, X, info = smm.lobpcg(A, 3, "SA", tol=tol)
    print(w, info)
    assert int(info.status) == SUCCESS and info.iterations == 0 and info.matvecs == 3 and info.nconv == 3
    assert float(np.max(np.abs(w.astype(np.float64) - 1.0))) <= 4 * float(np.finfo(dtype).eps)
    # 3k == rows: the full basis
    A = make(smm, cases.diagonal(np.arange(1.0, 25.0), dtype))
    a64 = np.diag(np.arange(1.0, 25.0))
    w, X, info = smm.lobpcg(A, 8, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS)
    check_pairs(a64, np.arange(1.0, 9.0), 24.0, w, X, info, 8, "SA", dtype, tol)
    # X0 = the hash start, generated outside: the same bits as X0 = None
    name, k = "lap2d_16x12", 4
    A = make(smm, cases.matrix(name, dtype))
    n = cases.ROWS[name]
    X0 = start_block(n, k, 5, dtype)
    own = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=5)
    given = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, X0=X0, seed=99)
    assert int(own[2].status) == SUCCESS and own[2].iterations == given[2].iterations
    assert np.array_equal(bits(own[0]), bits(given[0])) and np.array_equal(bits(own[1]), bits(given[1]))
    # two equal start columns: rank below k -- DIVERGED, and the outputs are not written
    X0[:, 2] = X0[:, 0]
    lib = _lib.load()
    P = ctypes.c_void_p
    wq, Xq, rq = np.full(k, 7.0, dtype=dtype), np.full(k * n, 7.0, dtype=dtype), np.full(k, 7.0, dtype=dtype)
    ints = [ctypes.c_int(-5) for _ in range(5)]
    start = np.ascontiguousarray(X0.T)
    fn = lib.smm_hip_lobpcg_f32 if dtype == np.float32 else lib.smm_hip_lobpcg_f64
    rc = fn(A._h, k, 1, 100, dtype(tol), None, start.ctypes.data_as(P), n, 0, wq.ctypes.data_as(P), Xq.ctypes.data_as(P), n, rq.ctypes.data_as(P),
            *[ctypes.byref(i) for i in ints])
    assert rc == 0 and ints[4].value == DIVERGED and ints[1].value == 0
    assert np.all(wq == 7.0) and np.all(Xq == 7.0) and np.all(rq == 7.0)


PRECOND_KINDS = {"JACOBI": "JACOBI", "SGS": "SYMMETRIC_GAUS_SEIDEL", "IC0": "IC0", "FSAI": "FSAI", "AMG": "AMG"}


def test_preconditioners(smm):
    """lap2d_33x29, SA, k = 4, fp64: every symmetric kind meets item 1's bounds; SGS and IC0 take strictly fewer iterations than none"""
    name, k, dtype, tol = "lap2d_33x29", 4, np.float64, 1e-10
    A = make(smm, cases.matrix(name, dtype))
    lam = cases.exact(name)
    plain = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS)[2]
    counts = {"none": plain.iterations}
    for kind, enum_name in PRECOND_KINDS.items():
        M = A.getPreconditioner(enum_name)
        w, X, info = smm.lobpcg(A, k, "SA", M=M, tol=tol, max_iterations=cases.MAX_ITERATIONS)
        print(kind, end=" ")
        check_pairs(dense(name), lam[:k], float(lam[-1]), w, X, info, k, "SA", dtype, tol, orth_bound=False)
        assert info.applies > 0 and info.matvecs == k + info.applies
        counts[kind] = info.iterations
    print("iterations", counts)
    assert counts["SGS"] < counts["none"] and counts["IC0"] < counts["none"]


def test_preconditioner_of_a_positive_definite_relative(smm):
    """shifted_16x12 = lap2d_16x12 - 3.1 I is indefinite: it takes the IC0 of lap2d_16x12"""
    tol = 1e-10
    L = make(smm, cases.matrix("lap2d_16x12", np.float64))
    A = make(smm, cases.matrix("shifted_16x12", np.float64))
    M = L.getPreconditioner("IC0")
    lam = cases.exact("shifted_16x12")
    w, X, info = smm.lobpcg(A, 4, "SA", M=M, tol=tol, max_iterations=cases.MAX_ITERATIONS)
    check_pairs(dense("shifted_16x12"), lam[:4], float(np.max(np.abs(lam))), w, X, info, 4, "SA", np.float64, tol, orth_bound=False)
    assert info.applies > 0 and info.matvecs == 4 + info.applies


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_same_bits_twice_and_another_seed(smm, dtype):
    name, k = "lap2d_33x29", 4
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    first = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=7)
    again = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=7)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(bits(first[1]), bits(again[1]))
    assert first[2].iterations == again[2].iterations and np.array_equal(bits(first[2].residuals), bits(again[2].residuals))
    other = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=8)
    assert not np.array_equal(bits(first[1]), bits(other[1]))  # another start block
    lam = cases.exact(name)
    for w, _, info in (first, other):
        assert int(info.status) == SUCCESS
        assert float(np.max(np.abs(w.astype(np.float64) - lam[:k]))) <= 10 * tol * float(np.max(np.abs(lam)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_device_pointers_on_offset_views_and_another_stream(smm, dtype):
    """smm_hip_lobpcg_dev_* on a stream of the caller's: the eigenvalues and the eigenvectors at element alignment inside larger buffers
    with guard bands, ldx = rows + 1; the elements between the vectors keep their NaN"""
    name, k, which = "lap2d_16x12", 4, "SA"
    tol = cases.TOL[np.dtype(dtype)]
    csr = cases.matrix(name, dtype)
    n = cases.ROWS[name]
    ldx = n + 1
    d_w = carve(k, dtype, fit(3, dtype), device="cuda:0")
    d_X = carve(k * ldx, dtype, fit(1, dtype), device="cuda:0")
    A = make(smm, csr)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    info = host.lobpcg_dev(A, k, which, d_w, d_X, ldx, tol=tol, max_iterations=cases.MAX_ITERATIONS, stream=s.cuda_stream)
    torch.cuda.synchronize()
    grid = d_X.view(k, ldx).cpu().numpy()
    lam = cases.exact(name)
    check_pairs(dense(name), lam[:k], float(lam[-1]), d_w.cpu().numpy(), grid[:, :n].T, info, k, which, dtype, tol)
    assert np.all(np.isnan(grid[:, n:]))
    for view, label in ((d_w, "w"), (d_X, "X")):
        assert_guards_intact(view, label)
    w, X, again = smm.lobpcg(A, k, which, tol=tol, max_iterations=cases.MAX_ITERATIONS)  # the host-array form: the same launches, the same bits
    assert again.iterations == info.iterations and np.array_equal(bits(w), bits(d_w.cpu().numpy()))


BLOCK_N = (1, 63, 64, 65, 255, 257, 957, 4099)
BLOCK_ML = ((1, 1), (3, 5), (8, 16), (16, 16), (17, 24), (24, 24))


def _block(n, cols, ld, dtype, residue, rng):
    """`cols` columns of n elements inside a guarded buffer of cols * ld NaNs; returns (view, host array (n, cols))"""
    host_block = rng.uniform(-1, 1, (n, cols)).astype(dtype)
    d = carve(cols * ld, dtype, residue, device="cuda:0")
    d.view(cols, ld)[:, :n] = torch.from_numpy(np.ascontiguousarray(host_block.T)).to("cuda:0")
    return d, host_block


def _layout(n, layout, dtype):
    """aligned: a 16-byte aligned base and ld = n rounded up to 64; offset: one element past a 16-byte boundary and an odd ld"""
    ld = (n + 63) // 64 * 64 + (0 if layout == "aligned" else 1)
    return ld, (0 if layout == "aligned" else fit(1, dtype))


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("m,l", BLOCK_ML, ids=_ID)
def test_multi_gram(smm, m, l, dtype, layout):
    """item 7: G = V^T W against fp64 numpy, |G_ij - exact| <= n eps sum_r |v_ri| |w_rj| (the worst-case bound of any summation order);
    the same bits on a second call; the square shapes with d_V == d_W as well; guards intact, nothing between n and ld touched"""
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(100 * m + l)
    for n in BLOCK_N:
        ld, residue = _layout(n, layout, dtype)
        d_V, V = _block(n, m, ld, dtype, residue, rng)
        d_W, W = _block(n, l, ld, dtype, residue, rng)
        ldg = m + 3
        d_G = carve(l * ldg, dtype, fit(1, dtype), device="cuda:0")
        torch.cuda.synchronize()
        pairs = [(d_W, W, ld)] + ([(d_V, V, ld)] if m == l else [])
        for d_B, B, ldb in pairs:
            host.multi_gram_dev(n, m, l, d_V, ld, d_B, ldb, d_G, ldg, dtype)
            torch.cuda.synchronize()
            first = d_G.view(l, ldg).cpu().numpy().copy()
            d_G.view(l, ldg)[:, :m] = float("nan")
            host.multi_gram_dev(n, m, l, d_V, ld, d_B, ldb, d_G, ldg, dtype)
            torch.cuda.synchronize()
            second = d_G.view(l, ldg).cpu().numpy()
            assert np.array_equal(bits(first[:, :m]), bits(second[:, :m])), n
            assert np.all(np.isnan(second[:, m:])), n
            got = second[:, :m].T.astype(np.float64)
            exact = V.astype(np.float64).T @ B.astype(np.float64)
            bound = n * eps * (np.abs(V).astype(np.float64).T @ np.abs(B).astype(np.float64))
            assert not np.any(np.isnan(got)), n
            assert np.all(np.abs(got - exact) <= bound), (n, float(np.max(np.abs(got - exact) / bound)))
        for view, label in ((d_V, "V"), (d_W, "W"), (d_G, "G")):
            assert_guards_intact(view, f"{label} n={n}")
        assert np.all(np.isnan(d_V.view(m, ld)[:, n:].cpu().numpy())) and np.all(np.isnan(d_W.view(l, ld)[:, n:].cpu().numpy()))


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("m,l", BLOCK_ML, ids=_ID)
def test_multi_block_axpy(smm, m, l, dtype, layout):
    """item 8: W -= V H, bit for bit the restatement's j-ascending chain (the library tested is the a*x+b flavour of _smm_fma); V
    untouched, guards intact, nothing between n and ld touched"""
    rng = np.random.default_rng(200 * m + l)
    for n in BLOCK_N:
        ld, residue = _layout(n, layout, dtype)
        d_V, V = _block(n, m, ld, dtype, residue, rng)
        d_W, W = _block(n, l, ld, dtype, residue, rng)
        H = rng.uniform(-1, 1, (m, l)).astype(dtype)
        ldh = m + 1
        d_H = carve(l * ldh, dtype, fit(1, dtype), device="cuda:0")
        d_H.view(l, ldh)[:, :m] = torch.from_numpy(np.ascontiguousarray(H.T)).to("cuda:0")
        v_before = d_V.clone()
        torch.cuda.synchronize()
        host.multi_block_axpy_dev(n, m, l, d_V, ld, d_H, ldh, d_W, ld, dtype)
        torch.cuda.synchronize()
        after = d_W.view(l, ld).cpu().numpy()
        want = block_axpy(V, H, W)
        assert np.array_equal(bits(after[:, :n].T), bits(want)), n
        assert np.all(np.isnan(after[:, n:])), n
        assert np.array_equal(bits(d_V.cpu().numpy()), bits(v_before.cpu().numpy())), n
        for view, label in ((d_V, "V"), (d_W, "W"), (d_H, "H")):
            assert_guards_intact(view, f"{label} n={n}")


def test_gram_feeds_block_axpy_without_a_host_read(smm):
    """the pair as the driver uses it: H = X^T Z on the device, Z -= X H; afterwards X^T Z is at rounding level"""
    n, k, nz, ld = 957, 6, 11, 960
    rng = np.random.default_rng(9)
    Xh = np.linalg.qr(rng.uniform(-1, 1, (n, k)))[0]
    d_X = torch.zeros((k, ld), dtype=torch.float64, device="cuda:0")
    d_X[:, :n] = torch.from_numpy(np.ascontiguousarray(Xh.T)).to("cuda:0")
    d_Z = torch.zeros((nz, ld), dtype=torch.float64, device="cuda:0")
    d_Z[:, :n] = torch.from_numpy(rng.uniform(-1, 1, (nz, n))).to("cuda:0")
    d_H = torch.zeros((nz, k), dtype=torch.float64, device="cuda:0")
    host.multi_gram_dev(n, k, nz, d_X, ld, d_Z, ld, d_H, k, np.float64)
    host.multi_block_axpy_dev(n, k, nz, d_X, ld, d_H, k, d_Z, ld, np.float64)
    host.multi_gram_dev(n, k, nz, d_X, ld, d_Z, ld, d_H, k, np.float64)
    torch.cuda.synchronize()
    assert float(d_H.abs().max()) <= 100 * n * float(np.finfo(np.float64).eps)


def test_refusals_leave_the_outputs_untouched(smm):
    """item 9: every SMM_HIP_ERR_INVALID condition of the three entry points, through the C ABI"""
    lib = _lib.load()
    P = ctypes.c_void_p
    A = make(smm, cases.matrix("chain_96", np.float64))
    A32 = make(smm, cases.matrix("chain_96", np.float32))
    start = np.array([0, 1, 2], dtype=np.int32)
    wide = smm.CSRMatrix(2, 3, start, np.array([0, 1], dtype=np.int32), np.array([1.0, 1.0]))
    tiny = make(smm, cases.diagonal(np.ones(5), np.float64))
    other = make(smm, cases.matrix("lap2d_16x12", np.float64))
    M_ilu = A.getPreconditioner("ILU0")      # a kind CG refuses
    M_size = other.getPreconditioner("JACOBI")  # another size
    M_32 = A32.getPreconditioner("JACOBI")
    w, X, res, X0 = np.full(8, 7.0), np.full(8 * 96, 7.0), np.full(8, 7.0), np.ones(8 * 96)
    ints = [ctypes.c_int(-5) for _ in range(5)]

    def call(a, k, which, its, M=None, x0=None, ldx0=96, w_arr=w, ldx=96):
        return lib.smm_hip_lobpcg_f64(a, k, which, its, 0.0, None if M is None else M._h, None if x0 is None else x0.ctypes.data_as(P), ldx0, 0,
                                      None if w_arr is None else w_arr.ctypes.data_as(P), X.ctypes.data_as(P), ldx, res.ctypes.data_as(P),
                                      *[ctypes.byref(i) for i in ints])

    refused = [
        ("null matrix", lambda: call(None, 2, 1, 10)),
        ("dtype", lambda: call(A32._h, 2, 1, 10)),
        ("not square", lambda: call(wide._h, 1, 1, 10)),
        ("k < 0", lambda: call(A._h, -1, 1, 10)),
        ("k > 8", lambda: call(A._h, 9, 1, 10)),
        ("3k > rows", lambda: call(tiny._h, 2, 1, 10)),
        ("which", lambda: call(A._h, 2, 2, 10)),
        ("maxIterations", lambda: call(A._h, 2, 1, -1)),
        ("null eigenvalues", lambda: call(A._h, 2, 1, 10, w_arr=None)),
        ("ldx < rows", lambda: call(A._h, 2, 1, 10, ldx=95)),
        ("ldx0 < rows", lambda: call(A._h, 2, 1, 10, x0=X0, ldx0=95)),
        ("a kind CG refuses", lambda: call(A._h, 2, 1, 10, M=M_ilu)),
        ("a preconditioner of another size", lambda: call(A._h, 2, 1, 10, M=M_size)),
        ("a preconditioner of the other dtype", lambda: call(A._h, 2, 1, 10, M=M_32)),
    ]
    for label, fn in refused:
        assert fn() == INVALID, label
        assert lib.smm_hip_last_error().decode().startswith("lobpcg:"), (label, lib.smm_hip_last_error())
        assert np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0) and all(i.value == -5 for i in ints), label
    assert "dense work" in (call(tiny._h, 2, 1, 10), lib.smm_hip_last_error().decode())[1]
    # the device-pointer form refuses the same way
    assert lib.smm_hip_lobpcg_dev_f64(A._h, 9, 1, 10, 0.0, None, None, 0, 0, None, None, 96, None, None, None, None, None, None, None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    # degenerate, not refused: k == 0 and rows == 0 report SUCCESS and touch nothing else
    empty = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    for handle in (A._h, empty._h):
        for i in ints:
            i.value = -5
        assert call(handle, 0 if handle is A._h else 3, 1, 10) == 0
        assert [i.value for i in ints] == [0, 0, 0, 0, 0] and np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0)
    # the two kernels
    d = torch.full((64 * 4,), 3.0, dtype=torch.float64, device="cuda:0")
    g = torch.full((16,), 3.0, dtype=torch.float64, device="cuda:0")
    dp, gp = host._dptr(d), host._dptr(g)
    for n, m, l, ldv, ldw, ldg in ((-1, 4, 4, 64, 64, 4), (64, 0, 4, 64, 64, 4), (64, 4, 0, 64, 64, 4), (64, 25, 4, 64, 64, 25), (64, 4, 25, 64, 64, 4),
                                   (64, 4, 4, 63, 64, 4), (64, 4, 4, 64, 63, 4), (64, 4, 4, 64, 64, 3)):
        assert lib.smm_hip_multi_gram_dev_f64(n, m, l, dp, ldv, dp, ldw, gp, ldg, None) == INVALID, (n, m, l, ldv, ldw, ldg)
        assert lib.smm_hip_last_error().decode().startswith("multi_gram:")
        assert lib.smm_hip_multi_block_axpy_dev_f64(n, m, l, dp, ldv, gp, ldg, dp, ldw, None) == INVALID, (n, m, l, ldv, ldw, ldg)
        assert lib.smm_hip_last_error().decode().startswith("multi_block_axpy:")
    assert lib.smm_hip_multi_gram_dev_f64(64, 4, 4, None, 64, dp, 64, gp, 4, None) == INVALID
    assert lib.smm_hip_multi_gram_dev_f64(64, 4, 4, dp, 64, dp, 64, None, 4, None) == INVALID
    assert lib.smm_hip_multi_block_axpy_dev_f64(64, 4, 4, dp, 64, None, 4, dp, 64, None) == INVALID
    assert lib.smm_hip_multi_block_axpy_dev_f64(64, 4, 4, dp, 64, gp, 4, None, 64, None) == INVALID
    torch.cuda.synchronize()
    assert bool((d == 3.0).all()) and bool((g == 3.0).all())
