"""eigsh on the GPU (csrc/smm_solvers_eigsh.hip) and its compression kernel (multi_rotate, csrc/smm_multivec.h), through the C ABI, the
Python binding and the device-pointer form (the drop-in C++ header: tests/test_cpp_eigsh.py).  The matrices are those of tests/eigsh_cases.py; the reference is
numpy.linalg.eigvalsh of the dense fp64 matrix.  Bounds, with lambda = eigvalsh, |A| = max|lambda| and tol = 1e-10 (fp64) / 1e-4 (fp32):
  |theta_i - lambda_i| <= 10 tol |A|;  ||A x_i - theta_i x_i||_2 <= 10 tol |A| (formed in fp64 on the host);  max|X^T X - I| <= 100 eps;
  residuals[i] <= tol |A|.  The factor 10 is the margin of the a-posteriori estimate rho_i over the true residual (the restatement's
ratio is <= 1.0 on every case: tests/test_eigsh_cpu.py prints it); none of them is tuned to the code under test.
The solves pass maxRestarts = 100 and must report SUCCESS: the restatement needs at most 25 restarts on these cases."""
import ctypes

import eigsh_cases as cases
import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, carve, carve_like, fit, snapshot

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS = 0
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


def check_pairs(a64, lam, w, X, info, k, which, dtype, tol):
    """items 1 to 3 of the issue on one solve; prints every figure before it asserts"""
    eps = float(np.finfo(dtype).eps)
    norm_a = float(np.max(np.abs(lam)))
    want = cases.wanted(lam, which, k)
    w64, X64 = w.astype(np.float64), np.asarray(X, dtype=np.float64)
    err = float(np.max(np.abs(w64 - want)))
    res = float(np.max(np.linalg.norm(a64 @ X64 - X64 * w64, axis=0)))
    orth = float(np.max(np.abs(X64.T @ X64 - np.eye(k))))
    rho = float(np.max(info.residuals))
    print("status", int(info.status), "restarts", info.restarts, "matvecs", info.matvecs, "nconv", info.nconv, "| err", err, "res", res, "bound",
          10 * tol * norm_a, "| orth", orth, "bound", 100 * eps, "| rho", rho, "bound", tol * norm_a)
    assert int(info.status) == SUCCESS and info.nconv == k
    assert w.dtype == dtype and X.shape == (a64.shape[0], k)
    assert err <= 10 * tol * norm_a
    assert res <= 10 * tol * norm_a
    assert orth <= 100 * eps
    assert rho <= tol * norm_a
    order = np.diff(w64)
    assert np.all(order < 0) if which == "LA" else np.all(order > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k,ncv", cases.combos(), ids=_ID)
def test_eigenpairs_order_and_counts(smm, name, which, k, ncv, dtype):
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    w, X, info = smm.eigsh(A, k, which, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS)
    check_pairs(dense(name), cases.exact(name), w, X, info, k, which, dtype, tol)
    l = k + (ncv - k) // 2
    assert info.matvecs == ncv + info.restarts * (ncv - l)  # no breakdown on these matrices
    assert 0 < info.restarts <= cases.MAX_RESTARTS


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_same_bits_twice_and_another_seed(smm, dtype):
    name, k, ncv = "lap2d_33x29", 4, 20
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    first = smm.eigsh(A, k, "SA", ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=7)
    again = smm.eigsh(A, k, "SA", ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=7)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(bits(first[1]), bits(again[1]))
    assert first[2].restarts == again[2].restarts and np.array_equal(bits(first[2].residuals), bits(again[2].residuals))
    other = smm.eigsh(A, k, "SA", ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=8)
    assert not np.array_equal(bits(first[1]), bits(other[1]))  # another start vector
    lam = cases.exact(name)
    for w, _, info in (first, other):
        assert int(info.status) == SUCCESS
        assert float(np.max(np.abs(w.astype(np.float64) - lam[:k]))) <= 10 * tol * float(np.max(np.abs(lam)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_identity(smm, dtype):
    """every start vector is an eigenvector: three breakdowns at m = 1, 2, 3, a fresh hash vector after each of the first two"""
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.diagonal(np.ones(50), dtype))
    w, X, info = smm.eigsh(A, 3, "LA", ncv=8)
    print(w, info)
    assert int(info.status) == SUCCESS and info.nconv == 3
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(X))
    assert float(np.max(np.abs(w.astype(np.float64) - 1.0))) <= 4 * eps
    X64 = X.astype(np.float64)
    assert float(np.max(np.abs(X64.T @ X64 - np.eye(3)))) <= 100 * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_multiple_eigenvalue(smm, dtype):
    """diag(1 x 20, 2 x 20, 5 x 20): the Krylov space of one start vector holds ONE vector of the 5-eigenspace; the copies come from the
    fresh starts (or from the rounding-level vector a breakdown that is not quite one leaves)"""
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.diagonal(np.repeat([1.0, 2.0, 5.0], 20), dtype))
    w, X, info = smm.eigsh(A, 3, "LA")
    print(w, info)
    assert int(info.status) == SUCCESS and info.nconv == 3
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(X))
    assert float(np.max(np.abs(w.astype(np.float64) - 5.0))) <= 10 * eps * 5.0
    X64 = X.astype(np.float64)
    assert float(np.max(np.abs(X64.T @ X64 - np.eye(3)))) <= 100 * eps
    assert float(np.max(np.abs(X64[:40]))) <= 100 * eps  # inside the 5-eigenspace: nothing on the rows of 1 and 2


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_invariant_subspace_of_the_start_vector(smm, dtype):
    """diag(1..192) from a v0 on rows 3, 50 and 100: the method cannot leave that subspace, as documented -- [101, 51], not [192, 191]"""
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.diagonal(np.arange(1.0, 193.0), dtype))
    v0 = np.zeros(192, dtype=dtype)
    v0[[3, 50, 100]] = [1.0, 2.0, 3.0]
    w, X, info = smm.eigsh(A, 2, "LA", v0=v0)
    print(w, info)
    assert int(info.status) == SUCCESS and info.nconv == 2 and info.restarts == 0 and info.matvecs == 3
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(X))
    assert float(np.max(np.abs(w.astype(np.float64) - [101.0, 51.0]))) <= 10 * eps * 101.0
    X64 = np.abs(X.astype(np.float64))
    assert abs(X64[100, 0] - 1) <= 100 * eps and abs(X64[50, 1] - 1) <= 100 * eps


ROTATE_N = (1, 63, 64, 65, 257, 1000)
ROTATE_ML = ((2, 1), (8, 8), (20, 12), (33, 32), (64, 63))


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("m,l", ROTATE_ML, ids=_ID)
def test_multi_rotate_alone(smm, m, l, dtype, layout):
    """V[:, :l] = V[:, :m] @ Y against fp64, |error| <= m eps (|V| |Y|) per element; NaN everywhere the kernel has no business: between
    n and ld, after the last column and around the buffer.  aligned: a 16-byte aligned base and ld = n rounded up to 64 (the 16-byte
    path where the padded m allows it); offset: one element past a 16-byte boundary and an odd ld (the element path)."""
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(100 * m + l)
    for n in ROTATE_N:
        ld = (n + 63) // 64 * 64 + (0 if layout == "aligned" else 1)
        V = rng.uniform(-1, 1, (n, m)).astype(dtype)
        Y = rng.uniform(-1, 1, (m, l)).astype(dtype)
        d = carve(m * ld, dtype, 0 if layout == "aligned" else 1, device="cuda:0")
        assert d.data_ptr() % 16 == (0 if layout == "aligned" else np.dtype(dtype).itemsize)
        grid = d.view(m, ld)  # row c: column c of the basis
        grid[:, :n] = torch.from_numpy(np.ascontiguousarray(V.T)).to("cuda:0")
        before = grid.cpu().numpy().copy()
        torch.cuda.synchronize()
        host.multi_rotate_dev(n, m, l, d, ld, Y, dtype)
        torch.cuda.synchronize()
        after = grid.cpu().numpy()
        assert_guards_intact(d, f"V n={n}")
        assert np.all(np.isnan(after[:, n:])), n  # between n and ld, and behind the last column's n elements
        assert np.array_equal(bits(after[l:, :n]), bits(before[l:, :n])), n  # columns l .. m-1 keep their bits
        got = after[:l, :n].T.astype(np.float64)
        assert not np.any(np.isnan(got)), n
        want = V.astype(np.float64) @ Y.astype(np.float64)
        bound = m * eps * (np.abs(V).astype(np.float64) @ np.abs(Y).astype(np.float64))
        assert np.all(np.abs(got - want) <= bound), (n, float(np.max(np.abs(got - want) / bound)))


def test_multi_rotate_refusals(smm):
    d = torch.zeros(64 * 4, dtype=torch.float64, device="cuda:0")
    saved = d.clone()
    Y = np.eye(4)
    lib = _lib.load()
    ptr = Y.ctypes.data_as(ctypes.c_void_p)
    for n, m, l, ld, ldy in ((-1, 4, 4, 64, 4), (64, 4, 0, 64, 4), (64, 3, 4, 64, 4), (64, 65, 4, 64, 65), (64, 4, 4, 63, 4), (64, 4, 4, 64, 3)):
        assert lib.smm_hip_multi_rotate_dev_f64(n, m, l, host._dptr(d), ld, ptr, ldy, None) == INVALID, (n, m, l, ld, ldy)
    assert lib.smm_hip_multi_rotate_dev_f64(64, 4, 4, host._dptr(d), 64, None, 4, None) == INVALID
    assert lib.smm_hip_multi_rotate_dev_f64(64, 4, 4, None, 64, ptr, 4, None) == INVALID
    assert lib.smm_hip_multi_rotate_dev_f64(0, 4, 4, None, 64, ptr, 4, None) == 0
    assert torch.equal(d, saved)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_device_pointers_on_offset_views_and_another_stream(smm, dtype):
    """smm_hip_eigsh_dev_* on a stream of the caller's: the start vector, the eigenvalues and the eigenvectors at element alignment
    inside larger buffers with guard bands, ldx = rows + 1; the elements between the vectors keep their NaN"""
    name, k, ncv, which = "lap2d_16x12", 4, 20, "LA"
    tol = cases.TOL[np.dtype(dtype)]
    csr = cases.matrix(name, dtype)
    n = cases.ROWS[name]
    ldx = n + 1
    v0 = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    d_v0 = carve_like(v0, fit(1, dtype), device="cuda:0")
    d_w = carve(k, dtype, fit(3, dtype), device="cuda:0")
    d_X = carve(k * ldx, dtype, fit(1, dtype), device="cuda:0")
    saved = snapshot(d_v0)
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    info = host.eigsh_dev(A, k, which, d_w, d_X, ldx, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, d_v0=d_v0, stream=s.cuda_stream)
    torch.cuda.synchronize()
    grid = d_X.view(k, ldx).cpu().numpy()
    check_pairs(dense(name), cases.exact(name), d_w.cpu().numpy(), grid[:, :n].T, info, k, which, dtype, tol)
    assert np.all(np.isnan(grid[:, n:]))
    assert np.array_equal(snapshot(d_v0).cpu().numpy(), saved.cpu().numpy())
    for view, label in ((d_v0, "v0"), (d_w, "w"), (d_X, "X")):
        assert_guards_intact(view, label)
    # the host-array form from the same start vector: the same library, the same launches, the same bits
    w, X, again = smm.eigsh(make(smm, csr), k, which, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, v0=v0)
    assert again.restarts == info.restarts and np.array_equal(bits(w), bits(d_w.cpu().numpy()))


def test_eigenvalues_only_and_the_default_ncv(smm):
    A = make(smm, cases.matrix("chain_96", np.float64))
    w, info = smm.eigsh(A, 3, "LA", tol=1e-10, return_eigenvectors=False)
    lam = cases.exact("chain_96")
    assert int(info.status) == SUCCESS and info.matvecs == 20 + info.restarts * (20 - (3 + 17 // 2))  # ncv = max(2k + 1, 20)
    assert float(np.max(np.abs(w - lam[::-1][:3]))) <= 10 * 1e-10 * float(lam[-1])


def test_chebyshev_bound_from_eigsh(smm):
    """INTEGRATION.md's example: lambda_max of lap2d_33x29 from eigsh(A, 1, "LA"), times 1.01, as the USER bound of a CHEBYSHEV
    preconditioner (whose bounds are on D^-1 A: the diagonal is 4 in every row).  CG takes no more iterations than with the Gershgorin
    bound on the same system."""
    csr = cases.matrix("lap2d_33x29", np.float64)
    A = make(smm, csr)
    n = cases.ROWS["lap2d_33x29"]
    w, _, info = smm.eigsh(A, 1, "LA", tol=1e-8)
    assert int(info.status) == SUCCESS and abs(float(w[0]) - float(cases.exact("lap2d_33x29")[-1])) <= 1e-6
    lmax = 1.01 * float(w[0]) / 4.0
    b = np.random.default_rng(11).uniform(-1, 1, n)
    counts = {}
    for label, kwargs in (("gershgorin", dict(bound="GERSHGORIN")), ("eigsh", dict(bound="USER", lambda_min=lmax / 30, lambda_max=lmax))):
        M = A.getPreconditioner("CHEBYSHEV", degree=3, **kwargs)
        x = np.zeros(n)
        it = {}
        assert int(smm.ConjugateGradient(A, b, x, x, -1, 1e-8, M, info=it)) == SUCCESS
        counts[label] = it["iterations"]
        assert float(np.linalg.norm(b - dense("lap2d_33x29") @ x)) <= 1e-6
    print("CG iterations", counts, "lambda_max of D^-1 A: user", lmax, "Gershgorin 2.0")
    assert counts["eigsh"] <= counts["gershgorin"]


def test_refusals_leave_the_outputs_untouched(smm):
    """every SMM_HIP_ERR_INVALID condition of the contract, through the C ABI; the message starts with "eigsh:" """
    lib = _lib.load()
    P = ctypes.c_void_p
    csr = cases.matrix("chain_96", np.float64)
    A = make(smm, csr)
    A32 = make(smm, cases.matrix("chain_96", np.float32))
    start = np.array([0, 1, 2], dtype=np.int32)
    wide = smm.CSRMatrix(2, 3, start, np.array([0, 1], dtype=np.int32), np.array([1.0, 1.0]))
    tiny = make(smm, cases.diagonal(np.ones(3), np.float64))
    w = np.full(8, 7.0)
    X = np.full(8 * 96, 7.0)
    res = np.full(8, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(4)]

    def call(a, k, which, ncv, restarts, w_arr=w, x_arr=X, ldx=96):
        args = [a, k, which, ncv, restarts, 0.0, None, 0, None if w_arr is None else w_arr.ctypes.data_as(P), None if x_arr is None else x_arr.ctypes.data_as(P), ldx,
                res.ctypes.data_as(P)] + [ctypes.byref(i) for i in ints]
        return lib.smm_hip_eigsh_f64(*args)

    refused = [
        ("null matrix", lambda: call(None, 2, 0, 0, 10)),
        ("dtype", lambda: call(A32._h, 2, 0, 0, 10)),
        ("not square", lambda: call(wide._h, 1, 0, 0, 10)),
        ("k < 0", lambda: call(A._h, -1, 0, 0, 10)),
        ("which", lambda: call(A._h, 2, 2, 0, 10)),
        ("restarts", lambda: call(A._h, 2, 0, 0, -1)),
        ("k > rows - 2", lambda: call(A._h, 95, 0, 0, 10)),
        ("k > rows - 2, tiny", lambda: call(tiny._h, 2, 0, 0, 10)),
        ("ncv < k + 2", lambda: call(A._h, 4, 0, 5, 10)),
        ("ncv > 64", lambda: call(A._h, 4, 0, 65, 10)),
        ("ncv > rows", lambda: call(tiny._h, 1, 0, 4, 10)),
        ("null eigenvalues", lambda: call(A._h, 2, 0, 0, 10, w_arr=None)),
        ("ldx < rows", lambda: call(A._h, 2, 0, 0, 10, ldx=95)),
    ]
    for label, fn in refused:
        assert fn() == INVALID, label
        assert lib.smm_hip_last_error().decode().startswith("eigsh:"), (label, lib.smm_hip_last_error())
        assert np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0) and all(i.value == -5 for i in ints), label
    # the device-pointer form refuses the same way
    assert lib.smm_hip_eigsh_dev_f64(A._h, 4, 0, 5, 10, 0.0, None, 0, None, None, 96, None, None, None, None, None, None) == INVALID
    # degenerate, not refused: k == 0 and rows == 0 report SUCCESS and touch nothing else
    empty = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    for handle in (A._h, empty._h):
        for i in ints:
            i.value = -5
        assert call(handle, 0 if handle is A._h else 3, 0, 0, 10) == 0
        assert [i.value for i in ints] == [0, 0, 0, 0] and np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0)
    # k == rows - 2 with ncv == rows is the edge that is allowed
    w3, X3, info = smm.eigsh(tiny, 1, "LA", ncv=3)
    assert int(info.status) == SUCCESS and abs(float(w3[0]) - 1.0) <= 1e-15
