"""svds on the GPU (csrc/smm_solvers_svds.hip), through the Python binding, the raw C ABI and the device-pointer form (the drop-in C++
header: tests/test_cpp_svds.py).  The matrices are those of tests/svds_cases.py; the reference is numpy.linalg.svd of the dense fp64
matrix.  Bounds, with sigma = numpy's values, |A| = sigma_0 and tol = 1e-10 (fp64) / 1e-4 (fp32):
  |s_i - sigma_i| <= 10 tol |A|;  max(||A v_i - s_i u_i||, ||A^T u_i - s_i v_i||) <= 10 tol |A| (formed in fp64 on the host);
  residuals[i] <= tol |A|;  max|U^T U - I| and max|V^T V - I| <= 4 x the largest loss the RESTATEMENT shows on these cases in that dtype
  (svds_cases.ORTH_LOSS_EPS, pinned by tests/test_svds_cpu.py: 69 eps in fp64, 3 eps in fp32; the factor 4 covers another summation order).
None of them is taken from the GPU's output.  The solves pass maxRestarts = 100 and must report SUCCESS: the restatement needs at most 24."""
import ctypes

import numpy as np
import pytest
import svds_cases as cases
import torch
from device_views import assert_guards_intact, carve, carve_like, fit, snapshot

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS, MAX_ITERATIONS_REACHED = 0, 2
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def make(smm, case):
    rows, cols, csr = case
    return smm.CSRMatrix(rows, cols, *csr)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def orth_loss(Q):
    Q = np.asarray(Q, dtype=np.float64)
    return float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))))


def check_values(s, sigma, k, tol):
    err = float(np.max(np.abs(s.astype(np.float64) - sigma[:k])))
    print("values: err", err, "bound", 10 * tol * float(sigma[0]))
    assert err <= 10 * tol * float(sigma[0])


def check_triplets(a64, sigma, U, s, V, info, k, dtype, tol):
    """test 1 of the issue on one solve; prints every figure before it asserts"""
    eps = float(np.finfo(dtype).eps)
    norm_a = float(sigma[0])
    s64, U64, V64 = s.astype(np.float64), np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    err = float(np.max(np.abs(s64 - sigma[:k])))
    res = float(max(np.max(np.linalg.norm(a64 @ V64 - U64 * s64, axis=0)), np.max(np.linalg.norm(a64.T @ U64 - V64 * s64, axis=0))))
    orth = max(orth_loss(U64), orth_loss(V64))
    allowed = 4 * cases.ORTH_LOSS_EPS[np.dtype(dtype)] * eps
    rho = float(np.max(info.residuals))
    print("status", int(info.status), "restarts", info.restarts, "matvecs", info.matvecs, "nconv", info.nconv, "| err", err, "res", res, "bound",
          10 * tol * norm_a, "| orth / eps", orth / eps, "bound / eps", allowed / eps, "| rho", rho, "bound", tol * norm_a)
    assert int(info.status) == SUCCESS and info.nconv == k
    assert s.dtype == dtype and U64.shape == (a64.shape[0], k) and V64.shape == (a64.shape[1], k)
    assert err <= 10 * tol * norm_a
    assert res <= 10 * tol * norm_a
    assert rho <= tol * norm_a
    assert np.all(np.diff(s64) < 0)
    assert orth <= allowed


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,k,ncv", cases.combos(), ids=_ID)
def test_triplets_order_and_counts(smm, name, k, ncv, dtype):
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    U, s, V, info = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS)
    check_triplets(cases.dense(name), cases.exact(name), U, s, V, info, k, dtype, tol)
    l = k + (ncv - k) // 2
    assert info.matvecs == 2 * (ncv + info.restarts * (ncv - l))  # no breakdown on these matrices
    assert 0 < info.restarts <= cases.MAX_RESTARTS


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_same_bits_twice_and_another_seed(smm, dtype):
    name, k, ncv = "grad2d_33x29", 4, 20
    tol = cases.TOL[np.dtype(dtype)]
    A = make(smm, cases.matrix(name, dtype))
    first = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=7)
    again = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=7)
    for i in range(3):
        assert np.array_equal(bits(first[i]), bits(again[i])), i
    assert first[3].restarts == again[3].restarts and np.array_equal(bits(first[3].residuals), bits(again[3].residuals))
    other = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, seed=8)
    assert not np.array_equal(bits(first[2]), bits(other[2]))  # another start vector
    for _, s, _, info in (first, other):
        assert int(info.status) == SUCCESS
        check_values(s, cases.exact(name), k, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_the_transpose_convention(smm, dtype):
    """a kept `at`, at=None and -- on a square matrix -- at built by transpose(): the same bits; svds(A^T) exchanges U and V"""
    k, ncv = 4, 20
    tol = cases.TOL[np.dtype(dtype)]
    for case in (cases.matrix("tall", dtype), cases.lsqr_cases.matrix("convdiff2d_12", dtype)):
        A = make(smm, case)
        At = A.transpose()
        built = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS)
        kept = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, at=At)
        again = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, at=At)  # the handle is kept across calls
        for other in (kept, again):
            for i in range(3):
                assert np.array_equal(bits(built[i]), bits(other[i])), i
            assert built[3].restarts == other[3].restarts and int(other[3].status) == SUCCESS
    sigma = cases.exact("tall")
    U, s, V, info = smm.svds(make(smm, cases.matrix("tall", dtype)), k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS)
    Ut, st, Vt, info_t = smm.svds(make(smm, cases.matrix("wide", dtype)), k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS)
    assert int(info.status) == int(info_t.status) == SUCCESS
    check_values(s, sigma, k, tol)
    check_values(st, sigma, k, tol)
    # The vectors of a simple singular value are fixed up to sign; each solve's are within sqrt(2) residual / gap of the exact ones (the
    # sin-theta theorem, gap: the distance to the nearest other singular value), the residual is at most 10 tol |A| by the bound above, and
    # two solves are compared: 2 sqrt(2) < 4.
    gap = float(np.min(-np.diff(sigma[:k + 1])))
    for i in range(k):
        for mine, theirs in ((U[:, i], Vt[:, i]), (V[:, i], Ut[:, i])):
            d = min(np.linalg.norm(mine.astype(np.float64) - theirs), np.linalg.norm(mine.astype(np.float64) + theirs))
            assert d <= 4 * 10 * tol * float(sigma[0]) / gap, (i, d)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_stream_against_pattern_and_auto(smm, dtype):
    """both handles forced to STREAM at one lane per row, to PATTERN (where the analysis takes them; a refusal is printed) and left to
    AUTO: the values agree with numpy's to the bound"""
    name, k, ncv = "grad2d_16x12", 4, 20
    tol = cases.TOL[np.dtype(dtype)]
    ran = []
    for family, lanes in (("AUTO", 0), ("STREAM", 1), ("PATTERN", 1)):
        A = make(smm, cases.matrix(name, dtype))
        At = A.transpose()
        if family != "AUTO":
            try:
                A.set_kernel(getattr(smm, "SPMV_" + family), lanes)
                At.set_kernel(getattr(smm, "SPMV_" + family), lanes)
            except smm.SmmHipError as e:
                assert family == "PATTERN", (family, str(e))
                print(name, family, "refused:", e)
                continue
        U, s, V, info = smm.svds(A, k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, at=At)
        print(family, np.dtype(dtype).name, "restarts", info.restarts)
        assert int(info.status) == SUCCESS
        check_values(s, cases.exact(name), k, tol)
        ran.append(family)
    assert "AUTO" in ran and "STREAM" in ran


RANK3 = np.array([3.0, 2.0, 1.0]) * np.sqrt(80.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_identity_over_zero(smm, dtype):
    """[I_50; 0]: every start vector is a singular vector, so beta-breakdowns with fresh vectors"""
    eps = float(np.finfo(dtype).eps)
    U, s, V, info = smm.svds(make(smm, cases.identity_over_zero(dtype)), 3, ncv=8)
    print(s, info)
    assert int(info.status) == SUCCESS and info.nconv == 3
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
    assert float(np.max(np.abs(s.astype(np.float64) - 1.0))) <= 4 * eps
    assert orth_loss(U) <= 100 * eps and orth_loss(V) <= 100 * eps


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_rank_three(smm, dtype):
    """three disjoint constant blocks: the Krylov space is exhausted after three steps"""
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.blocks_rank3(dtype))
    U, s, V, info = smm.svds(A, 3, ncv=8)
    print(s, info)
    assert int(info.status) == SUCCESS and info.nconv == 3
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
    assert float(np.max(np.abs(s.astype(np.float64) - RANK3))) <= 10 * eps * RANK3[0]
    assert orth_loss(U) <= 100 * eps and orth_loss(V) <= 100 * eps
    assert float(np.max(np.abs(V[24:].astype(np.float64)))) <= 100 * eps  # supported on the blocks' columns
    # rank below k: the outcome, not the branch
    U, s, V, info = smm.svds(A, 4, ncv=8, max_restarts=5)
    print(s, info)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V)) and np.all(np.isfinite(info.residuals))
    assert float(np.max(np.abs(s[:3].astype(np.float64) - RANK3))) <= 10 * eps * RANK3[0]
    if int(info.status) == SUCCESS:
        assert float(s[3]) <= 100 * eps * float(s[0])
    else:
        assert int(info.status) == MAX_ITERATIONS_REACHED and info.nconv == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_breakdown_invariant_subspace_of_the_start_vector(smm, dtype):
    """diag(1..192) from a v0 on rows 3, 50 and 100: the method cannot leave that subspace, as documented -- [101, 51]"""
    eps = float(np.finfo(dtype).eps)
    A = make(smm, cases.diagonal(np.arange(1.0, 193.0), dtype))
    v0 = np.zeros(192, dtype=dtype)
    v0[[3, 50, 100]] = [1.0, 2.0, 3.0]
    U, s, V, info = smm.svds(A, 2, v0=v0)
    print(s, info)
    assert int(info.status) == SUCCESS and info.nconv == 2 and info.restarts == 0
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
    assert float(np.max(np.abs(s.astype(np.float64) - [101.0, 51.0]))) <= 10 * eps * 101.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_device_pointers_on_offset_views_and_another_stream(smm, dtype):
    """smm_hip_svds_dev_* on a stream of the caller's: the start vector, the values and both factors at element alignment inside larger
    buffers with guard bands, ldu = rows + 1, ldv = cols + 3; then U = NULL, V = NULL and both: the same values, nothing else touched"""
    name, k, ncv = "grad2d_16x12", 4, 20
    tol = cases.TOL[np.dtype(dtype)]
    rows, cols, csr = cases.matrix(name, dtype)
    ldu, ldv = rows + 1, cols + 3
    v0 = np.random.default_rng(3).uniform(-1, 1, cols).astype(dtype)
    d_v0 = carve_like(v0, fit(1, dtype), device="cuda:0")
    saved = snapshot(d_v0)
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    A = smm.CSRMatrix.from_device(rows, cols, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    full = None
    for with_u, with_v in ((True, True), (False, True), (True, False), (False, False)):
        d_s = carve(k, dtype, fit(3, dtype), device="cuda:0")
        d_U = carve(k * ldu, dtype, fit(1, dtype), device="cuda:0")
        d_V = carve(k * ldv, dtype, fit(3, dtype), device="cuda:0")
        torch.cuda.synchronize()
        info = host.svds_dev(A, k, d_s, d_U if with_u else None, ldu, d_V if with_v else None, ldv, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, d_v0=d_v0,
                             stream=stream.cuda_stream)
        torch.cuda.synchronize()
        s = d_s.cpu().numpy()
        gu, gv = d_U.view(k, ldu).cpu().numpy(), d_V.view(k, ldv).cpu().numpy()
        assert int(info.status) == SUCCESS
        if with_u and with_v:
            check_triplets(cases.dense(name), cases.exact(name), gu[:, :rows].T, s, gv[:, :cols].T, info, k, dtype, tol)
            full = (s, gu, gv, info.restarts)
        else:
            assert np.array_equal(bits(s), bits(full[0])) and info.restarts == full[3]
        for grid, n, formed, want in ((gu, rows, with_u, full[1]), (gv, cols, with_v, full[2])):
            if formed:
                assert np.array_equal(bits(grid[:, :n]), bits(want[:, :n])) and np.all(np.isnan(grid[:, n:]))
            else:
                assert np.all(np.isnan(grid))  # the factor that was not asked for is not touched
        assert np.array_equal(snapshot(d_v0).cpu().numpy(), saved.cpu().numpy())
        for view, label in ((d_v0, "v0"), (d_s, "s"), (d_U, "U"), (d_V, "V")):
            assert_guards_intact(view, label)
    # the host-array form from the same start vector: the same library, the same launches, the same bits
    _, s, _, again = smm.svds(make(smm, (rows, cols, csr)), k, ncv=ncv, tol=tol, max_restarts=cases.MAX_RESTARTS, v0=v0)
    assert again.restarts == full[3] and np.array_equal(bits(s), bits(full[0]))


def test_refusals_and_edges_leave_the_outputs_untouched(smm):
    """every SMM_HIP_ERR_INVALID condition of the contract, through the C ABI; the message starts with "svds:" """
    lib = _lib.load()
    P = ctypes.c_void_p
    A = make(smm, cases.matrix("tall", np.float64))  # 168 x 144
    At = A.transpose()
    A32 = make(smm, cases.matrix("tall", np.float32))
    At32 = A32.transpose()
    Same = make(smm, cases.matrix("tall", np.float64))  # 168 x 144 where 144 x 168 is wanted
    fewer = cases.matrix("wide", np.float64)[2]
    fewer = (fewer[0].copy(), fewer[1][:-1].copy(), fewer[2][:-1].copy())
    fewer[0][-1] -= 1
    Fewer = smm.CSRMatrix(144, 168, *fewer)  # the transpose's shape with one entry less
    tiny = make(smm, cases.diagonal(np.ones(3), np.float64))
    s = np.full(8, 7.0)
    U = np.full(8 * 168, 7.0)
    V = np.full(8 * 144, 7.0)
    res = np.full(8, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(4)]

    def call(a, at, k, ncv, restarts, s_arr=s, u_arr=U, ldu=168, v_arr=V, ldv=144):
        ptr = lambda x: None if x is None else x.ctypes.data_as(P)  # noqa: E731
        return lib.smm_hip_svds_f64(a, at, k, ncv, restarts, 0.0, None, 0, ptr(s_arr), ptr(u_arr), ldu, ptr(v_arr), ldv, res.ctypes.data_as(P),
                                    *[ctypes.byref(i) for i in ints])

    refused = [
        ("null matrix", lambda: call(None, None, 2, 0, 10)),
        ("dtype", lambda: call(A32._h, None, 2, 0, 10)),
        ("at of the other dtype", lambda: call(A._h, At32._h, 2, 0, 10)),
        ("at of another shape", lambda: call(A._h, Same._h, 2, 0, 10)),
        ("at with another entry count", lambda: call(A._h, Fewer._h, 2, 0, 10)),
        ("a as at, not square", lambda: call(A._h, A._h, 2, 0, 10)),
        ("k < 0", lambda: call(A._h, None, -1, 0, 10)),
        ("restarts", lambda: call(A._h, None, 2, 0, -1)),
        ("k > min(rows, cols) - 2", lambda: call(A._h, None, 143, 0, 10)),
        ("k > min(rows, cols) - 2, tiny", lambda: call(tiny._h, None, 2, 0, 10)),
        ("ncv < k + 2", lambda: call(A._h, None, 4, 5, 10)),
        ("ncv > 64", lambda: call(A._h, None, 4, 65, 10)),
        ("ncv > min(rows, cols)", lambda: call(tiny._h, None, 1, 4, 10)),
        ("null singular_values", lambda: call(A._h, None, 2, 0, 10, s_arr=None)),
        ("ldu < rows", lambda: call(A._h, None, 2, 0, 10, ldu=167)),
        ("ldv < cols", lambda: call(A._h, None, 2, 0, 10, ldv=143)),
    ]
    for label, fn in refused:
        assert fn() == INVALID, label
        assert lib.smm_hip_last_error().decode().startswith("svds:"), (label, lib.smm_hip_last_error())
        assert np.all(s == 7.0) and np.all(U == 7.0) and np.all(V == 7.0) and np.all(res == 7.0) and all(i.value == -5 for i in ints), label
    # the device-pointer form refuses the same way
    assert lib.smm_hip_svds_dev_f64(A._h, None, 4, 5, 10, 0.0, None, 0, None, None, 168, None, 144, None, None, None, None, None, None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("svds:")
    # ldu and ldv are not looked at without the factor
    assert call(A._h, At._h, 2, 0, 2, u_arr=None, ldu=0, v_arr=None, ldv=0) == 0 and ints[1].value == 2 and np.all(U == 7.0) and np.all(V == 7.0)
    s[:] = 7.0
    res[:] = 7.0
    # degenerate, not refused: k == 0 and an empty matrix report SUCCESS and touch nothing else
    no_rows = smm.CSRMatrix(0, 5, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    no_cols = smm.CSRMatrix(5, 0, np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    for handle, k in ((A._h, 0), (no_rows._h, 3), (no_cols._h, 3)):
        for i in ints:
            i.value = -5
        assert call(handle, None, k, 0, 10) == 0
        assert [i.value for i in ints] == [0, 0, 0, 0] and np.all(s == 7.0) and np.all(U == 7.0) and np.all(V == 7.0) and np.all(res == 7.0)
    # k == min(rows, cols) - 2 with ncv == min(rows, cols) is the edge that is allowed; `a` as `at` is legal on a square matrix
    _, s3, _, info = smm.svds(tiny, 1, ncv=3, at=tiny)
    assert int(info.status) == SUCCESS and abs(float(s3[0]) - 1.0) <= 1e-15


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_norm2(smm, dtype):
    tol = cases.TOL[np.dtype(dtype)]
    for name in ("tall", "grad2d_16x12"):
        A = make(smm, cases.matrix(name, dtype))
        sigma = cases.exact(name)
        _, s, _, info = smm.svds(A, 1, tol=tol, vectors=False)
        norm = A.norm2(tol=tol)
        print(name, np.dtype(dtype).name, "norm2", norm, "sigma_0", float(sigma[0]), "restarts", info.restarts)
        assert int(info.status) == SUCCESS and norm == float(s[0])
        assert abs(norm - float(sigma[0])) <= 10 * tol * float(sigma[0])
