"""The generalised lobpcg (A x = lambda B x) on the GPU (csrc/smm_solvers_lobpcg.hip) and the two several-bases kernels it runs on
(multi_block_axpy_bases: csrc/smm_multiblock.h, multi_rotate_bases: csrc/smm_multivec.h), through the C ABI, the Python binding and the
device-pointer form (the drop-in C++ header: tests/test_cpp_lobpcg_gen.py).  The cases are those of tests/lobpcg_gen_cases.py; the
reference is dense numpy: the Cholesky factor of B, then eigh(L^-1 A L^-T).  Bounds, with |lambda| = max|lambda_i| and tol = 1e-10
(fp64) / 1e-4 (fp32):
  |theta_i - lambda_i| <= 10 tol |lambda|;  ||A x_i - theta_i B x_i||_2 <= 10 tol |lambda| ||B x_i||_2 (formed in fp64 on the host);
  max|X^T B X - I| <= 4 ORTH_WORST eps, ORTH_WORST the worst ratio of the CPU restatement (tests/lobpcg_gen_cases.py: 140 in fp64, 5.5
  in fp32) and 4 the allowance tests/test_gpu_lobpcg.py gives another summation order.  None of them is tuned to the code under test.
The solves pass maxIterations = 1000 and must report SUCCESS: the restatement needs at most 347 iterations on these cases.
The several-bases kernels are compared bit for bit with their single-basis entries on copies."""
import ctypes

import lobpcg_gen_cases as cases
import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, carve, fit
from lobpcg_restatement import start_block

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS, DIVERGED = 0, 1
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_DENSE = {}


def dense_pair(name):
    if name not in _DENSE:
        _DENSE[name] = tuple(cases.dense(m) for m in cases.pair(name, np.float64))
        for m in _DENSE[name]:
            m.setflags(write=False)
    return _DENSE[name]


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


def make_pair(smm, name, dtype):
    a, b = cases.pair(name, dtype)
    return make(smm, a), make(smm, b)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def check_pairs(name, w, X, info, k, which, dtype, tol, orth_bound=True):
    """the solver's bounds on one solve; prints every figure before it asserts"""
    a64, b64 = dense_pair(name)
    lam = cases.exact(name)
    norm = float(np.max(np.abs(lam)))
    eps = float(np.finfo(dtype).eps)
    w64, X64 = w.astype(np.float64), np.asarray(X, dtype=np.float64)
    BX = b64 @ X64
    err = float(np.max(np.abs(w64 - cases.wanted(lam, which, k))))
    res = float(np.max(np.linalg.norm(a64 @ X64 - BX * w64, axis=0) / np.linalg.norm(BX, axis=0)))
    orth = float(np.max(np.abs(X64.T @ BX - np.eye(k))))
    print("status", int(info.status), "iterations", info.iterations, "matvecs", info.matvecs, "bmatvecs", info.bmatvecs, "applies", info.applies, "nconv", info.nconv,
          "| err", err, "res", res, "bound", 10 * tol * norm, "| orth / eps", orth / eps, "bound", 4 * cases.ORTH_WORST[np.dtype(dtype)])
    assert int(info.status) == SUCCESS and info.nconv == k
    assert w.dtype == dtype and X.shape == (a64.shape[0], k)
    assert err <= 10 * tol * norm
    assert res <= 10 * tol * norm
    assert info.iterations <= cases.MAX_ITERATIONS
    assert info.bmatvecs == info.matvecs + k - 1  # 2k - 1 + the sum of |active| against k + the same sum
    if orth_bound:
        assert orth <= 4 * cases.ORTH_WORST[np.dtype(dtype)] * eps
    if k > 1:
        order = np.diff(w64)
        assert np.all(order <= 0) if which == "LA" else np.all(order >= 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k", cases.combos(), ids=_ID)
def test_eigenpairs_order_counts_and_b_orthonormality(smm, name, which, k, dtype):
    """Measured on an MI355X: the worst max|X^T B X - I| / eps over the cases is 12 in fp64 (shifted_33x29, SA, k = 4) and 5.7 in fp32
    (diag_33x29, SA, k = 4), against the bounds 560 and 22; at most 347 iterations in fp64 and 162 in fp32, the restatement's counts."""
    tol = cases.TOL[np.dtype(dtype)]
    A, B = make_pair(smm, name, dtype)
    w, X, info = smm.lobpcg(A, k, which, tol=tol, max_iterations=cases.MAX_ITERATIONS, B=B)
    check_pairs(name, w, X, info, k, which, dtype, tol)
    assert info.applies == 0 and k < info.matvecs <= k + k * info.iterations


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_same_bits_twice_the_hash_start_and_no_b(smm, dtype):
    name, k = "elasticity_8x6", 4
    tol = cases.TOL[np.dtype(dtype)]
    A, B = make_pair(smm, name, dtype)
    n = cases.ROWS[name]
    first = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=5, B=B)
    again = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=5, B=B)
    given = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, X0=start_block(n, k, 5, dtype), seed=99, B=B)
    assert int(first[2].status) == SUCCESS
    for other in (again, given):  # two runs, and the hash columns passed in as X0
        assert np.array_equal(bits(first[0]), bits(other[0])) and np.array_equal(bits(first[1]), bits(other[1]))
        assert first[2].iterations == other[2].iterations and np.array_equal(bits(first[2].residuals), bits(other[2].residuals))
    # b == NULL through the new entry: the bits and the counts of smm_hip_lobpcg_*
    plain = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=5)
    d_w = torch.zeros(k, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda:0")
    d_X = torch.zeros(k * n, dtype=d_w.dtype, device="cuda:0")
    info = host.lobpcg_gen_dev(A, None, k, "SA", d_w, d_X, n, tol=tol, max_iterations=cases.MAX_ITERATIONS, seed=5)
    assert np.array_equal(bits(plain[0]), bits(d_w.cpu().numpy())) and np.array_equal(bits(plain[1]), bits(d_X.view(k, n).cpu().numpy().T))
    assert info.bmatvecs == 0 and tuple(info[1:5]) == tuple(plain[2][1:5]) and np.array_equal(bits(info.residuals), bits(plain[2].residuals))
    assert type(plain[2]).__name__ == "LobpcgInfo" and type(first[2]).__name__ == "LobpcgGenInfo"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_edges(smm, dtype):
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    A, B = make_pair(smm, "chain_60", dtype)
    # B = a: every start block spans eigenvectors of the value 1 -- converged at iteration 0
    w, X, info = smm.lobpcg(A, 3, "SA", tol=tol, B=A)
    print(w, info)
    assert int(info.status) == SUCCESS and info.iterations == 0 and info.nconv == 3 and info.matvecs == 3 and info.bmatvecs == 5
    assert float(np.max(np.abs(w.astype(np.float64) - 1.0))) <= 4 * eps
    # B = -I: DIVERGED at the start, and the outputs are not written; two equal start columns likewise
    lib = _lib.load()
    P = ctypes.c_void_p
    n, k = 60, 3
    minus = make(smm, cases.diagonal(np.full(n, -1.0), dtype))
    X0 = start_block(n, k, 0, dtype)
    X0[:, 2] = X0[:, 0]
    fn = lib.smm_hip_lobpcg_gen_f32 if dtype == np.float32 else lib.smm_hip_lobpcg_gen_f64
    for b_handle, start in ((minus._h, None), (B._h, np.ascontiguousarray(X0.T))):
        wq, Xq, rq = np.full(k, 7.0, dtype=dtype), np.full(k * n, 7.0, dtype=dtype), np.full(k, 7.0, dtype=dtype)
        ints = [ctypes.c_int(-5) for _ in range(6)]
        rc = fn(A._h, b_handle, k, 1, 100, dtype(tol), None, None if start is None else start.ctypes.data_as(P), n, 0, wq.ctypes.data_as(P), Xq.ctypes.data_as(P), n,
                rq.ctypes.data_as(P), *[ctypes.byref(i) for i in ints])
        assert rc == 0 and ints[5].value == DIVERGED and ints[1].value == 0
        assert np.all(wq == 7.0) and np.all(Xq == 7.0) and np.all(rq == 7.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_device_pointers_on_offset_views_and_another_stream(smm, dtype):
    """smm_hip_lobpcg_gen_dev_* on a stream of the caller's: the eigenvalues and the eigenvectors at element alignment inside larger
    buffers with guard bands, ldx = rows + 1; the elements between the vectors keep their NaN"""
    name, k, which = "elasticity_3x3x3", 6, "SA"
    tol = cases.TOL[np.dtype(dtype)]
    n = cases.ROWS[name]
    ldx = n + 1
    d_w = carve(k, dtype, fit(3, dtype), device="cuda:0")
    d_X = carve(k * ldx, dtype, fit(1, dtype), device="cuda:0")
    A, B = make_pair(smm, name, dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    info = host.lobpcg_gen_dev(A, B, k, which, d_w, d_X, ldx, tol=tol, max_iterations=cases.MAX_ITERATIONS, stream=s.cuda_stream)
    torch.cuda.synchronize()
    grid = d_X.view(k, ldx).cpu().numpy()
    check_pairs(name, d_w.cpu().numpy(), grid[:, :n].T, info, k, which, dtype, tol)
    assert np.all(np.isnan(grid[:, n:]))
    for view, label in ((d_w, "w"), (d_X, "X")):
        assert_guards_intact(view, label)
    w, X, again = smm.lobpcg(A, k, which, tol=tol, max_iterations=cases.MAX_ITERATIONS, B=B)  # the host-array form: the same launches, the same bits
    assert again.iterations == info.iterations and np.array_equal(bits(w), bits(d_w.cpu().numpy()))


PRECOND_KINDS = {"JACOBI": "JACOBI", "SGS": "SYMMETRIC_GAUS_SEIDEL", "IC0": "IC0", "FSAI": "FSAI", "AMG": "AMG"}


def test_preconditioners_of_a(smm):
    """diag_33x29, SA, k = 4, fp64: every symmetric kind, built for A, meets the bounds; SGS and IC0 take strictly fewer iterations than
    none (tests/test_lobpcg_gen_cpu.py shows the same of the restatement with a numpy IC0)"""
    name, k, dtype, tol = "diag_33x29", 4, np.float64, 1e-10
    A, B = make_pair(smm, name, dtype)
    plain = smm.lobpcg(A, k, "SA", tol=tol, max_iterations=cases.MAX_ITERATIONS, B=B)[2]
    counts = {"none": plain.iterations}
    for kind, enum_name in PRECOND_KINDS.items():
        M = A.getPreconditioner(enum_name)
        w, X, info = smm.lobpcg(A, k, "SA", M=M, tol=tol, max_iterations=cases.MAX_ITERATIONS, B=B)
        print(kind, end=" ")
        check_pairs(name, w, X, info, k, "SA", dtype, tol, orth_bound=False)
        assert info.applies > 0 and info.matvecs == k + info.applies
        counts[kind] = info.iterations
    print("iterations", counts)
    assert counts["SGS"] < counts["none"] and counts["IC0"] < counts["none"]


def test_refusals_leave_the_outputs_untouched(smm):
    """every SMM_HIP_ERR_INVALID condition of smm_hip_lobpcg_gen_*, through the C ABI"""
    lib = _lib.load()
    P = ctypes.c_void_p
    A, B = make_pair(smm, "chain_60", np.float64)
    A32, B32 = make_pair(smm, "chain_60", np.float32)
    start = np.array([0, 1, 2], dtype=np.int32)
    wide = smm.CSRMatrix(2, 3, start, np.array([0, 1], dtype=np.int32), np.array([1.0, 1.0]))
    tiny = make(smm, cases.diagonal(np.ones(5), np.float64))
    other = make(smm, cases.pair("elasticity_8x6", np.float64)[1])
    M_ilu = A.getPreconditioner("ILU0")          # a kind CG refuses
    M_size = other.getPreconditioner("JACOBI")   # fits B's relative, not `a`
    M_32 = A32.getPreconditioner("JACOBI")
    w, X, res, X0 = np.full(8, 7.0), np.full(8 * 60, 7.0), np.full(8, 7.0), np.ones(8 * 60)
    ints = [ctypes.c_int(-5) for _ in range(6)]

    def call(a, b, k, which, its, M=None, x0=None, ldx0=60, w_arr=w, ldx=60):
        return lib.smm_hip_lobpcg_gen_f64(a, b, k, which, its, 0.0, None if M is None else M._h, None if x0 is None else x0.ctypes.data_as(P), ldx0, 0,
                                          None if w_arr is None else w_arr.ctypes.data_as(P), X.ctypes.data_as(P), ldx, res.ctypes.data_as(P),
                                          *[ctypes.byref(i) for i in ints])

    refused = [
        ("null matrix", lambda: call(None, B._h, 2, 1, 10)),
        ("dtype", lambda: call(A32._h, B32._h, 2, 1, 10)),
        ("not square", lambda: call(wide._h, B._h, 1, 1, 10)),
        ("k < 0", lambda: call(A._h, B._h, -1, 1, 10)),
        ("k > 8", lambda: call(A._h, B._h, 9, 1, 10)),
        ("3k > rows", lambda: call(tiny._h, tiny._h, 2, 1, 10)),
        ("which", lambda: call(A._h, B._h, 2, 2, 10)),
        ("maxIterations", lambda: call(A._h, B._h, 2, 1, -1)),
        ("null eigenvalues", lambda: call(A._h, B._h, 2, 1, 10, w_arr=None)),
        ("ldx < rows", lambda: call(A._h, B._h, 2, 1, 10, ldx=59)),
        ("ldx0 < rows", lambda: call(A._h, B._h, 2, 1, 10, x0=X0, ldx0=59)),
        ("a kind CG refuses", lambda: call(A._h, B._h, 2, 1, 10, M=M_ilu)),
        ("a preconditioner of another size", lambda: call(A._h, B._h, 2, 1, 10, M=M_size)),
        ("a preconditioner of the other dtype", lambda: call(A._h, B._h, 2, 1, 10, M=M_32)),
        ("b of the other dtype", lambda: call(A._h, B32._h, 2, 1, 10)),
        ("b not square", lambda: call(A._h, wide._h, 2, 1, 10)),
        ("b of other rows", lambda: call(A._h, other._h, 2, 1, 10)),
        ("b of other rows, k == 0", lambda: call(A._h, other._h, 0, 1, 10)),
    ]
    for label, fn in refused:
        assert fn() == INVALID, label
        assert lib.smm_hip_last_error().decode().startswith("lobpcg:"), (label, lib.smm_hip_last_error())
        assert np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0) and all(i.value == -5 for i in ints), label
    # the device-pointer form refuses the same way
    assert lib.smm_hip_lobpcg_gen_dev_f64(A._h, other._h, 2, 1, 10, 0.0, None, None, 0, 0, None, None, 60, None, None, None, None, None, None, None, None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    # degenerate, not refused: k == 0 reports SUCCESS and touches nothing else
    assert call(A._h, B._h, 0, 1, 10) == 0
    assert [i.value for i in ints] == [0, 0, 0, 0, 0, 0] and np.all(w == 7.0) and np.all(X == 7.0) and np.all(res == 7.0)


# ---- the two several-bases kernels ----
BASES_N = (0, 1, 63, 64, 65, 257, 4099)
AXPY_ML = ((1, 1), (8, 8), (16, 8), (24, 24))
ROTATE_ML = ((2, 1), (17, 8), (24, 16), (33, 4))  # (33, 4): the padding 64, where a lane owns one row whatever the alignment
LAYOUTS = ("aligned", "odd_ld", "second_offset")


def _basis(n, cols, ld, dtype, residue, rng):
    """`cols` columns of n elements inside a guarded buffer of cols * ld NaNs"""
    d = carve(cols * ld, dtype, residue, device="cuda:0")
    if n:
        d.view(cols, ld)[:, :n] = torch.from_numpy(np.ascontiguousarray(rng.uniform(-1, 1, (cols, n)).astype(dtype))).to("cuda:0")
    return d


def _layout(n, layout, i, dtype):
    """aligned: every basis on a 16-byte boundary, ld = n rounded up to 64; odd_ld: the same bases with an odd ld; second_offset: the
    second basis one element past a boundary, so that the bases of one launch differ in alignment"""
    ld = max(64, (n + 63) // 64 * 64) + (1 if layout == "odd_ld" else 0)
    return ld, (fit(1, dtype) if layout == "second_offset" and i == 1 else 0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("m,l", AXPY_ML, ids=_ID)
def test_multi_block_axpy_bases(smm, m, l, dtype, layout):
    """each pair bit for bit what multi_block_axpy_dev makes of a copy of it; V unchanged; guards and the elements between n and ld intact"""
    rng = np.random.default_rng(300 * m + l)
    H = torch.from_numpy(rng.uniform(-1, 1, (l, m)).astype(dtype)).to("cuda:0")  # column c of H is row c here: ldH = m
    for n in BASES_N:
        for nb in (1, 2, 3):
            lds = [_layout(n, layout, i, dtype) for i in range(nb)]
            ld = lds[0][0]
            V = [_basis(n, m, ld, dtype, residue, rng) for _, residue in lds]
            W = [_basis(n, l, ld, dtype, residue, rng) for _, residue in lds]
            v_before = [v.clone() for v in V]
            want = []
            for v, wv in zip(V, W):  # the single-basis entry on a copy laid out the same way
                copy = carve(l * ld, dtype, wv.data_ptr() % 16 // wv.element_size(), device="cuda:0")
                copy.copy_(wv)
                host.multi_block_axpy_dev(n, m, l, v, ld, H, m, copy, ld, dtype)
                want.append(copy)
            host.multi_block_axpy_bases_dev(n, m, l, V, ld, H, m, W, ld, dtype)
            torch.cuda.synchronize()
            for i in range(nb):
                got, ref = W[i].cpu().numpy(), want[i].cpu().numpy()
                assert np.array_equal(bits(got), bits(ref)), (n, nb, i)
                assert np.all(np.isnan(got.reshape(l, ld)[:, n:])) and not np.any(np.isnan(got.reshape(l, ld)[:, :n])), (n, nb, i)
                assert np.array_equal(bits(V[i].cpu().numpy()), bits(v_before[i].cpu().numpy())), (n, nb, i)
                assert_guards_intact(V[i], f"V[{i}] n={n}")
                assert_guards_intact(W[i], f"W[{i}] n={n}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("m,l", ROTATE_ML, ids=_ID)
def test_multi_rotate_bases(smm, m, l, dtype, layout):
    """each basis bit for bit what multi_rotate_dev makes of a copy of it; guards and the elements between n and ld intact"""
    rng = np.random.default_rng(400 * m + l)
    Y = rng.uniform(-1, 1, (m, l)).astype(dtype)
    for n in BASES_N:
        for nb in (1, 2, 3):
            lds = [_layout(n, layout, i, dtype) for i in range(nb)]
            ld = lds[0][0]
            V = [_basis(n, m, ld, dtype, residue, rng) for _, residue in lds]
            want = []
            for v in V:
                copy = carve(m * ld, dtype, v.data_ptr() % 16 // v.element_size(), device="cuda:0")
                copy.copy_(v)
                host.multi_rotate_dev(n, m, l, copy, ld, Y, dtype)
                want.append(copy)
            host.multi_rotate_bases_dev(n, m, l, V, ld, Y, dtype)
            torch.cuda.synchronize()
            for i in range(nb):
                got, ref = V[i].cpu().numpy(), want[i].cpu().numpy()
                assert np.array_equal(bits(got), bits(ref)), (n, nb, i)
                assert np.all(np.isnan(got.reshape(m, ld)[:, n:])) and not np.any(np.isnan(got.reshape(m, ld)[:, :n])), (n, nb, i)
                assert_guards_intact(V[i], f"V[{i}] n={n}")


def test_bases_refusals(smm):
    """the INVALID table of the two entries on real device pointers; nothing is touched"""
    lib = _lib.load()
    P = ctypes.c_void_p
    d = [torch.full((64 * 4,), 3.0, dtype=torch.float64, device="cuda:0") for _ in range(6)]
    g = torch.full((16,), 3.0, dtype=torch.float64, device="cuda:0")
    y = np.ones(16)
    yp = y.ctypes.data_as(P)

    def array(*items):
        return (P * len(items))(*[None if t is None else t.data_ptr() if hasattr(t, "data_ptr") else t for t in items])

    v, ww, gp = d[:3], d[3:], host._dptr(g)
    axpy, rot = lib.smm_hip_multi_block_axpy_bases_dev_f64, lib.smm_hip_multi_rotate_bases_dev_f64
    for n, m, l, nb, ldv, ldw, ldh in ((-1, 4, 4, 3, 64, 64, 4), (64, 0, 4, 3, 64, 64, 4), (64, 4, 0, 3, 64, 64, 4), (64, 25, 1, 3, 64, 64, 25), (64, 1, 25, 3, 64, 64, 1),
                                       (64, 4, 4, 3, 63, 64, 4), (64, 4, 4, 3, 64, 63, 4), (64, 4, 4, 3, 64, 64, 3), (64, 4, 4, 0, 64, 64, 4), (64, 4, 4, 4, 64, 64, 4)):
        assert axpy(n, m, l, nb, array(*v, v[0]), ldv, gp, ldh, array(*ww, ww[0]), ldw, None) == INVALID, (n, m, l, nb, ldv, ldw, ldh)
        assert lib.smm_hip_last_error().decode().startswith("multi_block_axpy_bases:")
    for vs, ws, h in ((None, array(*ww), gp), (array(*v), None, gp), (array(*v), array(*ww), None), (array(v[0], None, v[2]), array(*ww), gp),
                      (array(*v), array(ww[0], ww[1], None), gp), (array(*v), array(ww[0], ww[1], v[0]), gp), (array(*v), array(ww[0], v[2].data_ptr() + 8 * 255, ww[2]), gp)):
        assert axpy(64, 4, 4, 3, vs, 64, h, 4, ws, 64, None) == INVALID
        assert lib.smm_hip_last_error().decode().startswith("multi_block_axpy_bases:")
    for n, m, l, nb, ld, ldy in ((-1, 4, 4, 3, 64, 4), (64, 4, 0, 3, 64, 4), (64, 3, 4, 3, 64, 4), (64, 65, 4, 3, 64, 65), (64, 4, 4, 3, 63, 4), (64, 4, 4, 3, 64, 3),
                                 (64, 4, 4, 0, 64, 4), (64, 4, 4, 4, 64, 4)):
        assert rot(n, m, l, nb, array(*v, v[0]), ld, yp, ldy, None) == INVALID, (n, m, l, nb, ld, ldy)
        assert lib.smm_hip_last_error().decode().startswith("multi_rotate_bases:")
    for vs, yy in ((None, yp), (array(*v), None), (array(v[0], v[1], None), yp)):
        assert rot(64, 4, 4, 3, vs, 64, yy, 4, None) == INVALID
        assert lib.smm_hip_last_error().decode().startswith("multi_rotate_bases:")
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in d) and bool((g == 3.0).all())
