"""The sparse product on the device (csrc/smm_spgemm.hip) through the C ABI: smm_hip_csr_multiply_create / _multiply_into_*.  The
reference is the CPU definition (tests/spgemm_restatement.py): the pattern exactly, and in the default flavour the value BITS; the
SMM_WITH_STD_FMA flavour within spgemm_restatement.bound.  The SpMV-column rule holds bit for bit in both flavours."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import spgemm_cases as cases
import torch
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from spgemm_restatement import bound, dense, spgemm

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
STREAM, PATTERN = 2, 3
JACOBI = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def make(smm, csr, shape):
    return smm.CSRMatrix(shape[0], shape[1], *csr)


def arrays(M):
    start, pos = M.get_pattern()
    return start, pos, M.get_values()


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what} start")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what} positions")
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg=f"{what} value bits")


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(a, b, (m, k, n), the restatement's product), computed once per session and never written to"""
    build = {"small_rectangular": cases.small_rectangular, "cancellation": cases.cancellation, "order": cases.order_cases,
             "every_bin": cases.every_bin, "long_row_a": lambda d: cases.long_row(d, "a"), "long_row_b": lambda d: cases.long_row(d, "b"),
             "spmv_column": cases.spmv_column}[name]
    a, b, shape = build(dtype)
    want = spgemm(a, b, shape[2])
    for arr in (*a, *b, *want):
        arr.setflags(write=False)
    return a, b, shape, want


def product(smm, name, dtype):
    a, b, (m, k, n), want = case(name, dtype)
    A, B = make(smm, a, (m, k)), make(smm, b, (k, n))
    return A, B, A @ B, want


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_small_rectangular(smm, dtype):
    """empty rows in A, rows of B that are empty but referenced, an empty column, stored zeros in A; csr_info as csr_create reports it"""
    A, B, C, want = product(smm, "small_rectangular", dtype)
    assert (C.rows, C.cols, C.nnz, C.dtype) == (37, 29, len(want[1]), np.dtype(dtype))
    assert_same(arrays(C), want)
    assert want[0][4] == want[0][3] and 11 not in want[1]  # (the case holds what it says: an empty row, an empty column)
    F = make(smm, want, (37, 29))
    assert (C.first_active_start, C.get_kernel()) == (F.first_active_start, F.get_kernel())
    A.close()
    B.close()  # the product does not depend on its factors' lifetime
    assert_same(arrays(C), want, "after the factors are gone")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_cancellation_keeps_the_entry(smm, dtype):
    _, _, C, want = product(smm, "cancellation", dtype)
    got = arrays(C)
    assert_same(got, want)
    np.testing.assert_array_equal(got[1][:3], [0, 2, 3])
    np.testing.assert_array_equal(bits(got[2][:3]), bits(np.zeros(3, dtype=dtype)))  # +v b - v b: a stored +0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_terms_are_summed_in_stored_order(smm, dtype):
    """(big, 1, -big) arriving at one entry across p in all six orders: the six results differ among themselves, each is the restatement's"""
    _, _, C, want = product(smm, "order", dtype)
    got = arrays(C)
    assert_same(got, want)
    telling = got[2][got[1] == cases.ORDER_COLUMN]
    assert len(telling) == 6 and len(set(telling.tolist())) > 1


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_every_bin(smm, dtype):
    """rows of A of 0, 1, 2, 3, 4, 2^q - 1, 2^q, 2^q + 1 ... 4095 entries against 4096 short rows of B: every symbolic and numeric bin,
    the thresholds between them, ub from 0 to beyond any LDS table"""
    _, _, C, want = product(smm, "every_bin", dtype)
    lens = np.diff(want[0])
    assert lens.min() == 0 and lens.max() > 4096 and np.any((lens > 32) & (lens <= 512)) and np.any((lens > 512) & (lens <= 4096))
    assert_same(arrays(C), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("form", ["a", "b"])
def test_the_long_row(smm, dtype, form):
    """(a) 120 000 distinct entries in one row; (b) ub = 120 000 with at most 4001 distinct columns"""
    _, _, C, want = product(smm, "long_row_" + form, dtype)
    assert want[0][1] == (120000 if form == "a" else 4001) and want[0][2] == want[0][1]
    assert_same(arrays(C), want)
    again = arrays(product(smm, "long_row_" + form, dtype)[2])
    assert_same(again, want, "second run")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_columns_are_the_spmv_of_the_dense_columns(smm, dtype):
    """dense(C)[:, j] == A.rMult(dense(B)[:, j]) with set_kernel(STREAM, 1), bit for bit (n = 13)"""
    A, _, C, _ = product(smm, "spmv_column", dtype)
    a, b, (m, k, n), _ = case("spmv_column", dtype)
    A.set_kernel(STREAM, 1)
    c, bd = dense(arrays(C), n), dense(b, n)
    for j in range(n):
        out = np.zeros(m, dtype=dtype)
        A.rMult(np.ascontiguousarray(bd[:, j]), out)
        np.testing.assert_array_equal(bits(c[:, j]), bits(out), err_msg=f"column {j}")


class FmaLibrary:
    """the SMM_WITH_STD_FMA flavour through raw ctypes (the package binds the default flavour)"""

    def __init__(self):
        _lib._share_hip_runtime_with_torch()
        self.lib = ctypes.CDLL(_lib.library_path(fma=True))
        self.lib.smm_hip_last_error.restype = ctypes.c_char_p
        assert self.lib.smm_hip_uses_std_fma() == 1
        assert self.lib.smm_hip_init(0) == 0, self.lib.smm_hip_last_error()

    @staticmethod
    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def create(self, csr, shape):
        h = ctypes.c_void_p()
        suf = "f32" if csr[2].dtype == np.float32 else "f64"
        assert getattr(self.lib, f"smm_hip_csr_create_{suf}")(shape[0], shape[1], self.ptr(csr[0]), self.ptr(csr[1]), self.ptr(csr[2]), ctypes.byref(h)) == 0
        return h

    def multiply(self, ha, hb, dtype):
        h = ctypes.c_void_p()
        assert self.lib.smm_hip_csr_multiply_create(ha, hb, None, ctypes.byref(h)) == 0, self.lib.smm_hip_last_error()
        r, c, nnz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert self.lib.smm_hip_csr_info(h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(nnz), None, None) == 0
        start, pos, val = np.zeros(r.value + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value, dtype=dtype)
        assert self.lib.smm_hip_csr_get_pattern(h, self.ptr(start), self.ptr(pos)) == 0
        assert getattr(self.lib, "smm_hip_csr_get_values_" + ("f32" if np.dtype(dtype) == np.float32 else "f64"))(h, self.ptr(val)) == 0
        self.lib.smm_hip_csr_destroy(h)
        return start, pos, val


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_fma_flavour(dtype):
    """libsmm_hip_fma.so: the pattern exactly, the values within terms * eps * sum |a||b| of the restatement, and the SpMV-column rule
    bit for bit against that library's own row sums"""
    fma = FmaLibrary()
    suf = "f32" if dtype == np.float32 else "f64"
    for name in ("small_rectangular", "every_bin", "spmv_column"):
        a, b, (m, k, n), want = case(name, dtype)
        ha, hb = fma.create(a, (m, k)), fma.create(b, (k, n))
        got = fma.multiply(ha, hb, dtype)
        np.testing.assert_array_equal(got[0], want[0], err_msg=name)
        np.testing.assert_array_equal(got[1], want[1], err_msg=name)
        assert np.all(np.abs(got[2].astype(np.float64) - want[2].astype(np.float64)) <= bound(a, b, n)), name
        if name == "spmv_column":
            assert fma.lib.smm_hip_csr_set_kernel(ha, STREAM, 1) == 0
            c, bd = dense(got, n), dense(b, n)
            for j in range(n):
                out = np.zeros(m, dtype=dtype)
                assert getattr(fma.lib, f"smm_hip_spmv_{suf}")(ha, 0, None, fma.ptr(np.ascontiguousarray(bd[:, j])), fma.ptr(out)) == 0
                np.testing.assert_array_equal(bits(c[:, j]), bits(out), err_msg=f"column {j}")
        fma.lib.smm_hip_csr_destroy(ha)
        fma.lib.smm_hip_csr_destroy(hb)


def spmv_bound(csr, x, dtype):
    """terms * eps * sum |a||x| per row: two summation orders of one row"""
    start, pos, val = csr
    rows = np.repeat(np.arange(len(start) - 1), np.diff(start))
    mass = np.bincount(rows, weights=np.abs(val.astype(np.float64)) * np.abs(x.astype(np.float64)[pos]), minlength=len(start) - 1)
    return np.diff(start) * float(np.finfo(dtype).eps) * mass


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["poisson2d_32", "banded"])
def test_at_times_a(smm, dtype, name):
    """At = A.transpose(), C = At @ A: symmetric in pattern and value bits, a matrix like any other"""
    csr = gen.poisson2d(32, dtype=dtype) if name == "poisson2d_32" else cases.banded_nonsymmetric(dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr, (n, n))
    At = A.transpose()
    C = At @ A
    assert C.isSymmetric() == (True, True)
    got = arrays(C)
    assert_same(got, spgemm(arrays(At), csr, n))
    rng = np.random.default_rng(59)
    x = rng.uniform(-1, 1, n).astype(dtype)
    y, z, w = (np.zeros(n, dtype=dtype) for _ in range(3))
    C.rMult(x, y)
    A.rMult(x, z)
    At.rMult(z, w)
    # C x against At (A x): each side is off the exact value by at most its own bound; the exact values agree.  Per row i of the exact
    # form: (terms of C's row sum + the products behind its entries) roundings of at most sum_j sum_p |at_ip||a_pj||x_j|
    absA = cases.to_scipy((csr[0], csr[1], np.abs(csr[2]).astype(np.float64)), (n, n))
    mass = absA.T @ (absA @ np.abs(x.astype(np.float64)))
    terms = 2 * (np.diff(got[0]).max() + np.diff(csr[0]).max() + np.diff(arrays(At)[0]).max())
    assert np.all(np.abs(y.astype(np.float64) - w.astype(np.float64)) <= terms * float(np.finfo(dtype).eps) * mass)
    M = C.getPreconditioner(JACOBI)
    assert M.values().shape == (n,)
    if name == "poisson2d_32":
        S = A @ A
        S.set_kernel(PATTERN, 1)
        assert S.pattern_info()[1] == 13
        out_p, out_s = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
        S.rMult(x, out_p)
        S.set_kernel(STREAM, 1)
        S.rMult(x, out_s)
        np.testing.assert_array_equal(bits(out_p), bits(out_s))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_multiply_into(smm, dtype):
    a, b, (m, k, n), want = case("small_rectangular", dtype)
    A, B = make(smm, a, (m, k)), make(smm, b, (k, n))
    C = A @ B
    kernel = C.get_kernel()
    # new values, same patterns: the bits of a fresh multiply
    A.scale(-1.5)
    vb = (np.asarray(b[2]) * np.linspace(0.5, 2.0, len(b[2]))).astype(dtype)
    B.set_values(vb)
    C.multiply_into(A, B)
    assert_same(arrays(C), arrays(A @ B), "after scale and set_values")
    assert_same(arrays(C), spgemm((a[0], a[1], (a[2] * dtype(-1.5)).astype(dtype)), (b[0], b[1], vb), n), "against the restatement")
    # sub-patterns of the factors: +0.0 where nothing lands any more
    keep = np.ones(len(a[1]), dtype=bool)
    keep[::3] = False
    rows = np.repeat(np.arange(m), np.diff(a[0]))
    a_sub = (np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32), a[1][keep], np.asarray(a[2])[keep])
    As = make(smm, a_sub, (m, k))
    C.multiply_into(As, B)
    sub = spgemm(a_sub, (b[0], b[1], vb), n)
    full = np.zeros(len(want[1]), dtype=dtype)
    rows_c = np.repeat(np.arange(m), np.diff(want[0]))
    rows_s = np.repeat(np.arange(m), np.diff(sub[0]))
    where = np.searchsorted(rows_c.astype(np.int64) * n + want[1], rows_s.astype(np.int64) * n + sub[1])
    full[where] = sub[2]
    assert len(sub[1]) < len(want[1])
    assert_same(arrays(C), (want[0], want[1], full), "sub-pattern")
    # one extra entry of B whose product lands outside c: refused, c unchanged
    before = arrays(C)
    p = int(a[1][0])  # a row of B that A's row 0 names
    extra_col = 11  # the column no row of B holds
    b_rows = [list(b[1][b[0][r]:b[0][r + 1]]) for r in range(k)]
    b_rows[p] = sorted(b_rows[p] + [extra_col])
    b_more = cases.from_rows(b_rows, dtype, np.random.default_rng(61))
    Bm = make(smm, b_more, (k, n))
    with pytest.raises(smm.SmmHipError) as e:
        C.multiply_into(A, Bm)
    assert e.value.code == INVALID and "row 0" in str(e.value)
    assert_same(arrays(C), before, "after the refusal")
    assert C.get_kernel() == kernel
    # c over caller-owned device arrays behaves the same
    d = [torch.from_numpy(np.array(x)).to("cuda:0") for x in (want[0], want[1], np.full(len(want[1]), np.nan, dtype=dtype))]
    torch.cuda.synchronize()
    Cb = smm.CSRMatrix.from_device(m, n, d[0], d[1], d[2], dtype)
    Cb.multiply_into(A, B)
    assert_same((want[0], want[1], d[2].cpu().numpy()), arrays(A @ B), "borrowed arrays")
    held = d[2].clone()
    with pytest.raises(smm.SmmHipError):
        Cb.multiply_into(A, Bm)
    assert torch.equal(d[2].view(torch.uint8), held.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_refusals(smm, dtype):
    a, b, (m, k, n), want = case("small_rectangular", dtype)
    other = np.float64 if dtype == np.float32 else np.float32
    A, B = make(smm, a, (m, k)), make(smm, b, (k, n))
    C = A @ B
    lib = _lib.load()
    out = ctypes.c_void_p()
    with pytest.raises(smm.SmmHipError) as e:
        A.multiply(A)  # 53 columns against 37 rows
    assert e.value.code == INVALID
    with pytest.raises(smm.SmmHipError) as e:
        A.multiply(make(smm, (b[0], b[1], np.asarray(b[2]).astype(other)), (k, n)))
    assert e.value.code == INVALID
    assert lib.smm_hip_csr_multiply_create(None, B._h, None, ctypes.byref(out)) == INVALID
    assert lib.smm_hip_csr_multiply_create(A._h, None, None, ctypes.byref(out)) == INVALID
    assert lib.smm_hip_csr_multiply_create(A._h, B._h, None, None) == INVALID
    into = getattr(lib, "smm_hip_csr_multiply_into_" + ("f32" if dtype == np.float32 else "f64"))
    wrong = getattr(lib, "smm_hip_csr_multiply_into_" + ("f64" if dtype == np.float32 else "f32"))
    assert into(None, A._h, B._h, None) == INVALID
    assert wrong(C._h, A._h, B._h, None) == INVALID
    sq = gen.poisson2d(6, dtype=dtype)
    S = make(smm, sq, (36, 36))
    S2 = S @ S
    assert into(S2._h, S2._h, S._h, None) == INVALID  # c aliases a
    assert into(S2._h, S._h, S2._h, None) == INVALID  # c aliases b
    assert into(C._h, S._h, S._h, None) == INVALID  # shapes
    assert_same(arrays(S2), spgemm(sq, sq, 36))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_bad_matrices_are_refused_not_faulted(smm, dtype):
    """a column of A equal to k, a column of B equal to n and a start[] that does not ascend, in caller-owned device arrays inside guard
    bands: SMM_HIP_ERR_INVALID from the device flag, nothing created, nothing outside the arrays touched"""
    a, b, (m, k, n), want = case("small_rectangular", dtype)
    bad_a_col = np.array(a[1])
    bad_a_col[7] = k
    bad_b_col = np.array(b[1])
    bad_b_col[5] = n
    bad_start = np.array(a[0])
    bad_start[10], bad_start[11] = bad_start[11], bad_start[10] - 1
    assert bad_start[10] > bad_start[11]
    stream = torch.cuda.current_stream().cuda_stream
    C = make(smm, a, (m, k)) @ make(smm, b, (k, n))
    for what, a_arrays, b_arrays in (("column of A == k", (a[0], bad_a_col, a[2]), b), ("column of B == n", a, (b[0], bad_b_col, b[2])),
                                     ("start[] of A descends", (bad_start, a[1], a[2]), b)):
        views = []
        for csr in (a_arrays, b_arrays):
            nnz = int(csr[0][-1])
            views.append([carve_like(np.asarray(csr[0]), fit(1, np.int32), fill=nnz, device="cuda:0"),
                          carve_like(np.asarray(csr[1]), fit(2, np.int32), fill=0, device="cuda:0"),
                          carve_like(np.asarray(csr[2]), fit(3, dtype), device="cuda:0")])
        saved = [[snapshot(t) for t in v] for v in views]
        torch.cuda.synchronize()
        A = smm.CSRMatrix.from_device(m, k, *views[0], dtype)
        B = smm.CSRMatrix.from_device(k, n, *views[1], dtype)
        with pytest.raises(smm.SmmHipError) as e:
            A.multiply(B, stream)
        assert e.value.code == INVALID, what
        with pytest.raises(smm.SmmHipError) as e:
            C.multiply_into(A, B, stream)
        assert e.value.code == INVALID, what
        torch.cuda.synchronize()
        for v, snaps in zip(views, saved):
            for t, snap in zip(v, snaps):
                assert_unchanged(t, snap, what)
                assert_guards_intact(t, what)
    assert_same(arrays(C), want, "c after the refusals")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_from_device_offset_views(smm, dtype):
    """A and B over views at element alignment inside larger buffers: the product is right, the factors keep their bits, guards intact"""
    a, b, (m, k, n), want = case("spmv_column", dtype)
    views = []
    for csr in (a, b):
        nnz = int(csr[0][-1])
        views.append([carve_like(np.asarray(csr[0]), fit(1, np.int32), fill=nnz, device="cuda:0"),
                      carve_like(np.asarray(csr[1][:nnz]), fit(3, np.int32), fill=0, device="cuda:0"),
                      carve_like(np.asarray(csr[2][:nnz]), fit(1, dtype), device="cuda:0")])
    saved = [[snapshot(t) for t in v] for v in views]
    torch.cuda.synchronize()
    A = smm.CSRMatrix.from_device(m, k, *views[0], dtype)
    B = smm.CSRMatrix.from_device(k, n, *views[1], dtype)
    s = torch.cuda.Stream()
    C = A.multiply(B, s.cuda_stream)
    C.multiply_into(A, B, s.cuda_stream)
    torch.cuda.synchronize()
    assert_same(arrays(C), want)
    for v, snaps in zip(views, saved):
        for t, snap in zip(v, snaps):
            assert_unchanged(t, snap, "factor")
            assert_guards_intact(t, "factor")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_degenerate_shapes(smm, dtype):
    def empty(rows):
        return np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)

    a, b, (m, k, n), _ = case("small_rectangular", dtype)
    for what, (ca, sa), (cb, sb) in (("nnz(A) == 0", (empty(m), (m, k)), (b, (k, n))), ("nnz(B) == 0", (a, (m, k)), (empty(k), (k, n))),
                                     ("m == 0", (empty(0), (0, k)), (b, (k, n))), ("k == 0", (empty(m), (m, 0)), (empty(0), (0, n))),
                                     ("n == 0", (a, (m, k)), (empty(k), (k, 0)))):
        A, B = make(smm, ca, sa), make(smm, cb, sb)
        C = A @ B
        assert (C.rows, C.cols, C.nnz) == (sa[0], sb[1], 0), what
        assert_same(arrays(C), empty(sa[0]), what)
        C.multiply_into(A, B)
        assert_same(arrays(C), empty(sa[0]), what + " into")
    # a c that stores nothing is still a pattern: products that land outside it are refused, with the first such row named
    A, B_none, B = make(smm, a, (m, k)), make(smm, empty(k), (k, n)), make(smm, case("small_rectangular", dtype)[1], (k, n))
    C = A @ B_none
    assert C.nnz == 0
    first_row = int(np.flatnonzero(np.diff(case("small_rectangular", dtype)[3][0]))[0])
    with pytest.raises(smm.SmmHipError) as e:
        C.multiply_into(A, B)
    assert e.value.code == INVALID and f"row {first_row} " in str(e.value)
    assert_same(arrays(C), empty(m), "empty c after the refusal")


def test_cpp_header_case(tmp_path):
    """tests/cpp/spgemm_case.cpp: SMM::multiply / SMM::multiplyInto through the drop-in header, built and run the way gmres_case.cpp is"""
    exe = tmp_path / "spgemm_case"
    lib = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "smm_hip"), "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "spgemm_case.cpp"), "-L" + lib, "-lsmm_hip", "-Wl,-rpath," + lib], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "spgemm_case: OK" in run.stdout
