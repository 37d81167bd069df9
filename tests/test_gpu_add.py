"""The sparse sum on the device (csrc/smm_add.hip) through CSRMatrix.add / add_into and the C ABI smm_hip_csr_add_create_* / _add_into_*.
The reference is the CPU definition (tests/add_restatement.py): start[], positions[] exactly and the value BITS (signed zeros count), in
both library flavours.  Also against the device routes that existed before: the assembly of the concatenated scaled triplets, and
inplaceSubtract on equal patterns."""
import ctypes
import functools
import os
import subprocess

import add_cases as cases
import numpy as np
import pytest
import torch
from add_restatement import add, add_into, triplets

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
STREAM, PATTERN = 2, 3
MASKS, CONST = 1, 3
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
    """(a, b, (rows, cols)), built once per session and never written to"""
    a, b, shape = (cases.banded_pair if name == "banded_pair" else cases.CASES[name])(dtype)
    for arr in (*a, *b):
        arr.setflags(write=False)
    return a, b, shape


@functools.lru_cache(maxsize=None)
def restated(name, dtype, alpha, beta):
    a, b, (m, n) = case(name, dtype)
    want = add(a, alpha, b, beta, n)
    for arr in want:
        arr.setflags(write=False)
    return want


def operands(smm, name, dtype):
    a, b, shape = case(name, dtype)
    A = make(smm, a, shape)
    return A, (A if name == "a_is_b" else make(smm, b, shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_against_the_restatement(smm, name, dtype):
    a, b, shape = case(name, dtype)
    A, B = operands(smm, name, dtype)
    for alpha, beta in cases.SCALARS:
        want = restated(name, dtype, alpha, beta)
        C = A.add(B, alpha, beta)
        assert_same(arrays(C), want, f"{name} {alpha} {beta}")
        F = make(smm, want, shape)
        assert (C.rows, C.cols, C.nnz, C.first_active_start) == (F.rows, F.cols, F.nnz, F.first_active_start), name
        assert C.dtype == np.dtype(dtype)
    A.close()
    if B is not A:
        B.close()  # the sum does not depend on its operands' lifetime
    assert_same(arrays(C), restated(name, dtype, *cases.SCALARS[-1]), "after the operands are gone")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_operators(smm, dtype):
    A, B = operands(smm, "ragged", dtype)
    assert_same(arrays(A + B), restated("ragged", dtype, 1, 1))
    assert_same(arrays(A - B), restated("ragged", dtype, 1, -1))
    assert A.__add__(3.0) is NotImplemented and A.__sub__(np.ones(3)) is NotImplemented
    with pytest.raises(TypeError):
        A + 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["ragged", "banded_pair"])
def test_against_the_assembly_of_the_scaled_triplets(smm, name, dtype):
    """the device route the library had before: from_triplets on a's triplets scaled by alpha (in NumPy, in the dtype) followed by b's"""
    a, b, (m, n) = case(name, dtype)
    A, B = operands(smm, name, dtype)
    ra, ca, va = triplets(a)
    rb, cb, vb = triplets(b)
    for alpha, beta in ((1, 1), (0.3, -2.5)):
        vals = np.concatenate([dtype(alpha) * va, dtype(beta) * vb]).astype(dtype)
        T = smm.CSRMatrix.from_triplets(m, n, np.concatenate([ra, rb]), np.concatenate([ca, cb]), vals)
        C = A.add(B, alpha, beta)
        assert_same(arrays(C), arrays(T), f"{name} {alpha} {beta}")
        if name == "banded_pair":
            assert_same(arrays(C), add(a, alpha, b, beta, n), "restatement")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_same_pattern_is_inplace_subtract(smm, dtype):
    a, b, shape = case("same_pattern", dtype)
    A, B = operands(smm, "same_pattern", dtype)
    C = A.add(B, 1, -1)
    assert C.hasSameNonZeroPattern(A)
    S = make(smm, a, shape)
    S.inplaceSubtract(B)
    assert_same(arrays(C), arrays(S))


class FmaLibrary:
    """the SMM_WITH_STD_FMA flavour through raw ctypes (the package binds the default flavour), loaded as tests/test_gpu_fma_flavour.py does"""

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

    def add(self, ha, alpha, hb, beta, dtype):
        h = ctypes.c_void_p()
        suf, ct = ("f32", ctypes.c_float) if np.dtype(dtype) == np.float32 else ("f64", ctypes.c_double)
        fn = getattr(self.lib, f"smm_hip_csr_add_create_{suf}")
        fn.argtypes = [ctypes.c_void_p, ct, ctypes.c_void_p, ct, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        assert fn(ha, alpha, hb, beta, None, ctypes.byref(h)) == 0, self.lib.smm_hip_last_error()
        r, c, nnz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert self.lib.smm_hip_csr_info(h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(nnz), None, None) == 0
        start, pos, val = np.zeros(r.value + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value, dtype=dtype)
        assert self.lib.smm_hip_csr_get_pattern(h, self.ptr(start), self.ptr(pos)) == 0
        assert getattr(self.lib, f"smm_hip_csr_get_values_{suf}")(h, self.ptr(val)) == 0
        self.lib.smm_hip_csr_destroy(h)
        return start, pos, val


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_two_runs_and_both_flavours_give_the_same_bits(smm, dtype):
    fma = FmaLibrary()
    for name in ("ragged", "long_rows"):
        a, b, shape = case(name, dtype)
        A, B = operands(smm, name, dtype)
        first, second = arrays(A.add(B, 0.3, -2.5)), arrays(A.add(B, 0.3, -2.5))
        assert_same(first, second, "second run")
        ha, hb = fma.create(a, shape), fma.create(b, shape)
        assert_same(fma.add(ha, 0.3, hb, -2.5, dtype), first, "fma flavour")
        fma.lib.smm_hip_csr_destroy(ha)
        fma.lib.smm_hip_csr_destroy(hb)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_the_result_is_an_ordinary_handle(smm, oracle, dtype):
    a, b, (m, n) = case("ragged", dtype)
    A, B = operands(smm, "ragged", dtype)
    C = A.add(B, 0.3, -2.5)
    want = restated("ragged", dtype, 0.3, -2.5)
    x = np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)
    y = np.zeros(m, dtype=dtype)
    C.set_kernel(STREAM, 1)
    C.rMult(x, y)
    np.testing.assert_array_equal(bits(y), bits(oracle.spmv(want, 0, None, x)))
    Ct = C.transpose()
    assert (Ct.rows, Ct.cols, Ct.nnz) == (n, m, C.nnz)
    P = C @ Ct
    assert (P.rows, P.cols) == (m, m) and P.isSymmetric()[0]
    S = C.add(C)  # a handle made by add as both operands of the next one
    assert_same(arrays(S), add(want, 1, want, 1, n))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_add_into(smm, dtype):
    a, b, (m, n) = case("ragged", dtype)
    A, B = operands(smm, "ragged", dtype)
    C = A.add(B)
    kernel = C.get_kernel()
    # on the created pattern: the bits of create
    C.add_into(A, B, 0.3, -2.5)
    want = restated("ragged", dtype, 0.3, -2.5)
    assert_same(arrays(C), want, "created pattern")
    # on a superset (every column of every row): +0.0 on the extra entries
    full = (np.arange(0, (m + 1) * n, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), m), np.full(m * n, np.nan, dtype=dtype))
    F = make(smm, full, (m, n))
    F.add_into(A, B, 0.3, -2.5)
    on_full = add_into(full, a, 0.3, b, -2.5, n)
    rows = np.repeat(np.arange(m), np.diff(want[0]))
    extra = np.ones(m * n, dtype=bool)
    extra[rows * n + want[1]] = False
    got = F.get_values()
    np.testing.assert_array_equal(bits(got), bits(on_full))
    assert np.all(bits(got[extra]) == 0)
    # a pattern that lacks entries of rows 37 and 90: refused, the first row named, c bitwise unchanged
    keep = np.ones(len(want[1]), dtype=bool)
    keep[want[0][37]] = keep[want[0][90]] = False
    lacking_start = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=m), out=lacking_start[1:])
    lacking = (lacking_start, want[1][keep], np.linspace(1, 2, int(keep.sum())).astype(dtype))
    assert add_into(lacking, a, 0.3, b, -2.5, n) == 37
    L = make(smm, lacking, (m, n))
    L.set_kernel(STREAM, 2)
    with pytest.raises(smm.SmmHipError) as e:
        L.add_into(A, B, 0.3, -2.5)
    assert e.value.code == INVALID and "row 37 " in str(e.value), str(e.value)
    assert_same(arrays(L), lacking, "after the refusal")
    assert L.get_kernel() == (STREAM, 2) and C.get_kernel() == kernel
    # c over caller-owned device arrays: written in place on success, untouched on refusal
    d = [torch.from_numpy(np.array(x)).to("cuda:0") for x in (want[0], want[1], np.full(len(want[1]), np.nan, dtype=dtype))]
    torch.cuda.synchronize()
    Cb = smm.CSRMatrix.from_device(m, n, d[0], d[1], d[2], dtype)
    Cb.add_into(A, B, 0.3, -2.5)
    np.testing.assert_array_equal(bits(d[2].cpu().numpy()), bits(want[2]))
    dl = [torch.from_numpy(np.array(x)).to("cuda:0") for x in lacking]
    torch.cuda.synchronize()
    held = dl[2].clone()
    Lb = smm.CSRMatrix.from_device(m, n, dl[0], dl[1], dl[2], dtype)
    with pytest.raises(smm.SmmHipError):
        Lb.add_into(A, B, 0.3, -2.5)
    assert torch.equal(dl[2].view(torch.uint8), held.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_add_into_in_place(smm, dtype):
    a, d, (m, n) = case("poisson2d_8", dtype)
    sigma = 0.375
    A, D = operands(smm, "poisson2d_8", dtype)
    created = arrays(A.add(D, 1, sigma))
    assert_same(created, restated("poisson2d_8", dtype, 1, sigma))
    np.testing.assert_array_equal(created[1], a[1])  # D's pattern lies inside A's
    A.add_into(A, D, 1, sigma)  # c is a
    assert_same(arrays(A), created, "A <- A + sigma D")
    # c is a is b: A <- 0.5 A + 0.25 A
    a2, _, shape = case("a_is_b", dtype)
    S = make(smm, a2, shape)
    S.add_into(S, S, 0.5, 0.25)
    assert_same(arrays(S), add(a2, 0.5, a2, 0.25, shape[1]), "c is a is b")
    # c is b, with a's pattern inside it
    A2, D2 = operands(smm, "poisson2d_8", dtype)
    A2.add_into(D2, A2, sigma, 1)
    assert_same(arrays(A2), add(d, sigma, a, 1, n), "c is b")
    # the other way round does not fit: D lacks A's entries, row 0 first
    with pytest.raises(smm.SmmHipError) as e:
        D2.add_into(A2, D2, 1, 1)
    assert e.value.code == INVALID and "row 0 " in str(e.value)
    assert_same(arrays(D2), d, "D after the refusal")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_shape_and_dtype_mismatches(smm, dtype):
    a, b, shape = case("ragged", dtype)
    other = np.float64 if dtype == np.float32 else np.float32
    A, B = operands(smm, "ragged", dtype)
    C = A.add(B)
    before = arrays(C)
    P = make(smm, gen.poisson2d(6, dtype=dtype), (36, 36))
    W = make(smm, (b[0], b[1], np.asarray(b[2]).astype(other)), shape)
    for bad in (P, W):
        with pytest.raises(smm.SmmHipError) as e:
            A.add(bad)
        assert e.value.code == INVALID
        with pytest.raises(smm.SmmHipError) as e:
            C.add_into(A, bad)
        assert e.value.code == INVALID
    with pytest.raises(smm.SmmHipError) as e:
        P.add_into(A, B)  # c has another shape
    assert e.value.code == INVALID
    # the raw ABI: null handles, a null out, the other suffix
    lib = _lib.load()
    suf, wrong = ("f32", "f64") if dtype == np.float32 else ("f64", "f32")
    create, into = getattr(lib, "smm_hip_csr_add_create_" + suf), getattr(lib, "smm_hip_csr_add_into_" + suf)
    out = ctypes.c_void_p()
    assert create(None, 1.0, B._h, 1.0, None, ctypes.byref(out)) == INVALID
    assert create(A._h, 1.0, None, 1.0, None, ctypes.byref(out)) == INVALID
    assert create(A._h, 1.0, B._h, 1.0, None, None) == INVALID
    assert getattr(lib, "smm_hip_csr_add_create_" + wrong)(A._h, 1.0, B._h, 1.0, None, ctypes.byref(out)) == INVALID and not out.value
    assert into(None, A._h, 1.0, B._h, 1.0, None) == INVALID
    assert getattr(lib, "smm_hip_csr_add_into_" + wrong)(C._h, A._h, 1.0, B._h, 1.0, None) == INVALID
    assert create(A._h, 0.3, B._h, -2.5, None, ctypes.byref(out)) == 0  # ... and once through the raw ABI for real
    R = smm.CSRMatrix._adopt(out, dtype)
    assert_same(arrays(R), restated("ragged", dtype, 0.3, -2.5), "raw ABI")
    assert_same(arrays(C), before, "c after the refusals")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_value_edit_rules_after_add_into(smm, oracle, dtype):
    """A <- A + sigma I keeps the constant-diagonal encoding, A <- A + D with a varying D drops to MASKS; the SpMV after each is the oracle's"""
    csr = gen.poisson2d(150, 130, dtype=dtype)
    n = len(csr[0]) - 1
    x = np.random.default_rng(11).uniform(-1, 1, n).astype(dtype)

    def diagonal(values):
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), values.astype(dtype)

    def spmv(M):
        y = np.zeros(n, dtype=dtype)
        M.rMult(x, y)
        return y

    A = make(smm, csr, (n, n))
    A.set_kernel(PATTERN, 1)
    assert A.pattern_info()[0] == CONST
    spmv(A)
    tiles = A.tile_info()
    eye = diagonal(np.ones(n))
    A.add_into(A, make(smm, eye, (n, n)), 1, 0.5)
    v1 = add_into(csr, csr, 1, eye, 0.5, n)
    assert A.pattern_info()[0] == CONST and A.tile_info() == tiles and A.get_kernel()[0] == PATTERN
    np.testing.assert_array_equal(bits(spmv(A)), bits(oracle.spmv((csr[0], csr[1], v1), 0, None, x)))
    varying = diagonal(np.linspace(0.5, 1.5, n))
    A.add_into(A, make(smm, varying, (n, n)), 1, 1)
    v2 = add_into(csr, (csr[0], csr[1], v1), 1, varying, 1, n)
    assert A.pattern_info()[0] == MASKS and A.tile_info() == tiles and A.get_kernel()[0] == PATTERN
    np.testing.assert_array_equal(bits(A.get_values()), bits(v2))
    np.testing.assert_array_equal(bits(spmv(A)), bits(oracle.spmv((csr[0], csr[1], v2), 0, None, x)))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_bad_operands_are_refused_before_use(smm, dtype):
    """columns swapped inside a row, a repeated column (host-made handles), a column equal to cols (caller-owned device arrays): the
    device flag, SMM_HIP_ERR_INVALID, the operand and the first row named, nothing created"""
    a, b, (m, n) = case("ragged", dtype)
    lens = np.diff(a[0])
    row = int(np.flatnonzero((lens >= 2) & (np.arange(m) > 20))[0])
    k = int(a[0][row])
    swapped, repeated, outside = np.array(a[1]), np.array(a[1]), np.array(a[1])
    swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    repeated[k + 1] = repeated[k]
    outside[k + 1] = n
    later = int(a[0][row + 40])  # a second fault in a later row: the FIRST row is the one named
    swapped[later], swapped[later + 1] = swapped[later + 1], swapped[later]
    assert np.diff(a[0])[row + 40] >= 2
    good = make(smm, b, (m, n))
    C = make(smm, restated("ragged", dtype, 1, 1), (m, n))
    before = arrays(C)
    lib = _lib.load()
    create = getattr(lib, "smm_hip_csr_add_create_" + ("f32" if dtype == np.float32 else "f64"))
    for what, pos, on_device in (("swapped", swapped, False), ("repeated", repeated, False), ("outside", outside, True)):
        if on_device:
            d = [torch.from_numpy(np.array(t)).to("cuda:0") for t in (a[0], pos, a[2])]
            torch.cuda.synchronize()
            bad = smm.CSRMatrix.from_device(m, n, d[0], d[1], d[2], dtype)
        else:
            bad = make(smm, (a[0], pos, a[2]), (m, n))
        for name, (x, y) in (("a", (bad, good)), ("b", (good, bad))):
            out = ctypes.c_void_p(0xDEAD)
            assert create(x._h, 1.0, y._h, 1.0, None, ctypes.byref(out)) == INVALID, what
            assert not out.value, what  # nothing created
            with pytest.raises(smm.SmmHipError) as e:
                x.add(y)
            assert e.value.code == INVALID and f" of {name} " in str(e.value) and f"row {row} " in str(e.value), (what, str(e.value))
            with pytest.raises(smm.SmmHipError) as e:
                C.add_into(x, y)
            assert e.value.code == INVALID and f" of {name} " in str(e.value) and f"row {row} " in str(e.value), (what, str(e.value))
        with pytest.raises(smm.SmmHipError) as e:
            bad.add_into(good, good)  # as c
        assert e.value.code == INVALID and " of c " in str(e.value) and f"row {row} " in str(e.value), (what, str(e.value))
        if on_device:
            np.testing.assert_array_equal(d[1].cpu().numpy(), pos)
            np.testing.assert_array_equal(bits(d[2].cpu().numpy()), bits(a[2]))
    assert_same(arrays(C), before, "c after the refusals")
    # a start[] that does not ascend, in caller-owned arrays
    bad_start = np.array(a[0])
    bad_start[10], bad_start[11] = bad_start[11], bad_start[10] - 1
    assert bad_start[10] > bad_start[11]
    d = [torch.from_numpy(np.array(t)).to("cuda:0") for t in (bad_start, a[1], a[2])]
    torch.cuda.synchronize()
    bad = smm.CSRMatrix.from_device(m, n, d[0], d[1], d[2], dtype)
    with pytest.raises(smm.SmmHipError) as e:
        bad.add(good)
    assert e.value.code == INVALID and "start[] of a " in str(e.value) and "row 10 " in str(e.value), str(e.value)


def test_cpp_header_case(tmp_path):
    """tests/cpp/add_case.cpp: SMM::add / SMM::addInto and the in-place shift through the drop-in header, built and run the way
    spgemm_case.cpp is"""
    exe = tmp_path / "add_case"
    lib = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "smm_hip"), "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "add_case.cpp"), "-L" + lib, "-lsmm_hip", "-Wl,-rpath," + lib], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "add_case: OK" in run.stdout
