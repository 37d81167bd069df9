"""GPU tests of the CSR SpMM (several right-hand sides at once, csrc/smm_spmm.hip) through the C ABI: every column of a block result
against the single-vector SpMV of that column -- bit for bit wherever a row is summed by one lane, within the re-ordering bound of
test_gpu_spmv.bound() for rows longer than a tile."""
import ctypes

import numpy as np
import pytest
from conftest import kat_matrix
from test_gpu_spmv import bound
from test_oracle import gen_matrices

from oracle.oracle import OP_SUB
from sparse_matrix_math_amd import _lib, host
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
KMAX = 8
OPS = ("assign", "add", "sub")


def matrices(dtype):
    """name -> (csr, cols): the generator matrices, the 5 x 4 known-answer matrix, and banded matrices around the wave / tile edges"""
    out = {name: (csr, len(csr[0]) - 1) for name, csr in gen_matrices(dtype).items()}
    out["kat_5x4"] = (kat_matrix(dtype), 4)
    for rows in (1, 63, 64, 65, 257):
        out[f"banded_{rows}"] = (gen.banded_random_spd(rows, k=25, seed=0x5EED, max_offset=1 << 20, dtype=dtype), rows)
    return out


def blocks(rows, cols, dtype, seed=99):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (cols, KMAX)).astype(dtype), rng.uniform(-1, 1, (rows, KMAX)).astype(dtype)


def spmv_columns(A, X, L):
    """per op: (rows, KMAX) block whose column j is the single-vector result for column j, with the kernel the caller has set"""
    rows = L.shape[0]
    ref = {op: np.zeros((rows, KMAX), dtype=X.dtype) for op in OPS}
    for j in range(KMAX):
        x, l = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(L[:, j])
        for op in OPS:
            out = np.zeros(rows, dtype=X.dtype)
            {"assign": lambda: A.rMult(x, out), "add": lambda: A.rMultAdd(l, x, out), "sub": lambda: A.rMultSub(l, x, out)}[op]()
            ref[op][:, j] = out
    return ref


def spmm(A, op, L, X):
    out = np.full((L.shape[0], X.shape[1]), 77, dtype=X.dtype)
    if op == "assign":
        A.rMultBlock(X, out)
    elif op == "add":
        A.rMultAddBlock(L, X, out)
    else:
        A.rMultSubBlock(L, X, out)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_column_carries_the_spmv_bits(smm, dtype):
    for name, (csr, cols) in matrices(dtype).items():
        rows = len(csr[0]) - 1
        A = smm.CSRMatrix(rows, cols, *csr)
        X, L = blocks(rows, cols, dtype)
        A.set_kernel(2, 1)  # STREAM, one lane per row: the reference's order of summation
        ref = spmv_columns(A, X, L)
        for k in range(1, KMAX + 1):
            Xk, Lk = np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(L[:, :k])
            for op in OPS:
                np.testing.assert_array_equal(spmm(A, op, Lk, Xk), ref[op][:, :k], err_msg=f"{name} k={k} {op}")
        # the SpMV's own kernel choice does not reach the SpMM
        for family, lanes in ((1, 64), (3, 0)):
            try:
                A.set_kernel(family, lanes)
            except smm.SmmHipError:
                assert family == 3  # a matrix without a shared offset pattern refuses PATTERN
                continue
            for k in (3, 4, 8):
                Xk, Lk = np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(L[:, :k])
                np.testing.assert_array_equal(spmm(A, "sub", Lk, Xk), ref["sub"][:, :k], err_msg=f"{name} k={k} kernel {family}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_rows(smm, oracle, dtype):
    """the 700 x 9000 matrix of test_gpu_spmv.test_ragged_and_long_rows: rows of 0 .. 5000 entries, leading / trailing empty rows"""
    rng = np.random.default_rng(42)
    rows, cols = 700, 9000
    lens = rng.integers(0, 60, size=rows)
    lens[5] = 5000
    lens[300] = 2049
    lens[301] = 2048
    lens[:3] = 0
    lens[-4:] = 0
    start = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens, out=start[1:])
    pos = np.concatenate([np.sort(rng.choice(cols, size=n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.uniform(-1, 1, start[-1]).astype(dtype)
    csr = (start, pos, val)
    A = smm.CSRMatrix(rows, cols, *csr)
    X, L = blocks(rows, cols, dtype, seed=5)
    A.set_kernel(2, 1)
    ref = spmv_columns(A, X, L)["sub"]
    for k in (1, 3, 4, 8):
        Xk, Lk = np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(L[:, :k])
        out = spmm(A, "sub", Lk, Xk)
        tiles, cap, max_rows, _ = A.tile_info()
        assert tiles > 0 and 0 < cap < 5000 and max_rows <= 256
        short = lens <= cap  # rows the tile table does not mark as long: one lane, stored order
        assert not short[5]
        np.testing.assert_array_equal(out[short], ref[short, :k])
        for j in range(k):
            exact = oracle.spmv(csr, OP_SUB, np.ascontiguousarray(L[:, j]), np.ascontiguousarray(X[:, j])).astype(np.float64)
            err = np.abs(out[:, j].astype(np.float64) - exact)
            assert np.all(err <= bound(csr, X[:, j], dtype, L[:, j])), (k, j, int(np.argmax(err)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_equals_out_of_place(smm, dtype):
    csr = gen_matrices(dtype)["banded_2000"]
    rows = len(csr[0]) - 1
    A = smm.CSRMatrix(rows, rows, *csr)
    X, L = blocks(rows, rows, dtype, seed=3)
    for k in (3, 4, 8):
        Xk, Lk = np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(L[:, :k])
        for op, fn in (("add", A.rMultAddBlock), ("sub", A.rMultSubBlock)):
            keep = Lk.copy()
            out = spmm(A, op, Lk, Xk)
            np.testing.assert_array_equal(Lk, keep)  # Lhs untouched out of place
            inpl = Lk.copy()
            fn(inpl, Xk, inpl)
            np.testing.assert_array_equal(inpl, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_follows_edits_of_the_values(smm, dtype):
    """PATTERN keeps derived copies of the values; the SpMM reads the CSR arrays, which every edit keeps current"""
    csr = gen.poisson2d(32, dtype=dtype)
    rows = len(csr[0]) - 1
    A = smm.CSRMatrix(rows, rows, *csr)
    A.set_kernel(3, 0)
    X, L = blocks(rows, rows, dtype, seed=11)
    k = 4
    Xk, Lk = np.ascontiguousarray(X[:, :k]), np.ascontiguousarray(L[:, :k])

    def check(what):
        out = spmm(A, "add", Lk, Xk)
        for j in range(k):
            y = np.zeros(rows, dtype=dtype)
            A.rMultAdd(np.ascontiguousarray(L[:, j]), np.ascontiguousarray(X[:, j]), y)
            np.testing.assert_array_equal(out[:, j], y, err_msg=what)
        return out

    before = check("as created")
    A.scale(0.5)
    scaled = check("after scale")
    assert not np.array_equal(before, scaled)
    start, pos, _ = csr
    r = np.array([0, 500, rows - 1], dtype=np.int32)
    c = np.array([pos[start[0]], pos[start[500] + 1], pos[start[rows] - 1]], dtype=np.int32)
    assert A.update_entries(r, c, np.array([3.25, -7.5, 11.0], dtype=dtype)).all()
    edited = check("after update_entries")
    assert not np.array_equal(scaled, edited)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(smm, dtype):
    k = 4
    # nnz == 0
    E = smm.CSRMatrix(5, 4, np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    X = np.arange(16, dtype=dtype).reshape(4, k)
    L = np.arange(20, dtype=dtype).reshape(5, k) + 1
    np.testing.assert_array_equal(spmm(E, "add", L, X), L)
    np.testing.assert_array_equal(spmm(E, "sub", L, X), L)
    np.testing.assert_array_equal(spmm(E, "assign", L, X), 0)
    # rows == 0
    Z = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    Z.rMultBlock(np.zeros((0, k), dtype=dtype), np.zeros((0, k), dtype=dtype))
    # rejected arguments: SMM_HIP_ERR_INVALID from the library
    csr = gen.poisson2d(8, dtype=dtype)
    A = smm.CSRMatrix(64, 64, *csr)
    for bad_k in (0, 9):
        with pytest.raises(smm.SmmHipError) as e:
            A.spmm_dev(0, bad_k, None, None, None)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID
    other = np.float64 if dtype == np.float32 else np.float32
    Xo, Oo = np.ones((64, k), dtype=other), np.zeros((64, k), dtype=other)
    st = host._fn("smm_hip_spmm", host._suffix(other))(A._h, 0, k, ctypes.c_void_p(0), Xo.ctypes.data_as(ctypes.c_void_p), Oo.ctypes.data_as(ctypes.c_void_p))
    assert st == _lib.SMM_HIP_ERR_INVALID
    Xa = np.ones((64, k), dtype=dtype)
    with pytest.raises(smm.SmmHipError) as e:
        A.rMultBlock(Xa, Xa)  # x must not alias out (ref:1503)
    assert e.value.code == _lib.SMM_HIP_ERR_INVALID


def test_dropin_header_blocks(tmp_path):
    """tests/cpp/spmm_case.cpp: CSRMatrix::rMult(X, Out, k) and SMM::BiCGStabBatch / ConjugateGradientBatch of the drop-in header, every
    column against the single-vector calls"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "sparse_matrix_math_amd", "lib")
    exe = tmp_path / "spmm_case"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(root, 'include', 'smm_hip')}", f"-I{os.path.join(root, 'include')}", "-o", str(exe),
           os.path.join(root, "tests", "cpp", "spmm_case.cpp"), f"-L{lib}", "-lsmm_hip", f"-Wl,-rpath,{lib}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == "OK", r.stdout[-2000:]
