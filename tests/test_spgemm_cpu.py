"""The definition of the sparse product (tests/spgemm_restatement.py) checked on the CPU against scipy.sparse and against the oracle's
rMult, and the three new entry points in both shared libraries.  The GPU side is tests/test_gpu_spgemm.py."""
import ctypes

import numpy as np
import pytest
import spgemm_cases as cases
from spgemm_restatement import bound, dense, spgemm

from sparse_matrix_math_amd import _lib

DTYPES = [np.float32, np.float64]
NEW_SYMBOLS = ("smm_hip_csr_multiply_create", "smm_hip_csr_multiply_into_f32", "smm_hip_csr_multiply_into_f64")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def products(dtype):
    yield "small_rectangular", cases.small_rectangular(dtype)
    yield "cancellation", cases.cancellation(dtype)
    yield "spmv_column", cases.spmv_column(dtype)
    yield "every_bin", cases.every_bin(dtype)
    yield "long_row_b", cases.long_row(dtype, "b")
    p = cases.banded_nonsymmetric(dtype)
    yield "banded_squared", (p, p, (1500, 1500, 1500))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_restatement_against_scipy(dtype):
    """pattern: that of the product of the two patterns taken as all-ones matrices; values: within terms * eps * sum |a||b| per entry of
    the float64 product"""
    for name, (a, b, (m, k, n)) in products(dtype):
        start, pos, val = spgemm(a, b, n)
        ones = lambda csr: (csr[0], csr[1], np.ones(len(csr[1]), dtype=np.float64))  # noqa: E731
        want = (cases.to_scipy(ones(a), (m, k)) @ cases.to_scipy(ones(b), (k, n))).tocsr()
        want.sort_indices()
        assert np.all(want.data > 0), name  # (sums of ones: the structural product, nothing cancelled)
        np.testing.assert_array_equal(start, want.indptr, err_msg=name)
        np.testing.assert_array_equal(pos, want.indices, err_msg=name)
        # (scipy drops the entries whose sum is exactly 0 -- stored zeros, cancellation --: its values are read by (row, column))
        exact = (cases.to_scipy(a, (m, k), np.float64) @ cases.to_scipy(b, (k, n), np.float64)).tocsr()
        rows = np.repeat(np.arange(m), np.diff(start))
        assert exact.nnz <= len(pos), name
        want_val = np.asarray(exact[rows, pos]).reshape(-1) if len(pos) else np.zeros(0)
        assert np.all(np.abs(val.astype(np.float64) - want_val) <= bound(a, b, n)), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_restatement_columns_are_the_oracles_row_sums(oracle, dtype):
    """for finite values column j of A B is A.rMult of the dense column j of B, bit for bit"""
    for build in (cases.spmv_column, cases.small_rectangular, cases.cancellation, cases.order_cases):
        a, b, (m, k, n) = build(dtype)
        c = dense(spgemm(a, b, n), n)
        bd = dense(b, n)
        for j in range(n):
            want = oracle.spmv(a, 0, None, np.ascontiguousarray(bd[:, j]))
            np.testing.assert_array_equal(bits(c[:, j]), bits(want), err_msg=f"{build.__name__} column {j}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_restatement_keeps_the_stored_order(dtype):
    a, b, (m, k, n) = cases.order_cases(dtype)
    start, pos, val = spgemm(a, b, n)
    first = val[pos == cases.ORDER_COLUMN]
    assert len(first) == 6 and set(first.tolist()) == {0.0, 1.0}  # (big + 1) - big = 0, (big - big) + 1 = 1: the order shows
    np.testing.assert_array_equal(val[pos == 6], np.full(6, 3.0, dtype=dtype))
    offsets = [int(np.flatnonzero(b[1][b[0][r]:b[0][r + 1]] == cases.ORDER_COLUMN)[0]) for r in range(k)]
    assert all(len({offsets[3 * i], offsets[3 * i + 1], offsets[3 * i + 2]}) == 3 for i in range(m))  # another lane at every step


def test_both_libraries_export_the_product():
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), f"{name} missing from {_lib.library_path(fma=fma)}"
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
