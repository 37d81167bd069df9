"""The definition of the sparse sum (tests/add_restatement.py) checked on the CPU against the dense sum and against a plain Python loop
written straight from include/smm_hip.h, and the four new entry points in both shared libraries, the ctypes table and the header.  The GPU
side is tests/test_gpu_add.py."""
import ctypes
import os
import re

import add_cases as cases
import numpy as np
import pytest
from add_restatement import add, add_into, dense

from sparse_matrix_math_amd import _lib

DTYPES = [np.float32, np.float64]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smm_hip_csr_add_create_f32", "smm_hip_csr_add_create_f64", "smm_hip_csr_add_into_f32", "smm_hip_csr_add_into_f64")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_both_libraries_export_the_sum():
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), f"{name} missing from {_lib.library_path(fma=fma)}"
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())


def test_ctypes_table_loads():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6
    assert lib.smm_hip_csr_add_create_f32.argtypes[1] is ctypes.c_float and lib.smm_hip_csr_add_create_f64.argtypes[3] is ctypes.c_double
    assert lib.smm_hip_csr_add_into_f32.argtypes[2] is ctypes.c_float and lib.smm_hip_csr_add_into_f64.argtypes[4] is ctypes.c_double


def test_header_declares_the_four_calls():
    with open(os.path.join(ROOT, "include", "smm_hip.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    for suf, t in (("f32", "float"), ("f64", "double")):
        assert (f"int smm_hip_csr_add_create_{suf}(const smm_hip_csr* a, {t} alpha, const smm_hip_csr* b, {t} beta, smm_hip_stream stream, "
                "smm_hip_csr** out);") in text
        assert (f"int smm_hip_csr_add_into_{suf}(smm_hip_csr* c, const smm_hip_csr* a, {t} alpha, const smm_hip_csr* b, {t} beta, "
                "smm_hip_stream stream);") in text


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_is_the_dense_sum_on_the_union(name, dtype):
    a, b, (m, n) = cases.CASES[name](dtype)
    da, db = dense(a, n), dense(b, n)
    stored = np.zeros((m, n), dtype=bool)
    for csr in (a, b):
        rows = np.repeat(np.arange(m), np.diff(csr[0]))
        stored[rows, csr[1]] = True
    for alpha, beta in cases.SCALARS:
        start, pos, val = add(a, alpha, b, beta, n)
        assert start.dtype == np.int32 and pos.dtype == np.int32 and val.dtype == np.dtype(dtype)
        with np.errstate(all="ignore"):
            want = dtype(alpha) * da + dtype(beta) * db
        assert np.array_equal(dense((start, pos, val), n), want), (name, alpha, beta)  # IEEE ==
        rows = np.repeat(np.arange(m), np.diff(start))
        got = np.zeros((m, n), dtype=bool)
        got[rows, pos] = True
        assert len(pos) == int(start[-1]) == int(stored.sum()) and np.array_equal(got, stored), name  # exactly the union
        for i in range(m):
            assert np.all(np.diff(pos[start[i]:start[i + 1]]) > 0), (name, i)


def by_the_definition(a, alpha, b, beta, dtype):
    """a plain loop over rows, written from the header's text"""
    start, pos, val = [0], [], []
    alpha, beta = dtype(alpha), dtype(beta)
    for i in range(len(a[0]) - 1):
        in_a = {int(a[1][k]): a[2][k] for k in range(a[0][i], a[0][i + 1])}
        in_b = {int(b[1][k]): b[2][k] for k in range(b[0][i], b[0][i + 1])}
        for j in sorted(set(in_a) | set(in_b)):
            if j in in_a and j in in_b:
                u, v = dtype(alpha * in_a[j]), dtype(beta * in_b[j])
                c = dtype(u + v)
            elif j in in_a:
                c = dtype(alpha * in_a[j])
            else:
                c = dtype(beta * in_b[j])
            pos.append(j)
            val.append(c)
        start.append(len(pos))
    return np.array(start, dtype=np.int32), np.array(pos, dtype=np.int32), np.array(val, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_restatement_against_a_plain_loop(dtype):
    a, b, (m, n) = cases.ragged(dtype)
    for alpha, beta in cases.SCALARS:
        got, want = add(a, alpha, b, beta, n), by_the_definition(a, alpha, b, beta, dtype)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg=f"alpha {alpha} beta {beta}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_the_cases_hold_what_they_promise(dtype):
    a, b, (m, n) = cases.ragged(dtype)
    start, pos, val = add(a, 1, b, 1, n)
    row0 = dict(zip(pos[start[0]:start[1]].tolist(), bits(val[start[0]:start[1]]).tolist()))
    zero, minus_zero = int(bits(np.array([0.0], dtype=dtype))[0]), int(bits(np.array([-0.0], dtype=dtype))[0])
    assert row0[5] == zero  # a cancellation keeps its entry
    assert row0[1] == minus_zero and row0[96] == minus_zero  # a lone -0.0 is not u + 0
    row1 = dict(zip(pos[start[1]:start[2]].tolist(), val[start[1]:start[2]].tolist()))
    assert row1[3] == 0.0 and 7 in row1  # stored zeros stay
    la, lb = np.diff(a[0]), np.diff(b[0])
    assert la[64] == 97 and np.any((la == 0) & (lb > 0)) and np.any((la > 0) & (lb == 0)) and np.any((la == 0) & (lb == 0))
    a, b, (m, n) = cases.long_rows(dtype)
    la, lb = np.diff(a[0]), np.diff(b[0])
    assert list(la[:2]) == [cases.SEG, cases.SEG + 1] and list(lb[2:4]) == [cases.SEG, cases.SEG + 1]
    assert np.diff(add(a, 1, b, 1, n)[0])[4] == 5000
    a, b, (m, n) = cases.disjoint(dtype)
    assert add(a, 1, b, 1, n)[0][-1] == a[0][-1] + b[0][-1]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_add_into_of_the_restatement(dtype):
    a, b, (m, n) = cases.ragged(dtype)
    created = add(a, 0.3, b, -2.5, n)
    np.testing.assert_array_equal(bits(add_into(created, a, 0.3, b, -2.5, n)), bits(created[2]))
    # a superset: every column in every row
    full = (np.arange(0, (m + 1) * n, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), m), np.zeros(m * n, dtype=dtype))
    on_full = add_into(full, a, 0.3, b, -2.5, n)
    rows = np.repeat(np.arange(m), np.diff(created[0]))
    extra = np.ones(m * n, dtype=bool)
    extra[rows * n + created[1]] = False
    np.testing.assert_array_equal(bits(on_full[~extra]), bits(created[2]))
    assert extra.sum() > 0 and np.all(bits(on_full[extra]) == 0)  # +0.0: sign bit clear
    # a pattern that lacks one entry of row 37 (and one of a later row: the FIRST row is named)
    lens = np.diff(created[0])
    victims = [i for i in (37, 90) if lens[i] > 0]
    assert victims[0] == 37
    keep = np.ones(len(created[1]), dtype=bool)
    for i in victims:
        keep[created[0][i]] = False
    lacking_start = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=m), out=lacking_start[1:])
    assert add_into((lacking_start, created[1][keep], created[2][keep]), a, 0.3, b, -2.5, n) == 37
