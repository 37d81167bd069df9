"""The LONGROWS SpMV family without a GPU: the header's constant and prototypes, the exported names of both library flavours, the Python
constant, the generator's CSR and the NumPy restatement of the stated order (tests/longrows_restatement.py)."""
import ctypes
import os
import re

import longrows_restatement as lr
from longrows_cases import arrow_system, kkt_system, tall_system
from minres_restatement import minres
import numpy as np
import pytest
from test_gpu_minres import EPS as MINRES_EPS

import sparse_matrix_math_amd as smm
from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64  # the smallest segment the header allows


def header():
    with open(os.path.join(ROOT, "include", "smm_hip.h")) as f:
        return f.read()


def test_header_declares_the_family_and_the_two_calls():
    text = header()
    assert re.search(r"^#define SMM_SPMV_LONGROWS 5\b", text, re.M)
    flat = " ".join(text.split())
    assert "int smm_hip_csr_longrows_configure(smm_hip_csr* m, int split_len, int segment_len);" in flat
    assert "int smm_hip_csr_longrows_info(const smm_hip_csr* m, int* split_len, int* segment_len, int* long_rows, long long* segments);" in flat
    lo, hi = (int(re.search(rf"^#define SMM_LONGROWS_SEGMENT_{w} (\d+)", text, re.M).group(1)) for w in ("MIN", "MAX"))
    assert lo == G and hi % 64 == 0 and hi >= 1024
    assert int(re.search(r"^#define SMM_LONGROWS_SPLIT_MIN (\d+)", text, re.M).group(1)) <= 64  # tests can ask for a few hundred entries and fewer


@pytest.mark.parametrize("fma", [False, True], ids=["two-roundings", "std-fma"])
def test_both_libraries_export_the_names(fma):
    lib = ctypes.CDLL(_lib.library_path(fma=fma))
    for name in ("smm_hip_csr_longrows_configure", "smm_hip_csr_longrows_info"):
        assert getattr(lib, name) is not None


def test_the_python_layer_resolves_them():
    lib = _lib.load()
    assert lib.smm_hip_csr_longrows_configure.argtypes is not None and lib.smm_hip_csr_longrows_info.restype is ctypes.c_int
    assert smm.SPMV_LONGROWS == 5
    assert callable(smm.CSRMatrix.longrows_configure) and callable(smm.CSRMatrix.longrows_info)


@pytest.mark.parametrize("integer", [False, True])
def test_with_long_rows_yields_valid_csr(integer):
    rows, cols = 50, 700
    base = gen.random_rows(rows, cols, 0, 9, seed=3, empty_every=7)
    long_rows, long_lens = [0, 17, 18, 49], [3 * G + 1, G, 700, 2 * G + 7]
    start, pos, val = gen.with_long_rows(base[0], base[1], cols, long_rows, long_lens, seed=4, dtype=np.float32, integer=integer)
    assert start.dtype == np.int32 and pos.dtype == np.int32 and val.dtype == np.float32
    assert start[0] == 0 and start[-1] == len(pos) == len(val) and np.all(np.diff(start) >= 0)
    want = np.diff(base[0]).copy()
    want[long_rows] = long_lens
    np.testing.assert_array_equal(np.diff(start), want)
    for r in range(rows):
        c = pos[start[r]:start[r + 1]]
        assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < cols)), r
        if r not in long_rows:
            np.testing.assert_array_equal(c, base[1][base[0][r]:base[0][r + 1]])
    if integer:
        assert np.all(val == np.round(val)) and val.min() >= -4 and val.max() <= 4 and len(np.unique(val)) == 9
    else:
        assert np.all(np.abs(val) <= 1) and len(np.unique(val)) > len(val) // 2
    with pytest.raises(ValueError):
        gen.with_long_rows(base[0], base[1], cols, [3], [cols + 1])


def matrix(dtype, seed=11):
    rows, cols = 12, 900
    base = gen.random_rows(rows, cols, 0, 40, seed=seed)
    csr = gen.with_long_rows(base[0], base[1], cols, [2, 4, 7, 9, 10], [3 * G + 5, 5 * G + 3, 2 * G, 4 * G + 1, 6 * G + 9], seed=seed + 1, dtype=dtype)
    x = np.random.default_rng(seed + 2).uniform(-1, 1, cols).astype(dtype)
    return csr, x


def plain_chain(csr, x):
    start, pos, val = csr
    out = np.zeros(len(start) - 1, dtype=val.dtype)
    for r in range(len(out)):
        d = val.dtype.type(0)
        for k in range(start[r], start[r + 1]):
            d = val[k] * x[pos[k]] + d
        out[r] = d
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_long_row_is_the_plain_chain(dtype):
    csr, x = matrix(dtype)
    longest = int(np.diff(csr[0]).max())
    for split in (longest, longest + 100):
        np.testing.assert_array_equal(lr.spmv(*csr, x, split, G), plain_chain(csr, x))


@pytest.mark.parametrize("std_fma", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_row_within_the_bound(dtype, std_fma):
    """(len + 2) eps sum |a x| against a longdouble sum: the bound DESIGN section 3.1 states for more than one lane per row"""
    csr, x = matrix(dtype)
    start, pos, val = csr
    got = lr.spmv(*csr, x, G, G, std_fma=std_fma)
    eps = float(np.finfo(dtype).eps)
    checked = 0
    for r in range(len(start) - 1):
        v, xx = val[start[r]:start[r + 1]].astype(np.longdouble), x[pos[start[r]:start[r + 1]]].astype(np.longdouble)
        want, scale = float((v * xx).sum()), float(np.abs(v * xx).sum())
        assert abs(float(got[r]) - want) <= (len(v) + 2) * eps * scale, (r, len(v), got[r], want)
        checked += len(v) == 3 * G + 5
    assert checked == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_order_is_visible_in_the_bits(dtype):
    csr, x = matrix(dtype)
    short = np.diff(csr[0]) <= G
    a, b, c = lr.spmv(*csr, x, G, G), lr.spmv(*csr, x, G, 2 * G), lr.spmv(*csr, x, 3 * G + 5, G)
    np.testing.assert_array_equal(a[short], b[short])
    assert np.any(a[~short] != b[~short]), "segment_len 64 and 128 group the five long rows differently"
    assert c[2] == plain_chain(csr, x)[2] and np.any(a[~short] != plain_chain(csr, x)[~short])
    if dtype == np.float32:  # one rounding instead of two: other bits somewhere in the short rows and in the long one
        f = lr.spmv(*csr, x, G, G, std_fma=True)
        assert np.any(f != a) and np.allclose(f, a, rtol=1e-4, atol=1e-5)


def test_minres_restatement_converges_on_the_kkt_system(oracle):
    """before the GPU runs MINRES on it: the matrix is symmetric and indefinite, its constraint rows are dense, and the restatement converges"""
    csr, b, D = kkt_system(np.float64)
    ev = np.linalg.eigvalsh(D)
    assert np.array_equal(D, D.T) and ev.min() < 0 < ev.max()
    assert sorted(np.diff(csr[0]))[-2:] == [576, 576]
    st, x, it, _ = minres(oracle, csr, b, np.zeros(len(b)), -1, MINRES_EPS[np.float64])
    assert st == 0 and it < len(b) and np.linalg.norm(b - D @ x) <= 10 * MINRES_EPS[np.float64]


def test_the_arrow_matrix_is_positive_definite():
    csr, b, D = arrow_system(np.float64)
    assert np.array_equal(D, D.T) and np.linalg.eigvalsh(D).min() > 0.5
    assert int(np.diff(csr[0]).max()) == 577 and np.all(D[-1] != 0)  # the dense row, and its column in every other row
    np.testing.assert_allclose(D @ np.ones(len(b)), b, rtol=1e-12)  # b = the row sums: the answer is all ones


def test_the_tall_matrix_has_a_dense_column():
    csr, csr_t, b, D = tall_system(np.float64)
    assert D.shape == (300, 40) and int(np.diff(csr_t[0]).max()) == 300 and np.linalg.matrix_rank(D) == 40
