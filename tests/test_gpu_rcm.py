"""Reverse Cuthill-McKee on the GPU (csrc/smm_rcm.hip) through the C ABI, against its CPU restatement (tests/rcm_restatement.py): the
permutation, the component and level counts and both bandwidths exactly, in the host and the device-pointer form, with and without the
reversal; smm_hip_csr_bandwidth against numpy; the effect on the PATTERN family (a shuffled 40^3 Laplacian is refused before the ordering
and served after it, bit for bit); the refusals."""
import ctypes

import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, carve_like
from rcm_cases import NAMES, permute, rcm_case, restated, shuffle_of
from rcm_restatement import bandwidth
from test_gpu_cgs import make

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
NONE = 0      # SMM_PATTERN_NONE
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_ordering_equals_the_restatement(smm, name, dtype):
    csr = rcm_case(name, dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    for reverse in (True, False):
        want, info = restated(name, reverse)
        perm, got = A.rcm(reverse)
        print(name, np.dtype(dtype).name, "reverse", reverse, got, "restated", info)
        assert got == info
        np.testing.assert_array_equal(perm, want)
        again, got2 = A.rcm(reverse)  # integer atomics only: a second call gives the same
        np.testing.assert_array_equal(again, want)
        assert got2 == info
        d_perm = carve_like(np.full(n, -7, dtype=np.int32), 1 if reverse else 3, device="cuda:0")
        assert A.rcm_dev(d_perm, reverse) == info
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_perm.cpu().numpy(), want)
        assert_guards_intact(d_perm, "perm")
    if n:
        perm, info = restated(name)
        B = A.permute(perm)
        assert B.bandwidth() == bandwidth(csr, perm)
        assert B.bandwidth()[0] == info["bandwidth_after"]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_bandwidth_equals_numpy(smm, name, dtype):
    csr = rcm_case(name, dtype)
    assert make(smm, csr).bandwidth() == bandwidth(csr)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_bandwidth_of_a_rectangular_matrix(smm, dtype):
    csr = gen.random_rows(37, 91, 0, 6, seed=5, dtype=dtype, empty_every=4)
    assert smm.CSRMatrix(37, 91, *csr).bandwidth() == bandwidth(csr)
    csr = gen.random_rows(91, 37, 0, 6, seed=6, dtype=dtype)
    assert smm.CSRMatrix(91, 37, *csr).bandwidth() == bandwidth(csr)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_pattern_family_serves_the_reordered_matrix(smm, oracle, dtype):
    csr = gen.poisson3d(40, dtype=dtype)
    n = 64000
    shuffle = shuffle_of(n)
    assert bandwidth(csr, shuffle)[1] > 65536  # (106 203: more offsets than the CODES encoding takes)
    A = make(smm, csr).permute(shuffle.astype(np.int32))
    assert A.bandwidth() == bandwidth(csr, shuffle)
    assert code_of(lambda: A.set_kernel(smm.SPMV_PATTERN)) == INVALID
    perm, info = A.rcm()
    print(np.dtype(dtype).name, "shuffled 40^3 Laplacian:", info)
    B = A.permute(perm)
    assert B.bandwidth()[0] == info["bandwidth_after"] <= 1600
    B.set_kernel(smm.SPMV_PATTERN, 1)
    encoding, offsets = B.pattern_info()
    assert encoding != NONE and offsets == B.bandwidth()[1] <= 65536
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(dtype)
    px = np.ascontiguousarray(x[shuffle][perm])  # P x: entry i is the old entry of the row that became row i
    y = np.zeros(n, dtype=dtype)
    B.rMult(px, y)
    start, pos = B.get_pattern()
    np.testing.assert_array_equal(y, oracle.spmv((start, pos, B.get_values()), 0, None, px))  # bit for bit at one lane per row
    # ... and it is the product with the unshuffled matrix, renumbered
    np.testing.assert_array_equal(y, oracle.spmv(permute(permute(csr, shuffle), perm), 0, None, px))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals_leave_perm_untouched(smm, dtype):
    lib = _lib.load()
    perm = np.full(8, -7, dtype=np.int32)
    ptr = perm.ctypes.data_as(ctypes.c_void_p)
    none = ctypes.POINTER(ctypes.c_int)()
    none64 = ctypes.POINTER(ctypes.c_longlong)()
    W = smm.CSRMatrix(3, 4, np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 1, 3], dtype=np.int32), np.ones(3, dtype=dtype))
    assert lib.smm_hip_csr_rcm(W._h, ptr, 3, 1, none, none, none64, none64) == INVALID
    assert code_of(lambda: W.rcm()) == INVALID
    csr = rcm_case("three_components", dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    big = np.full(n, -7, dtype=np.int32)
    assert lib.smm_hip_csr_rcm(A._h, big.ctypes.data_as(ctypes.c_void_p), n - 1, 1, none, none, none64, none64) == INVALID
    assert lib.smm_hip_csr_rcm(A._h, ctypes.c_void_p(0), n, 1, none, none, none64, none64) == INVALID
    # a column outside the matrix in caller-owned device arrays: found by the device flag, never addressed
    bad = csr[1].copy()
    bad[len(bad) // 2] = n
    d_start, d_pos, d_val = (torch.from_numpy(a).to("cuda:0") for a in (csr[0], bad, csr[2]))
    D = smm.CSRMatrix.from_device(n, n, d_start, d_pos, d_val, dtype)
    assert lib.smm_hip_csr_rcm(D._h, big.ctypes.data_as(ctypes.c_void_p), n, 1, none, none, none64, none64) == INVALID
    d_perm = carve_like(np.full(n, -7, dtype=np.int32), 2, device="cuda:0")
    assert code_of(lambda: D.rcm_dev(d_perm)) == INVALID
    assert code_of(lambda: D.bandwidth()) == INVALID
    torch.cuda.synchronize()
    assert (perm == -7).all() and (big == -7).all() and bool((d_perm == -7).all())
    assert_guards_intact(d_perm, "perm")
    # the information outputs are optional
    good = np.zeros(n, dtype=np.int32)
    assert lib.smm_hip_csr_rcm(A._h, good.ctypes.data_as(ctypes.c_void_p), n, 1, none, none, none64, none64) == 0
    np.testing.assert_array_equal(good, restated("three_components")[0])
