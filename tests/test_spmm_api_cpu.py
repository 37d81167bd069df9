"""No GPU needed: the Python forms for several right-hand sides exist and check their blocks before the library is touched, and
tests/cpp/spmm_case.cpp compiles against the drop-in header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sparse_matrix_math_amd as smm
from sparse_matrix_math_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeMatrix:
    """what the wrappers read of a CSRMatrix; the null handle would fail any library call, and none may be made"""

    def __init__(self, rows, cols, dtype):
        self.rows, self.cols, self.dtype = rows, cols, np.dtype(dtype)
        self._suf = host._suffix(dtype)
        self._h = ctypes.c_void_p(0)

    rMultBlock = smm.CSRMatrix.rMultBlock
    rMultAddBlock = smm.CSRMatrix.rMultAddBlock
    rMultSubBlock = smm.CSRMatrix.rMultSubBlock
    _spmm = smm.CSRMatrix._spmm


@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(host, "_fn", touched)


def test_wrappers_exist():
    for name in ("rMultBlock", "rMultAddBlock", "rMultSubBlock", "spmm_dev"):
        assert callable(getattr(smm.CSRMatrix, name))
    for name in ("BiCGStabBatch", "ConjugateGradientBatch", "bicgstab_batch_dev", "cg_batch_dev"):
        assert callable(getattr(smm, name))
    assert smm.MAX_RHS == 8


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_blocks_are_checked_before_the_library(no_library, dtype):
    A = FakeMatrix(6, 6, dtype)
    good = np.zeros((6, 4), dtype=dtype)
    with pytest.raises(ValueError):  # k out of range
        A.rMultBlock(np.zeros((6, 9), dtype=dtype), np.zeros((6, 9), dtype=dtype))
    with pytest.raises(ValueError):
        A.rMultBlock(np.zeros((6, 0), dtype=dtype), np.zeros((6, 0), dtype=dtype))
    with pytest.raises(ValueError):  # blocks of different k
        A.rMultAddBlock(np.zeros((6, 3), dtype=dtype), good, good.copy())
    with pytest.raises(ValueError):  # wrong number of rows
        A.rMultBlock(np.zeros((5, 4), dtype=dtype), good)
    with pytest.raises(TypeError):  # not C-contiguous: a transposed view, a strided slice
        A.rMultBlock(np.zeros((4, 6), dtype=dtype).T, good)
    with pytest.raises(TypeError):
        A.rMultSubBlock(good, np.zeros((6, 8), dtype=dtype)[:, ::2], good.copy())
    with pytest.raises(TypeError):  # one vector is not a block
        A.rMultBlock(np.zeros(6, dtype=dtype), good)
    with pytest.raises(TypeError):  # dtype
        A.rMultBlock(np.zeros((6, 4), dtype=np.int32), good)
    for call in (lambda B, X: smm.BiCGStabBatch(A, B, X, 3, 1e-6), lambda B, X: smm.ConjugateGradientBatch(A, B, X, X, 3, 1e-6)):
        with pytest.raises(ValueError):
            call(np.zeros((6, 9), dtype=dtype), np.zeros((6, 9), dtype=dtype))
        with pytest.raises(ValueError):
            call(good, np.zeros((6, 3), dtype=dtype))
        with pytest.raises(TypeError):
            call(np.asfortranarray(np.ones((6, 4), dtype=dtype)), good)
        with pytest.raises(TypeError):
            call(good, np.zeros((6, 8), dtype=dtype)[:, ::2])


def test_header_case_compiles():
    """tests/cpp/spmm_case.cpp against include/smm_hip/sparse_matrix_math.h: rMult(X, Out, k), SMM::BiCGStabBatch, SMM::ConjugateGradientBatch"""
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(ROOT, "tests", "cpp", "spmm_case.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
