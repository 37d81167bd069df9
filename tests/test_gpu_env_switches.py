"""SMM_HIP_SPMV_FAMILY / SMM_HIP_SPMV_LANES are read at every create: in ONE process a handle follows what the environment says when it
is created, and a later handle follows a later change (the once-per-process side is held on the CPU: tests/cpp/env_case.cpp)."""
import numpy as np
import pytest
from test_gpu_spmv import bound

from oracle.oracle import OP_ASSIGN
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu


def test_a_new_handle_follows_the_environment_of_its_create(smm, oracle, monkeypatch):
    monkeypatch.delenv("SMM_HIP_SPMV_FAMILY", raising=False)
    monkeypatch.delenv("SMM_HIP_SPMV_LANES", raising=False)
    dtype = np.float64
    csr = gen.poisson2d(32, dtype=dtype)  # the smallest matrix that reaches the chooser
    rows = len(csr[0]) - 1
    x = np.random.default_rng(7).uniform(-1, 1, rows).astype(dtype)
    ref = oracle.spmv(csr, OP_ASSIGN, None, x)

    def create_and_check():
        A = smm.CSRMatrix(rows, rows, *csr)
        family, lanes = A.get_kernel()
        out = np.zeros(rows, dtype=dtype)
        A.rMult(x, out)
        if lanes == 1:
            np.testing.assert_array_equal(out, ref)
        else:
            assert np.all(np.abs(out - ref) <= bound(csr, x, dtype)), (family, lanes)
        return family, lanes

    first = create_and_check()
    assert first[0] in (smm.SPMV_VECTOR, smm.SPMV_STREAM) and first[1] >= 1
    monkeypatch.setenv("SMM_HIP_SPMV_LANES", "4")
    assert create_and_check() == (first[0], 4)
    monkeypatch.delenv("SMM_HIP_SPMV_LANES")
    monkeypatch.setenv("SMM_HIP_SPMV_FAMILY", str(smm.SPMV_VECTOR))
    assert create_and_check()[0] == smm.SPMV_VECTOR
    monkeypatch.delenv("SMM_HIP_SPMV_FAMILY")
    assert create_and_check() == first
