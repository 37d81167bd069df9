"""GPU tests of BiCGStabBatch / ConjugateGradientBatch (csrc/smm_solvers_batch.hip): every column of a block solve against the
single-vector solve of that column (status, iteration count) and against the reference algorithm (x, within the allowances
test_gpu_solvers.py uses); columns that leave the loop at different times, frozen columns, isolation of a NaN column."""
import numpy as np
import pytest
from test_gpu_solvers import RTOL, bicgstab_sensitivity, close, make
from test_oracle import gen_matrices

from oracle.oracle import PRECOND_JACOBI, PRECOND_NONE
from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
MATRICES = ["poisson2d_32", "banded_2000", "convdiff3d_12"]  # (ragged_300 has empty rows: skipped as in test_gpu_solvers.py)
SCALES = [1.0, 0.5, 2.0, -1.0, 0.25, -3.0, 1.5, 4.0]


def rhs_block(csr, k, dtype, seed=17):
    """b_j = row sums of A * s_j + a seeded random vector"""
    start, _, val = csr
    rows = len(start) - 1
    rng = np.random.default_rng(seed)
    B = np.empty((rows, k), dtype=dtype)
    sums = gen.row_sums(start, val)
    for j in range(k):
        B[:, j] = sums * dtype(SCALES[j]) + rng.uniform(-1, 1, rows).astype(dtype)
    return B


def column(B, j):
    return np.ascontiguousarray(B[:, j])


def check_bicgstab_fixed(smm, oracle, csr, A, k, it, dtype, jacobi):
    P = smm.SolverPreconditioner
    rows = A.rows
    M = A.getPreconditioner(P.JACOBI) if jacobi else None
    ocode = (PRECOND_JACOBI, oracle.jacobi_setup(csr)[1]) if jacobi else (PRECOND_NONE, None)
    B = rhs_block(csr, k, dtype)
    X = np.zeros((rows, k), dtype=dtype)
    info = {}
    sts = smm.BiCGStabBatch(A, B.copy(), X, it, 1e-30, M, info=info)
    assert len(sts) == k and info["iterations"].shape == (k,) and info["resnorm"].shape == (k,)
    for j in range(k):
        b = column(B, j)
        x1 = np.zeros(rows, dtype=dtype)
        i1 = {}
        st1 = smm.BiCGStab(A, b.copy(), x1, it, 1e-30, M, info=i1)
        assert int(sts[j]) == int(st1) and info["iterations"][j] == i1["iterations"] == it, (j, it)
        ref = oracle.bicgstab(csr, b, np.zeros(rows, dtype=dtype), it, 1e-30, *ocode)[1].astype(np.float64)
        allowed = max(RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))), 4 * bicgstab_sensitivity(oracle, csr, b, it, *ocode))
        err = float(np.max(np.abs(X[:, j].astype(np.float64) - ref)))
        assert err <= allowed, (j, it, jacobi, err, allowed)


@pytest.mark.parametrize("mname", MATRICES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_iterations_bicgstab(smm, oracle, dtype, mname):
    csr = gen_matrices(dtype)[mname]
    A = make(smm, csr)
    for jacobi in (False, True):
        for it in (1, 3, 10):
            check_bicgstab_fixed(smm, oracle, csr, A, 4, it, dtype, jacobi)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_iterations_bicgstab_k3_k8(smm, oracle, dtype):
    csr = gen_matrices(dtype)["convdiff3d_12"]
    A = make(smm, csr)
    for k in (3, 8):
        check_bicgstab_fixed(smm, oracle, csr, A, k, 3, dtype, True)


@pytest.mark.parametrize("mname", ["poisson2d_32", "banded_2000"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_iterations_cg(smm, oracle, dtype, mname):
    csr = gen_matrices(dtype)[mname]
    A = make(smm, csr)
    rows = A.rows
    for k, its in ((4, (1, 3, 10)), (3, (3,)), (8, (3,))):
        B = rhs_block(csr, k, dtype)
        for it in its:
            X = np.full((rows, k), 123, dtype=dtype)
            info = {}
            sts = smm.ConjugateGradientBatch(A, B, np.zeros((rows, k), dtype=dtype), X, it, 0.0, info=info)
            for j in range(k):
                b = column(B, j)
                x1 = np.full(rows, 123, dtype=dtype)
                i1 = {}
                st1 = smm.ConjugateGradient(A, b, np.zeros(rows, dtype=dtype), x1, it, 0.0, info=i1)
                assert int(sts[j]) == int(st1) == 2 and info["iterations"][j] == i1["iterations"] == it
                ref = oracle.cg(csr, b, np.zeros(rows, dtype=dtype), it, 0.0)[1].astype(np.float64)
                assert close(X[:, j], ref, dtype), (mname, k, it, j)


def true_residual(csr, b, x):
    start, pos, val = csr
    rows = len(start) - 1
    ax = np.zeros(rows)
    np.add.at(ax, np.repeat(np.arange(rows), np.diff(start)), val.astype(np.float64) * x.astype(np.float64)[pos])
    return float(np.linalg.norm(b.astype(np.float64) - ax))


@pytest.mark.parametrize("solver", ["bicgstab", "cg"])
def test_columns_leave_at_different_times(smm, solver):
    dtype, eps = np.float64, 1e-8
    csr = gen.convdiff3d(12, 0.3, dtype=dtype) if solver == "bicgstab" else gen.poisson2d(32, dtype=dtype)
    A = make(smm, csr)
    rows, k = A.rows, 4
    rng = np.random.default_rng(23)
    base = gen.row_sums(csr[0], csr[2])
    B = np.empty((rows, k), dtype=dtype)
    for j, scale in enumerate((1.0, 1e-3, 1e-6, 1.0)):
        B[:, j] = (base + rng.uniform(-1, 1, rows)) * scale

    def run(maxit):
        X = np.zeros((rows, k), dtype=dtype)
        info = {}
        if solver == "bicgstab":
            sts = smm.BiCGStabBatch(A, B.copy(), X, maxit, eps, info=info)
        else:
            sts = smm.ConjugateGradientBatch(A, B, np.zeros((rows, k), dtype=dtype), X, maxit, eps, info=info)
        return sts, info["iterations"], X

    sts, its, X = run(-1)
    assert len(set(int(i) for i in its)) > 1, its
    # freeze, exact: stop the whole batch where the first column left; that column's x is bit for bit the same.  (Run back to back: the
    # partial sums of a column follow the tile table, and a single-vector solve in between may re-cut it for its own kernel.)
    first = int(np.argmin(its))
    sts2, its2, X2 = run(int(its[first]))
    assert int(its2[first]) == int(its[first]) and int(sts2[first]) == 0
    np.testing.assert_array_equal(X2[:, first], X[:, first])
    for j in range(k):
        b = column(B, j)
        x1 = np.zeros(rows, dtype=dtype)
        i1 = {}
        if solver == "bicgstab":
            st1 = smm.BiCGStab(A, b.copy(), x1, -1, eps, info=i1)
        else:
            st1 = smm.ConjugateGradient(A, b, np.zeros(rows, dtype=dtype), x1, -1, eps, info=i1)
        assert int(sts[j]) == int(st1) == 0
        assert abs(int(its[j]) - i1["iterations"]) <= max(2, i1["iterations"] // 5), (j, its, i1)
        res = true_residual(csr, b, X[:, j])
        print(f"{solver} column {j}: iterations {its[j]} (single {i1['iterations']}), ||b - A x|| = {res:.3e}")
        assert res <= 10 * eps, (j, res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_isolation_bicgstab(smm, oracle, dtype):
    csr = gen.poisson2d(32, dtype=dtype)
    A = make(smm, csr)
    rows, k, it = A.rows, 4, 10
    B = rhs_block(csr, k, dtype)
    X0 = np.zeros((rows, k), dtype=dtype)
    B[:, 1] = gen.row_sums(csr[0], csr[2])  # b = A * ones and x0 = ones: an exact start (rr0 == 0 -> NaN after one pass)
    X0[:, 1] = 1
    B[:, 2] = 0                             # b = 0, x0 = 0
    X = X0.copy()
    info = {}
    sts = smm.BiCGStabBatch(A, B.copy(), X, it, 1e-30, info=info)
    for j in range(k):
        b = column(B, j)
        x1 = column(X0, j).copy()
        i1 = {}
        st1 = smm.BiCGStab(A, b.copy(), x1, it, 1e-30, info=i1)
        assert int(sts[j]) == int(st1) and info["iterations"][j] == i1["iterations"], j
        np.testing.assert_array_equal(np.isnan(X[:, j]), np.isnan(x1), err_msg=f"column {j}")
    assert info["iterations"][1] == 1 and np.isnan(X[:, 1]).all()  # edge/.../bicgstab_exact_x0
    for j in (0, 3):
        b = column(B, j)
        assert np.isfinite(X[:, j]).all() and info["iterations"][j] == it
        ref = oracle.bicgstab(csr, b, np.zeros(rows, dtype=dtype), it, 1e-30, PRECOND_NONE, None)[1].astype(np.float64)
        allowed = max(RTOL[dtype] * max(1.0, float(np.max(np.abs(ref)))), 4 * bicgstab_sensitivity(oracle, csr, b, it, PRECOND_NONE, None))
        assert float(np.max(np.abs(X[:, j].astype(np.float64) - ref))) <= allowed, j


@pytest.mark.parametrize("dtype", DTYPES)
def test_isolation_cg_and_iteration_limits(smm, dtype):
    csr = gen.poisson2d(32, dtype=dtype)
    A = make(smm, csr)
    rows, k = A.rows, 4
    B = rhs_block(csr, k, dtype)
    X0 = np.zeros((rows, k), dtype=dtype)
    B[:, 2] = gen.row_sums(csr[0], csr[2])  # exact start: 0 iterations, SUCCESS, x untouched (ref:2342-2344)
    X0[:, 2] = 1
    X = np.full((rows, k), 7, dtype=dtype)
    info = {}
    sts = smm.ConjugateGradientBatch(A, B, X0, X, 3, 1e-3, info=info)
    assert int(sts[2]) == 0 and info["iterations"][2] == 0
    np.testing.assert_array_equal(X[:, 2], 7)
    for j in (0, 1, 3):
        x1 = np.full(rows, 7, dtype=dtype)
        i1 = {}
        st1 = smm.ConjugateGradient(A, column(B, j), column(X0, j), x1, 3, 1e-3, info=i1)
        assert int(sts[j]) == int(st1) and info["iterations"][j] == i1["iterations"] == 3
        assert close(X[:, j], x1.astype(np.float64), dtype), j
    # maxIterations == 0: CG leaves x alone (MAX_ITERATIONS_REACHED, 0 passes); BiCGStab runs its body once (ref:2277-2281)
    X = np.full((rows, k), 7, dtype=dtype)
    sts = smm.ConjugateGradientBatch(A, B, X0, X, 0, 1e-6, info=info)
    assert [int(s) for s in sts] == [2, 2, 0, 2] and list(info["iterations"]) == [0] * k
    np.testing.assert_array_equal(X, 7)
    X = np.zeros((rows, k), dtype=dtype)
    sts = smm.BiCGStabBatch(A, B.copy(), X, 0, 1e-6, info=info)
    assert [int(s) for s in sts] == [2] * k and list(info["iterations"]) == [1] * k
    # maxIterations == -1 means rows, per column as in the single forms
    eps = 1e-3 if dtype == np.float32 else 1e-8
    Xc = np.zeros((rows, k), dtype=dtype)
    ic = {}
    stc = smm.ConjugateGradientBatch(A, B, np.zeros((rows, k), dtype=dtype), Xc, -1, eps, info=ic)
    Xb = np.zeros((rows, k), dtype=dtype)
    ib = {}
    stb = smm.BiCGStabBatch(A, B.copy(), Xb, -1, eps, info=ib)
    for j in range(k):
        i1 = {}
        st1 = smm.ConjugateGradient(A, column(B, j), np.zeros(rows, dtype=dtype), np.zeros(rows, dtype=dtype), -1, eps, info=i1)
        assert int(stc[j]) == int(st1) == 0 and abs(int(ic["iterations"][j]) - i1["iterations"]) <= max(2, i1["iterations"] // 5)
        st1 = smm.BiCGStab(A, column(B, j).copy(), np.zeros(rows, dtype=dtype), -1, eps, info=i1)
        assert int(stb[j]) == int(st1) == 0 and abs(int(ib["iterations"][j]) - i1["iterations"]) <= max(2, i1["iterations"] // 5)


def test_rejected_arguments(smm):
    P = smm.SolverPreconditioner
    csr = gen.poisson2d(32, dtype=np.float64)
    A = make(smm, csr)
    rows, k = A.rows, 4
    B = rhs_block(csr, k, np.float64)
    X = np.zeros((rows, k))
    for kind in (P.SYMMETRIC_GAUS_SEIDEL, P.ILU0, P.IC0, P.BLOCK_ILU0, P.BLOCK_SGS):
        M = A.getPreconditioner(kind)
        with pytest.raises(smm.SmmHipError) as e:
            smm.BiCGStabBatch(A, B.copy(), X, 3, 1e-30, M)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID, kind
        assert "JACOBI" in str(e.value)
    for call in (lambda: smm.bicgstab_batch_dev(A, 9, None, None, 3, 1e-30), lambda: smm.cg_batch_dev(A, 9, None, None, None, 3, 1e-30)):
        with pytest.raises(smm.SmmHipError) as e:
            call()
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID
    # NONE is the identity: the same numbers as no preconditioner
    Xn = np.zeros((rows, k))
    smm.BiCGStabBatch(A, B.copy(), Xn, 3, 1e-30, A.getPreconditioner(P.NONE))
    smm.BiCGStabBatch(A, B.copy(), X, 3, 1e-30)
    np.testing.assert_array_equal(Xn, X)
