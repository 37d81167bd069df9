"""The BLOCKS SpMV family on the GPU: detection against the numpy restatement of the fit rule, results bit for bit those of STREAM at
one lane per row (and the oracle's), offset views inside guard bands, value edits, the fused epilogues through the solver loops,
two host threads on one handle, and the bytes kernel_desc reports."""
import ctypes
import threading

import numpy as np
import pytest
import torch
from blocks_cases import BIT_SHAPES, MUTATIONS, blocked, mutated
from blocks_restatement import fits, largest_fit
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres

from oracle.oracle import PRECOND_JACOBI
from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
DEV = "cuda:0"
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731
_LIMITS = {}


def limits(smm):
    """{b: max_row_entries} as blocks_info reports them for a matrix that fits"""
    if not _LIMITS:
        for b in (2, 3, 4):
            csr, rows, cols = blocked("tiny", b)
            A = smm.CSRMatrix(rows, cols, *csr)
            assert A.blocks_info() == (0, 0, 0)
            assert A.find_blocks(b) == b
            size, blocks, cap = A.blocks_info()
            assert size == b and blocks == len(csr[1]) // (b * b) and cap >= 256 and cap % b == 0
            _LIMITS[b] = cap
    return _LIMITS


def vectors(rows, cols, dtype, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, cols).astype(dtype), rng.uniform(-1, 1, rows).astype(dtype)


def run(A, op, lhs, x):
    out = np.full(A.rows, np.nan, dtype=A.dtype)
    (A.rMult if op == 0 else A.rMultAdd if op == 1 else A.rMultSub)(*(([] if op == 0 else [lhs]) + [x, out]))
    return out


# ---- 1. detection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_detection_equals_the_restatement(smm, dtype):
    lim = limits(smm)
    cases = [(f"{name}/{b}", blocked(name, b, dtype)) for name in BIT_SHAPES + ["base"] for b in (2, 3, 4)]
    cases += [(f"{kind}/{b}", mutated(kind, b, dtype)) for kind in MUTATIONS for b in (2, 3, 4)]
    cases += [("six", blocked("six", 6, dtype))]
    for label, (csr, rows, cols) in cases:
        for ask in (0, 2, 3, 4):
            A = smm.CSRMatrix(rows, cols, *csr)  # a fresh handle: a miss leaves an earlier analysis in place
            want = largest_fit(csr[0], csr[1], rows, cols, lim) if ask == 0 else (ask if fits(csr[0], csr[1], rows, cols, ask, lim[ask]) else 0)
            got = A.find_blocks(ask)
            assert got == want, (label, ask, got, want)
            assert A.blocks_info()[0] == want
    csr, rows, cols = blocked("six", 6, dtype)
    assert smm.CSRMatrix(rows, cols, *csr).find_blocks(0) == 3


def test_a_later_size_replaces_the_analysis(smm):
    csr, rows, cols = blocked("wave", 4)
    A = smm.CSRMatrix(rows, cols, *csr)
    assert A.find_blocks(0) == 4 and A.find_blocks(2) == 2
    assert A.blocks_info()[:2] == (2, len(csr[1]) // 4)
    assert A.find_blocks(3) == 0 and A.blocks_info()[0] == 2  # a miss leaves the kept analysis in place


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_a_miss_is_refused_by_set_kernel(smm, dtype):
    csr, rows, cols = mutated("column_shifted", 3, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)
    before = A.get_kernel()
    assert A.find_blocks(0) == 0
    with pytest.raises(_lib.SmmHipError):
        A.set_kernel(smm.SPMV_BLOCKS)
    assert A.get_kernel() == before
    with pytest.raises(_lib.SmmHipError):
        A.find_blocks(5)
    csr, rows, cols = blocked("wave", 3, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)
    with pytest.raises(_lib.SmmHipError):
        A.set_kernel(smm.SPMV_BLOCKS, 2)  # one lane per block row only
    A.set_kernel(smm.SPMV_BLOCKS, 1)  # runs the analysis itself
    assert A.get_kernel() == (4, 1) and A.blocks_info()[0] == 3


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------
def bit_cases(smm, b, dtype):
    full = limits(smm)[b] // b
    return [(name, blocked(name, b, dtype)) for name in BIT_SHAPES] + [("full", blocked("full", b, dtype, full))]


@pytest.mark.parametrize("op", [0, 1, 2], ids=["ASSIGN", "ADD", "SUB"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("b", [2, 3, 4])
def test_bits_equal_stream_and_the_oracle(smm, oracle, b, dtype, op):
    for name, (csr, rows, cols) in bit_cases(smm, b, dtype):
        x, lhs = vectors(rows, cols, dtype)
        A = smm.CSRMatrix(rows, cols, *csr)
        A.set_kernel(smm.SPMV_STREAM, 1)
        want = run(A, op, lhs, x)
        A.set_kernel(smm.SPMV_BLOCKS)
        assert A.get_kernel() == (4, 1) and A.blocks_info()[0] >= b, name
        got = run(A, op, lhs, x)
        np.testing.assert_array_equal(got, want, err_msg=name)
        np.testing.assert_array_equal(got, oracle.spmv(csr, op, lhs if op else None, x), err_msg=name)
        if name == "full":
            assert int(np.diff(csr[0]).max()) == limits(smm)[b]


@pytest.mark.parametrize("b", [2, 3, 4])
def test_a_longer_row_does_not_fit(smm, b):
    csr, rows, cols = blocked("overfull", b, np.float64, limits(smm)[b] // b)
    assert int(np.diff(csr[0]).max()) == limits(smm)[b] + b
    A = smm.CSRMatrix(rows, cols, *csr)
    assert A.find_blocks(b) == 0


def test_fma_flavour_holds_the_bit_contract(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it): BLOCKS equals the fma oracle's chain"""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    for dtype, suf in ((np.float32, "f32"), (np.float64, "f64")):
        for b in (2, 3, 4):
            csr, rows, cols = blocked("tiles", b, dtype)
            x, lhs = vectors(rows, cols, dtype)
            h, found = P(), ctypes.c_int()
            assert getattr(lib, f"smm_hip_csr_create_{suf}")(rows, cols, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
            assert lib.smm_hip_csr_find_blocks(h, b, ctypes.byref(found)) == 0 and found.value == b
            assert lib.smm_hip_csr_set_kernel(h, 4, 0) == 0, lib.smm_hip_last_error()
            out = np.zeros(rows, dtype=dtype)
            assert getattr(lib, f"smm_hip_spmv_{suf}")(h, 2, ptr(lhs), ptr(x), ptr(out)) == 0, lib.smm_hip_last_error()
            np.testing.assert_array_equal(out, oracle_fma.spmv(csr, 2, lhs, x))
            lib.smm_hip_csr_destroy(h)


# ---- 3. range -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("b", [2, 3, 4])
def test_offset_views_inside_guard_bands(smm, b, dtype):
    csr, rows, cols = blocked("tiles", b, dtype)
    x, lhs = vectors(rows, cols, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)
    A.set_kernel(smm.SPMV_BLOCKS)
    stream = torch.cuda.current_stream().cuda_stream
    for op in (0, 1, 2):
        want = run(A, op, lhs, x)
        d_x = carve_like(x, fit(1, dtype), device=DEV)  # one element past a 16-byte boundary
        d_lhs = carve_like(lhs, fit(3, dtype), device=DEV)
        d_out = carve_like(np.zeros(rows, dtype=dtype), fit(1, dtype), device=DEV)
        assert d_x.data_ptr() % 16 == np.dtype(dtype).itemsize
        saved = [snapshot(d_x), snapshot(d_lhs)]
        A.spmv_dev(op, d_lhs if op else None, d_x, d_out, stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy(), want)
        assert_unchanged(d_x, saved[0], "x")
        assert_unchanged(d_lhs, saved[1], "lhs")
        for name, view in (("x", d_x), ("lhs", d_lhs), ("out", d_out)):
            assert_guards_intact(view, name)


# ---- 4. edits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_value_edits_need_no_refresh(smm, dtype):
    b = 3
    csr, rows, cols = blocked("tiles", b, dtype)
    x, lhs = vectors(rows, cols, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)  # the BLOCKS handle that is edited
    S = smm.CSRMatrix(rows, cols, *csr)  # the same edits under STREAM at one lane per row
    A.set_kernel(smm.SPMV_BLOCKS)
    S.set_kernel(smm.SPMV_STREAM, 1)
    rng = np.random.default_rng(8)
    er = rng.integers(0, rows, 50).astype(np.int32)
    ec = np.array([csr[1][csr[0][r]] if csr[0][r + 1] > csr[0][r] else 0 for r in er], dtype=np.int32)
    ev = rng.uniform(-2, 2, 50).astype(dtype)
    fresh = rng.uniform(-1, 1, len(csr[2])).astype(dtype)
    for step in ("scale", "update_entries", "set_values"):
        for M in (A, S):
            if step == "scale":
                M.scale(1.5)
            elif step == "update_entries":
                M.update_entries(er, ec, ev)
            else:
                M.set_values(fresh)
        np.testing.assert_array_equal(run(A, 1, lhs, x), run(S, 1, lhs, x), err_msg=step)
    assert A.get_kernel() == (4, 1)
    A.set_kernel(smm.SPMV_STREAM, 1)  # and on the edited handle itself
    want = run(A, 1, lhs, x)
    A.set_kernel(smm.SPMV_BLOCKS)
    np.testing.assert_array_equal(run(A, 1, lhs, x), want)


# ---- 5. solvers: the fused epilogues ------------------------------------------------------------------------------------------------
_SYSTEMS = {}


def system(dtype, symmetric):
    """b = 3, 400 block rows, diagonally dominant; symmetric: A + A^T on the symmetrised block pattern, made dominant again"""
    key = (np.dtype(dtype).name, symmetric)
    if key not in _SYSTEMS:
        s, p, _ = gen.random_rows(400, 400, 3, 6, seed=31, diag_dominant=True)
        if symmetric:
            mask = np.zeros((400, 400), dtype=bool)
            mask[np.repeat(np.arange(400), np.diff(s)), p] = True
            mask |= mask.T
            s = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
            p = np.nonzero(mask)[1].astype(np.int32)
        start, pos, val = gen.block_expand(s, p, 3, seed=32, dtype=np.float64, diag_dominant=not symmetric)
        if symmetric:
            n = 1200
            rows_of = np.repeat(np.arange(n), np.diff(start))
            D = np.zeros((n, n))
            D[rows_of, pos] = val
            D = D + D.T
            np.fill_diagonal(D, 0.0)
            np.fill_diagonal(D, np.abs(D).sum(axis=1) + 1.0)
            val = D[rows_of, pos]
        _SYSTEMS[key] = (start, pos, val.astype(dtype))
    return _SYSTEMS[key]


def deviation_bound(d_stream, scale, dtype):
    """the two runs differ only in how the fused dots are grouped over workgroups: 8 x STREAM's own deviation + 16 eps of the scale"""
    return 8 * d_stream + 16 * float(np.finfo(dtype).eps) * scale


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "bicgstab_jacobi", "gmres"])
def test_solver_loops_on_a_blocks_handle(smm, oracle, solver, dtype):
    IT, EPS = 5, 1e-30
    csr = system(dtype, solver == "cg")
    n = len(csr[0]) - 1
    rhs = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(n, dtype=dtype)
    if solver == "cg":
        st_o, x_o, it_o, _ = oracle.cg(csr, rhs, zero, IT, EPS)
    elif solver == "bicgstab":
        st_o, x_o, it_o, _ = oracle.bicgstab(csr, rhs, zero, IT, EPS)
    elif solver == "bicgstab_jacobi":
        st_o, x_o, it_o, _ = oracle.bicgstab(csr, rhs, zero, IT, EPS, PRECOND_JACOBI, oracle.jacobi_setup(csr)[1])
    else:
        st_o, x_o, it_o, _ = gmres(oracle, csr, rhs, zero, IT, EPS, 10)
    A = smm.CSRMatrix(n, n, *csr)
    got = {}
    for family in ("STREAM", "BLOCKS"):
        if family == "STREAM":
            A.set_kernel(smm.SPMV_STREAM, 1)
        else:
            A.set_kernel(smm.SPMV_BLOCKS)
            assert A.get_kernel() == (4, 1) and A.blocks_info()[0] == 3
        x, info = zero.copy(), {}
        if solver == "cg":
            st = smm.ConjugateGradient(A, rhs, zero, x, IT, EPS, info=info)
        elif solver == "bicgstab":
            st = smm.BiCGStab(A, rhs, x, IT, EPS, info=info)
        elif solver == "bicgstab_jacobi":
            st = smm.BiCGStab(A, rhs, x, IT, EPS, A.getPreconditioner(smm.SolverPreconditioner.JACOBI), info=info)
        else:
            st = smm.GMRES(A, rhs, x, IT, EPS, restart=10, info=info)
        assert (int(st), info["iterations"]) == (st_o, it_o), (family, int(st), info, st_o, it_o)
        got[family] = x
    if solver == "gmres":  # no oracle: the true residuals b - A x (float64) against the restatement's, on the scale of b
        dense = np.zeros((n, n))
        dense[np.repeat(np.arange(n), np.diff(csr[0])), csr[1]] = csr[2]
        res = lambda x: rhs.astype(np.float64) - dense @ x.astype(np.float64)  # noqa: E731
        d_s, d_b = (float(np.max(np.abs(res(got[f]) - res(x_o)))) for f in ("STREAM", "BLOCKS"))
        scale = float(np.max(np.abs(rhs)))
    else:
        d_s, d_b = (float(np.max(np.abs(got[f].astype(np.float64) - x_o))) for f in ("STREAM", "BLOCKS"))
        scale = float(np.max(np.abs(x_o)))
    print(solver, np.dtype(dtype).name, "d_STREAM", d_s, "d_BLOCKS", d_b, "bound", deviation_bound(d_s, scale, dtype))
    assert d_b <= deviation_bound(d_s, scale, dtype)


def test_bicgstab_converges_to_ones(smm):
    eps = 1e-8
    csr = system(np.float64, False)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    A.set_kernel(smm.SPMV_BLOCKS)
    x, info = np.zeros(n), {}
    st = smm.BiCGStab(A, gen.row_sums(csr[0], csr[2]), x, -1, eps, info=info)
    assert int(st) == 0 and 0 < info["iterations"] < n
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)  # the all-ones check of tests/test_gpu_solvers.py


# ---- 6. concurrency -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_two_threads_on_one_handle(smm, dtype):
    csr, rows, cols = blocked("tiles", 3, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)
    A.set_kernel(smm.SPMV_BLOCKS)
    xs = [vectors(rows, cols, dtype, seed=40 + i) for i in range(2)]
    want = [run(A, 1, lhs, x) for x, lhs in xs]
    d_x = [torch.from_numpy(x).to(DEV) for x, _ in xs]
    d_lhs = [torch.from_numpy(lhs).to(DEV) for _, lhs in xs]
    LOOPS = 20
    d_out = [[torch.zeros(rows, dtype=d_x[0].dtype, device=DEV) for _ in range(LOOPS)] for _ in range(2)]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    gate, errors = threading.Barrier(2), []

    def body(i):
        try:
            gate.wait()
            for j in range(LOOPS):
                A.spmv_dev(1, d_lhs[i], d_x[i], d_out[i][j], streams[i].cuda_stream)
            streams[i].synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append((i, e))

    pool = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for t in pool:
        t.start()
    for t in pool:
        t.join()
    assert not errors, errors
    for i in range(2):
        for j in range(LOOPS):
            np.testing.assert_array_equal(d_out[i][j].cpu().numpy(), want[i], err_msg=f"thread {i}, SpMV {j}")


# ---- 7. kernel_desc -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("b", [2, 3, 4])
def test_kernel_desc_prices_the_blocks_layout(smm, b, dtype):
    csr, rows, cols = blocked("wide", b, dtype)
    A = smm.CSRMatrix(rows, cols, *csr)
    assert A.find_blocks(b) == b
    A.set_kernel(smm.SPMV_BLOCKS)
    nnz, s = len(csr[1]), np.dtype(dtype).itemsize
    assert A.kernel_desc() == ("spmvBlocksKernel", nnz * s + (nnz // (b * b)) * 4 + (rows // b + 1) * 4 + cols * s + rows * s)
