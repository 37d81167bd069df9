"""Composing and slicing on the device (csrc/smm_compose.hip) through smm.bmat / CSRMatrix.submatrix / diagonal / scale_rows_cols and the C
ABI.  The reference is the CPU restatement (tests/compose_restatement.py, itself checked against dense NumPy by tests/test_compose_cpu.py):
start[], positions[] exactly and the value BITS, in fp32 and fp64."""
import ctypes
import functools

import compose_cases as cases
import compose_restatement as rs
import device_views as dv
import numpy as np
import pytest
import torch

from sparse_matrix_math_amd import _lib

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
STREAM, PATTERN = 2, 3
MASKS, CONST = 1, 3
DEV = "cuda:0"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


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
def block_case(name, dtype):
    """the case and its restatement, built once per session and never written to"""
    case = cases.BLOCK_CASES[name](dtype)
    blocks = [[None if k is None else case["mats"][k][0] for k in row] for row in case["table"]]
    shapes = [[None if k is None else case["mats"][k][1] for k in row] for row in case["table"]]
    want, shape = rs.bmat(blocks, shapes, dtype, case["coef"], case["row_sizes"], case["col_sizes"])
    for arr in want:
        arr.setflags(write=False)
    return case, want, shape


def handles(smm, case):
    """one handle per key (a key in several slots is ONE handle); a transposed key comes from CSRMatrix.transpose()"""
    hs = {}
    for key, (csr, shape) in case["mats"].items():
        if key not in case["transposed"]:
            hs[key] = make(smm, csr, shape)
    for key, of in case["transposed"].items():
        hs[key] = hs[of].transpose()
    return hs, [[None if k is None else hs[k] for k in row] for row in case["table"]]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.BLOCK_CASES))
def test_bmat_every_case_against_the_restatement(smm, name, dtype):
    case, want, shape = block_case(name, dtype)
    hs, table = handles(smm, case)
    K = smm.bmat(table, case["coef"], case["row_sizes"], case["col_sizes"])
    assert_same(arrays(K), want, name)
    F = make(smm, want, shape)
    assert (K.rows, K.cols, K.nnz, K.first_active_start) == (F.rows, F.cols, F.nnz, F.first_active_start) and K.dtype == np.dtype(dtype)
    if name == "leading_empty_rows":
        assert K.first_active_start == 4
    assert_same(arrays(smm.bmat(table, case["coef"], case["row_sizes"], case["col_sizes"])), arrays(K), "second run")
    for h in hs.values():
        h.close()  # the block matrix does not depend on its blocks' lifetime
    assert_same(arrays(K), want, "after the blocks are gone")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hstack_vstack_and_a_copy(smm, dtype):
    case, _, _ = block_case("three_by_three", dtype)
    A, C, D = (case["mats"][k] for k in "ACD")
    hA, hC, hD = (make(smm, *m) for m in (A, C, D))
    assert_same(arrays(smm.hstack([hA, hC])), rs.bmat([[A[0], C[0]]], [[A[1], C[1]]], dtype)[0], "hstack")
    assert_same(arrays(smm.vstack([hA, hD], coef=[-1, 0.5])), rs.bmat([[A[0]], [D[0]]], [[A[1]], [D[1]]], dtype, [-1, 0.5])[0], "vstack")
    copy = smm.bmat([[hA]])
    assert_same(arrays(copy), A[0], "1 x 1")
    assert copy.hasSameNonZeroPattern(hA)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_block_refresh_equals_a_fresh_create(smm, oracle, dtype):
    case, want, shape = block_case("kkt_coefs", dtype)
    hs, table = handles(smm, case)
    K = smm.bmat(table, case["coef"])
    x = np.random.default_rng(5).uniform(-1, 1, shape[1]).astype(dtype)

    def spmv_is_the_oracles(M, csr):
        y = np.zeros(shape[0], dtype=dtype)
        M.set_kernel(STREAM, 1)
        M.rMult(x, y)
        np.testing.assert_array_equal(bits(y), bits(oracle.spmv(csr, 0, None, x)))

    spmv_is_the_oracles(K, want)
    hs["H"].scale(2)
    B = case["mats"]["B"][0]
    rows = np.repeat(np.arange(20), np.diff(B[0]))[:7].astype(np.int32)
    assert hs["B"].update_entries(rows, B[1][:7], np.linspace(3, 4, 7).astype(dtype)).all()
    K.block_refresh(table, case["coef"])
    fresh = smm.bmat(table, case["coef"])
    assert_same(arrays(K), arrays(fresh), "refresh")
    H2 = (case["mats"]["H"][0][0], case["mats"]["H"][0][1], (dtype(2) * case["mats"]["H"][0][2]).astype(dtype))
    B2 = (B[0], B[1], np.concatenate([np.linspace(3, 4, 7).astype(dtype), B[2][7:]]))
    Bt = case["mats"]["Bt"][0]  # (the transpose handle was not refreshed: it keeps the old values)
    restated, _ = rs.bmat([[H2, Bt], [B2, None]], [[(144, 144), (144, 20)], [(20, 144), None]], dtype, case["coef"])
    assert_same(arrays(K), restated, "refresh against the restatement")
    spmv_is_the_oracles(K, restated)
    K.block_refresh(table)  # other coefficients: all ones
    assert_same(arrays(K), rs.bmat([[H2, Bt], [B2, None]], [[(144, 144), (144, 20)], [(20, 144), None]], dtype)[0], "refresh, coef None")
    # refused, nothing changed: another table shape, a slot that is NULL now, a block of another entry count, a handle bmat did not make
    before = arrays(K)
    other = make(smm, *cases.SOURCES["laplacian"](dtype))
    fewer = hs["B"].submatrix(None, slice(0, 100))
    for bad in ([[hs["H"], hs["Bt"], None], [hs["B"], None, None]], [[hs["H"], None], [hs["B"], None]], [[hs["H"], hs["Bt"]], [fewer, None]]):
        with pytest.raises(smm.SmmHipError) as e:
            K.block_refresh(bad)
        assert e.value.code == INVALID
    with pytest.raises(smm.SmmHipError) as e:
        other.block_refresh([[hs["H"]]])
    assert e.value.code == INVALID
    assert_same(arrays(K), before, "after the refusals")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_bmat_errors_leave_out_untouched(smm, dtype):
    case, _, _ = block_case("kkt", dtype)
    hs, _ = handles(smm, case)
    H, B, Bt = hs["H"]._h, hs["B"]._h, hs["Bt"]._h
    other = np.float64 if dtype == np.float32 else np.float32
    W = make(smm, (case["mats"]["B"][0][0], case["mats"]["B"][0][1], case["mats"]["B"][0][2].astype(other)), (20, 144))
    lib = _lib.load()
    suf, wrong = ("f32", "f64") if dtype == np.float32 else ("f64", "f32")
    create = getattr(lib, "smm_hip_csr_block_create_" + suf)

    def refused(p, q, slots, row_sizes=None, col_sizes=None, fn=create):
        out = ctypes.c_void_p(0xDEAD)
        table = (ctypes.c_void_p * len(slots))(*slots)
        rsz = None if row_sizes is None else (ctypes.c_int * len(row_sizes))(*row_sizes)
        csz = None if col_sizes is None else (ctypes.c_int * len(col_sizes))(*col_sizes)
        assert fn(p, q, table, None, rsz, csz, None, ctypes.byref(out)) == INVALID, lib.smm_hip_last_error()
        assert out.value == 0xDEAD

    refused(2, 2, [H, Bt, W._h, None])  # dtype mismatch among the blocks
    refused(2, 2, [H, Bt, B, None], fn=getattr(lib, "smm_hip_csr_block_create_" + wrong))
    refused(1, 2, [H, B])  # heights 144 and 20 in one block row
    refused(2, 1, [H, Bt])  # widths 144 and 20 in one block column
    refused(2, 2, [H, None, None, None])  # block row 1 and block column 1 cannot be derived
    refused(2, 2, [H, None, None, None], row_sizes=[-1, 5])  # ... the column still cannot
    refused(1, 1, [H], row_sizes=[100])  # a size that contradicts the block
    refused(9, 9, [None] * 81)  # more than 64 slots
    refused(0, 1, [None])
    refused(1, 1, [None])  # nothing gives a size
    big = 2**30
    refused(3, 1, [None] * 3, row_sizes=[big, big, big], col_sizes=[4])  # total rows beyond 2^31 - 1
    refused(1, 3, [None] * 3, row_sizes=[4], col_sizes=[big, big, big])
    assert create(1, 1, (ctypes.c_void_p * 1)(H), None, None, None, None, None) == INVALID  # out is null
    with pytest.raises(smm.SmmHipError) as e:
        smm.bmat([[hs["H"], hs["B"]]])
    assert e.value.code == INVALID
    Z = smm.bmat([[None, None]], row_sizes=[3], col_sizes=[2, 5], dtype=dtype)  # legal: a matrix without entries
    assert (Z.rows, Z.cols, Z.nnz) == (3, 7, 0)


# ---- submatrix ----
@functools.lru_cache(maxsize=None)
def source(name, dtype):
    csr, shape = cases.SOURCES[name](dtype)
    for arr in csr:
        arr.setflags(write=False)
    return csr, shape


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.SUB_CASES))
def test_submatrix_every_case_against_the_restatement(smm, name, dtype):
    src, rows, cols = cases.SUB_CASES[name]
    csr, shape = source(src, dtype)
    A = make(smm, csr, shape)
    want, out_shape, _ = rs.submatrix(csr, shape, rows, cols)
    S = A.submatrix(rows, cols)
    assert_same(arrays(S), want, name)
    assert (S.rows, S.cols, S.nnz) == (*out_shape, len(want[1]))
    F = make(smm, want, out_shape)
    assert S.first_active_start == F.first_active_start
    A.close()
    assert_same(arrays(S), want, "after the source is gone")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", sorted(cases.RANGE_CASES))
def test_range_form_equals_index_form(smm, name, dtype):
    src, r0, r1, c0, c1 = cases.RANGE_CASES[name]
    csr, shape = source(src, dtype)
    A = make(smm, csr, shape)
    by_range = A.submatrix(slice(r0, r1), slice(c0, c1))
    by_index = A.submatrix(np.arange(r0, r1, dtype=np.int32), np.arange(c0, c1, dtype=np.int32))
    assert_same(arrays(by_range), arrays(by_index), name)
    assert_same(arrays(by_range), rs.submatrix(csr, shape, np.arange(r0, r1), np.arange(c0, c1))[0], "restatement")
    mixed = A.submatrix(slice(r0, r1), np.arange(c0, c1, dtype=np.int32))
    assert_same(arrays(mixed), arrays(by_index), "a slice beside a list")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_submatrix_dev_through_offset_views(smm, dtype):
    csr, shape = source("ragged", dtype)
    A = make(smm, csr, shape)
    _, rows, cols = cases.SUB_CASES["repeated_rows"]
    want = rs.submatrix(csr, shape, rows, cols)[0]
    for residue in (0, 1, 3):
        d_rows = dv.carve_like(rows, residue, fill=0, device=DEV)
        d_cols = dv.carve_like(cols, (residue + 1) % 4, fill=0, device=DEV)
        held = dv.snapshot(d_rows), dv.snapshot(d_cols)
        torch.cuda.synchronize()
        S = A.submatrix_dev(dv.address(d_rows), len(rows), dv.address(d_cols), len(cols))
        assert_same(arrays(S), want, f"residue {residue}")
        dv.assert_unchanged(d_rows, held[0], "rows")
        dv.assert_unchanged(d_cols, held[1], "cols")
        dv.assert_guards_intact(d_rows, "rows")
        dv.assert_guards_intact(d_cols, "cols")
    S = A.submatrix_dev(None, 0, dv.address(d_cols), len(cols))  # NULL rows: all of them
    assert_same(arrays(S), rs.submatrix(csr, shape, None, cols)[0], "all rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_submatrix_refresh_equals_a_fresh_create(smm, dtype):
    for name in ("repeated_rows", "long_rows_some"):
        src, rows, cols = cases.SUB_CASES[name]
        csr, shape = source(src, dtype)
        A = make(smm, csr, shape)
        S = A.submatrix(rows, cols)
        A.scale(-0.5)
        S.submatrix_refresh(A)
        assert_same(arrays(S), arrays(A.submatrix(rows, cols)), f"{name} after scale")
        r = np.repeat(np.arange(shape[0]), np.diff(csr[0]))[::3].astype(np.int32)
        assert A.update_entries(r, csr[1][::3], np.arange(len(r)).astype(dtype)).all()
        S.submatrix_refresh(A)
        assert_same(arrays(S), arrays(A.submatrix(rows, cols)), f"{name} after update_entries")
        edited = (csr[0], csr[1], (dtype(-0.5) * csr[2]).astype(dtype))
        edited[2][::3] = np.arange(len(r)).astype(dtype)
        assert_same(arrays(S), rs.submatrix(edited, shape, rows, cols)[0], f"{name} restatement")
    other = make(smm, *source("wide", dtype))
    before = arrays(S)
    for bad_self, bad_src in ((S, other), (other, A)):  # another shape; a handle submatrix did not make
        with pytest.raises(smm.SmmHipError) as e:
            bad_self.submatrix_refresh(bad_src)
        assert e.value.code == INVALID
    assert_same(arrays(S), before, "after the refusals")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_submatrix_errors_name_the_first_position(smm, dtype):
    csr, shape = source("ragged", dtype)
    A = make(smm, csr, shape)
    lib = _lib.load()
    for rows, cols, text in (([0, 5, 131, -1], None, "rows_idx[2]"), (None, [0, 5, 9, 9, 4], "cols_idx[3]"), (None, [0, 97], "cols_idx[1]"), ([3, -7], [1, 2], "rows_idx[1]")):
        with pytest.raises(rs.Invalid):
            rs.submatrix(csr, shape, rows, cols)
        with pytest.raises(smm.SmmHipError) as e:
            A.submatrix(rows, cols)
        assert e.value.code == INVALID and text in str(e.value), str(e.value)
        out = ctypes.c_void_p(0xDEAD)
        r = None if rows is None else np.asarray(rows, dtype=np.int32)
        c = None if cols is None else np.asarray(cols, dtype=np.int32)
        st = lib.smm_hip_csr_submatrix_create(A._h, None if r is None else r.ctypes.data_as(ctypes.c_void_p), 0 if r is None else r.size,
                                              None if c is None else c.ctypes.data_as(ctypes.c_void_p), 0 if c is None else c.size, None, ctypes.byref(out))
        assert st == INVALID and out.value == 0xDEAD and text in lib.smm_hip_last_error().decode()
    out = ctypes.c_void_p(0xDEAD)
    for r0, r1, c0, c1 in ((0, 132, 0, 97), (5, 4, 0, 97), (0, 131, -1, 97), (0, 131, 0, 98)):
        assert lib.smm_hip_csr_submatrix_range_create(A._h, r0, r1, c0, c1, None, ctypes.byref(out)) == INVALID and out.value == 0xDEAD
    with pytest.raises(ValueError):
        A.submatrix(slice(0, 10, 2), None)


# ---- diagonal and scaling ----
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["laplacian", "ragged", "wide", "long_rows", "even_columns"])
def test_diagonal(smm, name, dtype):
    """square, tall (131 x 97), wide (97 x 131) matrices; ragged / wide / even_columns lack diagonal entries: the count and the zeros"""
    csr, shape = source(name, dtype)
    A = make(smm, csr, shape)
    want, missing = rs.diagonal(csr, shape)
    got, count = A.diagonal(return_missing=True)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert count == missing and len(got) == min(shape)
    np.testing.assert_array_equal(bits(A.diagonal()), bits(want))
    n = min(shape)
    for residue in dv.residues(dtype):
        d_out = dv.carve(n, dtype, residue, device=DEV)
        d_missing = dv.carve(1, np.int32, (residue + 1) % 4, fill=-7, device=DEV)
        torch.cuda.synchronize()
        A.diagonal_dev(dv.address(d_out), dv.address(d_missing))
        smm.synchronize()
        np.testing.assert_array_equal(bits(d_out.cpu().numpy()), bits(want))
        assert int(d_missing.cpu()[0]) == missing
        dv.assert_guards_intact(d_out, "out")
        dv.assert_guards_intact(d_missing, "missing")
    A.diagonal_dev(dv.address(d_out), None)  # the count is optional
    smm.synchronize()
    np.testing.assert_array_equal(bits(d_out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", ["ragged", "wide", "long_rows"])
def test_scale_rows_cols(smm, name, dtype):
    csr, shape = source(name, dtype)
    r, c = cases.vectors(shape, dtype)
    for rr, cc in ((r, c), (r, None), (None, c), (None, None)):
        A = make(smm, csr, shape)
        A.scale_rows_cols(rr, cc)
        assert_same(arrays(A), (csr[0], csr[1], rs.scale_rows_cols(csr, rr, cc)), f"{name} r={rr is not None} c={cc is not None}")
    for residue in dv.residues(dtype):
        A = make(smm, csr, shape)
        d_r, d_c = dv.carve_like(r, residue, device=DEV), dv.carve_like(c, (residue + 1) % len(dv.residues(dtype)), device=DEV)
        held = dv.snapshot(d_r), dv.snapshot(d_c)
        torch.cuda.synchronize()
        A.scale_rows_cols_dev(dv.address(d_r), dv.address(d_c))
        assert_same(arrays(A), (csr[0], csr[1], rs.scale_rows_cols(csr, r, c)), f"dev residue {residue}")
        dv.assert_unchanged(d_r, held[0], "r")
        dv.assert_unchanged(d_c, held[1], "c")
        dv.assert_guards_intact(d_r, "r")
        dv.assert_guards_intact(d_c, "c")
        A.scale_rows_cols_dev(None, None)
        assert_same(arrays(A), (csr[0], csr[1], rs.scale_rows_cols(csr, r, c)), "neither: bit-unchanged")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_scaling_a_constant_diagonal_matrix_reverifies_the_encoding(smm, oracle, dtype):
    from sparse_matrix_math_amd import generators as gen

    csr = gen.poisson2d(150, 130, dtype=dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr, (n, n))
    A.set_kernel(PATTERN, 1)
    assert A.pattern_info()[0] == CONST
    x = np.random.default_rng(11).uniform(-1, 1, n).astype(dtype)
    y = np.zeros(n, dtype=dtype)
    A.rMult(x, y)
    A.scale_rows_cols(None, None)
    assert A.pattern_info()[0] == CONST  # nothing was touched
    r, c = cases.vectors((n, n), dtype, seed=12)
    A.scale_rows_cols(r, c)
    values = rs.scale_rows_cols(csr, r, c)
    np.testing.assert_array_equal(bits(A.get_values()), bits(values))
    assert A.pattern_info()[0] == MASKS  # the diagonals are no longer constant: the encoding was re-verified, not kept stale
    A.set_kernel(0, 1)  # AUTO, one lane per row
    A.rMult(x, y)
    np.testing.assert_array_equal(bits(y), bits(oracle.spmv((csr[0], csr[1], values), 0, None, x)))


def test_kkt_end_to_end(smm):
    """K = [[H, Bt], [B, 0]] built on the device and solved by MINRES; S = B diag(H)^-1 Bt formed from diagonal, scale_rows_cols, multiply"""
    dtype = np.float64
    Hc, Bc = cases.e2e_blocks()
    H, B = make(smm, Hc, (144, 144)), make(smm, Bc, (20, 144))
    Bt = B.transpose()
    K = smm.bmat([[H, Bt], [B, None]])
    Hd, Bd = rs.dense(Hc, (144, 144)), rs.dense(Bc, (20, 144))
    Kd = np.block([[Hd, Bd.T], [Bd, np.zeros((20, 20))]])
    np.testing.assert_array_equal(rs.dense(arrays(K), (164, 164)), Kd)
    rhs = np.random.default_rng(7).uniform(-1, 1, 164)
    z = np.zeros(164)
    info = {}
    st = smm.MINRES(K, rhs.copy(), z, 2000, 1e-10, info=info)
    assert st == smm.SolverStatus.SUCCESS, (st, info)
    exact = np.linalg.solve(Kd, rhs)
    assert np.max(np.abs(z - exact)) <= 1e-6 * np.max(np.abs(exact)), (np.max(np.abs(z - exact)), info)
    d = H.diagonal()
    np.testing.assert_array_equal(d, np.diag(Hd))
    Bt_scaled = B.transpose()
    Bt_scaled.scale_rows_cols(1.0 / d, None)
    S = B.multiply(Bt_scaled)
    got = arrays(S)
    terms = Bd[:, None, :] * ((1.0 / d)[None, None, :] * Bd[None, :, :])  # [i, j, k] = b_ik * (b_jk / h_kk), each once rounded
    structural = (Bd[:, None, :] != 0) & (Bd[None, :, :] != 0)
    assert not np.any((Bd == 0) & rs.stored(Bc, (20, 144)))  # no stored zeros: structure is where the values are
    np.testing.assert_array_equal(rs.stored(got, (20, 20)), structural.any(axis=2))
    L = structural.sum(axis=2)
    bound = (L + 2) * np.finfo(dtype).eps * np.abs(terms).sum(axis=2)
    assert np.all(np.abs(rs.dense(got, (20, 20)) - terms.sum(axis=2)) <= bound)
