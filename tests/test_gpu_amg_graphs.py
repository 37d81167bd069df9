"""The multigrid set-up on the GPU (csrc/smm_precond_amg.hip) on the matrices of tests/amg_cases.py, against its CPU restatement: graphs
with a one-way strength relation, rows without a strong neighbour, singleton aggregates beside large ones, row lengths from 1 to 513 on
one level, a stall on level 0 and on deeper levels, a refusal.  tests/test_amg_cases_cpu.py shows that the restatement reaches those paths
on these matrices.  The checks are those of tests/test_gpu_amg.py, whose functions run here on the new names (its reference() serves
them): the structure exactly, the values and the one-lane-per-row cycle bit for bit, one fixed-step solve per family."""
import numpy as np
import pytest
import test_gpu_amg as base
from amg_cases import NAMES, REFUSED, case
from amg_restatement import dense_apply, dense_of, products
from chebyshev_restatement import diagonal, gershgorin
from test_gpu_amg import assert_same_csr, bits, code_of, make, one_lane_per_row, reference, triple

pytestmark = pytest.mark.gpu
DTYPES = base.DTYPES
ids = base.ids
BUILT = tuple(n for n in NAMES if n not in REFUSED)
VALUES = ("graph_directed_1500", "ragged_rows_1200", "chain_1200_c64")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", BUILT)
def test_structure_is_exact(smm, name, dtype):
    """levels, rows, nnz, operator complexity, the aggregates and the patterns of A_l, P_l and R_l; a level that stalled has none"""
    base.test_structure_is_exact(smm, name, dtype)
    csr, kw, ref, _, _ = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    last = len(ref) - 1
    assert M.amg_level(last)[1:] == (None, None)
    assert code_of(lambda: M.amg_aggregates(last)) == base.INVALID


def same_bits(got, want):
    return all(a.shape == b.shape for a, b in zip(got, want)) and all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and np.array_equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", VALUES)
def test_values_are_bit_for_bit(smm, name, dtype):
    """P_l, R_l and A_{l+1} against the restatement on every level: outright while the library's A_l is the restatement's bit for bit
    (level 0 is the caller's matrix), and with the restatement fed the library's own A_l otherwise, as tests/test_gpu_amg.py does"""
    csr, kw, ref, _, _ = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    assert M.amg_info()["levels"] == len(ref)
    for l, lv in enumerate(ref[:-1]):
        Al, Pl, Rl = M.amg_level(l)
        a = triple(Al)
        if l == 0:
            assert_same_csr(a, csr, "A_0")
        if same_bits(a, lv["A"]):
            P, R, A_next = lv["P"], lv["R"], ref[l + 1]["A"]
        else:
            fed = {"diag": diagonal(a), "lam": gershgorin(a), "agg": lv["agg"], "n_c": lv["n_c"]}
            P, R, _, A_next = products(a, fed)
        assert_same_csr(triple(Pl), P, f"P_{l}")
        assert_same_csr(triple(Rl), R, f"R_{l}")
        assert_same_csr(triple(M.amg_level(l + 1)[0]), A_next, f"A_{l + 1}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", VALUES)
def test_apply_bit_for_bit_at_one_lane_per_row(smm, oracle, name, dtype):
    """the seeded uniform right-hand side (the existing test's) and the row sums"""
    base.test_apply_bit_for_bit_at_one_lane_per_row(smm, oracle, name, dtype)
    csr, kw, _, b, _ = reference(name, dtype)
    M = make(smm, csr).getPreconditioner("AMG", **kw)
    one_lane_per_row(smm, M)
    fn = base.make_apply(oracle, base.library_levels(M), M.amg_coarse_inverse())
    z = np.full(len(b), np.nan, dtype=dtype)
    M.apply(b, z)
    np.testing.assert_array_equal(bits(z), bits(fn(b)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_stall_on_level_0_leaves_the_dense_solve(smm, dtype):
    """hubs_900: one level, no P and no R; the inverse within the bound of tests/test_gpu_amg.py::test_coarse_inverse (8 x the same figure
    of np.linalg.inv in double rounded to T), and the apply is that inverse times the vector bit for bit (the restated dense kernel)"""
    csr, kw, ref, b, r = reference("hubs_900", dtype)
    assert len(ref) == 1
    A = make(smm, csr)
    M = A.getPreconditioner("AMG", **kw)
    info = M.amg_info()
    assert info["levels"] == 1 and info["rows"] == [900] and info["nnz"] == [len(csr[1])] and info["operator_complexity"] == 1.0
    A0, P0, R0 = M.amg_level(0)
    assert P0 is None and R0 is None
    assert_same_csr(triple(A0), csr, "A_0")
    dense = dense_of(csr)
    n = len(dense)
    inv = M.amg_coarse_inverse()
    assert inv.shape == (n, n) and inv.dtype == np.dtype(dtype)
    exact = np.linalg.inv(dense)
    rounding = float(np.max(np.abs(exact.astype(dtype).astype(np.float64) @ dense - np.eye(n))))
    got = float(np.max(np.abs(inv.astype(np.float64) @ dense - np.eye(n))))
    print("hubs_900", np.dtype(dtype).name, "cond", float(np.linalg.cond(dense)), "|Inv A - I|", got, "reference rounded to T", rounding)
    assert got <= 8 * rounding
    for rhs in (b, r):
        z = np.full(n, np.nan, dtype=dtype)
        M.apply(rhs, z)
        np.testing.assert_array_equal(bits(z), bits(dense_apply(inv, rhs)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusal_leaves_the_matrix_usable(smm, oracle, dtype):
    """hubs_1500: no entry is strong, the level cannot shrink and has more than 1024 rows: SMM_HIP_ERR_PRECOND naming the size; the
    matrix handle then still serves a JACOBI preconditioner and an SpMV"""
    csr, kw = case("hubs_1500", dtype)
    A = make(smm, csr)
    with pytest.raises(base._lib.SmmHipError) as e:
        A.getPreconditioner("AMG", **kw)
    assert e.value.code == base.PRECOND and "1500" in str(e.value)
    J = A.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    np.testing.assert_array_equal(bits(J.values()), bits(diagonal(csr)))
    v = np.random.default_rng(5).uniform(-1, 1, 1500).astype(dtype)
    A.set_kernel(smm.SPMV_STREAM, 1)
    y = np.full(1500, np.nan, dtype=dtype)
    A.rMult(v, y)
    np.testing.assert_array_equal(bits(y), bits(oracle.spmv(csr, 0, None, v)))
    assert code_of(lambda: A.getPreconditioner("AMG", **kw)) == base.PRECOND  # and is refused again, the same way


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name", [("cg", "graph_sym_1500"), ("bicgstab", "graph_directed_1500")])
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, name, dtype):
    """the step count and the allowance of tests/test_gpu_amg.py; nothing is claimed about how fast either loop converges"""
    base.test_fixed_steps_match_the_restated_loops(smm, oracle, solver, name, dtype)

