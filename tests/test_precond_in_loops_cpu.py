"""The plumbing of tests/test_gpu_precond_in_loops.py without a GPU: the case tables cover exactly the pairs the kinds table marks as taken,
the omissions stay within their cap, and the helper that picks a restated loop per device loop really runs the preconditioner it is
given -- with a NumPy Jacobi as the black box, the restated loop differs from the one without by the margin the GPU test demands."""
import numpy as np
import pytest
from chebyshev_restatement import diagonal
from precond_loops_cases import (COLUMNS, DTYPES, LOOPS, LOWERED, OMITTED, REFINE, cases, check_reference, matrix, passes_of, reference, refine_cases, residual,
                                 restated, rhs, taken)
from test_gpu_precond_kinds import KINDS, TAKES, listed_clauses, listed_kinds


def test_the_kinds_table_is_written_out_in_full():
    assert len(KINDS) == len(set(KINDS)) == 17
    for solver, (prefix, takes) in TAKES.items():
        assert takes <= set(KINDS), solver
        assert prefix in ("cg", "bicgstab", "gmres", "idrs", "bicgstab_batch", "dist_bicgstab")
    # a Cholesky-type factor never reaches a loop for general matrices; ConjugateGradient takes no handle of kind NONE
    for solver in ("bicgstab", "gmres", "idrs", "bicgstab_batch", "dist_bicgstab", "refine_bicgstab", "refine_gmres"):
        assert not TAKES[solver][1] & {"IC0", "MULTICOLOR_IC0", "JSWEEP_IC0"}, solver
    assert "NONE" not in TAKES["cg"][1] and TAKES["refine_cg"][1] == TAKES["cg"][1]


def test_the_case_tables_cover_exactly_the_pairs_taken():
    listed = cases()
    assert len(listed) == len(set(listed))
    assert not set(listed) & set(OMITTED)
    everything = set(listed) | set(OMITTED)
    assert everything == {(loop, kind, dt) for loop, (key, _, _, _) in LOOPS.items() for kind in TAKES[key][1] for dt in DTYPES}
    # every solver of the kinds table has a loop here (BiCGStab two: host-driven and single-launch), the refinement driver its own test
    assert {key for key, _, _, _ in LOOPS.values()} | {key for _, key, _ in REFINE} == set(TAKES)
    assert set(refine_cases()) == {(inner, kind) for inner, key, _ in REFINE for kind in TAKES[key][1]}
    # the cap on omissions: at most one case in ten, never both dtypes of a pair
    assert 10 * len(OMITTED) <= len(everything)
    for loop, kind, _ in OMITTED:
        assert sum((loop, kind, dt) in OMITTED for dt in DTYPES) < len(DTYPES), (loop, kind)
    # a lowered count belongs to a listed case and is lower
    for key, passes in LOWERED.items():
        assert key in listed and 1 <= passes < LOOPS[key[0]][3], key
        assert passes_of(*key) == passes
    for loop in LOOPS:
        assert set(taken(loop)) == TAKES[LOOPS[loop][0]][1]


def test_the_clauses_of_a_refusal_are_read_apart():
    """the parser of tests/test_gpu_precond_kinds.py on the shapes a message takes (the texts written out)"""
    cg = ("cg: preconditioner must be IC0 / CHEBYSHEV / AMG / MULTICOLOR_SGS / MULTICOLOR_IC0, or FSAI of any power, or JSWEEP_SGS / JSWEEP_IC0 "
          "with equal step counts, created for this matrix")
    assert listed_clauses(cg) == (["IC0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_IC0"], ["FSAI"], ["JSWEEP_SGS", "JSWEEP_IC0"], "equal")
    batch = "bicgstab_batch: preconditioner must be JACOBI, or JSWEEP_SGS / JSWEEP_ILU0 with any step counts, created for this matrix"
    assert listed_clauses(batch) == (["JACOBI"], [], ["JSWEEP_SGS", "JSWEEP_ILU0"], "any")
    local = "dist_bicgstab: preconditioner must be JACOBI / ILU0 of the local diagonal block (smm_hip_dist_csr_local_block)"
    assert listed_clauses(local) == (["JACOBI", "ILU0"], [], [], None) and listed_kinds(local) == ["JACOBI", "ILU0"]
    assert listed_clauses("cg: a JSWEEP_SGS preconditioner is symmetric only with as many lower steps as upper ones") == ([], [], [], None)


def test_the_matrices_are_what_the_cases_need():
    for which, rows in (("spd", 144), ("general", 216)):
        for dt in DTYPES:
            start, pos, val = matrix(which, np.dtype(dt).type)
            n = len(start) - 1
            assert n == rows and val.dtype == np.dtype(dt)
            diag = diagonal((start, pos, val))
            assert len(np.unique(diag)) == 5  # a diagonal that is not constant: JACOBI can be told from no preconditioner
            dense = np.zeros((n, n))
            dense[np.repeat(np.arange(n), np.diff(start)), pos] = val
            assert np.array_equal(dense, dense.T) == (which == "spd")  # (symmetric bit for bit: one rounding of a_ij (d_i d_j))
            if which == "spd":
                assert np.linalg.eigvalsh(dense).min() > 0
    assert len({tuple(rhs(216, np.float64, j)) for j in range(COLUMNS)}) == COLUMNS


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("loop", list(LOOPS))
def test_the_restated_loop_runs_the_black_box_it_is_given(oracle, loop, dt):
    """a NumPy Jacobi as `apply`: the figures and the conditions of the GPU test, on the restatement alone"""
    dtype = np.dtype(dt).type
    csr = matrix(LOOPS[loop][1], dtype)
    b = rhs(len(csr[0]) - 1, dtype)
    diag = diagonal(csr)
    calls = []

    def jacobi(r):
        calls.append(1)
        return (np.ascontiguousarray(r, dtype=dtype) / diag).astype(dtype)

    passes = passes_of(loop, "JACOBI", dt)
    ref = reference(oracle, loop, "JACOBI", csr, b, passes, jacobi)
    tol = check_reference(ref, dtype, "JACOBI")
    print(loop, dt, "passes", passes, "sensitivity", ref["sensitivity"], "allowed", tol, "discrimination", ref["apart"], "residual before the last pass",
          ref["residual_before_last"], "threshold", ref["threshold"], "applies", len(calls))
    assert ref["iterations"] == passes and len(calls) >= passes
    assert ref["apart"] >= 100 * tol
    # the run without a preconditioner is the run with the identity: NONE compares against it
    plain = restated(oracle, loop, csr, b, passes)[1]
    same = restated(oracle, loop, csr, b, passes, lambda r: np.array(r, copy=True))[1]
    np.testing.assert_array_equal(plain, same)
    assert residual(csr, plain, b) < residual(csr, np.zeros_like(plain), b)
