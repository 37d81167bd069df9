"""Which solver takes which preconditioner kind: every SMM_PRECOND_* kind, and a JACOBI handle made for another matrix, offered to
ConjugateGradient, BiCGStab, GMRES, IDR(s), the batched BiCGStab, the row-partitioned BiCGStab and IterativeRefinement (once per inner
solver, the handle made on the fp32 copy).  TAKES below is written out by hand from the contract in include/smm_hip.h and is a record of
what the library answers, oddities included.  Where the header's words and the library differ, the library's answer stands here:
  - ConjugateGradient refuses a handle of kind NONE that every other loop treats as "no preconditioner" (so does IterativeRefinement with
    the inner CG, which hands the handle on);
  - the sentence at smm_hip_cg_* still says "every other kind: SMM_HIP_ERR_INVALID" after IC0 / CHEBYSHEV / AMG; the paragraphs of the
    later kinds add MULTICOLOR_SGS / MULTICOLOR_IC0, FSAI, and JSWEEP_SGS / JSWEEP_IC0 with equal step counts, and the library takes them;
  - the list at smm_hip_gmres_* ends with MULTICOLOR_ILU0; FSAI, SPAI, JSWEEP_SGS and JSWEEP_ILU0 are granted by their own paragraphs, and
    the library takes them (IDR(s) takes what GMRES takes);
  - smm_hip_dist_bicgstab_* names JACOBI / ILU0 / SGS of the local block; the library also takes BLOCK_ILU0 / BLOCK_SGS and a NONE handle;
  - the JSWEEP paragraph lists smm_hip_cgs_* and smm_hip_bicg_* among the takers: neither has a preconditioner argument."""
import re

import numpy as np
import pytest

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu

INVALID = -1  # SMM_HIP_ERR_INVALID
KINDS = ("NONE", "JACOBI", "ILU0", "SGS", "IC0", "BLOCK_ILU0", "BLOCK_SGS", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "MULTICOLOR_IC0",
         "FSAI", "SPAI", "JSWEEP_SGS", "JSWEEP_ILU0", "JSWEEP_IC0")
FOREIGN = "JACOBI of another matrix"
AINV = {"FSAI", "SPAI"}  # the kinds a refusal lists in the clause "... of any power"
JSWEEP = {"JSWEEP_SGS", "JSWEEP_ILU0", "JSWEEP_IC0"}  # ... and in the clause "... with equal / any step counts"
CG_TAKES = {"IC0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_IC0", "FSAI", "JSWEEP_SGS", "JSWEEP_IC0"}
GENERAL_TAKES = {"NONE", "JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "FSAI", "SPAI",
                 "JSWEEP_SGS", "JSWEEP_ILU0"}
# solver -> (the name its messages start with, the kinds it takes); the refinement driver answers with its inner solver's message
TAKES = {
    "cg": ("cg", CG_TAKES),
    "bicgstab": ("bicgstab", GENERAL_TAKES),
    "gmres": ("gmres", GENERAL_TAKES),
    "idrs": ("idrs", GENERAL_TAKES),
    "bicgstab_batch": ("bicgstab_batch", {"NONE", "JACOBI", "JSWEEP_SGS", "JSWEEP_ILU0"}),
    "dist_bicgstab": ("dist_bicgstab", {"NONE", "JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS"}),
    "refine_cg": ("cg", CG_TAKES),
    "refine_bicgstab": ("bicgstab", GENERAL_TAKES),
    "refine_gmres": ("gmres", GENERAL_TAKES),
}
STEP_COUNTS = {solver: "equal" if prefix == "cg" else "any" for solver, (prefix, _) in TAKES.items()}  # the word of the step-count clause
REFINE_INNER = {"refine_cg": "CG", "refine_bicgstab": "BICGSTAB", "refine_gmres": "GMRES"}


def enum_of(smm, kind):
    P = smm.SolverPreconditioner
    return P.SYMMETRIC_GAUS_SEIDEL if kind == "SGS" else P[kind]


_NAMES = r"((?:[A-Z][A-Z0-9_]*)(?: / [A-Z][A-Z0-9_]*)*)"


def listed_kinds(message):
    """the kinds a refusal offers instead: the names of the `A / B / C` list that follows "must be" """
    m = re.search(r"must be " + _NAMES, message)
    return m.group(1).split(" / ") if m else []


def listed_clauses(message):
    """(the plain list, the list "of any power", the list with step counts, "equal" or "any" or None) of a refusal.  The plain list is
    empty when the message starts its offer with one of the two clauses."""
    power = re.search(r"or " + _NAMES + r" of any power,", message)
    steps = re.search(r"or " + _NAMES + r" with (equal|any) step counts,", message)
    return (listed_kinds(message), power.group(1).split(" / ") if power else [], steps.group(1).split(" / ") if steps else [],
            steps.group(2) if steps else None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
def test_which_solver_takes_which_kind(smm, dtype):
    import torch

    from sparse_matrix_math_amd import distributed as dist

    lib = _lib.load()
    csr = gen.poisson2d(8, 8, dtype=dtype)  # 64 rows, symmetric positive definite: every kind can be created
    n = len(csr[0]) - 1
    assert n == 64 and len(KINDS) == len(smm.SolverPreconditioner) == 17
    A = smm.CSRMatrix(n, n, *csr)
    other = smm.CSRMatrix(n, n, csr[0], csr[1], (csr[2] * dtype(2)).astype(dtype))
    b = gen.row_sums(csr[0], csr[2])
    comm = dist.NativeComm.single()
    tens = [torch.tensor(a, device="cuda:0") for a in csr]
    D = dist.NativeDistMatrix(comm, n, [0, n], tens[0], tens[1], tens[2], dtype)
    local = D.local_blocks()[0]
    d_b = torch.tensor(b, device="cuda:0")
    handles = {k: (A.getPreconditioner(enum_of(smm, k)), smm.Preconditioner(local, enum_of(smm, k))) for k in KINDS}
    foreign = other.getPreconditioner(smm.SolverPreconditioner.JACOBI)
    handles[FOREIGN] = (foreign, foreign)
    # IterativeRefinement: an fp64 matrix, the handles on its fp32 copy -- made once, for the fp64 run of this test
    refine = dtype == np.float64
    if refine:
        A32 = A.astype(np.float32)
        other32 = other.astype(np.float32)
        handles32 = {k: A32.getPreconditioner(enum_of(smm, k)) for k in KINDS}
        handles32[FOREIGN] = other32.getPreconditioner(smm.SolverPreconditioner.JACOBI)

    def offer(solver, M, Mloc):
        """(x before, x after) of one solve of one iteration from x = 0.25"""
        if solver == "dist_bicgstab":
            d_x = torch.full((n,), 0.25, dtype=d_b.dtype, device="cuda:0")
            D._M = Mloc
            try:
                D.bicgstab(d_b, d_x, 1, 1e-30)
            finally:
                D._M = None
                torch.cuda.synchronize()
                offer.x = d_x.cpu().numpy()
            return
        if solver == "bicgstab_batch":
            offer.x = np.full((n, 2), 0.25, dtype=dtype)
            smm.BiCGStabBatch(A, np.stack([b, b], axis=1).copy(), offer.x, 1, 1e-30, M)
            return
        offer.x = np.full(n, 0.25, dtype=dtype)
        if solver in REFINE_INNER:
            smm.IterativeRefinement(A, b, offer.x, 1e-30, inner=REFINE_INNER[solver], a32=A32, M=M, maxOuter=1, maxInner=1)
        elif solver == "cg":
            smm.ConjugateGradient(A, b, offer.x.copy(), offer.x, 1, 1e-30, M)
        elif solver == "bicgstab":
            smm.BiCGStab(A, b, offer.x, 1, 1e-30, M)
        elif solver == "idrs":
            smm.IDRs(A, b, offer.x, 1, 1e-30, 2, M)
        else:
            smm.GMRES(A, b, offer.x, 1, 1e-30, 30, M)

    def attempt(solver, M, Mloc):
        try:
            offer(solver, M, Mloc)
            return 0, ""
        except _lib.SmmHipError as e:
            return e.code, lib.smm_hip_last_error().decode()

    wrong = []
    for solver, (prefix, takes) in TAKES.items():
        if solver in REFINE_INNER and not refine:
            continue
        for kind in handles:
            M, Mloc = (handles32[kind], None) if solver in REFINE_INNER else handles[kind]
            code, message = attempt(solver, M, Mloc)
            print(np.dtype(dtype).name, solver, kind, "->", code, message)
            want = 0 if kind in takes else INVALID
            if code != want:
                wrong.append((solver, kind, code, message))
                continue
            if code == INVALID:
                assert bool((offer.x == dtype(0.25)).all()), (solver, kind, "x was written")
                assert message.startswith(prefix + ": "), (solver, kind, message)
                assert set(listed_kinds(message)) <= takes, (solver, kind, message)
                # the three clauses together name every kind the solver takes (NONE stands for "no preconditioner": never offered), the
                # approximate inverses and the iterated sweeps each in the clause that names their parameter
                plain, power, steps, word = listed_clauses(message)
                assert set(plain) == takes - {"NONE"} - AINV - JSWEEP, (solver, kind, message)
                assert set(power) == takes & AINV and (" of any power," in message) == bool(takes & AINV), (solver, kind, message)
                assert set(steps) == takes & JSWEEP and word == (STEP_COUNTS[solver] if takes & JSWEEP else None), (solver, kind, message)
    assert not wrong, wrong

    # ConjugateGradient takes an iterated sweep only as a symmetric operator: 2 / 3 steps refused (x untouched, a message of its own that
    # names the kind and the call that changes the counts), 3 / 3 taken again; the loops for general matrices take any counts
    for kind in ("JSWEEP_SGS", "JSWEEP_IC0"):
        for solver, (M, Mloc) in [("cg", handles[kind])] + ([("refine_cg", (handles32[kind], None))] if refine else []):
            M.jsweep_set_sweeps(2, 3)
            code, message = attempt(solver, M, Mloc)
            print(np.dtype(dtype).name, solver, kind, "2 / 3 steps ->", code, message)
            assert code == INVALID and bool((offer.x == dtype(0.25)).all()), (solver, kind, code)
            assert message.startswith("cg: a " + kind + " preconditioner is symmetric only with as many lower steps as upper ones"), message
            assert "smm_hip_precond_jsweep_set_sweeps" in message
            M.jsweep_set_sweeps(3, 3)
            code, message = attempt(solver, M, Mloc)
            print(np.dtype(dtype).name, solver, kind, "3 / 3 steps ->", code, message)
            assert code == 0, (solver, kind, message)
    for kind in ("JSWEEP_SGS", "JSWEEP_ILU0"):
        M, Mloc = handles[kind]
        M.jsweep_set_sweeps(2, 3)
        for solver in ("bicgstab", "gmres", "idrs", "bicgstab_batch"):
            code, message = attempt(solver, M, Mloc)
            print(np.dtype(dtype).name, solver, kind, "2 / 3 steps ->", code, message)
            assert code == 0, (solver, kind, message)
        M.jsweep_set_sweeps(3, 3)

    for M, Mloc in handles.values():
        M.close()
        if Mloc is not M:
            Mloc.close()
    if refine:
        for M in handles32.values():
            M.close()
    D.close()
    comm.close()
