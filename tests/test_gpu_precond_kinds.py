"""Which solver takes which preconditioner kind: every SMM_PRECOND_* kind, and a JACOBI handle made for another matrix, offered to
ConjugateGradient, BiCGStab, GMRES, the batched BiCGStab and the row-partitioned BiCGStab.  TAKES below is a record of what the library
answers, oddities included (ConjugateGradient refuses a handle of kind NONE that the other loops treat as "no preconditioner")."""
import re

import numpy as np
import pytest
import torch

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu

INVALID = -1  # SMM_HIP_ERR_INVALID
KINDS = ("NONE", "JACOBI", "ILU0", "SGS", "IC0", "BLOCK_ILU0", "BLOCK_SGS", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_ILU0", "MULTICOLOR_IC0")
FOREIGN = "JACOBI of another matrix"
# solver -> (the name its messages start with, the kinds it takes)
TAKES = {
    "cg": ("cg", {"IC0", "CHEBYSHEV", "AMG", "MULTICOLOR_SGS", "MULTICOLOR_IC0"}),
    "bicgstab": ("bicgstab", set(KINDS) - {"IC0", "MULTICOLOR_IC0"}),
    "gmres": ("gmres", set(KINDS) - {"IC0", "MULTICOLOR_IC0"}),
    "bicgstab_batch": ("bicgstab_batch", {"NONE", "JACOBI"}),
    "dist_bicgstab": ("dist_bicgstab", {"NONE", "JACOBI", "ILU0", "SGS", "BLOCK_ILU0", "BLOCK_SGS"}),
}


def enum_of(smm, kind):
    P = smm.SolverPreconditioner
    return P.SYMMETRIC_GAUS_SEIDEL if kind == "SGS" else P[kind]


def listed_kinds(message):
    """the kinds a refusal offers instead: the names of the `A / B / C` list that follows "must be" """
    m = re.search(r"must be ((?:[A-Z][A-Z0-9_]*)(?: / [A-Z][A-Z0-9_]*)*)", message)
    return m.group(1).split(" / ") if m else []


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
def test_which_solver_takes_which_kind(smm, dtype):
    from sparse_matrix_math_amd import distributed as dist

    lib = _lib.load()
    csr = gen.poisson2d(8, 8, dtype=dtype)  # 64 rows, symmetric positive definite: every kind can be created
    n = len(csr[0]) - 1
    assert n == 64
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
        if solver == "cg":
            smm.ConjugateGradient(A, b, offer.x.copy(), offer.x, 1, 1e-30, M)
        elif solver == "bicgstab":
            smm.BiCGStab(A, b, offer.x, 1, 1e-30, M)
        else:
            smm.GMRES(A, b, offer.x, 1, 1e-30, 30, M)

    wrong = []
    for solver, (prefix, takes) in TAKES.items():
        for kind, (M, Mloc) in handles.items():
            try:
                offer(solver, M, Mloc)
                code, message = 0, ""
            except _lib.SmmHipError as e:
                code, message = e.code, lib.smm_hip_last_error().decode()
            print(np.dtype(dtype).name, solver, kind, "->", code, message)
            want = 0 if kind in takes else INVALID
            if code != want:
                wrong.append((solver, kind, code, message))
                continue
            if code == INVALID:
                assert bool((offer.x == dtype(0.25)).all()), (solver, kind, "x was written")
                assert message.startswith(prefix + ": "), (solver, kind, message)
                assert set(listed_kinds(message)) <= takes, (solver, kind, message)
    assert not wrong, wrong
    for M, Mloc in handles.values():
        M.close()
        if Mloc is not M:
            Mloc.close()
    D.close()
    comm.close()
