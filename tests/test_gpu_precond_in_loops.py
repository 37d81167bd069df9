"""An accepted preconditioner kind is applied, and applied right: every (loop, kind) pair that tests/test_gpu_precond_kinds.py records as
taken, in both dtypes, for a fixed number of passes with eps = 0 against the CPU restatement of that loop, in which the preconditioner
is a black box -- apply = M.apply on the same device handle.  Whether the apply itself is right is each kind's own test; what fails
here is a loop that ignores M, applies it on the wrong side or to a stale vector, or takes a fused path (the Jacobi division in the SpMV
epilogue, the SpMV inside a block apply, the single-launch BiCGStab, the batched loop's column-by-column sweeps) for a kind it was not
written for.  The cases, the matrices and the conditions on the restatement's side are tests/precond_loops_cases.py.

Tolerance: the fixed-pass rule of tests/test_gpu_cgs.py (`allowed` from the restated loop's own sensitivity).  Discrimination: for every
kind but NONE the restated run with `apply` and the one without differ by at least 100 x that tolerance, or the case proves nothing.

IterativeRefinement has no black-box restatement: for each inner solver and each kind it takes, SUCCESS and a true residual, in NumPy
fp64, within the eps asked for."""
import numpy as np
import pytest
from precond_loops_cases import COLUMNS, IDR_S, LOOPS, REFINE, RESTART, cases, check_reference, matrix, passes_of, reference, refine_cases, residual, rhs
from test_gpu_cgs import worst
from test_gpu_precond_kinds import enum_of

from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
PATTERN = 3  # SMM_SPMV_PATTERN
AMG_COARSE_ROWS = 16  # (the default, 256, would make the V-cycle of these matrices the dense solve alone)
REFINE_EPS = 1e-9


def make_precond(smm, A, kind):
    if kind == "AMG":
        return A.getPreconditioner(enum_of(smm, kind), coarse_rows=AMG_COARSE_ROWS)
    return A.getPreconditioner(enum_of(smm, kind))


def black_box(M, kind):
    """apply(r) -> M^-1 r through the handle; a handle of kind NONE means "no preconditioner" to the loops that take it"""
    if kind == "NONE":
        return None

    def apply(r):
        r = np.ascontiguousarray(r)
        z = np.empty_like(r)
        M.apply(r, z)
        return z

    return apply


class Device:
    """the matrix and the handle of one case, and its loop on the device: run(b, passes) -> [(variant, status, x, iterations)]"""

    def __init__(self, smm, loop, kind, csr):
        self.smm, self.loop = smm, loop
        self.n = len(csr[0]) - 1
        self.dtype = csr[2].dtype
        self.comm = self.D = None
        if loop == "dist_bicgstab":
            import torch

            from sparse_matrix_math_amd import distributed as dist

            self.comm = dist.NativeComm.single()
            tens = [torch.tensor(a, device="cuda:0") for a in csr]
            self.D = dist.NativeDistMatrix(self.comm, self.n, [0, self.n], tens[0], tens[1], tens[2], self.dtype.type)
            self.M = smm.Preconditioner(self.D.local_blocks()[0], enum_of(smm, kind))  # a local kind, on the local block's handle
            return
        self.A = smm.CSRMatrix(self.n, self.n, *csr)
        if loop == "bicgstab_resident":
            self.A.set_kernel(PATTERN, 1)  # (a matrix this small does not adopt the family by itself)
        self.M = make_precond(smm, self.A, kind)

    def run(self, b, passes):
        smm, n, dtype = self.smm, self.n, self.dtype
        info = {}
        if self.loop == "cg":
            out = []
            previous = host.cg_resident(-1)
            try:
                for mode in (host.CG_RESIDENT_OFF, host.CG_RESIDENT_REQUIRE):
                    host.cg_resident(mode)
                    x = np.zeros(n, dtype=dtype)
                    st = smm.ConjugateGradient(self.A, b, np.zeros(n, dtype=dtype), x, passes, 0.0, self.M, info=info)
                    out.append((f"cg_resident={mode}", int(st), x, info["iterations"]))
            finally:
                host.cg_resident(previous)
            return out
        if self.loop in ("bicgstab", "bicgstab_resident"):
            previous = host.bicgstab_resident(-1)
            try:
                host.bicgstab_resident(host.CG_RESIDENT_REQUIRE if self.loop == "bicgstab_resident" else host.CG_RESIDENT_OFF)
                x = np.zeros(n, dtype=dtype)
                st = smm.BiCGStab(self.A, b.copy(), x, passes, 0.0, self.M, info=info)
            finally:
                host.bicgstab_resident(previous)
            return [("", int(st), x, info["iterations"])]
        if self.loop == "gmres":
            x = np.zeros(n, dtype=dtype)
            st = smm.GMRES(self.A, b.copy(), x, passes, 0.0, RESTART, self.M, info=info)
            return [("", int(st), x, info["iterations"])]
        if self.loop == "idrs":
            x = np.zeros(n, dtype=dtype)
            st = smm.IDRs(self.A, b.copy(), x, passes, 0.0, IDR_S, self.M, info=info)
            return [("", int(st), x, info["iterations"])]
        if self.loop == "bicgstab_batch":  # b: (n, COLUMNS)
            X = np.zeros_like(b)
            sts = smm.BiCGStabBatch(self.A, b.copy(), X, passes, 0.0, self.M, info=info)
            return [(f"column {j}", int(sts[j]), np.ascontiguousarray(X[:, j]), int(info["iterations"][j])) for j in range(b.shape[1])]
        import torch

        d_b = torch.tensor(b, device="cuda:0")
        d_x = torch.zeros(n, dtype=d_b.dtype, device="cuda:0")
        self.D._M = self.M
        try:
            st, it, _ = self.D.bicgstab(d_b, d_x, passes, 0.0)
        finally:
            self.D._M = None
            torch.cuda.synchronize()
        return [("", int(st), d_x.cpu().numpy(), it)]

    def close(self):
        self.M.close()
        if self.D is not None:
            self.D.close()
            self.comm.close()


def measure(smm, oracle, loop, kind, dt, passes):
    """[(variant, reference figures, device status, device x, device iterations)] of one case: no assertion is made here"""
    dtype = np.dtype(dt).type
    csr = matrix(LOOPS[loop][1], dtype)
    n = len(csr[0]) - 1
    dev = Device(smm, loop, kind, csr)
    try:
        apply = black_box(dev.M, kind)
        if loop == "bicgstab_batch":
            B = np.stack([rhs(n, dtype, j) for j in range(COLUMNS)], axis=1).copy()
            refs = [reference(oracle, loop, kind, csr, np.ascontiguousarray(B[:, j]), passes, apply, j) for j in range(COLUMNS)]
            got = dev.run(B, passes)
        else:
            b = rhs(n, dtype)
            refs = [reference(oracle, loop, kind, csr, b, passes, apply)]
            got = dev.run(b, passes)
            refs = refs * len(got)
    finally:
        dev.close()
    return [(variant, ref, st, x, it) for ref, (variant, st, x, it) in zip(refs, got)]


@pytest.mark.parametrize("loop,kind,dt", cases(), ids=lambda v: str(v))
def test_the_loop_applies_the_kind_as_the_restated_loop_does(smm, oracle, loop, kind, dt):
    dtype = np.dtype(dt).type
    passes = passes_of(loop, kind, dt)
    failed = []
    for variant, ref, st, x, it in measure(smm, oracle, loop, kind, dt, passes):
        err = worst(x, ref["x"])
        print(loop, kind, dt, variant, "passes", passes, "max|x - ref|", err, "sensitivity", ref["sensitivity"], "max|x|", ref["scale"], "discrimination",
              ref["apart"], "residual before the last pass", ref["residual_before_last"], "threshold", ref["threshold"])
        tol = check_reference(ref, dtype, kind)
        print("   allowed", tol)
        assert st == ref["status"] and it == ref["iterations"], (variant, st, it, ref["status"], ref["iterations"])
        if not err <= tol:
            failed.append((variant, err, tol))
    assert not failed, failed


@pytest.mark.parametrize("inner,kind", refine_cases(), ids=lambda v: str(v))
def test_refinement_reaches_eps_with_every_kind_its_inner_solver_takes(smm, inner, kind):
    which = {i: m for i, _, m in REFINE}[inner]
    csr = matrix(which, np.float64)
    n = len(csr[0]) - 1
    b = rhs(n, np.float64)
    A = smm.CSRMatrix(n, n, *csr)
    A32 = A.astype(np.float32)
    M32 = make_precond(smm, A32, kind)
    x = np.zeros(n)
    info = {}
    try:
        st = smm.IterativeRefinement(A, b, x, REFINE_EPS, inner=inner, a32=A32, M=M32, info=info)
    finally:
        M32.close()
    res = residual(csr, x, b)
    print(inner, kind, "status", int(st), info, "||b - A x|| in NumPy fp64", res, "eps", REFINE_EPS)
    assert int(st) == 0
    assert res <= REFINE_EPS
