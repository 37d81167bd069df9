"""Mixed-precision iterative refinement, stated on the CPU.

A helper, not a test: this is the definition the GPU loop (csrc/smm_solvers_refine.hip) is compared with; include/smm_hip.h states the same
loop in words.  The method is an addition of this project (the reference has none), so there are no goldens.  The outer loop is float64
NumPy with the oracle's row sums and dot product; the inner solve is the oracle's ConjugateGradient or BiCGStab in float32 (NONE or
JACOBI), or tests/gmres_restatement.py's GMRES, on `csr32` from a zero start.  Every element-wise line rounds once: the two scalings
are by powers of two, so a fused multiply-add and a * x + b give the candidate the same bits."""
import numpy as np
from gmres_restatement import gmres

OP_SUB = 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
PRECOND_NONE, PRECOND_JACOBI = 0, 1


def rounded(csr):
    """the float32 matrix a32 stands for: the pattern, and every value rounded to nearest even"""
    return csr[0], csr[1], csr[2].astype(np.float32)


def inner_solve(oracle, inner, csr32, r32, max_inner, inner_eps, restart, jacobi):
    """(d32, iterations) of the float32 solve of A32 d32 = r32 from d32 = 0; the inner status is not looked at"""
    zero = np.zeros(len(r32), dtype=np.float32)
    diag = oracle.jacobi_setup(csr32)[1] if jacobi else None
    if inner == "CG":
        assert not jacobi, "ConjugateGradient takes no JACOBI preconditioner"
        _, d32, it, _ = oracle.cg(csr32, r32, zero, max_inner, inner_eps)
    elif inner == "BICGSTAB":
        _, d32, it, _ = oracle.bicgstab(csr32, r32, zero, max_inner, inner_eps, PRECOND_JACOBI if jacobi else PRECOND_NONE, diag)
    elif inner == "GMRES":
        apply = (lambda v: oracle.jacobi_apply(diag, np.ascontiguousarray(v))) if jacobi else None
        _, d32, it, _ = gmres(oracle, csr32, r32, zero, max_inner, inner_eps, restart, apply)
    else:
        raise ValueError(inner)
    return d32, it


def refine(oracle, csr, csr32, b, x0, eps, inner="CG", max_outer=20, max_inner=-1, inner_eps=1e-4, restart=30, jacobi=False):
    """returns (status, x, outer iterations, inner iterations, the true r.r of x); x0 is not modified"""
    assert csr[2].dtype == np.float64 and csr32[2].dtype == np.float32
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64, copy=True)
    eps = np.float64(eps)
    inner_eps = np.float32(inner_eps)
    outer = inner_total = 0
    rejected = False
    with np.errstate(all="ignore"):
        r = oracle.spmv(csr, OP_SUB, b, x)
        rr = oracle.dot(r, r)
        while rr > eps * eps and outer < max_outer:
            nrm = np.sqrt(rr)
            e = int(np.frexp(nrm)[1]) if np.isfinite(nrm) else 0  # sqrt(rr) = m 2^e, m in [0.5, 1)
            r32 = (r * np.ldexp(1.0, -e)).astype(np.float32)  # exact scaling, one rounding
            d32, it = inner_solve(oracle, inner, csr32, r32, max_inner, inner_eps, restart, jacobi)
            inner_total += it
            xc = np.ldexp(1.0, e) * d32.astype(np.float64) + x  # the product is exact: one rounding, as fma
            rc = oracle.spmv(csr, OP_SUB, b, xc)
            rrc = oracle.dot(rc, rc)
            if not rrc < rr:  # a NaN included: x keeps its bits
                rejected = True
                break
            x, r, rr = xc, rc, rrc
            outer += 1
    if rejected or not np.isfinite(rr):
        status = DIVERGED
    elif not rr > eps * eps:
        status = SUCCESS
    else:
        status = MAX_ITERATIONS_REACHED
    return status, x, outer, inner_total, float(rr)


def cases():
    """(name, matrix of gen_matrices, inner solver, restart, right-hand side from the float64 csr): the cases of the CPU and GPU tests"""
    from sparse_matrix_math_amd import generators as gen

    def ones(csr):
        return gen.row_sums(csr[0], csr[2])

    def sevenths(oracle_spmv, csr):
        xs = 1.0 + (np.arange(len(csr[0]) - 1) % 7) / 7.0  # all ones is an eigenvector of banded_2000
        return oracle_spmv(csr, 0, None, xs)

    return [("poisson2d_32/CG", "poisson2d_32", "CG", 30, lambda o, c: ones(c)),
            ("banded_2000/CG", "banded_2000", "CG", 30, lambda o, c: sevenths(o.spmv, c)),
            ("convdiff3d_12/BICGSTAB", "convdiff3d_12", "BICGSTAB", 30, lambda o, c: ones(c)),
            ("convdiff3d_12/GMRES", "convdiff3d_12", "GMRES", 20, lambda o, c: ones(c))]
