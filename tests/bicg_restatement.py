"""BiCG for general matrices restated on the CPU: BiCGSymmetric's text (ref:2028-2101) with the shadow sequence written out, as
include/smm_hip.h states it for smm_hip_bicg_*.

A helper, not a test: this is the definition the GPU loop (csrc/smm_solvers_bicg.hip) is compared with.  Sequential.  The row sums and
the dot products are the oracle's (`spmv`, `dot`: the reference's exact row and dot arithmetic); the element-wise lines are NumPy in
the matrix dtype, every operation rounding once -- the reference's plain += / -= forms (ref:2069-2070, 2091), not _smm_fma, so they
are the same bits under the SMM_WITH_STD_FMA flavour too (only the oracle's row sums differ there).  With At = A (the same arrays) it
is BiCGSymmetric: tests/test_bicg_cpu.py pins it to the oracle's bicgsymmetric bit for bit."""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2


def transpose(csr, cols=None):
    """(start, positions, values) of the transpose: a stable sort of the entries by column, so row j holds column j's entries with the
    source rows ascending; values bit for bit"""
    start, pos, val = csr
    rows = len(start) - 1
    cols = rows if cols is None else cols
    nnz = int(start[-1])
    pos, val = pos[:nnz], val[:nnz]
    perm = np.argsort(pos, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(start))
    start_t = np.zeros(cols + 1, dtype=np.int32)
    np.cumsum(np.bincount(pos, minlength=cols), out=start_t[1:])
    return start_t, np.ascontiguousarray(row_of[perm], dtype=np.int32), np.ascontiguousarray(val[perm])


def bicg(oracle, csr, csr_t, b, x0, max_iterations, eps):
    """returns (status, x, iterations, last r.r); x0 is not modified.  csr_t is the transpose (or csr itself: the caller asserts
    symmetry)"""
    start, pos, val = csr
    T = val.dtype.type
    rows = len(start) - 1
    eps = T(eps)
    x = np.array(x0, dtype=val.dtype, copy=True)
    b = np.ascontiguousarray(b, dtype=val.dtype)
    max_iterations = min(int(max_iterations), rows)  # ref:2030
    if max_iterations == -1:  # ref:2031-2033
        max_iterations = rows
    r = oracle.spmv(csr, OP_SUB, b, x)  # ref:2036
    rt, p, pt = r.copy(), r.copy(), r.copy()
    rr = oracle.dot(r, r)  # ref:2043
    rho = oracle.dot(rt, r)
    iterations = 0
    eps_squared = T(eps * eps)
    with np.errstate(all="ignore"):  # no breakdown test beyond the two of the reference: 0 / 0 and x / 0 go into x
        while True:  # do {
            ap = oracle.spmv(csr, OP_ASSIGN, None, p)  # ref:2048
            atp = oracle.spmv(csr_t, OP_ASSIGN, None, pt)
            denom = oracle.dot(ap, pt)  # ref:2049
            if eps > abs(denom) and rr > 1:  # ref:2056-2058
                return DIVERGED, x, iterations, rr
            alpha = T(rho / denom)
            x = x + alpha * p  # ref:2069
            r = r - alpha * ap  # ref:2070
            rt = rt - alpha * atp
            new_rho = oracle.dot(rt, r)
            new_rr = oracle.dot(r, r)  # ref:2075
            if new_rr > 1 and rr < eps:  # ref:2079-2081
                return DIVERGED, x, iterations, rr
            beta = T(new_rho / rho)
            p = r + beta * p  # ref:2091
            pt = rt + beta * pt
            rho, rr = new_rho, new_rr
            iterations += 1
            if not (rr > eps_squared and iterations < max_iterations):  # } while (...), ref:2096
                break
    status = MAX_ITERATIONS_REACHED if iterations > max_iterations else SUCCESS  # ref:2098-2100
    return status, x, iterations, rr


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, csr_t, b, it, base=None):
    """tests/test_gpu_solvers.py's bicgstab_sensitivity applied to this restatement: how far its own x moves after `it` fixed passes
    when b changes by one unit in the last place (three sign patterns).  A different summation order of the dot products is a
    perturbation of that kind."""
    rows = len(b)
    x0 = np.zeros(rows, dtype=b.dtype)
    if base is None:
        base = bicg(oracle, csr, csr_t, b, x0, it, 0.0)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = bicg(oracle, csr, csr_t, perturbed(b, seed), x0, it, 0.0)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
