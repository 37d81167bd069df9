"""ConjugateGradientSquared restated on the CPU, line for line after the reference's text (ref:2110-2178), with the ONE repair that
include/smm_hip.h states: `residualSquared` is declared before the `do`, so that the loop condition reads the value the body has just
computed (as published, ref:2171-2172, the template cannot be instantiated -- which is why there are no goldens for it).

A helper, not a test: this is the definition the GPU loop (csrc/smm_solvers_cgs.hip) is compared with.  Sequential.  The row sums and
the dot products are the oracle's (`spmv`, `spmv_inplace`, `dot`: the reference's exact row and dot arithmetic); the element-wise lines
are NumPy in the matrix dtype, written so that every operation rounds once, like _smm_fma's default a*x+b (ref:28-36).  With the
SMM_WITH_STD_FMA flavour those lines cannot be reproduced bit for bit in NumPy: compare that flavour by tolerance only."""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, MAX_ITERATIONS_REACHED = 0, 2


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def cgs(oracle, csr, b, x0, max_iterations, eps):
    """returns (status, x, iterations, last r.r); x0 is not modified"""
    start, pos, val = csr
    T = val.dtype.type
    rows = len(start) - 1
    eps = T(eps)
    x = np.array(x0, dtype=val.dtype, copy=True)
    b = np.ascontiguousarray(b, dtype=val.dtype)
    max_iterations = min(int(max_iterations), rows)  # ref:2111
    if max_iterations == -1:  # ref:2112-2114
        max_iterations = rows
    r = oracle.spmv(csr, OP_SUB, b, x)  # ref:2118
    p, u, r0 = r.copy(), r.copy(), r.copy()  # ref:2124-2126
    rr0 = oracle.dot(r, r0)  # ref:2128
    iterations = 0  # ref:2129
    eps_squared = T(eps * eps)  # ref:2130
    residual_squared = T(0)  # THE REPAIR: declared here, not at ref:2171
    with np.errstate(all="ignore"):  # no breakdown test (ref:2134, 2153): 0 / 0 and x / 0 go into x as in the reference
        while True:  # do {
            ap = oracle.spmv(csr, OP_ASSIGN, None, p)  # ref:2132
            denom = oracle.dot(ap, r0)  # ref:2133
            alpha = T(rr0 / denom)  # ref:2135
            q = _fma(-alpha, ap, u)  # ref:2146
            uq = u + q
            alpha_uq = alpha * uq  # ref:2147: an add, then a multiply
            x = x + alpha_uq  # ref:2148
            r = oracle.spmv_inplace(csr, OP_SUB, r, alpha_uq)  # ref:2151: out aliases lhs
            new_rr0 = oracle.dot(r, r0)  # ref:2152
            beta = T(new_rr0 / rr0)  # ref:2154
            u = _fma(beta, q, r)  # ref:2165
            p = _fma(beta, _fma(beta, p, q), u)  # ref:2166
            rr0 = new_rr0  # ref:2169
            iterations += 1  # ref:2170
            residual_squared = oracle.dot(r, r)  # ref:2171
            if not (residual_squared > eps_squared and iterations < max_iterations):  # } while (...), ref:2172
                break
    status = MAX_ITERATIONS_REACHED if iterations > max_iterations else SUCCESS  # ref:2174-2177
    return status, x, iterations, residual_squared


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, b, it, base=None):
    """tests/test_gpu_solvers.py's bicgstab_sensitivity applied to this restatement: how far its own x moves after `it` fixed passes
    when b changes by one unit in the last place (three sign patterns).  A different summation order of the dot products is a
    perturbation of that kind."""
    rows = len(b)
    x0 = np.zeros(rows, dtype=b.dtype)
    if base is None:
        base = cgs(oracle, csr, b, x0, it, 0.0)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = cgs(oracle, csr, perturbed(b, seed), x0, it, 0.0)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
