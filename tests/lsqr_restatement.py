"""LSQR (Paige and Saunders 1982) with damping, restated on the CPU line for line after the loop that include/smm_hip.h states.  The
reference has no LSQR: this is the definition the GPU loop (csrc/smm_solvers_lsqr.hip) is compared with.

A helper, not a test.  Sequential.  The row sums of A v and At ub are the oracle's (`spmv`: the reference's exact row arithmetic, on the
CSR arrays of A and of its transpose); the element-wise lines are NumPy in the matrix dtype, written so that every operation rounds
once, like _smm_fma's default a*x+b (ref:28-36) -- with the SMM_WITH_STD_FMA flavour they cannot be reproduced bit for bit: compare that
flavour by tolerance only.  The inner products ub.ub and vb.vb are partitioned as the kernels partition them (`kernel_dot` of
tests/minres_restatement.py, with the grid of the update kernel that forms them): ub and vb are 16-byte aligned buffers of the driver.

x IS UPDATED IN PLACE: x = _smm_fma(phi / rho, w, x).  The solve is for the correction dx = x - x0, and no separate dx is kept, so from
x0 = 0 x holds dx's bits; with damp > 0 it is dx that is damped.  t / beta is rounded as a quotient before _smm_fma(-beta, v, .)."""
import numpy as np
from minres_restatement import NPART, TPB, _fma, kernel_dot

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2


def solver_grid(n):
    """solverGrid (csrc/smm_solver_host.h)"""
    return max(1, min(-(-n // TPB), NPART))


def rotations(T, damp, rhobar, phibar, bb, beta, alpha):
    """the scalars of one step, each operation rounded in T: returns (rho, c, theta, rhobar', phi, phibar', psi)"""
    if damp == 0:
        rb1, psi, phibar1 = rhobar, T(0), phibar  # the first rotation is the identity, bit for bit
    else:
        rb1 = T(np.sqrt(T(T(rhobar * rhobar) + T(damp * damp))))
        c1 = T(rhobar / rb1)
        s1 = T(damp / rb1)
        psi = T(s1 * phibar)
        phibar1 = T(c1 * phibar)
    rho = T(np.sqrt(T(T(rb1 * rb1) + bb)))
    c = T(rb1 / rho)
    s = T(beta / rho)
    theta = T(s * alpha)
    new_rhobar = T(-c * alpha)
    phi = T(c * phibar1)
    new_phibar = T(s * phibar1)
    return rho, c, theta, new_rhobar, phi, new_phibar, psi


def lsqr(oracle, csr, csr_t, b, x0, max_iterations, eps, damp=0.0, history=None):
    """csr: A (rows x cols, rows = len(b), cols = len(x0)); csr_t: the CSR arrays of its transpose.  Returns (status, x, iterations,
    reason, res, arn); x0 is not modified.  history, when a list, receives (res, arn) after the start and after every step."""
    start, pos, val = csr
    dt = val.dtype
    T = dt.type
    rows, cols = len(start) - 1, len(csr_t[0]) - 1
    eps, damp = T(eps), T(damp)
    assert np.isfinite(eps) and eps >= 0 and np.isfinite(damp) and damp >= 0
    x = np.array(x0, dtype=dt, copy=True)
    b = np.ascontiguousarray(b, dtype=dt)
    assert len(b) == rows and len(x) == cols
    if rows == 0 or cols == 0:
        return SUCCESS, x, 0, (1 if rows == 0 else 2), T(0), T(0)
    max_iterations = cols if int(max_iterations) < 0 else int(max_iterations)
    gm, gn = solver_grid(rows), solver_grid(cols)
    eps2 = T(eps * eps)

    def finish(status, iterations, res, arn):
        if status is None:
            status = SUCCESS if (res <= eps2 or arn <= eps2) else MAX_ITERATIONS_REACHED
        reason = 0
        if status == SUCCESS:
            reason = 1 if res <= eps2 else 2
        return status, x, iterations, reason, res, arn

    with np.errstate(all="ignore"):
        ub = b.copy() if not x.any() and np.isfinite(val).all() else oracle.spmv(csr, OP_SUB, b, x)
        bb = kernel_dot(ub, ub)
        beta = T(np.sqrt(bb))
        t = oracle.spmv(csr_t, OP_ASSIGN, None, ub)
        vb = np.zeros(cols, dtype=dt) if beta == 0 else t / beta
        aa = kernel_dot(vb, vb, gn)
        alpha = T(np.sqrt(aa))
        ab = T(alpha * beta)
        res, arn = bb, T(ab * ab)
        if history is not None:
            history.append((float(res), float(arn)))
        if not np.isfinite(beta) or not np.isfinite(alpha):
            return finish(DIVERGED, 0, res, arn)
        if bb == 0 or aa == 0 or not (res > eps2) or not (arn > eps2) or max_iterations <= 0:
            return finish(None, 0, res, arn)
        v = vb / alpha
        w = v.copy()
        phibar, rhobar, psi2 = beta, alpha, T(0)
        iterations = 0
        status = None
        while True:
            q = oracle.spmv(csr, OP_ASSIGN, None, v)
            ub = _fma(-T(alpha / beta), ub, q)
            bb = kernel_dot(ub, ub, gm)
            beta = T(np.sqrt(bb))
            t = oracle.spmv(csr_t, OP_ASSIGN, None, ub)
            vb = np.zeros(cols, dtype=dt) if beta == 0 else _fma(-beta, v, t / beta)
            aa = kernel_dot(vb, vb, gn)
            alpha = T(np.sqrt(aa))
            rho, c, theta, new_rhobar, phi, new_phibar, psi = rotations(T, damp, rhobar, phibar, bb, beta, alpha)
            if not (np.isfinite(beta) and np.isfinite(alpha) and np.isfinite(rho) and np.isfinite(new_phibar)) or rho == 0:
                status = DIVERGED  # the step is not taken
                break
            rhobar, phibar = new_rhobar, new_phibar
            x = _fma(T(phi / rho), w, x)
            v = np.zeros(cols, dtype=dt) if alpha == 0 else vb / alpha
            w = _fma(-T(theta / rho), w, v)
            psi2 = T(psi2 + T(psi * psi))
            res = T(T(phibar * phibar) + psi2)
            ar = T(T(alpha * abs(c)) * phibar)
            arn = T(ar * ar)
            iterations += 1
            if history is not None:
                history.append((float(res), float(arn)))
            if beta == 0 or alpha == 0 or not (res > eps2) or not (arn > eps2) or iterations >= max_iterations:
                break
    return finish(status, iterations, res, arn)


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, csr_t, b, it, damp=0.0, base=None):
    """how far the restatement's own x moves after `it` fixed steps from x0 = 0 when b changes by one unit in the last place (three
    sign patterns), as tests/minres_restatement.py measures it.  A different summation order of an inner product or of a row sum is a
    perturbation of that kind."""
    cols = len(csr_t[0]) - 1
    x0 = np.zeros(cols, dtype=b.dtype)
    if base is None:
        base = lsqr(oracle, csr, csr_t, b, x0, it, 0.0, damp)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = lsqr(oracle, csr, csr_t, perturbed(b, seed), x0, it, 0.0, damp)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
