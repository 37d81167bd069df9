"""Restarted GMRES(m) with classical Gram-Schmidt applied twice and right preconditioning, stated on the CPU.

A helper, not a test: this is the definition the GPU loop (csrc/smm_solvers_gmres.hip) is compared with.  The method is an addition of
this project (the reference has no GMRES), so there are no goldens and no quirks to preserve.  Sequential.  The row sums and the dot
products are the oracle's (`spmv`, `dot`); the element-wise lines are NumPy in the matrix dtype, written so that every operation rounds
once, like _smm_fma's default a*x+b (ref:28-36).  With the SMM_WITH_STD_FMA flavour those lines cannot be reproduced bit for bit in
NumPy: compare that flavour by tolerance only.

`iterations` counts Arnoldi steps (one SpMV and one orthogonalisation each): a step whose column has to be dropped (d == 0 or not
finite) has been taken and is counted, although it adds nothing to x."""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
MAX_RESTART = 64


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def gmres(oracle, csr, b, x0, max_iterations, eps, restart, apply=None):
    """returns (status, x, iterations, last r.r); x0 is not modified.  apply(rhs) -> z is M^-1 (right preconditioning: the residual
    that is tested is the true one)."""
    start, pos, val = csr
    T = val.dtype.type
    rows = len(start) - 1
    m = int(restart)
    assert 1 <= m <= MAX_RESTART
    eps = T(eps)
    eps_squared = T(eps * eps)
    x = np.array(x0, dtype=val.dtype, copy=True)
    b = np.ascontiguousarray(b, dtype=val.dtype)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        max_iterations = rows  # no other clamp: a restarted run may need more than `rows` steps
    precondition = (lambda v: np.ascontiguousarray(apply(v), dtype=val.dtype)) if apply is not None else (lambda v: v)
    iterations = 0
    diverged = False
    with np.errstate(all="ignore"):
        r = oracle.spmv(csr, OP_SUB, b, x)
        rr = oracle.dot(r, r)
        while rr > eps_squared and iterations < max_iterations and not diverged:
            beta = np.sqrt(rr)
            V = [r / beta]
            g = np.zeros(m + 1, dtype=val.dtype)
            g[0] = beta
            R = np.zeros((m, m), dtype=val.dtype)  # H after the rotations: upper triangular
            cs = np.zeros(m, dtype=val.dtype)
            sn = np.zeros(m, dtype=val.dtype)
            k = 0
            for j in range(m):
                w = oracle.spmv(csr, OP_ASSIGN, None, precondition(V[j]))
                h = None
                for _ in range(2):  # classical Gram-Schmidt, twice: all products of a pass come from the same w
                    hp = [oracle.dot(V[i], w) for i in range(j + 1)]
                    for i in range(j + 1):
                        w = _fma(-hp[i], V[i], w)
                    h = hp if h is None else [T(h[i] + hp[i]) for i in range(j + 1)]
                hn = np.sqrt(oracle.dot(w, w))  # H[j+1][j]
                col = np.array(h, dtype=val.dtype)
                for i in range(j):  # the earlier rotations
                    t = T(cs[i] * col[i]) + T(sn[i] * col[i + 1])
                    col[i + 1] = T(-sn[i] * col[i]) + T(cs[i] * col[i + 1])
                    col[i] = t
                a, c = col[j], hn
                d = np.sqrt(T(a * a) + T(c * c))
                iterations += 1
                if d == 0 or not np.isfinite(d):
                    diverged = True  # the column is dropped: k stays j
                    break
                cs[j], sn[j] = a / d, c / d
                col[j] = T(cs[j] * a) + T(sn[j] * c)
                R[: j + 1, j] = col
                g[j + 1] = -sn[j] * g[j]
                g[j] = cs[j] * g[j]
                k = j + 1
                if hn != 0:
                    V.append(w / hn)
                if not (T(g[j + 1] * g[j + 1]) > eps_squared) or iterations >= max_iterations or hn == 0:
                    break
            if k > 0:
                y = np.zeros(k, dtype=val.dtype)
                for i in range(k - 1, -1, -1):  # back-substitution, the known terms subtracted from the last one down
                    s = g[i]
                    for col_l in range(k - 1, i, -1):
                        s = s - T(R[i, col_l] * y[col_l])
                    y[i] = s / R[i, i]
                t = y[0] * V[0]
                for i in range(1, k):
                    t = _fma(y[i], V[i], t)
                x = x + precondition(t)
            r = oracle.spmv(csr, OP_SUB, b, x)
            rr = oracle.dot(r, r)
    if diverged or not np.isfinite(rr):
        status = DIVERGED
    elif rr <= eps_squared:
        status = SUCCESS
    else:
        status = MAX_ITERATIONS_REACHED
    return status, x, iterations, rr


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, b, it, restart, base=None, apply=None):
    """tests/test_gpu_solvers.py's bicgstab_sensitivity applied to this restatement: how far its own x moves after `it` fixed steps
    when b changes by one unit in the last place (three sign patterns).  A different summation order of the dot products is a
    perturbation of that kind."""
    rows = len(b)
    x0 = np.zeros(rows, dtype=b.dtype)
    if base is None:
        base = gmres(oracle, csr, b, x0, it, 0.0, restart, apply)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = gmres(oracle, csr, perturbed(b, seed), x0, it, 0.0, restart, apply)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
