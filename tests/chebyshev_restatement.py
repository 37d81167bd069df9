"""The Chebyshev polynomial preconditioner in D^-1 A, stated on the CPU.

A helper, not a test: this is the definition csrc/smm_precond_cheb.hip is compared with (include/smm_hip.h, SMM_PRECOND_CHEBYSHEV, states
it in words).  The preconditioner is an addition of this project (the reference has none like it), so there are no goldens and no quirks
to preserve.  The row sums and the dot products are the oracle's (`spmv`, `dot`); the element-wise lines are NumPy in the matrix dtype,
written so that every operation rounds once, like _smm_fma's default a*x+b (ref:28-36).  With the SMM_WITH_STD_FMA flavour those lines
cannot be reproduced bit for bit in NumPy: compare that flavour by tolerance only.

Also here: the preconditioned ConjugateGradient stated like the oracle's IC0 loop (ref:2414-2505) and BiCGStab stated like the oracle's
template (ref:2191-2283), each with M^-1 given as a function, and the sensitivity measure of tests/gmres_restatement.py for any of them."""
import numpy as np

from gmres_restatement import perturbed

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
GERSHGORIN, POWER, USER = 0, 1, 2
MAX_DEGREE = 64


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def diagonal(csr):
    """the stored diagonal, taken with its sign: per row the first stored entry whose column is the row (0 where there is none)"""
    start, pos, val = csr
    n = len(start) - 1
    diag = np.zeros(n, dtype=val.dtype)
    rowof = np.repeat(np.arange(n), np.diff(start))
    hit = np.nonzero(pos == rowof)[0][::-1]  # reversed: the first hit of a row is written last
    diag[rowof[hit]] = val[hit]
    return diag


def coefficients(degree, lmin, lmax, dtype):
    """(T(1 / theta), c1[0 .. degree], c2[0 .. degree]) with index 0 unused: the scalars in double, each cast to T once"""
    assert 0 <= degree <= MAX_DEGREE and 0 < lmin < lmax
    T = np.dtype(dtype).type
    lmin, lmax = float(lmin), float(lmax)
    theta = (lmax + lmin) / 2
    delta = (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [T(0)], [T(0)]
    for _ in range(degree):
        nxt = 1.0 / (2.0 * sigma - rho)
        c1.append(T(nxt * rho))
        c2.append(T(2.0 * nxt / delta))
        rho = nxt
    return T(1.0 / theta), c1, c2


def gershgorin(csr):
    """max_i (sum_j |a_ij|) / |a_ii|: every row summed in double, sequentially, in stored order; divided in double"""
    start, pos, val = csr
    n = len(start) - 1
    length = np.diff(start)
    mag = np.abs(val.astype(np.float64))
    total = np.zeros(n, dtype=np.float64)
    for k in range(int(length.max()) if n else 0):  # the k-th stored entry of every row that has one: sequential inside each row
        rows = np.nonzero(length > k)[0]
        total[rows] = total[rows] + mag[start[rows] + k]
    return float(np.max(total / np.abs(diagonal(csr).astype(np.float64))))


def power_bound(oracle, csr, steps):
    """min(gershgorin, 1.1 * the last Rayleigh quotient) after `steps` steps of the power method on D^-1 A from v[i] = 1 + (i mod 7) / 8:
    w = (A v) / diag; rq = (v.w) / (v.v); v = w * T(1 / sqrt(w.w)) -- dot products in T, the quotient and the root in double.
    A heuristic, not a bound."""
    start, pos, val = csr
    T = val.dtype.type
    n = len(start) - 1
    diag = diagonal(csr)
    v = (T(1) + (np.arange(n) % 7).astype(val.dtype) / T(8)).astype(val.dtype)
    rq = 0.0
    for _ in range(steps):
        w = oracle.spmv(csr, OP_ASSIGN, None, v) / diag
        vw, vv, ww = float(oracle.dot(v, w)), float(oracle.dot(v, v)), float(oracle.dot(w, w))
        rq = vw / vv
        v = w * T(1.0 / np.sqrt(ww))
    return min(gershgorin(csr), 1.1 * rq)


def apply(oracle, csr, diag, coeffs, r):
    """z = M^-1 r"""
    inv_theta, c1, c2 = coeffs
    r = np.ascontiguousarray(r, dtype=csr[2].dtype)
    t = r / diag
    d = t * inv_theta
    z = d.copy()
    for k in range(1, len(c1)):
        q = oracle.spmv(csr, OP_SUB, r, z)
        t = q / diag
        u = c2[k] * t
        d = _fma(c1[k], d, u)
        z = z + d
    return z


def make_apply(oracle, csr, degree, lmin, lmax):
    """M^-1 as a function of one vector"""
    diag = diagonal(csr)
    coeffs = coefficients(degree, lmin, lmax, csr[2].dtype)
    return lambda r: apply(oracle, csr, diag, coeffs, r)


def pcg(oracle, csr, b, x0, maxit, eps, apply):
    """ConjugateGradient with M^-1 = apply, the loop of ref:2414-2505 as oracle/smm_oracle_impl.inc states it for IC0.
    Returns (status, x, iterations, last r.r)."""
    val = csr[2]
    T = val.dtype.type
    rows = len(csr[0]) - 1
    eps_squared = T(T(eps) * T(eps))
    x0 = np.ascontiguousarray(x0, dtype=val.dtype)
    x = x0.copy()
    with np.errstate(all="ignore"):
        r = oracle.spmv(csr, OP_SUB, np.ascontiguousarray(b, dtype=val.dtype), x0)
        z = apply(r)
        rz = oracle.dot(r, z)
        rr = oracle.dot(r, r)
        p = z.copy()
        if eps_squared > rr:
            return SUCCESS, x, 0, rr
        if maxit == -1:
            maxit = rows
        cur = x0
        it = 0
        for i in range(maxit):
            Ap = oracle.spmv(csr, OP_ASSIGN, None, p)
            alpha = T(rz / oracle.dot(Ap, p))
            x = _fma(alpha, p, cur)
            r = _fma(-alpha, Ap, r)
            z = apply(r)
            new_rz = oracle.dot(r, z)
            rr = oracle.dot(r, r)
            it = i + 1
            if eps_squared > rr:
                return SUCCESS, x, it, rr
            beta = T(new_rz / rz)
            p = _fma(beta, p, z)
            rz = new_rz
            cur = x
    return MAX_ITERATIONS_REACHED, x, it, rr


def bicgstab(oracle, csr, b, x0, maxit, eps, apply):
    """BiCGStab<Preconditioner, T> (ref:2191-2283) as oracle/smm_oracle_impl.inc states it, with M^-1 = apply.
    Returns (status, x, iterations, last ||r||)."""
    val = csr[2]
    T = val.dtype.type
    rows = len(csr[0]) - 1
    maxit = min(maxit, rows)
    if maxit == -1:
        maxit = rows
    x = np.array(x0, dtype=val.dtype, copy=True)
    with np.errstate(all="ignore"):
        r = apply(oracle.spmv(csr, OP_SUB, np.ascontiguousarray(b, dtype=val.dtype), x))
        r0 = r.copy()
        p = r.copy()
        rr0 = oracle.dot(r, r0)
        it = 0
        while True:
            ap = apply(oracle.spmv(csr, OP_ASSIGN, None, p))
            alpha = T(rr0 / oracle.dot(ap, r0))
            s = _fma(-alpha, ap, r)
            As = apply(oracle.spmv(csr, OP_ASSIGN, None, s))
            omega = T(oracle.dot(As, s) / oracle.dot(As, As))
            x = _fma(alpha, p, _fma(omega, s, x))
            r = _fma(-omega, As, s)
            res = np.sqrt(oracle.dot(r, r))
            new_rr0 = oracle.dot(r, r0)
            beta = T(T(new_rr0 * alpha) / T(rr0 * omega))
            p = _fma(beta, _fma(-omega, ap, p), r)
            rr0 = new_rr0
            it += 1
            if not (res > T(eps) and it < maxit):
                break
    return (MAX_ITERATIONS_REACHED if it > maxit else SUCCESS), x, it, res


def sensitivity(solve, b, base=None):
    """tests/gmres_restatement.py's measure for any restated solve: how far x = solve(b) moves when b changes by one unit in the last
    place (three sign patterns).  A different summation order of the row sums or dot products is a perturbation of that kind."""
    if base is None:
        base = solve(b)
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = solve(perturbed(b, seed))
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
