"""IDR(s) in the biorthogonal form (van Gijzen and Sonneveld 2011) with right preconditioning, stated on the CPU.

A helper, not a test: this is the definition the GPU loop (csrc/smm_solvers_idrs.hip) is compared with.  The method is an addition of
this project (the reference has no IDR(s)), so there are no goldens and no quirks to preserve.  Sequential.  The row sums and the dot
products are the oracle's (`spmv`, `dot`); the element-wise lines are NumPy in the matrix dtype, written so that every operation rounds
once, like _smm_fma's default a*x+b (ref:28-36).  With the SMM_WITH_STD_FMA flavour those lines cannot be reproduced bit for bit in
NumPy: compare that flavour by tolerance only.

`iterations` counts SpMVs: every inner step and every dimension-reduction step is one.  The shadow space P is an (s, rows) array, row i
the i-th shadow vector; `shadow` makes the one the library generates from a seed."""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
MAX_S = 8
_MASK = (1 << 64) - 1


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def splitmix64(z):
    """one step of splitmix64 on a Python int: the state advanced by the golden-ratio constant, then the output mix"""
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def shadow_hash(seed, col, row):
    """h of element (row, col) of the generated shadow space"""
    return splitmix64(splitmix64(splitmix64(int(seed) & _MASK) ^ int(col)) ^ int(row))


def _splitmix64_array(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def raw_shadow(rows, s, seed, dtype):
    """(s, rows): ((h >> 40) + 0.5) 2^-23 - 1 = (2 (h >> 40) + 1 - 2^24) 2^-24, an odd multiple of 2^-24 inside (-1, 1): exact in fp32 too"""
    P = np.empty((s, rows), dtype=dtype)
    idx = np.arange(rows, dtype=np.uint64)
    for col in range(s):
        hc = np.uint64(splitmix64(splitmix64(int(seed) & _MASK) ^ col))
        h = _splitmix64_array(hc ^ idx)
        m = 2 * (h >> np.uint64(40)).astype(np.int64) + 1 - (1 << 24)
        P[col] = (m.astype(np.float64) * 2.0 ** -24).astype(dtype)  # (exact in fp64, and the cast rounds nothing)
    return P


def shadow(oracle, rows, s, seed, dtype):
    """the library's own P: the hash, then classical Gram-Schmidt applied twice and a division by the norm, column by column"""
    T = np.dtype(dtype).type
    P = raw_shadow(rows, s, seed, dtype)
    for j in range(s):
        p = P[j].copy()
        for _ in range(2 if j else 0):  # all products of a pass come from the same p
            hp = [oracle.dot(P[i].copy(), p) for i in range(j)]
            for i in range(j):
                p = _fma(T(-hp[i]), P[i], p)
        P[j] = p / T(np.sqrt(oracle.dot(p, p)))
    return P


def idrs(oracle, csr, b, x0, max_iterations, eps, s, P=None, seed=0, apply=None):
    """returns (status, x, iterations, last r.r); x0 is not modified.  P: (s, rows) or None (generated from `seed`).  apply(rhs) -> z is
    M^-1 (right preconditioning: the residual that is tested is the recurrence residual of the original system)."""
    start, pos, val = csr
    dt = val.dtype
    T = dt.type
    rows = len(start) - 1
    s = int(s)
    assert 1 <= s <= MAX_S
    eps = T(eps)
    eps_squared = T(eps * eps)
    x = np.array(x0, dtype=dt, copy=True)
    b = np.ascontiguousarray(b, dtype=dt)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        max_iterations = rows
    if P is None:
        P = shadow(oracle, rows, s, seed, dt)
    P = [np.ascontiguousarray(P[i], dtype=dt) for i in range(s)]
    precondition = (lambda v: np.ascontiguousarray(apply(v), dtype=dt)) if apply is not None else (lambda v: v)
    iterations = 0
    diverged = False
    with np.errstate(all="ignore"):
        r = oracle.spmv(csr, OP_SUB, b, x)
        rr = oracle.dot(r, r)
        G = [np.zeros(rows, dtype=dt) for _ in range(s)]
        U = [np.zeros(rows, dtype=dt) for _ in range(s)]
        M = np.eye(s, dtype=dt)
        om = T(1)
        over = False
        while rr > eps_squared and iterations < max_iterations and not over:
            f = np.array([oracle.dot(P[i], r) for i in range(s)], dtype=dt)
            for k in range(s):
                c = np.zeros(s, dtype=dt)
                for i in range(k, s):  # forward substitution on the trailing block
                    acc = f[i]
                    for j in range(k, i):
                        acc = T(acc - T(M[i, j] * c[j]))
                    c[i] = T(acc / M[i, i])
                v = r
                for i in range(k, s):
                    v = _fma(T(-c[i]), G[i], v)
                z = precondition(v)
                u = om * z
                for i in range(k, s):
                    u = _fma(c[i], U[i], u)
                g = oracle.spmv(csr, OP_ASSIGN, None, np.ascontiguousarray(u))
                h = [oracle.dot(P[i], g) for i in range(s)]  # all from the same g
                a = np.zeros(s, dtype=dt)
                for i in range(k):
                    acc = h[i]
                    for j in range(i):
                        acc = T(acc - T(M[i, j] * a[j]))
                    a[i] = T(acc / M[i, i])
                col = np.zeros(s, dtype=dt)
                for i in range(k, s):
                    acc = h[i]
                    for j in range(k):
                        acc = T(acc - T(M[i, j] * a[j]))
                    col[i] = acc
                for i in range(k):
                    g = _fma(T(-a[i]), G[i], g)
                    u = _fma(T(-a[i]), U[i], u)
                G[k], U[k] = g, u
                M[:, k] = col
                if col[k] == 0 or not np.isfinite(col[k]):
                    diverged = over = True
                    break
                beta = T(f[k] / col[k])
                r = _fma(T(-beta), g, r)
                x = _fma(beta, u, x)
                rr = oracle.dot(r, r)
                iterations += 1
                if not (rr > eps_squared and iterations < max_iterations):
                    over = True
                    break
                for i in range(k + 1, s):
                    f[i] = T(f[i] - T(beta * M[i, k]))
            if over:
                break
            z = precondition(r)
            t = oracle.spmv(csr, OP_ASSIGN, None, np.ascontiguousarray(z))
            tt = oracle.dot(t, t)
            tr = oracle.dot(t, r)
            if tt == 0 or not np.isfinite(tt):
                diverged = True
                break
            rho = T(abs(tr) / np.sqrt(T(tt * rr)))
            om = T(tr / tt)
            if rho < T(0.7):  # "maintaining the convergence"
                om = T(om * T(T(0.7) / rho))
            x = _fma(om, z, x)
            r = _fma(T(-om), t, r)
            rr = oracle.dot(r, r)
            iterations += 1
    if rr <= eps_squared:
        status = SUCCESS
    elif diverged:
        status = DIVERGED
    else:
        status = MAX_ITERATIONS_REACHED
    return status, x, iterations, rr


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, b, it, s, P, base=None, apply=None):
    """tests/test_gpu_solvers.py's bicgstab_sensitivity applied to this restatement: how far its own x moves after `it` fixed steps
    when b changes by one unit in the last place (three sign patterns).  A different summation order of the dot products is a
    perturbation of that kind."""
    rows = len(b)
    x0 = np.zeros(rows, dtype=b.dtype)
    if base is None:
        base = idrs(oracle, csr, b, x0, it, 0.0, s, P, apply=apply)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = idrs(oracle, csr, perturbed(b, seed), x0, it, 0.0, s, P, apply=apply)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
