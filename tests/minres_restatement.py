"""MINRES (Paige and Saunders 1975) with a symmetric positive definite preconditioner, restated on the CPU line for line after the loop
that include/smm_hip.h states.  The reference has no MINRES: this is the definition the GPU loop (csrc/smm_solvers_minres.hip) is
compared with.

A helper, not a test.  Sequential.  The row sums are the oracle's (`spmv`: the reference's exact row arithmetic); the element-wise lines
are NumPy in the matrix dtype, written so that every operation rounds once, like _smm_fma's default a*x+b (ref:28-36) -- with the
SMM_WITH_STD_FMA flavour they cannot be reproduced bit for bit: compare that flavour by tolerance only.

The inner products are partitioned as the kernels partition them (`kernel_dot`): 16-byte packs dealt to the lanes of 256-lane workgroups
four packs per lane and trip (streamMap, csrc/smm_device.h), every lane summing its elements in ascending order; the butterfly over
the 64 lanes of a wave; the four waves left to right; then the NPART partials, each of 256 lanes adding every 256th in ascending order
and the same workgroup sum again (sumParts, csrc/smm_solver_scal.h).  That is exact for r2.r2 and r2.y, whose vectors are 16-byte aligned
buffers of the driver.  alfa = v.(A v) is formed in the SpMV's epilogue, whose partition follows the kernel family's tiles: it is
modelled by the same streaming partition, and a family's other summation order is a perturbation of the size `sensitivity` measures.

`apply` is the preconditioner as a black box: apply(r) returns M^-1 r in r's dtype; None: no preconditioner (y and r2 are one vector)."""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
NPART = 2048  # csrc/smm_internal.h
TPB, WAVE, UNROLL = 256, 64, 4  # STREAM_TPB, the wavefront, STREAM_U


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def _block_sum(acc):
    """blockSum256 over the last axis (256 lanes): butterfly inside each wave, then ((w0 + w1) + w2) + w3"""
    v = acc.reshape(acc.shape[:-1] + (TPB // WAVE, WAVE))
    lane = np.arange(WAVE)
    o = WAVE // 2
    while o > 0:
        v = v + v[..., lane ^ o]
        o >>= 1
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def kernel_dot(a, b, grid=NPART):
    """a.b summed in the order of dotPartialsKernel / minresLanczos (grid workgroups) and sumParts, in the vectors' dtype"""
    dt = a.dtype
    n = len(a)
    per = 16 // dt.itemsize
    nvec = n // per
    chunk = UNROLL * TPB
    prod = a * b
    active = max(1, min(grid, -(-nvec // chunk)))  # the workgroups that own any element: the others' partials are +0
    acc = np.zeros((active, TPB), dtype=dt)
    blk = np.arange(active)[:, None]
    t = np.arange(TPB)[None, :]
    base = blk * chunk
    while base.min() < nvec:
        for u in range(UNROLL):
            pack = base + u * TPB + t
            ok = pack < nvec
            for e in range(per):
                idx = np.where(ok, pack * per + e, 0)
                acc = np.where(ok, acc + prod[idx], acc)
        base = base + grid * chunk
    i = nvec * per + blk * TPB + t  # the last n % per elements: one element per lane
    while i.min() < n:
        ok = i < n
        acc = np.where(ok, acc + prod[np.where(ok, i, 0)], acc)
        i = i + grid * TPB
    partials = np.zeros(NPART, dtype=dt)
    partials[:active] = _block_sum(acc)
    lanes = np.zeros(TPB, dtype=dt)
    for row in partials.reshape(NPART // TPB, TPB):
        lanes = lanes + row
    return dt.type(_block_sum(lanes))


def minres(oracle, csr, b, x0, max_iterations, eps, apply=None, history=None):
    """returns (status, x, iterations, last phibar^2); x0 is not modified.  history, when a list, receives phibar after the start and
    after every step."""
    start, pos, val = csr
    dt = val.dtype
    T = dt.type
    rows = len(start) - 1
    eps = T(eps)
    tiny = T(np.finfo(dt).eps)
    x = np.array(x0, dtype=dt, copy=True)
    b = np.ascontiguousarray(b, dtype=dt)
    if rows == 0:
        return SUCCESS, x, 0, T(0)
    max_iterations = rows if int(max_iterations) == -1 else max(0, min(int(max_iterations), rows))
    solve = (lambda r: r) if apply is None else (lambda r: np.ascontiguousarray(apply(r), dtype=dt))
    with np.errstate(all="ignore"):
        r1 = oracle.spmv(csr, OP_SUB, b, x)
        y = solve(r1)
        ry = kernel_dot(r1, y)
        beta1 = T(np.sqrt(ry))
        res = ry
        if ry < 0 or not np.isfinite(beta1):
            return DIVERGED, x, 0, res
        if history is not None:
            history.append(float(beta1))
        if not (ry > eps * eps) or max_iterations <= 0:
            return (SUCCESS if res <= eps * eps else MAX_ITERATIONS_REACHED), x, 0, res
        r2 = r1.copy()
        oldb, beta, dbar, epsln, phibar, cs, sn = T(0), beta1, T(0), T(0), beta1, T(-1), T(0)
        w = np.zeros(rows, dtype=dt)
        w2 = np.zeros(rows, dtype=dt)
        v = y / beta
        iterations = 0
        status = None
        while True:
            av = oracle.spmv(csr, OP_ASSIGN, None, v)
            alfa = kernel_dot(av, v)
            t = av
            if iterations > 0:
                t = _fma(-T(beta / oldb), r1, t)
            t = _fma(-T(alfa / beta), r2, t)
            r1, r2 = r2, t
            y = solve(r2)
            ry = kernel_dot(r2, y)
            new_beta = T(np.sqrt(ry))
            oldeps = epsln
            delta = T(T(cs * dbar) + T(sn * alfa))
            gbar = T(T(sn * dbar) - T(cs * alfa))
            new_epsln = T(sn * new_beta)
            new_dbar = T(-cs * new_beta)
            root = T(np.sqrt(T(T(gbar * gbar) + T(new_beta * new_beta))))
            gamma = root if (root > tiny or root != root) else tiny
            new_cs = T(gbar / gamma)
            new_sn = T(new_beta / gamma)
            phi = T(new_cs * phibar)
            new_phibar = T(new_sn * phibar)
            if ry < 0 or not np.isfinite(new_beta) or not np.isfinite(new_phibar):
                status = DIVERGED  # the step is not taken
                break
            oldb, beta, epsln, dbar, cs, sn, phibar = beta, new_beta, new_epsln, new_dbar, new_cs, new_sn, new_phibar
            w1, w2 = w2, w
            w = _fma(-delta, w2, _fma(-oldeps, w1, v)) / gamma
            x = _fma(phi, w, x)
            iterations += 1
            res = T(phibar * phibar)
            if history is not None:
                history.append(float(phibar))
            if beta == 0 or not (res > eps * eps) or iterations >= max_iterations:
                break
            v = y / beta
    if status is None:
        status = SUCCESS if res <= eps * eps else MAX_ITERATIONS_REACHED
    return status, x, iterations, res


def perturbed(b, seed):
    """b moved by one unit in the last place, each element up or down by a seeded sign pattern"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=len(b)).astype(b.dtype)
    return np.nextafter(b, b + sign).astype(b.dtype)


def sensitivity(oracle, csr, b, it, base=None, apply=None):
    """how far the restatement's own x moves after `it` fixed steps from x0 = 0 when b changes by one unit in the last place (three
    sign patterns), as tests/cgs_restatement.py measures it.  A different summation order of an inner product is a perturbation of
    that kind."""
    rows = len(b)
    x0 = np.zeros(rows, dtype=b.dtype)
    if base is None:
        base = minres(oracle, csr, b, x0, it, 0.0, apply)[1]
    base = base.astype(np.float64)
    worst = 0.0
    for seed in range(3):
        x = minres(oracle, csr, perturbed(b, seed), x0, it, 0.0, apply)[1]
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - base))))
    return worst
