"""eigsh, restated line by line in numpy: thick-restart Lanczos (Wu and Simon 2000) with full reorthogonalisation, the definition
csrc/smm_solvers_eigsh.hip is compared with (include/smm_hip.h states it in words).  Vectors and their sums are in the matrix's dtype;
the small eigenproblem is fp64 for both dtypes, as in the library -- which solves it by cyclic Jacobi where this file calls
numpy.linalg.eigh: any accurate fp64 symmetric solver is admissible there, and nothing downstream of it is compared bit for bit.
The sums are numpy's, not the kernels' partitioned ones: the comparison with the GPU is by bounds, not by bits."""
import numpy as np

LARGEST, SMALLEST = 0, 1
MAX_NCV = 64
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
_M64 = (1 << 64) - 1


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hash_vector(n, seed, col, dtype):
    """element row = ((h >> 40) + 0.5) 2^-23 - 1 with h = mix(mix(mix(seed) ^ col) ^ row): IDR(s)'s shadow generator, exact in fp32"""
    hc = _mix(_mix(seed & _M64) ^ col)
    m = np.array([2 * (_mix(hc ^ row) >> 40) + 1 - (1 << 24) for row in range(n)], dtype=np.int64)
    return (m.astype(np.float64) / 16777216.0).astype(dtype)


def resolve_ncv(rows, k, ncv):
    return min(rows, max(2 * k + 1, 20)) if not ncv else ncv


def eigsh(a, k, which, ncv=0, max_restarts=100, tol=0.0, v0=None, seed=0, history=None):
    """a: a dense symmetric array whose dtype is the working precision.  Returns a dict: status, w, X, residuals, nconv, restarts, matvecs.
    history, when a list, receives (m, l, broke) per cycle."""
    T = a.dtype.type
    n = a.shape[0]
    eps = float(np.finfo(a.dtype).eps)
    ncv = resolve_ncv(n, k, ncv)
    assert k >= 1 and k + 2 <= ncv <= min(n, MAX_NCV) and which in (LARGEST, SMALLEST)
    bound = float(tol) if tol > 0 else eps
    V = np.zeros((n, ncv + 1), dtype=a.dtype)
    out = dict(status=SUCCESS, w=None, X=None, residuals=None, nconv=0, restarts=0, matvecs=0)

    def orthogonalise(j):
        """column j against the j columns before it, classical Gram-Schmidt twice; returns the two passes' products and w . w"""
        w = V[:, j]
        hs = []
        for _ in range(2):
            h = V[:, :j].T @ w
            for i in range(j):  # i ascending, one product and one sum each
                w = (-h[i]) * V[:, i] + w
            hs.append(h)
        V[:, j] = w
        return hs[0], hs[1], T(np.dot(w, w))

    l, fresh, need_start = 0, 0, True
    kept = np.zeros(0)
    arrow = np.zeros(0)
    scale = T(0)
    while True:
        if len(kept):
            scale = max(scale, T(np.max(np.abs(kept))))
        bad = False
        if need_start:
            if l == 0 and v0 is not None:
                V[:, 0] = np.asarray(v0, dtype=a.dtype)
                ww = T(np.dot(V[:, 0], V[:, 0]))
            else:
                V[:, l] = hash_vector(n, seed, fresh, a.dtype)
                fresh += 1
                ww = T(np.dot(V[:, 0], V[:, 0])) if l == 0 else orthogonalise(l)[2]
            d = np.sqrt(ww)
            if not (d > 0) or not np.isfinite(d):
                bad = True
            else:
                V[:, l] = V[:, l] / d
            need_start = False
        alpha = np.zeros(ncv, dtype=a.dtype)
        beta = np.zeros(ncv, dtype=a.dtype)
        broke = -1
        for j in range(l, ncv):
            if bad:
                break
            V[:, j + 1] = a @ V[:, j]
            out["matvecs"] += 1
            h1, h2, ww = orthogonalise(j + 1)
            alpha[j] = h1[j] + h2[j]
            beta[j] = np.sqrt(ww)
            if not np.isfinite(alpha[j]) or not np.isfinite(beta[j]):
                bad = True
                break
            scale = max(scale, abs(alpha[j]), beta[j])
            if beta[j] <= T(eps) * scale:  # breakdown: v_{j+1} is not formed, nothing divides by this beta
                broke = j
                break
            V[:, j + 1] = V[:, j + 1] / beta[j]
        if bad:
            out["status"] = DIVERGED
            return out
        m = broke + 1 if broke >= 0 else ncv
        t = np.zeros((m, m))
        for i in range(l):
            t[i, i] = kept[i]
            t[i, l] = t[l, i] = arrow[i]
        for j in range(l, m):
            t[j, j] = float(alpha[j])
            if j + 1 < m:
                t[j, j + 1] = t[j + 1, j] = float(beta[j])
        if not np.all(np.isfinite(t)):
            out["status"] = DIVERGED
            return out
        theta, y = np.linalg.eigh(t)  # ascending
        order = np.arange(m)[::-1] if which == LARGEST else np.arange(m)
        last = 0.0 if broke >= 0 else float(beta[m - 1])
        norm_a = float(np.max(np.abs(theta)))
        have = min(k, m)
        rho = np.abs(last * y[m - 1, order])
        nconv = int(np.sum(rho[:have] <= bound * norm_a))
        if history is not None:
            history.append((m, l, broke >= 0))
        if nconv == k or (broke >= 0 and m >= k) or out["restarts"] >= max_restarts:
            out["w"] = theta[order[:have]].astype(a.dtype)
            out["X"] = rotate(V[:, :m], y[:, order[:have]].astype(a.dtype))
            out["residuals"] = rho[:have].astype(a.dtype)
            out["nconv"] = nconv
            out["status"] = SUCCESS if nconv == k else MAX_ITERATIONS_REACHED
            return out
        l_new = m if broke >= 0 else k + (ncv - k) // 2
        pick = order[:l_new]
        V[:, :l_new] = rotate(V[:, :m], y[:, pick].astype(a.dtype))
        if broke < 0:
            V[:, l_new] = V[:, m]
        kept = theta[pick].copy()
        arrow = np.zeros(l_new) if broke >= 0 else last * y[m - 1, pick]
        need_start = broke >= 0
        l = l_new
        out["restarts"] += 1


def rotate(V, Y):
    """the compression kernel: out[:, c] = V[:, 0] Y[0, c], then Y[j, c] V[:, j] + out[:, c] for j ascending, all in V's dtype"""
    out = np.empty((V.shape[0], Y.shape[1]), dtype=V.dtype)
    for c in range(Y.shape[1]):
        acc = Y[0, c] * V[:, 0]
        for j in range(1, V.shape[1]):
            acc = Y[j, c] * V[:, j] + acc
        out[:, c] = acc
    return out
