"""svds, restated line by line in numpy: thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005, restarted with
Ritz vectors) with full reorthogonalisation of both bases, the definition csrc/smm_solvers_svds.hip is compared with (include/smm_hip.h
states it in words).  Vectors and their sums are in the matrix's dtype; the small SVD is fp64 for both dtypes, as in the library --
which computes it by one-sided Jacobi where this file calls numpy.linalg.svd: any accurate fp64 SVD is admissible there, and nothing
downstream of it is compared bit for bit.  The sums are numpy's, not the kernels' partitioned ones: the comparison with the GPU is by
bounds, not by bits.

The entries of the projected matrix B are the recurrence's: alpha_j and beta_j are the NORMS left by the two Gram-Schmidt passes, and the
arrow is s_i = beta_{m-1} X[m-1][i] of the restart.  No Gram-Schmidt product (h, g) enters B; they serve orthogonality only."""
import numpy as np
from eigsh_restatement import hash_vector, rotate

MAX_NCV = 64
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
NONE, ALPHA, BETA = "none", "alpha", "beta"  # how a cycle ended


def resolve_ncv(rows, cols, k, ncv):
    return min(rows, cols, max(2 * k + 1, 20)) if not ncv else ncv


def _rotate(Q, Y):
    return rotate(Q, Y) if Y.shape[1] else np.zeros((Q.shape[0], 0), dtype=Q.dtype)


def svds(a, k, ncv=0, max_restarts=100, tol=0.0, v0=None, seed=0, history=None):
    """a: a dense rows x cols array whose dtype is the working precision.  Returns a dict: status, s, U, V, residuals, nconv, restarts,
    matvecs.  history, when a list, receives (m, l, how the cycle ended) per cycle."""
    T = a.dtype.type
    rows, cols = a.shape
    at = np.ascontiguousarray(a.T)
    eps = float(np.finfo(a.dtype).eps)
    ncv = resolve_ncv(rows, cols, k, ncv)
    assert k >= 1 and k + 2 <= ncv <= min(rows, cols, MAX_NCV)
    bound = float(tol) if tol > 0 else eps
    V = np.zeros((cols, ncv + 1), dtype=a.dtype)
    U = np.zeros((rows, ncv), dtype=a.dtype)
    out = dict(status=SUCCESS, s=None, U=None, V=None, residuals=None, nconv=0, restarts=0, matvecs=0)

    def orthogonalise(Q, n, w):
        """w against the first n columns of Q, classical Gram-Schmidt twice; returns w and w . w"""
        for _ in range(2):
            h = Q[:, :n].T @ w
            for i in range(n):  # i ascending, one product and one sum each
                w = (-h[i]) * Q[:, i] + w
        return w, T(np.dot(w, w))

    l, fresh, need_start = 0, 0, True
    kept = np.zeros(0)
    arrow = np.zeros(0)
    scale = T(0)
    while True:
        if len(kept):
            scale = max(scale, T(np.max(kept)))
        bad = False
        if need_start:
            if l == 0 and v0 is not None:
                V[:, 0] = np.asarray(v0, dtype=a.dtype)
                ww = T(np.dot(V[:, 0], V[:, 0]))
            else:
                w = hash_vector(cols, seed, fresh, a.dtype)
                fresh += 1
                V[:, l], ww = (w, T(np.dot(w, w))) if l == 0 else orthogonalise(V, l, w)
            d = np.sqrt(ww)
            if not (d > 0) or not np.isfinite(d):
                bad = True
            else:
                V[:, l] = V[:, l] / d
            need_start = False
        alpha = np.zeros(ncv, dtype=a.dtype)
        beta = np.zeros(ncv, dtype=a.dtype)
        broke, how = -1, NONE
        for j in range(l, ncv):
            if bad:
                break
            w, ww = orthogonalise(U, j, a @ V[:, j])
            out["matvecs"] += 1
            alpha[j] = np.sqrt(ww)
            if not np.isfinite(alpha[j]):
                bad = True
                break
            scale = max(scale, alpha[j])
            if alpha[j] <= T(eps) * scale:  # u_j is not formed, nothing divides by this alpha
                broke, how = j, ALPHA
                break
            U[:, j] = w / alpha[j]
            w, ww = orthogonalise(V, j + 1, at @ U[:, j])
            out["matvecs"] += 1
            beta[j] = np.sqrt(ww)
            if not np.isfinite(beta[j]):
                bad = True
                break
            scale = max(scale, beta[j])
            if beta[j] <= T(eps) * scale:  # v_{j+1} is not formed, nothing divides by this beta
                broke, how = j, BETA
                break
            V[:, j + 1] = w / beta[j]
        if bad:
            out["status"] = DIVERGED
            return out
        # m triplets from U[:, :m] and V[:, :mv]
        m = {NONE: ncv, BETA: broke + 1, ALPHA: broke}[how]
        mv = m + 1 if how == ALPHA else m
        b = np.zeros((m, mv))
        for i in range(min(l, m)):
            b[i, i] = kept[i]
            b[i, l] = arrow[i]  # (l < mv: column l is v_l's, which every cycle has)
        for j in range(l, m):
            b[j, j] = float(alpha[j])
            if j + 1 < mv:
                b[j, j + 1] = float(beta[j])
        if not np.all(np.isfinite(b)):
            out["status"] = DIVERGED
            return out
        if m:
            x, sigma, yh = np.linalg.svd(b, full_matrices=False)  # descending; x is m x m, y is mv x m
            y = yh.T
        else:
            x, sigma, y = np.zeros((0, 0)), np.zeros(0), np.zeros((mv, 0))
        last = float(beta[m - 1]) if how == NONE else 0.0
        sigma0 = float(sigma[0]) if m else 0.0
        rho = np.abs(last * x[m - 1, :]) if m else np.zeros(0)
        have = min(k, m)
        nconv = int(np.sum(rho[:have] <= bound * sigma0))
        if history is not None:
            history.append((m, l, how))
        if nconv == k or (how != NONE and m >= k) or out["restarts"] >= max_restarts:
            out["s"] = sigma[:have].astype(a.dtype)
            out["U"] = _rotate(U[:, :m], x[:, :have].astype(a.dtype))
            out["V"] = _rotate(V[:, :mv], y[:, :have].astype(a.dtype))
            out["residuals"] = rho[:have].astype(a.dtype)
            out["nconv"] = nconv
            out["status"] = SUCCESS if nconv == k else MAX_ITERATIONS_REACHED
            return out
        l_new = m if how != NONE else k + (ncv - k) // 2
        if l_new:
            U[:, :l_new] = _rotate(U[:, :m], x[:, :l_new].astype(a.dtype))
            V[:, :l_new] = _rotate(V[:, :mv], y[:, :l_new].astype(a.dtype))
        if how == NONE:
            V[:, l_new] = V[:, m]
        kept = sigma[:l_new].copy()
        arrow = last * x[m - 1, :l_new] if how == NONE else np.zeros(l_new)
        need_start = how != NONE
        l = l_new
        out["restarts"] += 1
