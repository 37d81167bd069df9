"""lobpcg, restated line by line in numpy: the locally optimal block preconditioned conjugate gradient method (Knyazev 2001) with the
SVQB orthonormalisation of the search block (Stathopoulos and Wu 2002), the definition csrc/smm_solvers_lobpcg.hip is compared with
(include/smm_hip.h states it in words).  Vectors and their sums are in the matrix's dtype; the small eigenproblems are fp64 for both
dtypes, as in the library -- which solves them by cyclic Jacobi where this file calls numpy.linalg.eigh: any accurate fp64 symmetric
solver is admissible there.  The sums are numpy's, not the kernels' partitioned ones: the comparison with the GPU is by bounds, not by
bits -- except block_axpy, whose fma chain has one order only."""
import numpy as np
from eigsh_restatement import hash_vector, rotate

LARGEST, SMALLEST = 0, 1
MAX_K, MAX_BASIS = 8, 24
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2


def gram(V, W):
    """multi_gram: G = V^T W, accumulated in the dtype of the columns (any summation order is admissible)"""
    return V.T @ W


def block_axpy(V, H, W):
    """multi_block_axpy: W[:, c] = W[:, c] - sum_j H[j][c] V[:, j], j ascending, one product and one sum per term (the a*x+b flavour of
    _smm_fma), all in the dtype of the columns; returns the new W"""
    out = W.copy()
    for c in range(W.shape[1]):
        acc = W[:, c].copy()
        for j in range(V.shape[1]):
            acc = (-H[j, c]) * V[:, j] + acc
        out[:, c] = acc
    return out


def start_block(n, k, seed, dtype):
    """the hash columns (seed, col = 0 .. k-1), as they are before the orthonormalisation: the X0 that gives the bits of X0 = None"""
    return np.stack([hash_vector(n, seed, col, dtype) for col in range(k)], axis=1)


def orthonormalise(X):
    """column by column: classical Gram-Schmidt twice against the columns before it, then a division by the norm (the shadow space of
    IDR(s) is made the same way).  None: a column whose norm is not finite, or whose norm after the two passes is at most sqrt(eps) of
    its norm before them -- the block has rank below k to working precision."""
    T = X.dtype.type
    root = T(np.sqrt(np.finfo(X.dtype).eps))
    X = X.copy()
    for j in range(X.shape[1]):
        w = X[:, j].copy()
        d0 = np.sqrt(T(np.dot(w, w)))
        for _ in range(2 if j else 0):
            h = X[:, :j].T @ w
            for i in range(j):
                w = (-h[i]) * X[:, i] + w
        d = np.sqrt(T(np.dot(w, w)))
        if not np.isfinite(d0) or not np.isfinite(d) or not (d > root * d0):
            return None
        X[:, j] = w / d
    return X


def _ritz(t, which):
    """the eigenpairs of the symmetrised fp64 matrix in the order of `which`; None: a value that is not finite"""
    t = 0.5 * (t + t.T)
    if not np.all(np.isfinite(t)):
        return None
    theta, c = np.linalg.eigh(t)
    if which == LARGEST:
        theta, c = theta[::-1], c[:, ::-1]
    return theta, c


def lobpcg(a, k, which, max_iterations=1000, tol=0.0, M=None, X0=None, seed=0):
    """a: a dense symmetric array whose dtype is the working precision; M: None or a function r -> M^-1 r on one column.  Returns a
    dict: status, w, X, residuals, nconv, iterations, matvecs, applies."""
    T = a.dtype.type
    n = a.shape[0]
    eps = float(np.finfo(a.dtype).eps)
    assert 1 <= k <= MAX_K and 3 * k <= n and which in (LARGEST, SMALLEST)
    bound = float(tol) if tol > 0 else eps
    out = dict(status=SUCCESS, w=None, X=None, residuals=None, nconv=0, iterations=0, matvecs=0, applies=0)

    def diverged():
        out["status"] = DIVERGED
        return out

    X = orthonormalise(np.asarray(X0, dtype=a.dtype)[:, :k] if X0 is not None else start_block(n, k, seed, a.dtype))
    if X is None:
        return diverged()
    AX = np.stack([a @ X[:, j] for j in range(k)], axis=1)
    out["matvecs"] = k
    r = _ritz(gram(X, AX).astype(np.float64), which)
    if r is None:
        return diverged()
    theta, C = r
    X, AX = rotate(X, C.astype(a.dtype)), rotate(AX, C.astype(a.dtype))
    P = np.zeros((n, 0), dtype=a.dtype)
    AP = np.zeros((n, 0), dtype=a.dtype)
    scale = 0.0
    it = 0
    while True:
        th = theta[:k].astype(a.dtype)
        R = AX - X * th  # one product and one difference per element
        rn = np.array([np.sqrt(T(np.dot(R[:, j], R[:, j]))) for j in range(k)], dtype=a.dtype)
        if not np.all(np.isfinite(rn)) or not np.all(np.isfinite(theta)):
            return diverged()
        scale = max(scale, float(np.max(np.abs(theta))))  # every Ritz value of the last Rayleigh-Ritz step, not the k wanted ones only
        active = [j for j in range(k) if not (float(rn[j]) <= bound * scale)]
        out.update(w=th, X=X, residuals=rn, nconv=k - len(active), iterations=it)
        if not active:
            return out
        if it == max_iterations:
            out["status"] = MAX_ITERATIONS_REACHED
            return out
        W = np.stack([R[:, j] if M is None else np.asarray(M(R[:, j]), dtype=a.dtype) for j in active], axis=1)
        AW = np.stack([a @ W[:, c] for c in range(len(active))], axis=1)
        out["matvecs"] += len(active)
        out["applies"] += len(active) if M is not None else 0
        Z, AZ = np.hstack([P, W]), np.hstack([AP, AW])  # in the order of the memory: the kept directions first
        for _ in range(2):
            H = gram(X, Z)
            Z, AZ = block_axpy(X, H, Z), block_axpy(AX, H, AZ)
            G = gram(Z, Z).astype(np.float64)
            if not np.all(np.isfinite(G)):
                return diverged()
            G = 0.5 * (G + G.T)
            d = np.sqrt(np.diag(G))
            live = np.nonzero(d > 0)[0]
            if len(live) == 0:
                Z, AZ = Z[:, :0], AZ[:, :0]
                break
            w_, Q = np.linalg.eigh(G[np.ix_(live, live)] / np.outer(d[live], d[live]))
            keep = np.nonzero(w_ > len(live) * eps * np.max(w_))[0][::-1]  # the largest first
            Y = np.zeros((Z.shape[1], len(keep)))
            Y[live, :] = (Q[:, keep] / np.sqrt(w_[keep])) / d[live][:, None]
            Y = Y.astype(a.dtype)
            Z, AZ = rotate(Z, Y), rotate(AZ, Y)
        nz = Z.shape[1]
        S, AS = np.hstack([X, Z]), np.hstack([AX, AZ])
        r = _ritz(gram(S, AS).astype(np.float64), which)
        if r is None:
            return diverged()
        theta, C = r
        take = active[: min(len(active), nz)]
        CP = np.zeros((k + nz, len(take)))
        CP[k:, :] = C[k:, take]  # the part of the step that lies in Z
        Y = np.hstack([C[:, :k], CP]).astype(a.dtype)
        S, AS = rotate(S, Y), rotate(AS, Y)
        X, P = S[:, :k], S[:, k:]
        AX, AP = AS[:, :k], AS[:, k:]
        it += 1
