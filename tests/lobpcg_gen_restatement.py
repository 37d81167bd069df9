"""lobpcg for the generalised problem A x = lambda B x, restated line by line in numpy: the loop of tests/lobpcg_restatement.py with a
third basis BS = [BX BP BW] carried beside S and AS, the orthonormality taken in B's inner product and the residual
R_j = AX_j - theta_j BX_j tested against ||BX_j|| -- the definition the generalised loop of csrc/smm_solvers_lobpcg.hip is compared
with (include/smm_hip.h states it in words).  S is B-orthonormal after the two SVQB passes, so the small problem stays the standard
one on T = S^T AS.  Precision and the comparison with the GPU are as in lobpcg_restatement: by bounds, not by bits."""
import lobpcg_restatement as standard
import numpy as np
from eigsh_restatement import hash_vector, rotate  # noqa: F401  (hash_vector: the start block's columns, through start_block)
from lobpcg_restatement import DIVERGED, LARGEST, MAX_ITERATIONS_REACHED, MAX_K, SMALLEST, SUCCESS, _ritz, block_axpy, gram, start_block


def b_orthonormalise(X, b):
    """column by column: q = B w, d0 = sqrt(w . q); classical Gram-Schmidt twice against the columns before it with the products taken
    against BX; q = B w again, d = sqrt(w . q); X_j = w / d, BX_j = q / d.  Returns (X, BX, products with B), or None: a d0 or d that
    is not finite (the root of a negative w . q is one), or !(d > sqrt(eps) d0)."""
    T = X.dtype.type
    root = T(np.sqrt(np.finfo(X.dtype).eps))
    X = X.copy()
    BX = np.zeros_like(X)
    products = 0
    with np.errstate(invalid="ignore"):
        for j in range(X.shape[1]):
            w = X[:, j].copy()
            q = b @ w
            products += 1
            d0 = np.sqrt(T(np.dot(w, q)))
            for _ in range(2 if j else 0):
                h = BX[:, :j].T @ w
                for i in range(j):
                    w = (-h[i]) * X[:, i] + w
            if j:
                q = b @ w
                products += 1
            d = np.sqrt(T(np.dot(w, q)))
            if not np.isfinite(d0) or not np.isfinite(d) or not (d > root * d0):
                return None
            X[:, j] = w / d
            BX[:, j] = q / d
    return X, BX, products


def lobpcg(a, k, which, max_iterations=1000, tol=0.0, M=None, X0=None, seed=0, B=None, history=None):
    """a, B: dense symmetric arrays of the working precision, B positive definite (None: the standard problem, handed to
    lobpcg_restatement.lobpcg); M: None or a function r -> M^-1 r on one column, an approximation of A^-1.  Returns lobpcg_restatement's
    dict and bmatvecs.  history, when a list, receives |active| per iteration."""
    if B is None:
        out = standard.lobpcg(a, k, which, max_iterations, tol, M, X0, seed)
        out["bmatvecs"] = 0
        return out
    T = a.dtype.type
    n = a.shape[0]
    b = np.asarray(B, dtype=a.dtype)
    eps = float(np.finfo(a.dtype).eps)
    assert 1 <= k <= MAX_K and 3 * k <= n and which in (LARGEST, SMALLEST) and b.shape == a.shape
    bound = float(tol) if tol > 0 else eps
    out = dict(status=SUCCESS, w=None, X=None, residuals=None, nconv=0, iterations=0, matvecs=0, applies=0, bmatvecs=0)

    def diverged():
        out["status"] = DIVERGED
        return out

    start = b_orthonormalise(np.asarray(X0, dtype=a.dtype)[:, :k] if X0 is not None else start_block(n, k, seed, a.dtype), b)
    if start is None:
        return diverged()
    X, BX, out["bmatvecs"] = start
    AX = np.stack([a @ X[:, j] for j in range(k)], axis=1)
    out["matvecs"] = k
    r = _ritz(gram(X, AX).astype(np.float64), which)
    if r is None:
        return diverged()
    theta, C = r
    C = C.astype(a.dtype)
    X, AX, BX = rotate(X, C), rotate(AX, C), rotate(BX, C)
    P, AP, BP = (np.zeros((n, 0), dtype=a.dtype) for _ in range(3))
    scale = 0.0
    it = 0
    while True:
        th = theta[:k].astype(a.dtype)
        R = AX - BX * th  # one product and one difference per element
        rn = np.array([np.sqrt(T(np.dot(R[:, j], R[:, j]))) for j in range(k)], dtype=a.dtype)
        bn = np.array([np.sqrt(T(np.dot(BX[:, j], BX[:, j]))) for j in range(k)], dtype=a.dtype)
        if not np.all(np.isfinite(rn)) or not np.all(np.isfinite(bn)) or not np.all(bn > 0) or not np.all(np.isfinite(theta)):
            return diverged()
        scale = max(scale, float(np.max(np.abs(theta))))
        active = [j for j in range(k) if not (float(rn[j]) <= bound * scale * float(bn[j]))]
        out.update(w=th, X=X, residuals=rn, nconv=k - len(active), iterations=it)
        if not active:
            return out
        if it == max_iterations:
            out["status"] = MAX_ITERATIONS_REACHED
            return out
        if history is not None:
            history.append(len(active))
        W = np.stack([R[:, j] if M is None else np.asarray(M(R[:, j]), dtype=a.dtype) for j in active], axis=1)
        AW = np.stack([a @ W[:, c] for c in range(len(active))], axis=1)
        BW = np.stack([b @ W[:, c] for c in range(len(active))], axis=1)
        out["matvecs"] += len(active)
        out["bmatvecs"] += len(active)
        out["applies"] += len(active) if M is not None else 0
        Z, AZ, BZ = np.hstack([P, W]), np.hstack([AP, AW]), np.hstack([BP, BW])
        for _ in range(2):
            H = gram(BX, Z)
            Z, AZ, BZ = block_axpy(X, H, Z), block_axpy(AX, H, AZ), block_axpy(BX, H, BZ)
            G = gram(Z, BZ).astype(np.float64)
            if not np.all(np.isfinite(G)):
                return diverged()
            G = 0.5 * (G + G.T)
            with np.errstate(invalid="ignore"):
                d = np.sqrt(np.diag(G))
            live = np.nonzero(d > 0)[0]
            if len(live) == 0:
                Z, AZ, BZ = Z[:, :0], AZ[:, :0], BZ[:, :0]
                break
            w_, Q = np.linalg.eigh(G[np.ix_(live, live)] / np.outer(d[live], d[live]))
            keep = np.nonzero(w_ > len(live) * eps * np.max(w_))[0][::-1]  # the largest first
            Y = np.zeros((Z.shape[1], len(keep)))
            Y[live, :] = (Q[:, keep] / np.sqrt(w_[keep])) / d[live][:, None]
            Y = Y.astype(a.dtype)
            Z, AZ, BZ = rotate(Z, Y), rotate(AZ, Y), rotate(BZ, Y)
        nz = Z.shape[1]
        S, AS, BS = np.hstack([X, Z]), np.hstack([AX, AZ]), np.hstack([BX, BZ])
        r = _ritz(gram(S, AS).astype(np.float64), which)
        if r is None:
            return diverged()
        theta, C = r
        take = active[: min(len(active), nz)]
        CP = np.zeros((k + nz, len(take)))
        CP[k:, :] = C[k:, take]  # the part of the step that lies in Z
        Y = np.hstack([C[:, :k], CP]).astype(a.dtype)
        S, AS, BS = rotate(S, Y), rotate(AS, Y), rotate(BS, Y)
        X, P = S[:, :k], S[:, k:]
        AX, AP = AS[:, :k], AS[:, k:]
        BX, BP = BS[:, :k], BS[:, k:]
        it += 1
