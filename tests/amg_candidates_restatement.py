"""SMM_PRECOND_AMG created with near-null-space candidates (smm_hip_precond_create_amg_candidates_*), stated on the CPU in NumPy.

A helper, not a test: the definition csrc/smm_precond_amg.hip is compared with (include/smm_hip.h states it in words).  Everything the
two ways of creating the kind share -- strength, roots, aggregates, S, the products, the smoother, the coarse inverse, the cycle -- is
tests/amg_restatement.py's, unchanged.  What is stated here, per level l with block size b_l (dofs_per_node on level 0, k below):

  node graph   b_l > 1: N = Tb^T ((A o A) Tb), Tb the n x n / b_l matrix with one 1 per row at column i // b_l, both products
               spgemm_restatement.spgemm, the transpose stable; then every value's square root.  N_IJ is the Frobenius norm of block
               (I, J) of A.  Strength, roots and aggregates run on N with N's own diagonal; dof i takes aggregate agg[i // b_l].
  QR           the member dofs of aggregate a in ascending order are its rows 0 .. m - 1; V = their rows of B_l (m x k).  EVERY inner
               product of two columns x, y is wave_dot(x, y): lane t = rank mod 64 sums the ranks t, t + 64, ... in ascending order
               from +0.0 with _fma, then the xor butterfly 32, 16, .. 1 -- a function of m alone.  Column by column, c ascending:
                 norm0 = sqrt(wave_dot(v_c, v_c))                     (before any orthogonalisation)
                 for j < c ascending:  r_jc = wave_dot(q_j, v_c);  if column j was kept: v_c = _fma(-r_jc, q_j, v_c)
                 nrm = sqrt(wave_dot(v_c, v_c))
                 kept iff nrm > DROP_TOL * norm0 (one product in T):  r_cc = nrm, q_c = v_c / nrm;  else q_c = 0, r_cc = 0, row c of R = 0
               (a dropped column's q is zero, so its r_jc are +0.0).  T (n x n_agg k) holds q_c of a row's aggregate at column a k + c for
               the KEPT c only, ascending; B_{l+1} (n_agg k x k) holds R at rows a k .. a k + k - 1.
  A_{l+1}      R (A P) + E, E the diagonal matrix with a stored 1 at every coarse dof whose column was dropped (add_restatement.add with
               alpha = beta = 1); no dropped column on the level: R (A P) itself.
  stall rule   10 n_agg k >= 9 n: the level is the coarsest."""
import numpy as np
from add_restatement import add
from amg_restatement import (COARSE_ROWS, DENSE_LIMIT, MAX_LEVELS, THETA, AmgRefused, aggregates, check_diagonal, roots, smoother_matrix, strength,
                             transpose)
from chebyshev_restatement import _fma, diagonal, gershgorin
from spgemm_restatement import spgemm

DROP_TOL = 2.0 ** -13  # SMM_AMG_DROP_TOL
LDS_ROWS = 256         # SMM_AMG_QR_LDS_ROWS: aggregates of more rows are orthogonalised in global memory (same bits)


def node_graph(csr, b):
    start, pos, val = csr
    n = len(start) - 1
    nodes = n // b
    with np.errstate(all="ignore"):
        squared = (start, pos, val * val)
    Tb = (np.arange(n + 1, dtype=np.int32), (np.arange(n, dtype=np.int32) // b).astype(np.int32), np.ones(n, dtype=val.dtype))
    N = spgemm(transpose(Tb, nodes), spgemm(squared, Tb, nodes), nodes)
    with np.errstate(all="ignore"):
        return N[0], N[1], np.sqrt(N[2])


def wave_dot(x, y):
    acc = np.zeros(64, dtype=x.dtype)
    with np.errstate(all="ignore"):
        for r0 in range(0, len(x), 64):
            w = min(64, len(x) - r0)
            acc[:w] = _fma(x[r0:r0 + w], y[r0:r0 + w], acc[:w])
        lanes = np.arange(64)
        o = 32
        while o:
            acc = acc + acc[lanes ^ o]
            o >>= 1
    return acc[0]


def thin_qr(V):
    """(Q m x k with zero columns where dropped, R k x k, kept flags) of one aggregate's block"""
    T = V.dtype.type
    m, k = V.shape
    Q = np.zeros((m, k), dtype=V.dtype)
    R = np.zeros((k, k), dtype=V.dtype)
    kept = np.zeros(k, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(k):
            v = V[:, c].copy()
            norm0 = np.sqrt(wave_dot(v, v))
            for j in range(c):
                r = wave_dot(Q[:, j], v)
                if kept[j]:
                    R[j, c] = r
                    v = _fma(-r, Q[:, j], v)
            nrm = np.sqrt(wave_dot(v, v))
            if nrm > T(DROP_TOL) * norm0:
                kept[c] = True
                R[c, c] = nrm
                Q[:, c] = v / nrm
    return Q, R, kept


def tentative(agg, n_agg, B):
    """(T as a CSR triple, B_next, kept flags per coarse dof) from the dof aggregates and B_l (n x k)"""
    n, k = B.shape
    order = np.argsort(agg, kind="stable")
    bounds = np.searchsorted(agg[order], np.arange(n_agg + 1))
    B_next = np.zeros((n_agg * k, k), dtype=B.dtype)
    kept = np.zeros(n_agg * k, dtype=bool)
    Qrow = np.zeros((n, k), dtype=B.dtype)
    for a in range(n_agg):
        rows = order[bounds[a]:bounds[a + 1]]
        Q, R, keep = thin_qr(B[rows])
        Qrow[rows] = Q
        B_next[a * k:(a + 1) * k] = R
        kept[a * k:(a + 1) * k] = keep
    mask = kept.reshape(n_agg, k)[agg]  # [dof][c]
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(mask.sum(axis=1), out=start[1:])
    cols = (agg.astype(np.int64)[:, None] * k + np.arange(k)[None, :])
    return (start, cols[mask].astype(np.int32), Qrow[mask]), B_next, kept


def identity_rows(kept, dtype):
    dropped = ~kept
    start = np.zeros(len(kept) + 1, dtype=np.int32)
    np.cumsum(dropped, out=start[1:])
    return start, np.flatnonzero(dropped).astype(np.int32), np.ones(int(dropped.sum()), dtype=dtype)


def products(csr, lv):
    """P, R, A P and A_next of a level whose T is known (lv: diag, lam, T, kept, n_c)"""
    n_c = lv["n_c"]
    S = smoother_matrix(csr, lv["diag"], lv["lam"])
    P = spgemm(S, lv["T"], n_c)
    R = transpose(P, n_c)
    AP = spgemm(csr, P, n_c)
    A_next = spgemm(R, AP, n_c)
    if not lv["kept"].all():
        A_next = add(A_next, 1.0, identity_rows(lv["kept"], csr[2].dtype), 1.0, n_c)
    return P, R, AP, A_next


def hierarchy(csr, B, dofs_per_node=1, theta=THETA, max_levels=MAX_LEVELS, coarse_rows=COARSE_ROWS, keep=None):
    """the levels: dicts {A, diag, lam, B[, N, agg, n_agg, n_c, T, kept, dropped, P, R, AP]}; the last one has no P.  keep: the levels of an
    earlier hierarchy whose aggregates, T and B_l are kept (smm_hip_precond_amg_refresh)"""
    dtype = csr[2].dtype
    B = np.asarray(B, dtype=dtype).reshape(len(csr[0]) - 1, -1)
    k = B.shape[1]
    levels = []
    A = csr
    while True:
        l = len(levels)
        n = len(A[0]) - 1
        lv = {"A": A, "diag": check_diagonal(A), "lam": gershgorin(A) if n else 1.0, "B": B, "dropped": 0}
        levels.append(lv)
        if n <= coarse_rows or l + 1 == max_levels or (keep is not None and "P" not in keep[l]):
            break
        b = dofs_per_node if l == 0 else k
        if keep is not None:
            for key in ("agg", "n_agg", "n_c", "T", "kept", "dropped"):
                lv[key] = keep[l][key]
            B_next = keep[l + 1]["B"]
        else:
            G = node_graph(A, b) if b > 1 else A
            d = diagonal(G) if b > 1 else lv["diag"]
            strong = strength(G, d, theta * 0.5 ** l)
            state, _ = roots(G, strong)
            node_agg, n_agg, _, _ = aggregates(G, strong, state)
            lv.update(N=G, node_agg=node_agg, agg=np.repeat(node_agg, b).astype(np.int32), n_agg=n_agg, n_c=n_agg * k)
            if 10 * lv["n_c"] >= 9 * n:
                for key in ("N", "node_agg", "agg", "n_agg", "n_c"):
                    lv.pop(key)
                break
            lv["T"], B_next, lv["kept"] = tentative(lv["agg"], n_agg, B)
            lv["dropped"] = int((~lv["kept"]).sum())
        lv["P"], lv["R"], lv["AP"], A = products(A, lv)
        B = B_next
    sizes = [len(v["A"][0]) - 1 for v in levels]
    if sizes[-1] > DENSE_LIMIT:
        raise AmgRefused(f"the coarsest level has {sizes[-1]} rows: {sizes}")
    return levels
