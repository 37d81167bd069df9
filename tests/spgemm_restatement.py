"""The sparse product C = A B as include/smm_hip.h defines it, stated on the CPU in NumPy, in the matrix dtype.

A helper, not a test: this is the definition the device kernels (csrc/smm_spgemm.hip) are compared with.  The product is an addition of
this project (the reference multiplies a matrix by a vector only), so there are no goldens.

Pattern: (i, j) is stored iff some p has (i, p) stored in A and (p, j) stored in B; rows ascend, columns ascend inside a row; nothing is
dropped by value.  Values: c = +0.0, then for the stored entries (i, p) of A's row i IN STORED ORDER that have (p, j) in B:
c = _fma(a_ip, b_pj, c), with _fma = a * x + b (two roundings, ref:28-36).  The SMM_WITH_STD_FMA flavour cannot be reproduced bit for bit
in NumPy: compare that flavour with `bound`.

Vectorised: the scalar products are expanded as (i, rank of p inside row i, j); the products of ONE rank fall on distinct entries of C
(one p per row and rank, and the columns of a row of B are distinct), so the sums are formed rank by rank with plain fancy indexing."""
import numpy as np


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def expand(a_csr, b_csr):
    """every scalar product of A B: (row i, rank of the A entry inside its row, index of the A entry, index of the B entry)"""
    sa, pa, _ = a_csr
    sb, _, _ = b_csr
    m = len(sa) - 1
    nnz_a = int(sa[m])
    sa = np.asarray(sa, dtype=np.int64)
    sb = np.asarray(sb, dtype=np.int64)
    row_of = np.repeat(np.arange(m, dtype=np.int64), np.diff(sa))
    rank_of = np.arange(nnz_a, dtype=np.int64) - sa[row_of]
    p = np.asarray(pa[:nnz_a], dtype=np.int64)
    len_b = sb[p + 1] - sb[p]
    ent = np.repeat(np.arange(nnz_a, dtype=np.int64), len_b)
    first = np.cumsum(len_b) - len_b
    q = sb[p[ent]] + (np.arange(int(len_b.sum()), dtype=np.int64) - first[ent])
    return row_of[ent], rank_of[ent], ent, q


def spgemm(a_csr, b_csr, n):
    """(start, positions, values) of A B; B has n columns"""
    _, _, va = a_csr
    _, pb, vb = b_csr
    m = len(a_csr[0]) - 1
    dtype = va.dtype
    i, rank, ent, q = expand(a_csr, b_csr)
    j = np.asarray(pb, dtype=np.int64)[q]
    keys, slot = np.unique(i * max(n, 1) + j, return_inverse=True)
    start = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(keys // max(n, 1), minlength=m), out=start[1:])
    positions = (keys % max(n, 1)).astype(np.int32)
    values = np.zeros(len(keys), dtype=dtype)
    order = np.argsort(rank, kind="stable")
    cuts = np.searchsorted(rank[order], np.arange((int(rank.max()) if len(rank) else -1) + 2))
    with np.errstate(all="ignore"):
        for t in range(len(cuts) - 1):
            sel = order[cuts[t]:cuts[t + 1]]
            where = slot[sel]
            values[where] = _fma(va[ent[sel]], vb[q[sel]], values[where])
    return start, positions, values


def bound(a_csr, b_csr, n, dtype=None):
    """per stored entry of A B: terms * eps * sum |a_ip| |b_pj|.  A recursive sum of `terms` products, each step rounding at most twice
    (a * x + b) or once (fma), is off the exact sum by at most gamma_terms * sum |a||b|, gamma_k = k u / (1 - k u), u = eps / 2 (Higham,
    Accuracy and Stability of Numerical Algorithms, section 3.1: every product passes through at most `terms` roundings); two such
    evaluations -- another order, the other flavour, or float64 against the dtype -- differ by at most twice that, terms * eps *
    sum |a||b| to first order."""
    _, _, va = a_csr
    _, pb, vb = b_csr
    dtype = np.dtype(dtype or va.dtype)
    i, _, ent, q = expand(a_csr, b_csr)
    j = np.asarray(pb, dtype=np.int64)[q]
    keys, slot = np.unique(i * max(n, 1) + j, return_inverse=True)
    terms = np.bincount(slot, minlength=len(keys))
    mass = np.bincount(slot, weights=np.abs(va[ent].astype(np.float64)) * np.abs(vb[q].astype(np.float64)), minlength=len(keys))
    return terms * float(np.finfo(dtype).eps) * mass


def dense(csr, n):
    """the dense form of a CSR triple, in its dtype"""
    start, pos, val = csr
    m = len(start) - 1
    out = np.zeros((m, n), dtype=val.dtype)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(start, dtype=np.int64)))
    out[rows, pos[:len(rows)]] = val[:len(rows)]
    return out
