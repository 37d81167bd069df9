"""The sparse sum C = alpha A + beta B as include/smm_hip.h defines it, stated on the CPU in NumPy, in the matrix dtype.

A helper, not a test: this is the definition the device kernels (csrc/smm_add.hip) are compared with.  The sum over two different
patterns is an addition of this project (the reference's inplaceAdd / inplaceSubtract need equal patterns), so there are no goldens.

Pattern: (i, j) is stored iff it is stored in A or in B; rows ascend, columns ascend strictly inside a row; nothing is dropped by value.
Values: u = alpha * a_ij (one rounding) where A stores (i, j), v = beta * b_ij (one rounding) where B stores it; c_ij = u + v (one more
rounding) where both do, u where only A does, v where only B does -- never u + 0, so a lone -0.0 keeps its sign.

Vectorised with np.unique over the keys row * cols + col of the concatenated entries, as spgemm_restatement.py does."""
import numpy as np


def _keys(csr, cols):
    start, pos, _ = csr
    start = np.asarray(start, dtype=np.int64)
    m = len(start) - 1
    nnz = int(start[m])
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(start))
    return rows * max(cols, 1) + np.asarray(pos[:nnz], dtype=np.int64)


def _scaled(scalar, csr):
    val = csr[2]
    nnz = int(csr[0][-1])
    with np.errstate(all="ignore"):
        return (val.dtype.type(scalar) * val[:nnz]).astype(val.dtype)


def _combine(slot_a, u, slot_b, v, n, dtype):
    """values on n slots: u where only A lands, v where only B lands, u + v where both do, +0.0 elsewhere"""
    values = np.zeros(n, dtype=dtype)
    has_a = np.zeros(n, dtype=bool)
    has_a[slot_a] = True
    values[slot_a] = u
    both = has_a[slot_b]
    with np.errstate(all="ignore"):
        values[slot_b[both]] = values[slot_b[both]] + v[both]
    values[slot_b[~both]] = v[~both]
    return values


def add(a_csr, alpha, b_csr, beta, cols):
    """(start, positions, values) of alpha A + beta B; both have `cols` columns"""
    m = len(a_csr[0]) - 1
    dtype = a_csr[2].dtype
    ka, kb = _keys(a_csr, cols), _keys(b_csr, cols)
    keys, slot = np.unique(np.concatenate([ka, kb]), return_inverse=True)
    slot = slot.reshape(-1)
    start = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(np.bincount(keys // max(cols, 1), minlength=m), out=start[1:])
    positions = (keys % max(cols, 1)).astype(np.int32)
    values = _combine(slot[:len(ka)], _scaled(alpha, a_csr), slot[len(ka):], _scaled(beta, b_csr), len(keys), dtype)
    return start, positions, values


def add_into(c_csr, a_csr, alpha, b_csr, beta, cols):
    """the values of alpha A + beta B on C's pattern (+0.0 where neither stores an entry); or, when an operand stores an entry C does not,
    the int number of the first such row"""
    dtype = a_csr[2].dtype
    kc = _keys(c_csr, cols)  # ascending: rows ascend, columns ascend inside a row
    ka, kb = _keys(a_csr, cols), _keys(b_csr, cols)
    slots = []
    missing = []
    for k in (ka, kb):
        s = np.searchsorted(kc, k)
        found = (s < len(kc)) & (kc[np.minimum(s, max(len(kc) - 1, 0))] == k) if len(kc) else np.zeros(len(k), dtype=bool)
        missing.append(k[~found] // max(cols, 1))
        slots.append(s)
    missing = np.concatenate(missing)
    if len(missing):
        return int(missing.min())
    return _combine(slots[0], _scaled(alpha, a_csr), slots[1], _scaled(beta, b_csr), len(kc), dtype)


def dense(csr, n):
    """the dense form of a CSR triple, in its dtype"""
    start, pos, val = csr
    m = len(start) - 1
    out = np.zeros((m, n), dtype=val.dtype)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(start, dtype=np.int64)))
    out[rows, pos[:len(rows)]] = val[:len(rows)]
    return out


def triplets(csr):
    """(rows, cols, values) of the stored entries, in stored order"""
    start, pos, val = csr
    nnz = int(start[-1])
    rows = np.repeat(np.arange(len(start) - 1, dtype=np.int32), np.diff(np.asarray(start, dtype=np.int64)))
    return rows, np.asarray(pos[:nnz], dtype=np.int32), np.asarray(val[:nnz])
