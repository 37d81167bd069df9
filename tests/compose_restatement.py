"""The four compose operations of csrc/smm_compose.hip restated in plain NumPy on CSR triples (start, positions, values), in the rounding
order include/smm_hip.h states (a helper, not a test).  tests/test_compose_cpu.py checks every function against dense NumPy -- np.block,
fancy indexing, np.diag, r[:, None] * A * c[None, :] --; the GPU tests compare the library with these functions bit for bit.

  bmat       entries of block (I, J) at (row offset of I + i, column offset of J + j); inside a row the segments in ascending block
             column; value = coef * v in the dtype (one rounding), coef == 1 copies the bits; nothing is dropped by value.
  submatrix  row i is the source's row rows[i] restricted to the strictly ascending columns cols, renumbered; values bit for bit; also
             returns map[k] = the source index of output entry k.
  diagonal   out[i] = a_ii for i < min(rows, cols), 0 where none is stored, and the number of those.
  scale_rows_cols  v_ij <- (r_i * v_ij) * c_j, two roundings in this order; a vector that is None skips its factor."""
import numpy as np


class Invalid(ValueError):
    """what the library answers SMM_HIP_ERR_INVALID to"""


def row_of_entries(start):
    return np.repeat(np.arange(len(start) - 1, dtype=np.int64), np.diff(start))


def dense(csr, shape):
    """the dense matrix of a triple with distinct columns per row (a stored zero is a zero)"""
    start, pos, val = csr
    d = np.zeros(shape, dtype=val.dtype)
    d[row_of_entries(start), pos] = val
    return d


def stored(csr, shape):
    """the boolean matrix of the stored entries"""
    start, pos, _ = csr
    m = np.zeros(shape, dtype=bool)
    m[row_of_entries(start), pos] = True
    return m


def block_sizes(blocks, shapes, row_sizes=None, col_sizes=None):
    """(heights, widths) of a p x q table: blocks[I][J] is a triple or None, shapes[I][J] its (rows, cols) or None"""
    p, q = len(blocks), len(blocks[0])
    h, w = [-1] * p, [-1] * q
    for i in range(p):
        for j in range(q):
            if blocks[i][j] is None:
                continue
            m, n = shapes[i][j]
            if (h[i] >= 0 and h[i] != m) or (w[j] >= 0 and w[j] != n):
                raise Invalid(f"block ({i}, {j}) is {m} x {n}")
            h[i], w[j] = m, n
    for sizes, given, what in ((h, row_sizes, "row"), (w, col_sizes, "column")):
        for k in range(len(sizes)):
            g = -1 if given is None or given[k] is None else int(given[k])
            if sizes[k] >= 0 and g >= 0 and g != sizes[k]:
                raise Invalid(f"block {what} {k}: {g} given, the blocks have {sizes[k]}")
            if sizes[k] < 0:
                sizes[k] = g
            if sizes[k] < 0:
                raise Invalid(f"block {what} {k} has no size")
    return h, w


def bmat(blocks, shapes, dtype, coef=None, row_sizes=None, col_sizes=None):
    """-> ((start, positions, values), (rows, cols))"""
    dtype = np.dtype(dtype)
    p, q = len(blocks), len(blocks[0])
    if p * q > 64:
        raise Invalid("more than 64 slots")
    for i in range(p):
        for j in range(q):
            if blocks[i][j] is not None and blocks[i][j][2].dtype != dtype:
                raise Invalid(f"block ({i}, {j}) holds the other element type")
    h, w = block_sizes(blocks, shapes, row_sizes, col_sizes)
    rows, cols = sum(h), sum(w)
    col_off = np.concatenate([[0], np.cumsum(w)]).astype(np.int64)
    nnz = sum(len(b[1]) for r in blocks for b in r if b is not None)
    if max(rows, cols, nnz) > 2**31 - 1:
        raise Invalid("beyond 2^31 - 1")
    coef = None if coef is None else np.asarray(coef, dtype=dtype).reshape(p, q)
    start = [0]
    pos_parts, val_parts = [], []
    for i in range(p):
        for lr in range(h[i]):
            n = 0
            for j in range(q):
                b = blocks[i][j]
                if b is None:
                    continue
                s0, s1 = int(b[0][lr]), int(b[0][lr + 1])
                pos_parts.append(b[1][s0:s1].astype(np.int64) + col_off[j])
                v = b[2][s0:s1]
                if coef is not None and coef[i, j] != 1:
                    v = (coef[i, j] * v).astype(dtype)  # one product in the dtype: one rounding
                val_parts.append(v)
                n += s1 - s0
            start.append(start[-1] + n)
    pos = np.concatenate(pos_parts + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    val = np.concatenate(val_parts + [np.zeros(0, dtype=dtype)]).astype(dtype)
    return (np.asarray(start, dtype=np.int32), pos, val), (rows, cols)


def check_indices(rows, nrows, cols, ncols):
    """raises Invalid naming the first offending position, as the library's error text does"""
    if rows is not None:
        bad = np.flatnonzero((np.asarray(rows) < 0) | (np.asarray(rows) >= nrows))
        if len(bad):
            raise Invalid(f"rows_idx[{bad[0]}]")
    if cols is not None:
        c = np.asarray(cols, dtype=np.int64)
        wrong = (c < 0) | (c >= ncols)
        wrong[1:] |= c[1:] <= c[:-1]
        bad = np.flatnonzero(wrong)
        if len(bad):
            raise Invalid(f"cols_idx[{bad[0]}]")


def submatrix(csr, shape, rows=None, cols=None):
    """-> ((start, positions, values), (nr, nc), map); rows / cols None = all"""
    start, pos, val = csr
    check_indices(rows, shape[0], cols, shape[1])
    rows = np.arange(shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(shape[1]) if cols is None else np.asarray(cols, dtype=np.int64)
    col_map = np.full(shape[1], -1, dtype=np.int64)
    col_map[cols] = np.arange(len(cols))
    out_start = [0]
    src = []
    for r in rows:
        idx = np.arange(start[r], start[r + 1], dtype=np.int64)
        idx = idx[col_map[pos[idx]] >= 0]
        src.append(idx)
        out_start.append(out_start[-1] + len(idx))
    src = np.concatenate(src + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return (np.asarray(out_start, dtype=np.int32), col_map[pos[src]].astype(np.int32), val[src].copy()), (len(rows), len(cols)), src.astype(np.int32)


def diagonal(csr, shape):
    """-> (d[min(rows, cols)], the number of diagonal entries not stored)"""
    start, pos, val = csr
    n = min(shape)
    d = np.zeros(n, dtype=val.dtype)
    missing = 0
    for i in range(n):
        k = np.flatnonzero(pos[start[i]:start[i + 1]] == i)
        if len(k):
            d[i] = val[start[i] + k[0]]
        else:
            missing += 1
    return d, missing


def scale_rows_cols(csr, r=None, c=None):
    """-> the values after v <- (r_i v) c_j, each product rounded in the dtype"""
    start, pos, val = csr
    out = val.copy()
    if r is not None:
        out = (np.asarray(r, dtype=val.dtype)[row_of_entries(start)] * out).astype(val.dtype)
    if c is not None:
        out = (out * np.asarray(c, dtype=val.dtype)[pos]).astype(val.dtype)
    return out
