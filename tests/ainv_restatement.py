"""The approximate-inverse preconditioners FSAI and SPAI (SMM_PRECOND_FSAI / SMM_PRECOND_SPAI), stated on the CPU in NumPy.

A helper, not a test: this is the definition csrc/smm_precond_ainv.hip is compared with (include/smm_hip.h states it in words).  The
kinds are additions of this project (the reference has nothing like them), so there are no goldens and no quirks to preserve.

  pattern   Pat = a (power 1) or the structural product of `power` copies of a; J_i = the distinct columns of row i of Pat, ascending;
            FSAI keeps the columns <= i.
  source    look(X, r, c) = the first stored entry of row r of X with column c, +0.0 when there is none.
            FSAI: Src = a, b = e_{n-1}.  SPAI: At = transpose(a), Src = N = a At (tests/spgemm_restatement.py), b[p] = look(At, i, J[p]).
            S[p][q] = look(Src, J[p], J[q]) for q <= p; the upper triangle is never read.
  solve     the three loops of `solve_systems`, every operation rounding once in the matrix dtype, s - l m as _smm_fma(-l, m, s).
  result    FSAI: row i of G = y / sqrt(y[n-1]); SPAI: row i of M = y; both on the columns J_i.
  apply     FSAI: w = G r, z = Gt w; SPAI: z = M r -- oracle.spmv with OP_ASSIGN.

The systems of all rows are solved side by side: padded to the longest one with rows of the identity (a padded entry contributes
t = -0 * x and s + t = s bit for bit), each step of the loops is then one element-wise NumPy operation over all rows, which rounds
exactly like the scalar loop.  With the SMM_WITH_STD_FMA flavour these lines cannot be reproduced in NumPy: compare it by tolerance."""
import numpy as np
from bicg_restatement import transpose
from spgemm_restatement import spgemm

OP_ASSIGN = 0
FSAI, SPAI = 12, 13
MAX_ROW, MAX_POWER = 64, 4


class AinvError(Exception):
    """what the library answers with SMM_HIP_ERR_PRECOND; `row` is the row the message names, `length` the row length where it names one"""

    def __init__(self, what, row, length=None):
        super().__init__(f"{what}: row {row}" + (f" has {length} entries" if length is not None else ""))
        self.what, self.row, self.length = what, row, length


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def row_sets(csr):
    """the distinct columns of every row, ascending"""
    start, pos, _ = csr
    return [np.unique(pos[start[i]:start[i + 1]]) for i in range(len(start) - 1)]


def pattern(csr, kind, power):
    """J_i for every row; raises AinvError for a missing diagonal or a row longer than MAX_ROW (the smallest such row)"""
    assert kind in (FSAI, SPAI) and 1 <= power <= MAX_POWER
    base = row_sets(csr)
    rows = base
    for _ in range(power - 1):  # the structural product with one more copy of a
        rows = [np.unique(np.concatenate([base[c] for c in r])) if len(r) else r for r in rows]
    if kind == FSAI:
        rows = [r[r <= i] for i, r in enumerate(rows)]
    for i, r in enumerate(rows):
        if i not in r:
            raise AinvError("missing diagonal", i)
        if len(r) > MAX_ROW:
            raise AinvError("row too long", i, len(r))
    return rows


def look_table(csr):
    """{(r, c): index of the first stored entry of row r with column c}"""
    start, pos, _ = csr
    table = {}
    for r in range(len(start) - 1):
        for k in range(start[r], start[r + 1]):
            table.setdefault((r, int(pos[k])), k)
    return table


def gather(csr, kind, J):
    """(S[rows][nmax][nmax] with the lower triangles filled and the identity in the padding, b[rows][nmax], n[rows])"""
    val = csr[2]
    dtype = val.dtype
    rows = len(J)
    n = np.array([len(j) for j in J], dtype=np.int64)
    nmax = int(n.max()) if rows else 0
    S = np.zeros((rows, nmax, nmax), dtype=dtype)
    S[:, np.arange(nmax), np.arange(nmax)] = 1
    b = np.zeros((rows, nmax), dtype=dtype)
    if kind == SPAI:
        at = transpose(csr)
        src = spgemm(csr, at, rows)
        at_table = look_table(at)
    else:
        src = csr
    table = look_table(src)
    for i, cols in enumerate(J):
        for p, r in enumerate(cols):
            for q in range(p + 1):
                k = table.get((int(r), int(cols[q])))
                S[i, p, q] = src[2][k] if k is not None else 0
        if kind == SPAI:
            for p, c in enumerate(cols):
                k = at_table.get((i, int(c)))
                b[i, p] = at[2][k] if k is not None else 0
        else:
            b[i, len(cols) - 1] = 1
    return S, b, n


def solve_systems(S, b, n):
    """the three loops for all rows at once; returns (y, failed[rows]).  S and b are overwritten."""
    rows, nmax = b.shape
    failed = np.zeros(rows, dtype=bool)
    y = np.zeros_like(b)
    with np.errstate(all="ignore"):
        for j in range(nmax):
            d = S[:, j, j]
            failed |= (j < n) & ~((d > 0) & np.isfinite(d))
            S[:, j, j] = np.sqrt(d)
            S[:, j + 1:, j] = S[:, j + 1:, j] / S[:, j, j][:, None]                       # i > j
            lcol = S[:, j + 1:, j]
            S[:, j + 1:, j + 1:] = _fma(-lcol[:, :, None], lcol[:, None, :], S[:, j + 1:, j + 1:])  # i > j, j < k <= i (k > i is never read)
        for j in range(nmax):
            y[:, j] = b[:, j] / S[:, j, j]
            b[:, j + 1:] = _fma(-S[:, j + 1:, j], y[:, j][:, None], b[:, j + 1:])         # i > j
        for j in range(nmax - 1, -1, -1):
            y[:, j] = y[:, j] / S[:, j, j]
            y[:, :j] = _fma(-S[:, j, :j], y[:, j][:, None], y[:, :j])                     # i < j
    return y, failed


def build(csr, kind, power=1):
    """G (FSAI) or M (SPAI) as (start, positions, values); raises AinvError as the library answers SMM_HIP_ERR_PRECOND"""
    dtype = csr[2].dtype
    J = pattern(csr, kind, power)
    rows = len(J)
    S, b, n = gather(csr, kind, J)
    y, failed = solve_systems(S, b, n)
    if failed.any():
        raise AinvError("failed row", int(np.nonzero(failed)[0][0]))
    start = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(n, out=start[1:])
    positions = np.concatenate(J).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    values = np.zeros(int(start[-1]), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(rows):
            row = y[i, :n[i]]
            values[start[i]:start[i + 1]] = row / np.sqrt(row[n[i] - 1]) if kind == FSAI else row
    return start, positions, values


def make_apply(oracle, csr, kind, power=1, built=None):
    """M^-1 as a function of one vector"""
    g = build(csr, kind, power) if built is None else built
    dtype = csr[2].dtype
    if kind == SPAI:
        return lambda r: oracle.spmv(g, OP_ASSIGN, None, np.ascontiguousarray(r, dtype=dtype))
    gt = transpose(g)
    return lambda r: oracle.spmv(gt, OP_ASSIGN, None, oracle.spmv(g, OP_ASSIGN, None, np.ascontiguousarray(r, dtype=dtype)))
