"""The aggregation multigrid preconditioner (SMM_PRECOND_AMG), stated on the CPU in NumPy.

A helper, not a test: this is the definition csrc/smm_precond_amg.hip is compared with (include/smm_hip.h states it in words).  The kind is
an addition of this project, so there are no goldens.  Integer results (strength, roots, aggregates, every pattern) are exact; the values of
S = I - omega D^-1 A are NumPy in the matrix dtype, every operation rounding once; P = S T, R = P^T and A_next = R (A P) come from
spgemm_restatement.spgemm and a stable transpose; the smoother is chebyshev_restatement.apply; the SpMVs of the cycle are the oracle's.

Keys of the root selection: the triple (state, h(i), i) is packed into one 64-bit word.  A decided non-root (state 0) never wins a maximum
that an undecided row takes part in, so it is packed as 0, and states 1 / 2 take one bit: (state - 1) << 63 | h(i) << 31 | i."""
import numpy as np
from chebyshev_restatement import GERSHGORIN, OP_ASSIGN, OP_SUB, _fma, coefficients, diagonal, gershgorin
from chebyshev_restatement import apply as cheb_apply
from spgemm_restatement import spgemm

OP_ADD = 1
THETA, MAX_LEVELS, COARSE_ROWS, SMOOTH_DEGREE, EIG_RATIO = 0.08, 10, 256, 2, 30.0
DENSE_LIMIT = 1024  # the most rows the coarsest level may have
assert GERSHGORIN == 0


class AmgRefused(Exception):
    """what the library reports as SMM_HIP_ERR_PRECOND"""


def hash32(i):
    """the 32-bit murmur3 finaliser of i + 1"""
    h = (np.asarray(i, dtype=np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def row_of(start):
    n = len(start) - 1
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(start, dtype=np.int64)))


def strength(csr, diag, theta_l):
    """per stored entry: j != i and a_ij^2 >= theta_l^2 |a_ii| |a_jj|, in double, the right side multiplied from the left"""
    start, pos, val = csr
    rows = row_of(start)
    a = val.astype(np.float64)
    d = np.abs(diag.astype(np.float64))
    rhs = ((theta_l * theta_l) * d[rows]) * d[pos]
    return (pos != rows) & (a * a >= rhs)


def pack(state, n):
    idx = np.arange(n, dtype=np.uint64)
    key = (np.uint64(1) << np.uint64(63)) * (state == 2).astype(np.uint64) | (hash32(idx) << np.uint64(31)) | idx
    return np.where(state == 0, np.uint64(0), key)


def hop(key, rows, cols):
    out = key.copy()
    np.maximum.at(out, rows, key[cols])
    return out


def roots(csr, strong):
    """(state per row: 2 root / 0 not, rounds taken)"""
    start, pos, _ = csr
    n = len(start) - 1
    rows = row_of(start)[strong]
    cols = np.asarray(pos, dtype=np.int64)[strong]
    state = np.ones(n, dtype=np.int32)
    idx = np.arange(n, dtype=np.uint64)
    rounds = 0
    while (state == 1).any():
        k2 = hop(hop(pack(state, n), rows, cols), rows, cols)
        own = (k2 & np.uint64(0x7FFFFFFF)) == idx
        top = (k2 >> np.uint64(63)) == np.uint64(1)
        undecided = state == 1
        state = np.where(undecided & own, 2, np.where(undecided & top, 0, state)).astype(np.int32)
        rounds += 1
    return state, rounds


def aggregates(csr, strong, state):
    """(aggregate number per row, aggregate count, phase-2 passes that assigned something, rows left over)"""
    start, pos, _ = csr
    n = len(start) - 1
    rows = row_of(start)[strong]
    cols = np.asarray(pos, dtype=np.int64)[strong]
    big = np.iinfo(np.int32).max
    is_root = state == 2
    number = np.cumsum(is_root) - 1
    n_roots = int(is_root.sum())
    agg = np.where(is_root, number, -1).astype(np.int64)
    best = np.full(n, big, dtype=np.int64)  # phase 1: the smallest root number among the strong neighbours
    sel = is_root[cols]
    np.minimum.at(best, rows[sel], agg[cols[sel]])
    agg = np.where((agg < 0) & (best < big), best, agg)
    passes = 0
    while True:  # phase 2: from the previous assignment as a whole
        best = np.full(n, big, dtype=np.int64)
        sel = agg[cols] >= 0
        np.minimum.at(best, rows[sel], agg[cols[sel]])
        take = (agg < 0) & (best < big)
        if not take.any():
            break
        agg = np.where(take, best, agg)
        passes += 1
    left = agg < 0
    agg = np.where(left, n_roots + np.cumsum(left) - 1, agg)
    return agg.astype(np.int32), n_roots + int(left.sum()), passes, int(left.sum())


def tentative(agg, dtype):
    n = len(agg)
    return np.arange(n + 1, dtype=np.int32), agg.astype(np.int32), np.ones(n, dtype=dtype)


def omega_of(lam):
    return 4.0 / (3.0 * lam)


def smoother_matrix(csr, diag, lam):
    """S = I - omega D^-1 A on A's pattern: s = T(omega) / d_i; off the diagonal -(s a_ij), on it 1 - s a_ii"""
    start, pos, val = csr
    T = val.dtype.type
    rows = row_of(start)
    with np.errstate(all="ignore"):
        s = T(omega_of(lam)) / diag[rows]
        t = s * val
        out = np.where(pos == rows, T(1) - t, -t).astype(val.dtype)
    return start, pos, out


def transpose(csr, cols):
    """stable by column; values bit for bit"""
    start, pos, val = csr
    order = np.argsort(pos, kind="stable")
    tstart = np.zeros(cols + 1, dtype=np.int32)
    np.cumsum(np.bincount(pos, minlength=cols), out=tstart[1:])
    return tstart, row_of(start)[order].astype(np.int32), val[order]


def check_diagonal(csr):
    start, pos, val = csr
    n = len(start) - 1
    rows = row_of(start)
    has = np.zeros(n, dtype=bool)
    has[rows[pos == rows]] = True
    d = diagonal(csr)
    if n and (not has.all() or (np.abs(d) < val.dtype.type(1e-5)).any() or (np.diff(start) == 0).any()):
        raise AmgRefused("empty row, missing diagonal or |d|<1e-5")
    return d


def level_operators(csr, theta_l, agg=None):
    """one coarsening step of A_l: dict with diag, lam, strong, state, agg, n_c, P, R, AP, A_next (agg given: the aggregates are kept)"""
    n = len(csr[0]) - 1
    diag = check_diagonal(csr)
    lam = gershgorin(csr)
    out = {"diag": diag, "lam": lam}
    if agg is None:
        strong = strength(csr, diag, theta_l)
        state, rounds = roots(csr, strong)
        agg, n_c, passes, left = aggregates(csr, strong, state)
        out.update(strong=strong, state=state, rounds=rounds, passes=passes, left=left)
    else:
        n_c = int(agg.max()) + 1 if n else 0
    out.update(agg=agg, n_c=n_c)
    return out


def products(csr, lv):
    """P, R, A P and A_next of a level whose aggregates are known"""
    n = len(csr[0]) - 1
    n_c = lv["n_c"]
    S = smoother_matrix(csr, lv["diag"], lv["lam"])
    P = spgemm(S, tentative(lv["agg"], csr[2].dtype), n_c)
    R = transpose(P, n_c)
    AP = spgemm(csr, P, n_c)
    A_next = spgemm(R, AP, n_c)
    assert len(P[0]) - 1 == n
    return P, R, AP, A_next


def hierarchy(csr, theta=THETA, max_levels=MAX_LEVELS, coarse_rows=COARSE_ROWS, keep=None):
    """the levels: a list of dicts {A, diag, lam[, agg, n_c, P, R, AP, ...]}; the last one has no P.  keep: a list of aggregate arrays of
    an earlier hierarchy (what smm_hip_precond_amg_refresh does)"""
    levels = []
    A = csr
    while True:
        l = len(levels)
        n = len(A[0]) - 1
        if n <= coarse_rows or l + 1 == max_levels or (keep is not None and l >= len(keep)):
            lv = {"A": A, "diag": check_diagonal(A), "lam": gershgorin(A) if n else 1.0}
            levels.append(lv)
            break
        lv = level_operators(A, theta * 0.5 ** l, None if keep is None else keep[l])
        lv["A"] = A
        levels.append(lv)
        if 10 * lv["n_c"] >= 9 * n:  # would not shrink: this level is the coarsest
            for k in ("agg", "n_c"):
                lv.pop(k)
            break
        lv["P"], lv["R"], lv["AP"], A = products(A, lv)
    sizes = [len(v["A"][0]) - 1 for v in levels]
    if sizes[-1] > DENSE_LIMIT:
        raise AmgRefused(f"the coarsest level has {sizes[-1]} rows: {sizes}")
    return levels


def operator_complexity(levels):
    return sum(len(v["A"][1]) for v in levels) / max(1, len(levels[0]["A"][1]))


def dense_of(csr):
    start, pos, val = csr
    n = len(start) - 1
    out = np.zeros((n, n), dtype=np.float64)
    out[row_of(start), pos] = val.astype(np.float64)
    return out


def coarse_inverse(csr):
    """the inverse of the coarsest matrix in double, rounded to T once (the library's Gauss-Jordan is compared with this by tolerance)"""
    n = len(csr[0]) - 1
    if n == 0:
        return np.zeros((0, 0), dtype=csr[2].dtype)
    return np.linalg.inv(dense_of(csr)).astype(csr[2].dtype)


def dense_apply(inv, b):
    """one wavefront per row: lane k sums columns k, k + 64, ... in ascending order from +0.0 with _fma; then the xor butterfly 32 .. 1"""
    n = inv.shape[0]
    acc = np.zeros((n, 64), dtype=inv.dtype)
    with np.errstate(all="ignore"):
        for c0 in range(0, n, 64):
            w = min(64, n - c0)
            acc[:, :w] = _fma(inv[:, c0:c0 + w], b[c0:c0 + w][None, :], acc[:, :w])
        lanes = np.arange(64)
        o = 32
        while o:
            acc = acc + acc[:, lanes ^ o]
            o >>= 1
    return acc[:, 0].copy()


def make_apply(oracle, levels, inv, smooth_degree=SMOOTH_DEGREE, eig_ratio=EIG_RATIO):
    """the V-cycle as a function of one vector; inv: the dense coarse inverse in T (the library's, or coarse_inverse(levels[-1]['A']))"""
    dtype = levels[0]["A"][2].dtype
    coeffs = [coefficients(smooth_degree, v["lam"] / eig_ratio, v["lam"], dtype) for v in levels]

    def smooth(l, r):
        return cheb_apply(oracle, levels[l]["A"], levels[l]["diag"], coeffs[l], r)

    def cycle(l, b):
        lv = levels[l]
        if "P" not in lv:
            return dense_apply(inv, b)
        with np.errstate(all="ignore"):
            x = smooth(l, b)
            r = oracle.spmv(lv["A"], OP_SUB, b, x)
            rc = oracle.spmv(lv["R"], OP_ASSIGN, None, r)
            ec = cycle(l + 1, rc)
            x = oracle.spmv(lv["P"], OP_ADD, x, ec)
            r = oracle.spmv(lv["A"], OP_SUB, b, x)
            d = smooth(l, r)
            return x + d

    def fn(r):
        r = np.ascontiguousarray(r, dtype=dtype)
        if len(r) == 0:
            return r.copy()
        return cycle(0, r)

    return fn
