"""The multicolour reordering stated on the CPU: the colouring, the permutation, B = P A Pᵀ and M^-1 r = Pᵀ sweeps_B(P r).

A helper, not a test: this is the definition csrc/smm_color.hip and csrc/smm_precond_mc.hip are compared with (include/smm_hip.h,
SMM_PRECOND_MULTICOLOR_* and "a COLOURING of the rows", states it in words).  The kinds are additions of this project, so there are no
goldens.  The sweeps and the factorisations are the oracle's own (`sgs_apply`, `ilu0_*`, `ic0_*`) on the permuted matrix; everything
else is integer work or moves values without arithmetic.  The solver loops are tests/chebyshev_restatement.py's `pcg` and `bicgstab`
and tests/gmres_restatement.py's `gmres` with M^-1 = make_apply(...)."""
import numpy as np

SGS, ILU0, IC0 = "SGS", "ILU0", "IC0"
_MASK = (1 << 64) - 1


def splitmix64(x):
    """one step of the splitmix64 generator from the state x (Python integers, 64-bit wrapping arithmetic)"""
    z = (x + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def keys(n):
    """key(i) = splitmix64(i + 1): a bijection of the 64-bit integers, so no two rows tie"""
    return [splitmix64(i + 1) for i in range(n)]


def neighbours(csr):
    """per row the rows it is adjacent to: j != i with (i, j) or (j, i) stored (explicit zeros count)"""
    start, pos, _ = csr
    n = len(start) - 1
    adj = [set() for _ in range(n)]
    for i in range(n):
        for j in pos[start[i]:start[i + 1]]:
            j = int(j)
            if j != i:
                adj[i].add(j)
                adj[j].add(i)
    return adj


def color(csr):
    """(colors, ncolors): the rows in DESCENDING key order, each given the smallest colour none of its coloured neighbours holds"""
    n = len(csr[0]) - 1
    adj = neighbours(csr)
    key = keys(n)
    colors = np.full(n, -1, dtype=np.int32)
    for i in sorted(range(n), key=lambda v: key[v], reverse=True):
        held = {int(colors[j]) for j in adj[i] if colors[j] >= 0}
        c = 0
        while c in held:
            c += 1
        colors[i] = c
    return colors, (int(colors.max()) + 1 if n else 0)


def is_proper(csr, colors):
    """no stored off-diagonal entry joins two rows of one colour"""
    start, pos, _ = csr
    rowof = np.repeat(np.arange(len(start) - 1), np.diff(start))
    cols = pos[:start[-1]]
    off = rowof != cols
    return not bool(np.any(colors[rowof[off]] == colors[cols[off]]))


def permutation(colors):
    """perm[]: the rows sorted by colour, stably (the original index ascends inside a colour); new row i is row perm[i]"""
    return np.argsort(colors, kind="stable").astype(np.int32)


def bounds(colors, ncolors):
    """the ncolors + 1 row bounds of the colours in the permuted numbering"""
    return np.searchsorted(np.sort(colors, kind="stable"), np.arange(ncolors + 1)).astype(np.int32)


def permute(csr, perm):
    """B = P A Pᵀ: b(i, j) = a(perm[i], perm[j]), columns ascending inside each row, values carried bit for bit"""
    start, pos, val = csr
    n = len(start) - 1
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    length = np.diff(start)[perm]
    bstart = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(length, out=bstart[1:])
    bpos = np.empty(int(start[-1]), dtype=np.int32)
    bval = np.empty(int(start[-1]), dtype=val.dtype)
    for i in range(n):
        r = perm[i]
        cols = inv[pos[start[r]:start[r + 1]]]
        order = np.argsort(cols, kind="stable")
        bpos[bstart[i]:bstart[i + 1]] = cols[order]
        bval[bstart[i]:bstart[i + 1]] = val[start[r]:start[r + 1]][order]
    return bstart, bpos, bval


def factor(oracle, bcsr, base):
    """the oracle's factor of B on B's pattern (None for SGS, which sweeps B itself)"""
    if base == SGS:
        return None
    err, f = oracle.ilu0_factorize(bcsr) if base == ILU0 else oracle.ic0_factorize(bcsr)
    assert err == 0, err
    return f


def setup(oracle, csr, base, colors=None):
    """(colors, ncolors, perm, B, factor): everything a handle keeps"""
    if colors is None:
        colors, ncolors = color(csr)
    else:
        colors = np.asarray(colors, dtype=np.int32)
        ncolors = int(colors.max()) + 1 if len(colors) else 0
    perm = permutation(colors)
    bcsr = permute(csr, perm)
    return colors, ncolors, perm, bcsr, factor(oracle, bcsr, base)


def make_apply(oracle, csr, base, colors=None):
    """M^-1 as a function of one vector: permute, the oracle's two sweeps on B, unpermute"""
    _, _, perm, bcsr, f = setup(oracle, csr, base, colors)

    def apply(r):
        pr = np.ascontiguousarray(np.asarray(r, dtype=csr[2].dtype)[perm])
        if base == SGS:
            err, y = oracle.sgs_apply(bcsr, pr)
        elif base == ILU0:
            err, y = oracle.ilu0_apply(bcsr, f, pr)
        else:
            err, y = oracle.ic0_apply(bcsr, f, pr)
        assert err == 0, err
        z = np.empty_like(y)
        z[perm] = y
        return z

    return apply
