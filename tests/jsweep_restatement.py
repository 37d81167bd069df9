"""The iterated triangular sweeps (SMM_PRECOND_JSWEEP_SGS / _ILU0 / _IC0) stated on the CPU in NumPy.

A helper, not a test: this is the definition csrc/smm_precond_jsweep.hip is compared with (include/smm_hip.h, SMM_PRECOND_JSWEEP_*, states
it in words).  The kinds are additions of this project, so there are no goldens.  The factor is the exact kind's (the oracle's
`ilu0_factorize` / `ic0_factorize`; SGS sweeps the matrix itself).  A Jacobi step is the exact sweep's row walk for all rows at once with
every y[col] taken from the previous iterate: the rows are independent, so the walk is vectorised over the rows and runs entry by entry in
the stored order, in the working dtype, multiply then add (the default library does not fuse).  The solver loops are
tests/chebyshev_restatement.py's `pcg` and `bicgstab` and tests/gmres_restatement.py's `gmres` with M^-1 = make_apply(...)."""
import numpy as np
from chebyshev_restatement import bicgstab, pcg  # noqa: F401  (the loops built on apply: imported from here by the tests)

SGS, ILU0, IC0 = "SGS", "ILU0", "IC0"
SGS_LO, SGS_UP, ILU_LO, ILU_UP, IC_LO, IC_UP = range(6)
MODES = {SGS: (SGS_LO, SGS_UP), ILU0: (ILU_LO, ILU_UP), IC0: (IC_LO, IC_UP)}


def split(start, positions):
    """(lower, upper, diag): per row the entry numbers the exact sweeps walk, in their order -- lower from the row's start while col < row,
    upper from the row's end backwards while col > row -- padded with -1 to the longest row, and the entry the lower walk stops at"""
    n = len(start) - 1
    lo, up = [], []
    diag = np.zeros(n, dtype=np.int64)
    for i in range(n):
        b, e = int(start[i]), int(start[i + 1])
        k = b
        while k < e and positions[k] < i:
            k += 1
        lo.append(list(range(b, k)))
        diag[i] = k
        q = e - 1
        while q >= b and positions[q] > i:
            q -= 1
        up.append(list(range(e - 1, q, -1)))

    def padded(rows):
        width = max([len(r) for r in rows], default=0)
        out = np.full((n, width), -1, dtype=np.int64)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
        return out

    return padded(lo), padded(up), diag


def levels(start, positions):
    """(levels of the lower sweep, levels of the upper sweep): level of a row = 1 + the largest level among the rows its walk reads"""
    lo, up, _ = split(start, positions)
    n = len(start) - 1
    out = []
    for idx, order in ((lo, range(n)), (up, range(n - 1, -1, -1))):
        level = np.zeros(n, dtype=np.int64)
        for i in order:
            ks = idx[i][idx[i] >= 0]
            if len(ks):
                level[i] = 1 + level[positions[ks]].max()
        out.append(int(level.max()) + 1 if n else 0)
    return tuple(out)


def _start(mode, own):
    return np.zeros_like(own) if mode == SGS_UP else own.copy()


def _term(mode, acc, value, xv):
    if mode == SGS_UP:
        return value * xv + acc
    if mode in (SGS_LO, ILU_LO, ILU_UP):
        return (-value) * xv + acc
    prod = value * xv  # IC: multiply, then subtract
    return acc - prod


def _finish(mode, acc, own, d):
    if mode == SGS_UP:
        return own - acc / d
    if mode == ILU_LO:
        return acc
    return acc / d


def _step(mode, idx, positions, values, d, own, prev):
    acc = _start(mode, own)
    for k in range(idx.shape[1]):
        rows = np.nonzero(idx[:, k] >= 0)[0]
        at = idx[rows, k]
        acc[rows] = _term(mode, acc[rows], values[at], prev[positions[at]])
    return _finish(mode, acc, own, d)


def _phase(mode, idx, positions, values, d, own, sweeps):
    y = _finish(mode, _start(mode, own), own, d)  # iterate 0: the walk with no terms
    for _ in range(sweeps):
        y = _step(mode, idx, positions, values, d, own, y)
    return y


def apply(start, positions, factor_values, base, sweeps_lower, sweeps_upper, rhs, parts=None):
    """z = M^-1 rhs: sweeps_lower Jacobi steps of the lower sweep on own = rhs, then sweeps_upper steps of the upper sweep on own = the
    lower phase's result.  factor_values: the values the exact sweeps walk (A's for SGS, the factor for ILU0 / IC0), on A's pattern.
    parts: split(start, positions), when the caller keeps it."""
    values = np.ascontiguousarray(factor_values)
    own = np.ascontiguousarray(rhs, dtype=values.dtype)
    lo, up, diag = parts if parts is not None else split(start, positions)
    if len(own) == 0:
        return own.copy()
    d = values[diag]
    mlo, mup = MODES[base]
    with np.errstate(all="ignore"):
        y = _phase(mlo, lo, positions, values, d, own, sweeps_lower)
        return _phase(mup, up, positions, values, d, y, sweeps_upper)


def factor(oracle, csr, base):
    """the values the sweeps walk: the oracle's ILU0 / IC0 factor on A's pattern, A's own values for SGS"""
    if base == SGS:
        return csr[2]
    err, f = oracle.ilu0_factorize(csr) if base == ILU0 else oracle.ic0_factorize(csr)
    assert err == 0, err
    return f


def exact(oracle, csr, base, f, rhs):
    """the exact kind's apply: the oracle's sequential sweeps"""
    rhs = np.ascontiguousarray(rhs, dtype=csr[2].dtype)
    err, z = oracle.sgs_apply(csr, rhs) if base == SGS else oracle.ilu0_apply(csr, f, rhs) if base == ILU0 else oracle.ic0_apply(csr, f, rhs)
    assert err == 0, err
    return z


def make_apply(oracle, csr, base, sweeps_lower=3, sweeps_upper=None, values=None):
    """M^-1 as a function of one vector"""
    f = factor(oracle, csr, base) if values is None else values
    parts = split(csr[0], csr[1])
    su = sweeps_lower if sweeps_upper is None else sweeps_upper
    return lambda r: apply(csr[0], csr[1], f, base, sweeps_lower, su, r, parts)
