"""The LONGROWS SpMV family's arithmetic, restated in NumPy from include/smm_hip.h (SMM_SPMV_LONGROWS), literally:

  a row of at most split_len entries   d = 0; d = fma(v[k], x[p[k]], d) for k in stored order;
  a longer row                         segments of segment_len entries counted from the row's first entry; per segment 64 chains
                                       c[l] = 0; c[l] = fma(v[j], x[p[j]], c[l]) over the entries j = l, l + 64, ... of the segment, then
                                       c[l] = c[l] + c[l xor o] for o = 32, 16, 8, 4, 2, 1 (all l at once), the segment's sum is c[0];
                                       the row is d = 0; d = d + (segment sum i), i ascending.

Every operation is NumPy in the matrix dtype and rounds once.  fma(a, x, b) is a * x + b with two roundings (libsmm_hip.so) or, with
std_fma=True, the exact a * x + b rounded once (libsmm_hip_fma.so): formed as a fraction and rounded to the nearest number of the dtype,
ties to even -- slow, meant for a few thousand entries."""
from fractions import Fraction

import numpy as np

WAVE = 64


def _round_once(q, T):
    """the Fraction q rounded to the nearest T, ties to even"""
    f = T(float(q))  # within one unit of the answer (fp64: float() rounds correctly already)
    if not np.isfinite(f):
        return f
    best = f
    for cand in (np.nextafter(f, T(-np.inf)), np.nextafter(f, T(np.inf))):
        if not np.isfinite(cand):
            continue
        dc, db = abs(Fraction(float(cand)) - q), abs(Fraction(float(best)) - q)
        if dc < db or (dc == db and (cand.view(np.uint32 if T is np.float32 else np.uint64) & 1) == 0):
            best = cand
    return best


def _fma(a, x, b, std_fma):
    """elementwise over arrays (or scalars) of one dtype"""
    if not std_fma:
        return a * x + b
    a, x, b = np.broadcast_arrays(np.asarray(a), np.asarray(x), np.asarray(b))
    T = a.dtype.type
    out = np.empty(a.shape, dtype=a.dtype)
    flat = out.reshape(-1)
    for i, (ai, xi, bi) in enumerate(zip(a.reshape(-1), x.reshape(-1), b.reshape(-1))):
        q = Fraction(float(ai)) * Fraction(float(xi)) + Fraction(float(bi))
        flat[i] = _round_once(q, T) if q != 0 else T(float(ai) * float(xi)) + bi  # (an exact zero keeps IEEE's sign rules)
    return out


def segment_sum(v, xx, std_fma=False):
    """one segment: v and xx are its values and the x entries they meet, in stored order"""
    T = v.dtype.type
    n = len(v)
    rounds = (n + WAVE - 1) // WAVE
    pv = np.zeros(rounds * WAVE, dtype=v.dtype)
    px = np.zeros(rounds * WAVE, dtype=v.dtype)
    pv[:n], px[:n] = v, xx
    have = (np.arange(rounds * WAVE) < n).reshape(rounds, WAVE)
    pv, px = pv.reshape(rounds, WAVE), px.reshape(rounds, WAVE)
    c = np.zeros(WAVE, dtype=v.dtype)
    for i in range(rounds):  # lane l takes entries l, l + 64, ...; a lane without an entry keeps its sum
        c = np.where(have[i], _fma(pv[i], px[i], c, std_fma), c)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        c = c + c[lanes ^ o]
    return T(c[0])


def long_row(v, xx, segment_len, std_fma=False):
    T = v.dtype.type
    d = T(0)
    for b in range(0, len(v), segment_len):
        d = d + segment_sum(v[b:b + segment_len], xx[b:b + segment_len], std_fma)
    return d


def chain(v, xx, std_fma=False):
    """a short row: one chain from 0 in stored order"""
    T = v.dtype.type
    d = T(0)
    for a, b in zip(v, xx):
        d = T(_fma(a, b, d, std_fma))
    return d


def spmv(start, pos, val, x, split_len, segment_len, std_fma=False):
    """A x row by row in the stated order; x and the result have val's dtype"""
    start = np.asarray(start, dtype=np.int64)
    rows = len(start) - 1
    x = np.asarray(x, dtype=val.dtype)
    out = np.zeros(rows, dtype=val.dtype)
    lens = np.diff(start)
    short = lens <= split_len
    if std_fma:
        for r in np.flatnonzero(short):
            out[r] = chain(val[start[r]:start[r + 1]], x[pos[start[r]:start[r + 1]]], True)
    else:
        # every short row's chain at once, entry by entry
        for j in range(int(lens[short].max()) if short.any() else 0):
            m = short & (lens > j)
            k = start[:-1][m] + j
            out[m] = val[k] * x[pos[k]] + out[m]
    for r in np.flatnonzero(~short):
        out[r] = long_row(val[start[r]:start[r + 1]], x[pos[start[r]:start[r + 1]]], segment_len, std_fma)
    return out
