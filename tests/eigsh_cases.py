"""The matrices of the eigsh tests (tests/test_eigsh_cpu.py, tests/test_gpu_eigsh.py): symmetric, small, and without multiple
eigenvalues among the five at either end (the smallest gap there is >= 3e-3; 0.01 at diag_sq_300's small end).

  lap2d_16x12     the five-point Laplacian on a 16 x 12 grid     192 rows (a rectangular grid: the square one has double eigenvalues)
  shifted_16x12   lap2d_16x12 - 3.1 I                            192 rows, indefinite
  chain_96        tridiagonal -1 2 -1                             96 rows
  diag_sq_300     diag((i + 1)^2 / 300)                          300 rows, LARGEST only: its small end is clustered and takes about 160
                                                                 restarts, which is plain Lanczos's nature
  lap2d_33x29     the five-point Laplacian on a 33 x 29 grid     957 rows: crosses the 64- and 256-row tile edges with a ragged tail
"""
import numpy as np

from sparse_matrix_math_amd import generators as gen

NAMES = ("lap2d_16x12", "shifted_16x12", "chain_96", "diag_sq_300", "lap2d_33x29")
ROWS = {"lap2d_16x12": 192, "shifted_16x12": 192, "chain_96": 96, "diag_sq_300": 300, "lap2d_33x29": 957}
ENDS = {name: ("LA",) if name == "diag_sq_300" else ("LA", "SA") for name in NAMES}
SHAPES = ((4, 20), (6, 32))  # (k, ncv)
SMALL_SHAPE = (1, 8)          # on the two 192-row cases as well
SMALL_SHAPE_ON = ("lap2d_16x12", "shifted_16x12")
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}
MAX_RESTARTS = 100


def _shift_diagonal(csr, sigma, dtype):
    start, pos, val = csr
    val = val.copy()
    rows = np.repeat(np.arange(len(start) - 1), np.diff(start))
    val[pos == rows] -= np.dtype(dtype).type(sigma)
    return start, pos, val


def diagonal(values, dtype=np.float64):
    n = len(values)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(values, dtype=dtype)


def chain(n, dtype=np.float64):
    start, pos, val = [0], [], []
    for r in range(n):
        for c, v in ((r - 1, -1.0), (r, 2.0), (r + 1, -1.0)):
            if 0 <= c < n:
                pos.append(c)
                val.append(v)
        start.append(len(pos))
    return np.array(start, dtype=np.int32), np.array(pos, dtype=np.int32), np.array(val, dtype=dtype)


def matrix(name, dtype=np.float64):
    if name == "lap2d_16x12":
        return gen.poisson2d(16, 12, dtype=dtype)
    if name == "shifted_16x12":
        return _shift_diagonal(gen.poisson2d(16, 12, dtype=dtype), 3.1, dtype)
    if name == "chain_96":
        return chain(96, dtype)
    if name == "diag_sq_300":
        return diagonal((np.arange(300) + 1.0) ** 2 / 300.0, dtype)
    if name == "lap2d_33x29":
        return gen.poisson2d(33, 29, dtype=dtype)
    raise KeyError(name)


def dense(csr):
    start, pos, val = csr
    rows = len(start) - 1
    out = np.zeros((rows, rows), dtype=np.float64)
    r = np.repeat(np.arange(rows), np.diff(start))
    out[r, pos] = val
    return out


def combos():
    """(name, which, k, ncv) of every eigenvalue case the issue lists"""
    out = []
    for name in NAMES:
        shapes = SHAPES + ((SMALL_SHAPE,) if name in SMALL_SHAPE_ON else ())
        for which in ENDS[name]:
            for k, ncv in shapes:
                out.append((name, which, k, ncv))
    return out


_EXACT = {}


def exact(name):
    """eigvalsh of the dense fp64 matrix, ascending; computed once and read-only"""
    if name not in _EXACT:
        ev = np.linalg.eigvalsh(dense(matrix(name, np.float64)))
        ev.setflags(write=False)
        _EXACT[name] = ev
    return _EXACT[name]


def wanted(ev, which, k):
    """the k eigenvalues of the ascending `ev` in the order eigsh returns them"""
    return ev[::-1][:k] if which == "LA" else ev[:k]
