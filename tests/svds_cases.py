"""The matrices of the svds tests (tests/test_svds_cpu.py, tests/test_gpu_svds.py, tests/test_cpp_svds.py), all rectangular and small.
Built with NumPy and the package generators (through tests/lsqr_cases.py).

  tall, wide, sparse_random   tests/lsqr_cases.py's: 168 x 144, its transpose, and 300 x 120 with an empty row and an empty column
  grad2d_16x12                the forward differences of a 16 x 12 grid (180 along x, then 176 along y): 356 x 192.  Rectangular, because
                              the square grid has double singular values
  grad2d_33x29                the same of a 33 x 29 grid: 1852 x 957; both dimensions cross the 64- and 256-row tile edges with ragged tails
  grad2d_33x29_t              its transpose: 957 x 1852

A matrix is (rows, cols, (start, positions, values)); every stored value is exact in fp32 but sparse_random's."""
import lsqr_cases
import numpy as np

NAMES = ("tall", "wide", "sparse_random", "grad2d_16x12", "grad2d_33x29", "grad2d_33x29_t")
SHAPE = {"tall": (168, 144), "wide": (144, 168), "sparse_random": (300, 120), "grad2d_16x12": (356, 192), "grad2d_33x29": (1852, 957),
         "grad2d_33x29_t": (957, 1852)}
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}
MAX_RESTARTS = 100
# Restarts of the restatement (tests/svds_restatement.py) from the hash vector of seed 0 to TOL, as (fp64, fp32) per (name, k, ncv) --
# recorded from the restatement itself and pinned by tests/test_svds_cpu.py.
RESTARTS = {
    ("tall", 4, 20): (5, 3), ("tall", 6, 32): (2, 1), ("wide", 4, 20): (5, 3), ("wide", 6, 32): (2, 1),
    ("sparse_random", 4, 20): (4, 2), ("sparse_random", 6, 32): (2, 1), ("grad2d_16x12", 4, 20): (9, 5), ("grad2d_16x12", 6, 32): (5, 3),
    ("grad2d_33x29", 4, 20): (24, 14), ("grad2d_33x29", 6, 32): (14, 8), ("grad2d_33x29_t", 4, 20): (23, 14), ("grad2d_33x29_t", 6, 32): (14, 9),
    ("tall", 1, 8): (11, 4), ("wide", 1, 8): (11, 4),
}
# max(|U^T U - I|, |V^T V - I|) of the restatement's factors over every combination, in units of the dtype's eps, rounded up -- recorded
# from the restatement and pinned (as an upper bound) by tests/test_svds_cpu.py.  The GPU tests allow four times this: the margin for
# another summation order.  It is never taken from the GPU's own output.
ORTH_LOSS_EPS = {np.dtype(np.float64): 69, np.dtype(np.float32): 3}  # measured: 69.0 and 2.89


def combos():
    out = [(name, k, ncv) for name in NAMES for k, ncv in ((4, 20), (6, 32))]
    return out + [(name, 1, 8) for name in ("tall", "wide")]


def _grad_dense(nx, ny):
    rows = []
    idx = lambda ix, iy: iy * nx + ix  # noqa: E731
    for iy in range(ny):
        for ix in range(nx - 1):
            r = np.zeros(nx * ny)
            r[idx(ix, iy)], r[idx(ix + 1, iy)] = -1.0, 1.0
            rows.append(r)
    for iy in range(ny - 1):
        for ix in range(nx):
            r = np.zeros(nx * ny)
            r[idx(ix, iy)], r[idx(ix, iy + 1)] = -1.0, 1.0
            rows.append(r)
    return np.array(rows)


_DENSE = {}
_SIGMA = {}


def _built(name):
    """(the dense fp64 matrix, the mask of its stored entries or None)"""
    if name not in _DENSE:
        if name in lsqr_cases.NAMES:
            _DENSE[name] = lsqr_cases._built(name)
        elif name == "grad2d_16x12":
            _DENSE[name] = (_grad_dense(16, 12), None)
        elif name == "grad2d_33x29":
            _DENSE[name] = (_grad_dense(33, 29), None)
        elif name == "grad2d_33x29_t":
            _DENSE[name] = (np.ascontiguousarray(_grad_dense(33, 29).T), None)
        else:
            raise KeyError(name)
    return _DENSE[name]


def matrix(name, dtype=np.float64):
    a, keep = _built(name)
    return a.shape[0], a.shape[1], lsqr_cases.from_dense(a, dtype, keep)


def dense(name, dtype=np.float64):
    """the matrix as stored in `dtype`, as a dense fp64 array"""
    rows, cols, csr = matrix(name, dtype)
    return lsqr_cases.dense(csr, cols)


def exact(name):
    """numpy.linalg.svd's singular values of the dense fp64 matrix, descending (computed once; read-only)"""
    if name not in _SIGMA:
        _SIGMA[name] = np.linalg.svd(dense(name), compute_uv=False)
        _SIGMA[name].setflags(write=False)
    return _SIGMA[name]


def blocks_rank3(dtype=np.float64):
    """80 x 60: three disjoint constant blocks c_b ones(10 x 8), c = 3, 2, 1, block b on rows 10 b .. and columns 8 b ..; rank 3,
    singular values c_b sqrt(80)"""
    a = np.zeros((80, 60))
    for b, c in enumerate((3.0, 2.0, 1.0)):
        a[10 * b:10 * b + 10, 8 * b:8 * b + 8] = c
    return 80, 60, lsqr_cases.from_dense(a, dtype)


def identity_over_zero(dtype=np.float64):
    """[I_50; 0]: 60 x 50"""
    a = np.zeros((60, 50))
    a[:50, :50] = np.eye(50)
    return 60, 50, lsqr_cases.from_dense(a, dtype)


def diagonal(d, dtype=np.float64):
    n = len(d)
    return n, n, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, dtype=dtype))
