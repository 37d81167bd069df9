"""Matrices for the FSAI / SPAI tests (tests/test_ainv_cpu.py, tests/test_gpu_ainv.py).  A helper, not a test."""
import numpy as np
from test_chebyshev_cpu import spd5
from test_oracle import gen_matrices

TRIDIAGONAL_ROWS = (1, 2, 63, 64, 65, 257)  # the sub-group packing (8 systems per wavefront) and the grid tail


def negated_row5(dtype):
    """spd5 with row 2 multiplied by -1 -- not positive definite (the construction of tests/test_gpu_chebyshev.py, which is a GPU module)"""
    start, pos, val = spd5(dtype)
    val = val.copy()
    val[start[2]:start[3]] *= -1
    return start, pos, val


def from_dense(dense, dtype):
    start = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int32)
    return start, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(dtype)


def ladder(dtype, modulus=64, rows=300):
    """symmetric, strictly diagonally dominant: row i couples to the min(i, i mod modulus) rows before it (and, by symmetry, to the rows
    after it that couple to it), so FSAI's row lengths take every value 1 .. modulus; off-diagonal values are small dyadic numbers"""
    dense = np.zeros((rows, rows))
    for i in range(rows):
        for j in range(i - min(i, i % modulus), i):
            dense[i, j] = dense[j, i] = -(1 + (i + 2 * j) % 5) / 64.0
    dense[np.arange(rows), np.arange(rows)] = 1.0 + np.abs(dense).sum(axis=1)
    return from_dense(dense, dtype)


def tridiagonal(rows, dtype):
    dense = 2.5 * np.eye(rows) - np.eye(rows, k=1) - np.eye(rows, k=-1)
    return from_dense(dense, dtype)


def descending(dtype):
    """a 5-row symmetric positive definite band whose rows are stored in DESCENDING column order, row 2 holding column 1 twice: look()
    must take the first stored one (-0.5) and never the second (0.125)"""
    start, pos, val = [0], [], []
    for i in range(5):
        for j in range(min(4, i + 1), max(0, i - 1) - 1, -1):
            pos.append(j)
            val.append(3.0 if i == j else -0.5)
            if (i, j) == (2, 1):
                pos.append(1)
                val.append(0.125)
        start.append(len(pos))
    return np.array(start, dtype=np.int32), np.array(pos, dtype=np.int32), np.array(val, dtype=dtype)


def case(name, dtype):
    if name == "spd5":
        return spd5(dtype)
    if name == "negated_row5":
        return negated_row5(dtype)
    if name == "ladder":
        return ladder(dtype, 64)
    if name == "ladder24":
        return ladder(dtype, 24)
    if name == "descending":
        return descending(dtype)
    if name.startswith("tridiagonal_"):
        return tridiagonal(int(name.split("_")[1]), dtype)
    return gen_matrices(dtype)[name]


def dense_of(csr):
    """the dense matrix look() describes: of entries stored twice the FIRST counts"""
    start, pos, val = csr
    n = len(start) - 1
    A = np.zeros((n, n), dtype=np.float64)
    for r in range(n):
        for k in range(start[r + 1] - 1, start[r] - 1, -1):  # backwards: the first stored entry is written last
            A[r, pos[k]] = val[k]
    return A


def dense_sum_of(csr):
    """the dense matrix the SpMV and the sparse product see: entries stored twice add up"""
    start, pos, val = csr
    n = len(start) - 1
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (np.repeat(np.arange(n), np.diff(start)), pos), val)
    return A
