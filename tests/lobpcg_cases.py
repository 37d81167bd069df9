"""The cases of the lobpcg tests (tests/test_lobpcg_cpu.py, tests/test_gpu_lobpcg.py): the matrices of tests/eigsh_cases.py, unchanged,
with block sizes k.

  lap2d_16x12, shifted_16x12    k = 1, 4, 6
  chain_96                      k = 4, 6      (k = 1 is deliberately absent: one vector without a preconditioner needs over 1000
                                               iterations at the large end in fp64 -- the block is what makes the method converge there)
  lap2d_33x29                   k = 4, 6, 8   957 rows: ragged against the 64- and 256-row tile edges

every one at both ends (SA, LA) and in both dtypes; tol 1e-10 (fp64) / 1e-4 (fp32) as for eigsh; maxIterations 1000."""
import eigsh_cases as cases
import numpy as np

matrix, dense, exact, wanted, diagonal, ROWS, TOL = cases.matrix, cases.dense, cases.exact, cases.wanted, cases.diagonal, cases.ROWS, cases.TOL
BLOCKS = {"lap2d_16x12": (1, 4, 6), "shifted_16x12": (1, 4, 6), "chain_96": (4, 6), "lap2d_33x29": (4, 6, 8)}
ENDS = ("SA", "LA")
MAX_ITERATIONS = 1000
MAX_K, MAX_BASIS = 8, 24
# max|X^T X - I| / eps of the restatement, the worst over the cases above per dtype, rounded up (tests/test_lobpcg_cpu.py prints every
# ratio and asserts that none exceeds these: 129.0 on lap2d_16x12 SA k = 6 in fp64, 5.37 on lap2d_33x29 LA k = 8 in fp32).  X is carried by
# rotations, so the loss grows with the iteration count.  The GPU's bound is 4 times this, the factor for another summation order.
ORTH_WORST = {np.dtype(np.float64): 130.0, np.dtype(np.float32): 5.5}


def combos():
    """(name, which, k) of every eigenvalue case the issue lists"""
    return [(name, which, k) for name, ks in BLOCKS.items() for which in ENDS for k in ks]


def lap2d_16x16(dtype=np.float64):
    """the square grid: its second and third eigenvalues coincide, and so do the fifth and the sixth; the seventh is apart"""
    from sparse_matrix_math_amd import generators as gen

    return gen.poisson2d(16, 16, dtype=dtype)


def triple_diagonal(dtype=np.float64):
    """diag(1 x 20, 2 x 20, 5 x 20)"""
    return diagonal(np.repeat([1.0, 2.0, 5.0], 20), dtype)
