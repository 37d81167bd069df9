"""The BLOCKS SpMV family without a GPU: the public header declares the new names and the built library exports them, gen.block_expand
produces matrices that satisfy the numpy restatement of the fit rule (tests/blocks_restatement.py), and each single mutation of
tests/blocks_cases.py breaks it."""
import ctypes
import os
import re

import numpy as np
import pytest
from blocks_cases import BIT_SHAPES, MUTATIONS, blocked, mutated
from blocks_restatement import fits, largest_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_LIMIT = 1 << 30


def test_header_declares_and_library_exports_the_names():
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    assert re.search(r"#define\s+SMM_SPMV_BLOCKS\s+4\b", header)
    assert re.search(r"int\s+smm_hip_csr_find_blocks\(smm_hip_csr\*\s*m,\s*int\s+block_size,\s*int\*\s*found\);", header)
    assert re.search(r"int\s+smm_hip_csr_blocks_info\(const\s+smm_hip_csr\*\s*m,\s*int\*\s*block_size,\s*long long\*\s*blocks,\s*int\*\s*max_row_entries\);", header)
    for name in ("libsmm_hip.so", "libsmm_hip_fma.so"):
        path = os.path.join(ROOT, "sparse_matrix_math_amd", "lib", name)
        if not os.path.exists(path):
            pytest.fail(f"{name} not built (build() makes it)")
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "smm_hip_csr_find_blocks") and hasattr(lib, "smm_hip_csr_blocks_info")
    import sparse_matrix_math_amd as smm
    from sparse_matrix_math_amd import _lib

    assert smm.SPMV_BLOCKS == 4
    _lib.load()  # every prototype of _lib.py resolves, the two new ones included


@pytest.mark.parametrize("b", [2, 3, 4])
@pytest.mark.parametrize("name", BIT_SHAPES + ["base"])
def test_block_expand_satisfies_the_rule(name, b):
    (start, pos, val), rows, cols = blocked(name, b)
    assert len(start) == rows + 1 and start[0] == 0 and start[-1] == len(pos) == len(val)
    assert fits(start, pos, rows, cols, b, NO_LIMIT)
    for r in range(rows):  # a valid CSR: columns ascend strictly inside a row and stay inside the matrix
        row = pos[start[r]:start[r + 1]]
        assert np.all(np.diff(row) > 0) and (len(row) == 0 or (row[0] >= 0 and row[-1] < cols))


def test_block_expand_diag_dominant():
    from sparse_matrix_math_amd import generators as gen

    s, p, _ = gen.random_rows(30, 30, 2, 5, seed=3, diag_dominant=True)
    start, pos, val = gen.block_expand(s, p, 3, seed=4, dtype=np.float32, diag_dominant=True)
    assert val.dtype == np.float32 and fits(start, pos, 90, 90, 3, NO_LIMIT)
    for r in range(90):
        row, v = pos[start[r]:start[r + 1]], val[start[r]:start[r + 1]].astype(np.float64)
        d = v[row == r]
        assert len(d) == 1 and d[0] > np.abs(v).sum() - d[0]


@pytest.mark.parametrize("b", [2, 3, 4])
@pytest.mark.parametrize("kind", MUTATIONS)
def test_every_single_mutation_breaks_the_rule(kind, b):
    (start, pos, _), rows, cols = mutated(kind, b)
    assert not fits(start, pos, rows, cols, b, NO_LIMIT)


@pytest.mark.parametrize("b", [2, 3, 4])
def test_the_row_length_limit(b):
    (start, pos, _), rows, cols = blocked("base", b)
    longest = int(np.diff(start).max())
    assert fits(start, pos, rows, cols, b, longest) and not fits(start, pos, rows, cols, b, longest - b)


def test_six_blocks_fit_three_and_two_not_four():
    (start, pos, _), rows, cols = blocked("six", 6)
    assert fits(start, pos, rows, cols, 3, NO_LIMIT) and fits(start, pos, rows, cols, 2, NO_LIMIT) and not fits(start, pos, rows, cols, 4, NO_LIMIT)
    assert largest_fit(start, pos, rows, cols, {4: NO_LIMIT, 3: NO_LIMIT, 2: NO_LIMIT}) == 3
