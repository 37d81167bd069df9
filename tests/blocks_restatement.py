"""The fit rule of the BLOCKS SpMV family (include/smm_hip.h, SMM_SPMV_BLOCKS) restated in numpy, entry by entry -- the definition
smm_hip_csr_find_blocks is compared with."""
import numpy as np

SIZES = (4, 3, 2)  # the order block size 0 tries them in


def fits(start, positions, rows, cols, b, max_row_entries):
    """the CSR matrix is a sparse matrix of dense b x b blocks on block-aligned columns, no row longer than max_row_entries"""
    start = np.asarray(start, dtype=np.int64)
    positions = np.asarray(positions, dtype=np.int64)
    if rows % b or cols % b:
        return False
    for R in range(rows // b):
        first = positions[start[R * b]:start[R * b + 1]]
        if len(first) % b or len(first) > max_row_entries:
            return False
        lead = first[::b]
        if np.any(lead % b) or np.any(lead < 0) or np.any(lead + b > cols):
            return False
        want = (lead[:, None] + np.arange(b)[None, :]).reshape(-1)
        for i in range(b):
            row = positions[start[R * b + i]:start[R * b + i + 1]]
            if len(row) != len(want) or np.any(row != want):
                return False
    return True


def largest_fit(start, positions, rows, cols, max_row_entries):
    """what find_blocks(0) keeps; max_row_entries: {b: limit}"""
    for b in SIZES:
        if fits(start, positions, rows, cols, b, max_row_entries[b]):
            return b
    return 0
