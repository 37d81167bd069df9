"""Helpers shared by the GMRES tests (not a test): the build line of tests/cpp/gmres_case.cpp and the symmetric permutation of a CSR
matrix that the block preconditioners are defined on."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "gmres_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_mutators_cpu.py"""
    exe = tmp_path / "gmres_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def permuted(csr, order):
    """P A P^T as sorted CSR: row p of the result is row order[p] of A, columns renumbered by the inverse of `order` (the block kinds with
    a brick partition are, by definition, the block kinds of this matrix with contiguous blocks)"""
    import scipy.sparse as sp

    start, pos, val = csr
    n = len(start) - 1
    A = sp.csr_matrix((val, pos, start), shape=(n, n))
    Ap = A[order][:, order].tocsr()
    Ap.sort_indices()
    return Ap.indptr.astype(np.int32), Ap.indices.astype(np.int32), Ap.data.astype(val.dtype)
