"""Helpers shared by the IDR(s) tests (not a test): the fixed-step case list, the references computed once per session, and the build line
of tests/cpp/idrs_case.cpp."""
import os
import shutil
import subprocess

import numpy as np
from idrs_restatement import idrs, perturbed, sensitivity, shadow
from test_oracle import gen_matrices

from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "idrs_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
MATRICES = ("poisson2d_32", "banded_2000", "convdiff3d_12")
SEED = 2011  # of the shadow spaces the comparisons pass in

# (s, dtype, steps): s in {1, 4} x steps {3, 10, 25} in both dtypes; s = 8 x {3, 10} in fp64 and {3} in fp32 (later steps with s = 8 in
# fp32 are too sensitive on the Poisson matrix for the comparison to mean anything).  With s = 4 the steps 3, 10 and 25 end inside a
# cycle, on the dimension-reduction step and across cycles.
STEPS = [(s, dt, it) for s in (1, 4) for dt in (np.float32, np.float64) for it in (3, 10, 25)]
STEPS += [(8, np.float64, 3), (8, np.float64, 10), (8, np.float32, 3)]
# Dropped, as the rule says, because the restatement's own sensitivity breaks the cap of test_gpu_cgs.allowed (1e-2 max(1, max|x|)) with
# these generators and this P -- measured on the CPU: poisson2d_32 fp32 25 steps 7.0e-2 (s = 1) and 9.2e-2 (s = 4); convdiff3d_12 fp32
# s = 4 2.6e-1 after 10 steps (max|x| = 7.1) and 1.3e-2 after 25.  Their fp64 twins stay.
TOO_SENSITIVE = {("poisson2d_32", 1, np.float32, 25), ("poisson2d_32", 4, np.float32, 25), ("convdiff3d_12", 4, np.float32, 10),
                 ("convdiff3d_12", 4, np.float32, 25)}
FIXED = [(m, s, dt, it) for m in MATRICES for s, dt, it in STEPS if (m, s, dt, it) not in TOO_SENSITIVE]

# eps of the near-breakdown system.  With JACOBI the restatement's own count at 1e-3 moves by 17 under a one-ulp change of b (126 against
# 109 .. 111; at 2e-3 .. 5e-3 by 11 .. 14), more than half of the allowance max(2, it // 5): another eps, not a wider allowance -- at 1e-2
# it is 116 against 107 .. 109.
NEAR_EPS = {False: 1e-3, True: 1e-2}

_REF = {}


def matrix(mname, dtype):
    key = ("matrix", mname, np.dtype(dtype).name)
    if key not in _REF:
        csr = gen_matrices(dtype)[mname]
        _REF[key] = (csr, gen.row_sums(csr[0], csr[2]))
    return _REF[key]


def shadow_space(oracle, rows, s, dtype, seed=SEED):
    key = ("P", rows, s, np.dtype(dtype).name, seed)
    if key not in _REF:
        _REF[key] = shadow(oracle, rows, s, seed, dtype)
    return _REF[key]


def reference(oracle, tag, csr, b, it, s, apply=None):
    """(status, x, iterations, sensitivity, P) of the restatement after `it` fixed steps from x0 = 0, computed once per case"""
    key = ("fixed", tag, csr[2].dtype.name, it, s)
    if key not in _REF:
        P = shadow_space(oracle, len(b), s, b.dtype)
        st, x, k, _ = idrs(oracle, csr, b, np.zeros(len(b), dtype=b.dtype), it, 0.0, s, P, apply=apply)
        _REF[key] = (st, x, k, sensitivity(oracle, csr, b, it, s, P, x, apply), P)
    return _REF[key]


def near_breakdown(oracle, jacobi):
    """convdiff3d(32, 0.3) in fp32, s = 4, eps = NEAR_EPS: (csr, b, P, diag or None, iterations of the restatement, iterations under the
    three perturbed b); the restatement takes seconds, so once per session"""
    key = ("near", bool(jacobi))
    if key not in _REF:
        dtype, s, eps = np.float32, 4, NEAR_EPS[bool(jacobi)]
        csr = gen.convdiff3d(32, 0.3, dtype=dtype)
        b = gen.row_sums(csr[0], csr[2])
        P = shadow_space(oracle, len(b), s, dtype)
        diag = None
        apply = None
        if jacobi:
            err, diag = oracle.jacobi_setup(csr)
            assert err == 0
            apply = lambda v: oracle.jacobi_apply(diag, np.ascontiguousarray(v))  # noqa: E731
        zero = np.zeros(len(b), dtype=dtype)
        st, x, it, _ = idrs(oracle, csr, b, zero, -1, eps, s, P, apply=apply)
        assert st == 0 and np.isfinite(x).all()
        moved = [idrs(oracle, csr, perturbed(b, seed), zero, -1, eps, s, P, apply=apply)[2] for seed in range(3)]
        _REF[key] = (csr, b, P, diag, it, moved)
    return _REF[key]


def build_case(tmp_path):
    """the g++ line of tests/gmres_helpers.py for tests/cpp/idrs_case.cpp"""
    exe = tmp_path / "idrs_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe
