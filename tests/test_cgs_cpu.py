"""ConjugateGradientSquared without a GPU: the CPU restatement (tests/cgs_restatement.py, the definition the GPU loop is compared
with) behaves as ref:2110-2178 with the one repair says, and tests/cpp/cgs_case.cpp -- written against the reference's API, the
README's call shape -- compiles and links against the drop-in header for float and double with -Wall -Werror."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from cgs_restatement import cgs
from test_oracle import gen_matrices

from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "cgs_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_mutators_cpu.py"""
    exe = tmp_path / "cgs_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("mname", ["poisson2d_32", "convdiff3d_12"])
def test_restatement_converges_to_ones(oracle, mname):
    csr = gen_matrices(np.float64)[mname]
    b = gen.row_sums(csr[0], csr[2])
    st, x, it, rr = cgs(oracle, csr, b, np.zeros(len(b)), -1, 1e-6)
    print(mname, "passes", it, "r.r", rr, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == 0 and 0 < it < len(b)
    assert rr <= 1e-6 * 1e-6  # it left by the residual test, not by the pass count
    # |x - 1| <= |A^-1| |r| with |r| <= eps: |A^-1| = 1 / (8 sin^2(pi / 66)) = 55 for the 32 x 32 Laplacian, less for the other matrix
    np.testing.assert_allclose(x, 1.0, rtol=100 * 1e-6)


def test_restatement_max_iterations_zero(oracle):
    """the body always runs once; iterations (1) > maxIterations (0): MAX_ITERATIONS_REACHED (ref:2131, 2172-2176)"""
    csr = gen_matrices(np.float64)["poisson2d_32"]
    b = gen.row_sums(csr[0], csr[2])
    st, x, it, _ = cgs(oracle, csr, b, np.zeros(len(b)), 0, 1e-6)
    assert (st, it) == (2, 1)
    assert np.isfinite(x).all() and np.any(x != 0)


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::ConjugateGradientSquared<float> / <double> with the reference's signature (two function pointers in the case) and the
    README's call shape; -Wall -Werror.  Without a GPU the call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double"}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip) == (0, 0), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name == "float" else 1e-6)
        else:
            assert (status, hip) == (1, -3), words
