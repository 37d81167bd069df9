"""tests/cpp/lobpcg_gen_case.cpp: SMM::lobpcg(A, B, ...) -- the generalised problem A x = lambda B x -- for float and double through the
drop-in header, without a preconditioner, with the IC0 of A, and with B = A.  It compiles with -Wall -Werror and links against the
library everywhere; without a GPU every call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it, on a GPU the two smallest analytic
eigenvalues of the chain of 60 linear elements come back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "lobpcg_gen_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_eigsh.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "lobpcg_gen_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_case(tmp_path):
    r = subprocess.run([str(build_case(tmp_path))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double", "double_ic0", "double_same"}
    return lines


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """as tests/test_cpp_eigsh.py does it: SUCCESS where there is a GPU, DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it where there is none"""
    for words in run_case(tmp_path).values():
        assert (int(words[2]), int(words[4])) == ((0, 0) if os.path.exists("/dev/kfd") else (1, -3)), words


@pytest.mark.gpu
def test_cpp_case_on_the_gpu(tmp_path):
    c = np.cos(np.arange(1, 61) * np.pi / 61)
    lam = 6.0 * (1.0 - c) / (2.0 + c)  # ascending
    norm = float(lam[-1])
    lines = run_case(tmp_path)
    for name, words in lines.items():
        tol = 1e-4 if name == "float" else 1e-10
        assert (int(words[2]), int(words[4]), int(words[6])) == (0, 0, 2), words
        got = [float.fromhex(v) for v in words[14:16]]
        if name == "double_same":  # B = A: every eigenvalue is 1, at iteration 0, after the start's 2k - 1 products with B
            assert max(abs(g - 1.0) for g in got) <= 4 * np.finfo(np.float64).eps and int(words[8]) == 0 and int(words[12]) == 3
            continue
        assert max(abs(g - e) for g, e in zip(got, lam[:2])) <= 10 * tol * norm
        assert float.fromhex(words[17]) <= 10 * tol * norm  # max ||A x - theta B x|| / ||B x||, formed by the case itself in double
        assert 0 < int(words[8]) <= 1000 and int(words[12]) > 3
    assert int(lines["double"][10]) == 0 and int(lines["double_ic0"][10]) > 0
    assert int(lines["double_ic0"][8]) < int(lines["double"][8])  # the IC0 of A cuts the iteration count
