"""tests/cpp/eigsh_case.cpp: SMM::eigsh<float> / <double> through the drop-in header.  It compiles with -Wall -Werror and links against
the library everywhere; without a GPU every call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it, on a GPU the two largest
eigenvalues of the chain of 12 rows come back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "eigsh_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_minres_cpu.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "eigsh_case"
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
    assert set(lines) == {"float", "double"}
    return lines


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """as tests/test_minres_cpu.py does it: SUCCESS where there is a GPU, DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it where there is none"""
    for words in run_case(tmp_path).values():
        assert (int(words[2]), int(words[4])) == ((0, 0) if os.path.exists("/dev/kfd") else (1, -3)), words


@pytest.mark.gpu
def test_cpp_case_on_the_gpu(tmp_path):
    want = [2 - 2 * np.cos(j * np.pi / 13) for j in (12, 11)]
    for name, words in run_case(tmp_path).items():
        tol = 1e-4 if name == "float" else 1e-10
        assert (int(words[2]), int(words[4]), int(words[6])) == (0, 0, 2), words
        got = [float.fromhex(v) for v in words[8:10]]
        assert max(abs(g - e) for g, e in zip(got, want)) <= 10 * tol * 4.0
        assert float.fromhex(words[11]) <= 10 * tol * 4.0  # max ||A x - theta x||, formed by the case itself in double
