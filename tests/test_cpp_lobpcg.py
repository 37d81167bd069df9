"""tests/cpp/lobpcg_case.cpp: SMM::lobpcg<float> / <double> through the drop-in header, without a preconditioner and with IC0.  It
compiles with -Wall -Werror and links against the library everywhere; without a GPU every call reports DIVERGED with
SMM_HIP_ERR_NO_DEVICE beside it, on a GPU the four smallest eigenvalues of the 16 x 12 grid Laplacian come back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "lobpcg_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_eigsh.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "lobpcg_case"
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
    assert set(lines) == {"float", "double", "double_ic0"}
    return lines


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """as tests/test_cpp_eigsh.py does it: SUCCESS where there is a GPU, DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it where there is none"""
    for words in run_case(tmp_path).values():
        assert (int(words[2]), int(words[4])) == ((0, 0) if os.path.exists("/dev/kfd") else (1, -3)), words


@pytest.mark.gpu
def test_cpp_case_on_the_gpu(tmp_path):
    lam = np.sort([4 - 2 * np.cos(i * np.pi / 17) - 2 * np.cos(j * np.pi / 13) for i in range(1, 17) for j in range(1, 13)])
    norm_a = float(lam[-1])
    lines = run_case(tmp_path)
    for name, words in lines.items():
        tol = 1e-4 if name == "float" else 1e-10
        assert (int(words[2]), int(words[4]), int(words[6])) == (0, 0, 4), words
        got = [float.fromhex(v) for v in words[12:16]]
        assert max(abs(g - e) for g, e in zip(got, lam[:4])) <= 10 * tol * norm_a
        assert float.fromhex(words[17]) <= 10 * tol * norm_a  # max ||A x - theta x||, formed by the case itself in double
        assert 0 < int(words[8]) <= 1000
    assert int(lines["double"][10]) == 0 and int(lines["double_ic0"][10]) > 0
    assert int(lines["double_ic0"][8]) < int(lines["double"][8])  # IC0 cuts the iteration count
