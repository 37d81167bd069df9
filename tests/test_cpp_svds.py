"""tests/cpp/svds_case.cpp: SMM::svds<float> / <double> and CSRMatrix::norm2 through the drop-in header, on the `tall` matrix of
tests/svds_cases.py.  It compiles with -Wall -Werror and links against the library everywhere; without a GPU every call reports DIVERGED
with SMM_HIP_ERR_NO_DEVICE beside it, on a GPU the four largest singular triplets come back within the bounds of tests/test_gpu_svds.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import svds_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "svds_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_eigsh.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "svds_case"
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
    """SUCCESS where there is a GPU, DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it where there is none"""
    for words in run_case(tmp_path).values():
        assert (int(words[2]), int(words[4])) == ((0, 0) if os.path.exists("/dev/kfd") else (1, -3)), words


@pytest.mark.gpu
def test_cpp_case_on_the_gpu(tmp_path):
    sigma = cases.exact("tall")
    k, ncv = 4, 20
    for name, words in run_case(tmp_path).items():
        dtype = np.dtype(np.float32 if name == "float" else np.float64)
        tol, eps = cases.TOL[dtype], float(np.finfo(dtype).eps)
        bound = 10 * tol * float(sigma[0])
        assert (int(words[2]), int(words[4]), int(words[6])) == (0, 0, k), words
        restarts, matvecs = int(words[8]), int(words[10])
        assert 0 < restarts <= cases.MAX_RESTARTS and matvecs == 2 * (ncv + restarts * (ncv - (k + (ncv - k) // 2)))
        got = np.array([float.fromhex(v) for v in words[12:16]])
        assert float(np.max(np.abs(got - sigma[:k]))) <= bound and np.all(np.diff(got) < 0)
        assert float.fromhex(words[17]) <= bound  # the triplets' residuals, formed by the case itself in double
        assert float.fromhex(words[19]) <= 4 * cases.ORTH_LOSS_EPS[dtype] * eps
        assert abs(float.fromhex(words[21]) - float(sigma[0])) <= bound  # norm2()
