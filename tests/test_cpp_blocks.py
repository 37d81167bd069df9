"""tests/cpp/blocks_case.cpp: findBlocks / blocksInfo / setSpmvKernel(SMM_SPMV_BLOCKS) / rMult through the drop-in header, compiled
with -Wall -Werror.  Without a GPU the calls report SMM_HIP_ERR_NO_DEVICE; on a GPU the b = 2 matrix is found, served by the BLOCKS
family and multiplied to the bits of STREAM at one lane per row."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "blocks_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cgs_cpu.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "blocks_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_case(tmp_path):
    r = subprocess.run([str(build_case(tmp_path))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    words = lines[0].split()
    return dict(zip(words[0::2], words[1::2])), [float.fromhex(ln.split()[1]) for ln in lines[1:]], words


def test_case_compiles_against_the_dropin_header(tmp_path):
    head, y, words = run_case(tmp_path)
    assert len(y) == 12
    if os.path.exists("/dev/kfd"):
        assert (head["found"], head["set"], head["equal"]) == ("2", "0", "1"), words
    else:
        assert (head["found"], head["set"]) == ("-1", "-3"), words  # SMM_HIP_ERR_NO_DEVICE


@pytest.mark.gpu
def test_case_on_the_gpu(tmp_path):
    head, y, words = run_case(tmp_path)
    assert (head["found"], head["size"], head["set"], head["equal"], head["hip"]) == ("2", "2", "0", "1", "0"), words
    assert words[3] == words[5] == "18" and int(head["cap"]) >= 256, words  # "blocks 18 of 18"
    # the same product on the host
    n, A = 12, np.zeros((12, 12))
    for R in range(6):
        for c in (R, (R + 1) % 6, (R + 3) % 6):
            for i in range(2):
                for j in range(2):
                    A[R * 2 + i, c * 2 + j] = 0.1 + 0.37 * (R * 2 + i) - 0.21 * (c * 2 + j) + (3.0 if i == j else 0.0)
    np.testing.assert_allclose(y, A @ (1.0 / (np.arange(n) + 3)), rtol=1e-13)
