"""tests/cpp/longrows_case.cpp: configureLongRows / longRowsInfo / setSpmvKernel(SMM_SPMV_LONGROWS) / rMult through the drop-in header,
compiled with -Wall -Werror.  Without a GPU the calls report SMM_HIP_ERR_NO_DEVICE; on a GPU the three rows past 64 entries are cut into
9 segments and the integer product equals the case's own host loop bit for bit."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "longrows_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_blocks.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "longrows_case"
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
    assert len(y) == 6 and y[2] == 0.0 and all(v == int(v) for v in y)
    if os.path.exists("/dev/kfd"):
        assert (head["cfg"], head["set"], head["equal"]) == ("0", "0", "1"), words
    else:
        assert (head["cfg"], head["set"]) == ("-3", "-3"), words  # SMM_HIP_ERR_NO_DEVICE


@pytest.mark.gpu
def test_case_on_the_gpu(tmp_path):
    head, _, words = run_case(tmp_path)
    assert (head["cfg"], head["set"], head["equal"], head["hip"]) == ("0", "0", "1", "0"), words
    assert head["bad"] == "-1", words  # SMM_HIP_ERR_INVALID: 100 is no multiple of 64
    assert (head["split"], head["seg"], head["long"], head["segs"]) == ("64", "64", "3", "9"), words  # rows of 200, 65, 130: 4 + 2 + 3
