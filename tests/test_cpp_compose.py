"""tests/cpp/compose_case.cpp: SMM::blockMatrix / blockRefresh / submatrix / submatrixRefresh / diagonal and CSRMatrix::scaleRowsCols through
the drop-in header, compiled with -Wall -Werror by the g++ line of tests/test_cpp_longrows.py.  Without a GPU every call reports
SMM_HIP_ERR_NO_DEVICE; on a GPU the (1,1) block cut out of K = [[H, Bt], [B, 0]] has H's pattern and H's value bits."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "compose_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
CALLS = ("transpose", "block", "sub", "range", "scale", "refresh")


def run_case(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "compose_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    return dict(zip(words[0::2], words[1::2])), words


def test_case_compiles_against_the_dropin_header(tmp_path):
    head, words = run_case(tmp_path)
    if os.path.exists("/dev/kfd"):
        assert all(head[k] == "0" for k in CALLS) and (head["pattern"], head["values"]) == ("1", "1"), words
    else:
        assert all(head[k] == "-3" for k in CALLS), words  # SMM_HIP_ERR_NO_DEVICE
        assert (head["pattern"], head["values"], head["diag"], head["scaled"], head["refreshed"]) == ("0", "0", "0", "0", "0"), words


@pytest.mark.gpu
def test_case_on_the_gpu(tmp_path):
    head, words = run_case(tmp_path)
    assert all(head[k] == "0" for k in CALLS) and head["hip"] == "0", words
    assert (head["pattern"], head["values"]) == ("1", "1"), words  # the (1,1) block cut back out of K is H
    assert (head["diag"], head["missing"]) == ("1", "20"), words  # 4 on H's rows, nothing stored on the zero block's
    assert (head["scaled"], head["refreshed"]) == ("1", "1"), words
