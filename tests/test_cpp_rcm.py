"""tests/cpp/rcm_case.cpp: SMM::rcm / SMM::permute / SMM::bandwidth through the drop-in header, compiled with -Wall -Werror.  Without a GPU
the calls report SMM_HIP_ERR_NO_DEVICE; on a GPU the scrambled 6 x 5 grid gets the restatement's ordering and the permuted matrix the
announced bandwidth."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from rcm_restatement import bandwidth, rcm_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "rcm_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_blocks.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "rcm_case"
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
    return dict(zip(words[0::2], words[1::2])), [int(ln.split()[1]) for ln in lines[1:]], words


def scrambled_grid():
    """the matrix of the case: the 5-point Laplacian of a 6 x 5 grid, grid point 7 k mod 30 numbered k"""
    nx, ny, n = 6, 5, 30
    name = np.empty(n, dtype=np.int64)
    name[(7 * np.arange(n)) % n] = np.arange(n)
    dense = np.zeros((n, n))
    for y in range(ny):
        for x in range(nx):
            g = y * nx + x
            dense[name[g], name[g]] = 4.0
            for ok, h in ((x > 0, g - 1), (x < nx - 1, g + 1), (y > 0, g - nx), (y < ny - 1, g + nx)):
                if ok:
                    dense[name[g], name[h]] = -1.0
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum((dense != 0).sum(axis=1), out=start[1:])
    return start, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0]


def test_case_compiles_against_the_dropin_header(tmp_path):
    head, perm, words = run_case(tmp_path)
    if os.path.exists("/dev/kfd"):
        assert (head["rcm"], head["permute"]) == ("0", "0") and len(perm) == 30, words
    else:
        assert (head["rcm"], head["permute"]) == ("-3", "-3") and perm == [], words  # SMM_HIP_ERR_NO_DEVICE


@pytest.mark.gpu
def test_case_on_the_gpu(tmp_path):
    head, perm, words = run_case(tmp_path)
    csr = scrambled_grid()
    want, info = rcm_levels(csr, True)
    assert (head["rcm"], head["permute"], head["hip"]) == ("0", "0", "0"), words
    np.testing.assert_array_equal(perm, want)
    assert (int(head["components"]), int(head["levels"]), int(head["before"]), int(head["after"])) == (info["components"], info["levels"], info["bandwidth_before"],
                                                                                                         info["bandwidth_after"]), words
    assert (int(head["width"]), int(head["offsets"])) == bandwidth(csr, want), words
    assert int(head["after"]) <= 6 < int(head["before"]), words  # back to the grid's own bandwidth or better
