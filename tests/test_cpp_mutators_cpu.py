"""CSRMatrix's value mutators through the drop-in C++ header (include/smm_hip/sparse_matrix_math.h): operator*=, inplaceAdd /
inplaceSubtract, updateEntry / addEntry, zeroValues, hasSameNonZeroPattern and the writable iterators.  tests/cpp/mutators_case.cpp
is written against the reference's API only; here it is compiled with g++ against the drop-in header and run without a device mirror
(the host path, no GPU needed), and -- where the reference is mounted -- also against the real reference header: the two printouts
(every value as %a) must be identical.  The GPU half (edits through the device mirror) is in tests/test_gpu_csr_update.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "mutators_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
REFERENCE = "/root/reference/include/sparse_matrix_math.h"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build_dropin(tmp_path):
    exe = tmp_path / "mutators_dropin"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(exe, mirror=False):
    env = dict(os.environ, SMM_CASE_MIRROR="1" if mirror else "0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def dropin_output(tmp_path_factory):
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    return run(build_dropin(tmp_path_factory.mktemp("mutators")))[0]


def section(out, dtype):
    return out.split(f"== {dtype}\n")[1].split("== ")[0].splitlines()


def entries(text):
    """'step: (r,c)=v ...' -> ['(r,c)', 'v'] pairs"""
    return [e.split("=") for e in text.split(": ", 1)[1].split()] if ": " in text else []


def line(lines, prefix):
    found = [ln for ln in lines if ln.startswith(prefix)]
    assert found, prefix
    return found[0]


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_host_path_semantics(dropin_output, dtype):
    """what the reference's mutators do, checked on the printout itself"""
    lines = section(dropin_output, dtype)
    assert line(lines, "same a b") == "same a b 1, a c 0, a a 1"
    assert line(lines, "update (1,2)") == "update (1,2) 1"
    assert line(lines, "update (0,2)") == "update (0,2) 0"  # not stored: nothing changes
    assert line(lines, "update (3,3)") == "update (3,3) 0"  # empty row
    assert line(lines, "update (4,4)") == "update (4,4) 1, again 1"
    assert line(lines, "add (2,2)") == "add (2,2) 0"
    assert "(4,4)=0x1.9p+2" in line(lines, "updated:")  # the last of two updates of one entry stays: 6.25
    assert "(1,2)=0x1.7p+3" in line(lines, "updated:")  # 11.5
    assert line(lines, "row 3 empty") == "row 3 empty 1"
    assert line(lines, "row 3:") == "row 3:"
    zeroed = entries(line(lines, "zeroed:"))
    assert len(zeroed) == 10 and all(v == "0x0p+0" for _, v in zeroed)  # +0, no sign
    # zero - b is -b, entry for entry; b itself is untouched by every edit of a
    neg = [v for _, v in entries(line(lines, "zero minus b:"))]
    b = [v for _, v in entries(line(lines, "b untouched:").split(": ", 1)[1])]
    assert neg == [(x[1:] if x.startswith("-") else "-" + x) for x in b]
    # added then subtracted: back to the scaled values except where the two roundings differ; added to itself doubles each value
    scaled = entries(line(lines, "scaled:"))
    doubled = entries(line(lines, "added to itself:"))
    sub = entries(line(lines, "subtracted:"))
    assert [float.fromhex(d[1]) for d in doubled] == [2 * float.fromhex(s[1]) for s in sub]
    assert [s[0] for s in scaled] == [d[0] for d in doubled]
    assert line(lines, "empty update") == "empty update 0, same 1"
    assert line(lines, "empty:") == "empty:"


def test_matches_the_reference_header(dropin_output, tmp_path):
    if not os.path.exists(REFERENCE):
        pytest.skip("the reference header is not mounted here")
    if not os.path.exists(CLANG):
        pytest.skip("needs clang++")
    exe = tmp_path / "mutators_reference"
    cmd = [CLANG, "-std=c++17", "-O1", "-fdelayed-template-parsing", "-ffp-contract=off", "-w", f"-I{os.path.dirname(REFERENCE)}", CASE, "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    ref_out = run(exe)[0]
    assert dropin_output.splitlines() == ref_out.splitlines()
