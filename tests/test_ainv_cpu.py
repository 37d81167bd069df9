"""FSAI / SPAI without a GPU: the CPU restatement (tests/ainv_restatement.py, the definition the device code is compared with) is the
factored / least-squares approximate inverse include/smm_hip.h says it is, and lowers the iteration counts of the restated loops; the
public surfaces (Python enum, exported symbols, the drop-in C++ header) exist."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from ainv_cases import TRIDIAGONAL_ROWS, case, dense_of, dense_sum_of
from ainv_restatement import FSAI, SPAI, AinvError, build, make_apply, pattern
from chebyshev_restatement import bicgstab, pcg

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "ainv_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
F64 = np.float64
SYMBOLS = ("smm_hip_precond_create_ainv", "smm_hip_precond_ainv_refresh", "smm_hip_precond_ainv_info", "smm_hip_precond_ainv_matrix")

FSAI_CASES = [("spd5", 1), ("poisson2d_32", 1), ("poisson2d_32", 2), ("poisson2d_32", 3), ("banded_2000", 1), ("ladder", 1), ("descending", 1)] + [
    (f"tridiagonal_{n}", 1) for n in TRIDIAGONAL_ROWS]
SPAI_CASES = [("convdiff3d_12", 1), ("convdiff3d_12", 2), ("convdiff3d_12", 3), ("poisson2d_32", 1), ("poisson2d_32", 2), ("ladder24", 1)] + [(f"tridiagonal_{n}", 1) for n in TRIDIAGONAL_ROWS]

_BUILT = {}


def built(name, kind, power):
    key = (name, kind, power)
    if key not in _BUILT:
        _BUILT[key] = build(case(name, F64), kind, power)
    return _BUILT[key]


def build_case(tmp_path):
    """the g++ line of tests/test_chebyshev_cpu.py for tests/cpp/ainv_case.cpp"""
    exe = tmp_path / "ainv_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("name,power", FSAI_CASES)
def test_fsai_rows_solve_the_local_systems(name, power):
    """every row of G equals numpy.linalg.solve of A[J, J] y = e_last scaled by 1 / sqrt(y_last) to 1e-12 (relative to the row's largest
    entry), and |diag(G A G^T) - 1| <= 8 ulp with the diagonal formed in extended precision from the restatement's G"""
    A = dense_of(case(name, F64))
    start, pos, val = built(name, FSAI, power)
    worst_row, worst_diag = 0.0, 0.0
    for i in range(len(start) - 1):
        J = pos[start[i]:start[i + 1]]
        g = val[start[i]:start[i + 1]]
        assert J[-1] == i and np.all(np.diff(J) > 0)
        e = np.zeros(len(J))
        e[-1] = 1
        sub = np.tril(A[np.ix_(J, J)])
        sub = sub + np.tril(sub, -1).T  # the upper triangle is never read
        y = np.linalg.solve(sub, e)
        ref = y / np.sqrt(y[-1])
        worst_row = max(worst_row, float(np.max(np.abs(g - ref)) / np.max(np.abs(ref))))
        gl = g.astype(np.longdouble)
        worst_diag = max(worst_diag, float(abs(gl @ sub.astype(np.longdouble) @ gl - 1)))
    print(name, power, "rows", worst_row, "diag", worst_diag / np.finfo(F64).eps, "ulp")
    assert worst_row <= 1e-12
    assert worst_diag <= 8 * np.finfo(F64).eps


@pytest.mark.parametrize("name,power", SPAI_CASES)
def test_spai_rows_are_the_least_squares_rows(name, power):
    """every row of M equals numpy.linalg.lstsq of min || m A[J, :] - e_i^T || to 1e-10 relative (power 3, the 63-entry rows: every 37th
    row).  The `descending` case is not here: it stores one entry twice, the product a a^T adds the two up while look() takes the first,
    so its rows are the least-squares rows of no single matrix; the GPU test compares it with the restatement bit for bit."""
    A = dense_sum_of(case(name, F64))
    start, pos, val = built(name, SPAI, power)
    worst = 0.0
    for i in range(0, len(start) - 1, 37 if power == 3 else 1):
        J = pos[start[i]:start[i + 1]]
        rows = A[J, :]
        keep = np.nonzero(np.any(rows != 0, axis=0))[0]  # (columns no row of J touches add nothing but a zero residual)
        e = (keep == i).astype(F64)
        ref = np.linalg.lstsq(rows[:, keep].T, e, rcond=None)[0]
        worst = max(worst, float(np.max(np.abs(val[start[i]:start[i + 1]] - ref)) / np.max(np.abs(ref))))
    print(name, power, worst)
    assert worst <= 1e-10


def test_ladder_row_lengths():
    lengths = [len(j) for j in pattern(case("ladder", F64), FSAI, 1)]
    assert set(lengths) == set(range(1, 65))
    assert max(len(j) for j in pattern(case("ladder24", F64), SPAI, 1)) < 64


def test_row_lengths_on_the_12_cube():
    """the radius-3 octahedron of the 7-point stencil holds 1 + 6 + 18 + 38 = 63 points; radius 4 holds more than 64"""
    csr = case("convdiff3d_12", F64)
    assert max(len(j) for j in pattern(csr, SPAI, 3)) == 63
    with pytest.raises(AinvError) as e:
        pattern(csr, SPAI, 4)
    assert e.value.what == "row too long" and e.value.length > 64


def test_errors_of_the_restatement():
    with pytest.raises(AinvError) as e:
        build(case("negated_row5", F64), FSAI)
    assert e.value.what == "failed row" and e.value.row == 2  # the smallest row whose system holds the negated row
    start, pos, val = case("spd5", F64)
    keep = np.ones(len(pos), dtype=bool)
    keep[start[3] + 1] = False
    s2 = start.copy()
    s2[4:] -= 1
    with pytest.raises(AinvError) as e:
        build((s2, pos[keep], val[keep]), SPAI)
    assert e.value.what == "missing diagonal" and e.value.row == 3


def test_fsai_lowers_the_iteration_count_of_cg(oracle):
    """restated ConjugateGradient on poisson2d_32, b = A 1, eps 1e-8: strictly fewer iterations with FSAI than without, and strictly
    decreasing in the power"""
    csr = case("poisson2d_32", F64)
    b = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(len(b))
    counts = [pcg(oracle, csr, b, zero, -1, 1e-8, lambda r: r.copy())[2]]
    for power in (1, 2, 3):
        st, x, it, _ = pcg(oracle, csr, b, zero, -1, 1e-8, make_apply(oracle, csr, FSAI, power, built("poisson2d_32", FSAI, power)))
        assert st == 0
        np.testing.assert_allclose(x, 1.0, rtol=1e-6)
        counts.append(it)
    print("cg iterations: none, p = 1, 2, 3:", counts)
    assert counts[0] > counts[1] > counts[2] > counts[3]


def test_spai_lowers_the_iteration_count_of_bicgstab(oracle):
    csr = case("convdiff3d_12", F64)
    b = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(len(b))
    counts = [bicgstab(oracle, csr, b, zero, 10000, 1e-8, lambda r: r.copy())[2]]
    for power in (1, 2):
        st, x, it, _ = bicgstab(oracle, csr, b, zero, 10000, 1e-8, make_apply(oracle, csr, SPAI, power, built("convdiff3d_12", SPAI, power)))
        assert st == 0
        np.testing.assert_allclose(x, 1.0, rtol=1e-6)
        counts.append(it)
    print("bicgstab iterations: none, p = 1, 2:", counts)
    assert counts[0] > counts[1] and counts[0] > counts[2]


def test_public_surface():
    """the enum members, the four entry points and their prototypes: what the parent of this feature does not have"""
    assert host.SolverPreconditioner.FSAI == 12 and host.SolverPreconditioner.SPAI == 13
    assert host.SolverPreconditioner["FSAI"].value == 12
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in SYMBOLS:
            assert hasattr(lib, name), (name, fma)
            assert name in _lib.exported_symbols()
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for line in ("#define SMM_PRECOND_FSAI 12", "#define SMM_PRECOND_SPAI 13", "#define SMM_AINV_MAX_ROW 64", "#define SMM_AINV_MAX_POWER 4"):
        assert line in header
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, host.SolverPreconditioner.JACOBI, power=2)  # refused before the handle is touched
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, "FSAI", power=2, degree=3)


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::ApproximateInversePreconditioner<float> / <double> through ConjugateGradient, BiCGStab and GMRES; -Wall -Werror.  Without a GPU
    every call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {f"{t}-{s}" for t in ("float", "double") for s in ("cg", "bicgstab", "gmres")}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip) == (0, 0), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name.startswith("float") else 1e-6)
        else:
            assert (status, hip) == (1, -3), words
