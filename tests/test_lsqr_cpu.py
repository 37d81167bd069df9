"""LSQR without a GPU: the test matrices are what tests/lsqr_cases.py says they are; the CPU restatement (tests/lsqr_restatement.py, the
definition the GPU loop is compared with) reaches numpy.linalg.lstsq's answer on every one of them in fp64 -- the minimum-norm one where
there is a choice -- and solve(AtA + damp^2 I, At b) with damping, in the recorded number of steps; its two estimates follow the true
quantities and the residual one never grows; damp == 0 makes the first rotation the identity bit for bit; every fixed-pass case of
tests/test_gpu_lsqr.py is well enough conditioned to be compared; the new symbols are declared and exported; tests/cpp/lsqr_case.cpp
compiles against the drop-in header with -Wall -Werror.

Every case's error against lstsq is printed: it is the yardstick of the converged runs in tests/test_gpu_lsqr.py."""
import os
import re
import shutil
import subprocess

import lsqr_cases as cases
import numpy as np
import pytest
from lsqr_restatement import lsqr, rotations, sensitivity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "lsqr_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
DAMPS = [0.0, cases.DAMP]
FIXED_ITS = (1, 3, 10)
SENSITIVITY_CAP = 1e-2  # of max(1, max|x_ref|): the cap of the fixed-pass rule (tests/test_gpu_cgs.py `allowed`)

_SOLVED = {}


def build_case(tmp_path):
    """the g++ line of tests/test_cpp_eigsh.py"""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = tmp_path / "lsqr_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def system(name, dtype):
    """(csr, csr of the transpose, b, cols)"""
    rows, cols, csr = cases.matrix(name, dtype)
    return csr, cases.transposed(csr, cols), cases.rhs(name, dtype), cols


def solved(oracle, name, dtype, damp):
    """the restatement from x0 = 0 to EPS[dtype], once per case: (status, x, iterations, reason, res, arn, history)"""
    key = (name, np.dtype(dtype).name, damp)
    if key not in _SOLVED:
        csr, csr_t, b, cols = system(name, dtype)
        history = []
        _SOLVED[key] = lsqr(oracle, csr, csr_t, b, np.zeros(cols, dtype=dtype), -1, cases.EPS[dtype], damp, history) + (history,)
    return _SOLVED[key]


def answer(name, dtype, damp):
    return cases.lstsq(name, dtype) if damp == 0 else cases.damped(name, damp, dtype)


@pytest.mark.parametrize("name", cases.NAMES)
def test_matrices_are_what_the_cases_say(name):
    rows, cols, csr = cases.matrix(name)
    start, pos, val = csr
    a = cases.dense(csr, cols)
    assert (rows, cols) == cases.SHAPE[name] == a.shape and len(start) == rows + 1
    assert all(np.all(np.diff(pos[start[r]:start[r + 1]]) > 0) for r in range(rows))  # sorted, distinct columns
    assert np.linalg.matrix_rank(a) == cases.RANK[name]
    t = cases.transposed(csr, cols)
    assert np.array_equal(cases.dense(t, rows), a.T) and len(t[1]) == len(pos)
    for dtype in DTYPES:
        assert cases.matrix(name, dtype)[2][2].dtype == dtype
    if name == "tall":
        assert abs(np.linalg.cond(a) - 43) < 1
        assert np.array_equal(a.T, cases.dense(cases.matrix("wide")[2], rows))
    if name == "grad2d_12":
        assert not (a @ np.ones(cols)).any()  # the constants are the null space
    if name == "sparse_random":
        lens = np.diff(start)
        assert lens[cases.EMPTY_ROW] == 0 and not (pos == cases.EMPTY_COL).any() and abs(len(pos) / (rows * cols) - 0.05) < 0.01
    if name == "convdiff2d_12":
        assert not np.array_equal(a, a.T)
    # consistent or not, as the cases say
    b = cases.rhs(name)
    r = b - a @ cases.lstsq(name)
    assert (np.linalg.norm(r) < 1e-10) == (name in cases.CONSISTENT)


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_reaches_the_least_squares_answer_fp64(oracle, name, damp):
    dtype = np.float64
    eps = cases.EPS[dtype]
    csr, csr_t, b, cols = system(name, dtype)
    st, x, it, reason, res, arn, history = solved(oracle, name, dtype, damp)
    ref = answer(name, dtype, damp)
    a = cases.dense(csr, cols)
    r = b - a @ x
    true_res = float(r @ r + damp * damp * (x @ x))
    true_ar = float(np.linalg.norm(a.T @ r - damp * damp * x))
    err = float(np.max(np.abs(x - ref)))
    print(name, "damp", damp, "steps", it, "reason", reason, "res", float(res), "true", true_res, "arn", float(arn), "true |At r|", true_ar, "max|x - lstsq|", err)
    assert (st, reason) == (0, cases.STEPS[damp][name][0][1]) and 0 < it < cols
    assert it == cases.STEPS[damp][name][0][0]
    assert err <= 1e-8 * max(1.0, float(np.max(np.abs(ref))))
    assert true_ar <= 10 * eps  # the condition tests/test_gpu_lsqr.py puts on the GPU's answer, met with room
    assert abs(float(res) - true_res) <= 1e-10 * max(1.0, true_res)
    assert len(history) == it + 1 and all(history[k + 1][0] <= history[k][0] for k in range(it))
    if damp == 0 and cases.RANK[name] < cols:  # the minimum-norm answer: nothing of the null space
        null = np.linalg.svd(a)[2][cases.RANK[name]:]
        assert float(np.max(np.abs(null @ x))) <= 1e-8
    if name == "sparse_random":
        assert x[cases.EMPTY_COL] == 0.0


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_fp32_meets_the_gpu_test_conditions(oracle, name, damp):
    dtype = np.float32
    eps = cases.EPS[dtype]
    csr, csr_t, b, cols = system(name, dtype)
    st, x, it, reason, res, arn, _ = solved(oracle, name, dtype, damp)
    ref = answer(name, dtype, damp)
    a = cases.dense(csr, cols)
    x64 = x.astype(np.float64)
    r = b.astype(np.float64) - a @ x64
    true_ar = float(np.linalg.norm(a.T @ r - damp * damp * x64))
    err = float(np.max(np.abs(x64 - ref)))
    print(name, "damp", damp, "steps", it, "reason", reason, "true |At r|", true_ar, "max|x - lstsq|", err)
    assert (st, it, reason) == (0,) + cases.STEPS[damp][name][1] and it < cols
    assert true_ar <= 100 * eps
    assert err <= 1e-2


def test_zero_damping_makes_the_first_rotation_the_identity():
    """bit for bit: rb1 = rhobar with its sign (sqrt(rhobar^2) would drop it and round), psi = 0, phibar unchanged -- so a run with
    damp = 0 has the scalars of the undamped recurrence, and a tiny damp whose square vanishes beside rhobar^2 does not"""
    rng = np.random.default_rng(11)
    for dtype in DTYPES:
        T = dtype
        for _ in range(200):
            rhobar, phibar, beta, alpha = (T(v) for v in rng.uniform(-2, 2, 4))
            beta, alpha = abs(beta), abs(alpha)
            bb = T(beta * beta)
            rho, c, theta, new_rhobar, phi, new_phibar, psi = rotations(T, T(0), rhobar, phibar, bb, beta, alpha)
            want_rho = T(np.sqrt(T(T(rhobar * rhobar) + bb)))
            want_c = T(rhobar / want_rho)
            assert psi == 0 and not np.signbit(psi)
            assert (rho, c, phi, new_phibar) == (want_rho, want_c, T(want_c * phibar), T(T(beta / want_rho) * phibar))
            assert np.sign(c) == np.sign(rhobar)
            tiny = rotations(T, T(1e-30), rhobar, phibar, bb, beta, alpha)
            assert tiny[0] == rho and abs(tiny[1]) == abs(c) and tiny[1] >= 0  # the general branch takes |rhobar|: the sign moves into phibar


@pytest.mark.parametrize("name", cases.CONSISTENT)
def test_a_nonzero_start_and_what_damping_acts_on(oracle, name):
    """consistent cases: the undamped answer from x0 != 0 solves the system (wide: x0 plus the minimum-norm correction); with damp > 0
    x - x0 is the damped answer of the residual system"""
    dtype = np.float64
    csr, csr_t, b, cols = system(name, dtype)
    a = cases.dense(csr, cols)
    x0 = np.random.default_rng(3).uniform(-1, 1, cols)
    st, x, it, reason, _, _ = lsqr(oracle, csr, csr_t, b, x0, -1, cases.EPS[dtype])
    dx = np.linalg.lstsq(a, b - a @ x0, rcond=1e-10)[0]
    assert (st, reason) == (0, 1) and float(np.max(np.abs(x - (x0 + dx)))) <= 1e-8
    damp = cases.DAMP
    st, x, it, reason, _, _ = lsqr(oracle, csr, csr_t, b, x0, -1, cases.EPS[dtype], damp)
    dx = np.linalg.solve(a.T @ a + damp * damp * np.eye(cols), a.T @ (b - a @ x0))
    assert (st, reason) == (0, 2) and float(np.max(np.abs(x - (x0 + dx)))) <= 1e-8
    assert float(np.max(np.abs(x - cases.damped(name, damp)))) > 1e-3  # (it is NOT x that is damped)


def test_edges_of_the_restatement(oracle):
    dtype = np.float64
    csr, csr_t, b, cols = system("tall", dtype)
    zero = np.zeros(cols)
    st, x, it, reason, res, arn = lsqr(oracle, csr, csr_t, b, zero, 0, 1e-8)
    assert (st, it, reason) == (2, 0, 0) and not x.any() and res == np.dot(b, b) > 0
    st, x, it, reason, res, arn = lsqr(oracle, csr, csr_t, b, zero, 5, 0.0)
    assert (st, it, reason) == (2, 5, 0) and res > 0 and arn > 0
    st, x, it, reason, res, arn = lsqr(oracle, csr, csr_t, np.zeros(len(b)), zero, -1, 1e-8)
    assert (st, it, reason, float(res)) == (0, 0, 1, 0.0) and not x.any()
    # b orthogonal to the range of A: a vector of the null space of At (24 of them; At n = 0 up to rounding, so arn is tiny and eps decides)
    a = cases.dense(csr, cols)
    null = np.linalg.svd(a.T)[2][cols:]
    st, x, it, reason, res, arn = lsqr(oracle, csr, csr_t, null[0], zero, -1, 1e-8)
    assert (st, it, reason) == (0, 0, 2) and not x.any() and abs(float(res) - 1.0) < 1e-12
    # more steps than cols are allowed
    st, x, it, reason, res, arn = lsqr(oracle, csr, csr_t, b, zero, 3 * cols, 0.0)
    assert it > cols and np.isfinite(x).all() and st in (0, 2)
    # no entries: reason 2 at once
    empty = (np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    empty_t = (np.zeros(3, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    st, x, it, reason, res, arn = lsqr(oracle, empty, empty_t, np.ones(3), np.zeros(2), -1, 1e-8)
    assert (st, it, reason, float(res), float(arn)) == (0, 0, 2, 3.0, 0.0)
    # rows == 0 and cols == 0
    assert lsqr(oracle, (np.zeros(1, dtype=np.int32),) + empty[1:], empty_t, np.zeros(0), np.zeros(2), -1, 1e-8)[2:4] == (0, 1)
    assert lsqr(oracle, empty, (np.zeros(1, dtype=np.int32),) + empty[1:], np.ones(3), np.zeros(0), -1, 1e-8)[2:4] == (0, 2)


@pytest.mark.parametrize("damp", DAMPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_fixed_pass_cases_are_well_conditioned(oracle, name, dtype, damp):
    """the sensitivity of every fixed-pass case of the GPU test stays under the cap of its tolerance rule"""
    csr, csr_t, b, cols = system(name, dtype)
    for it in FIXED_ITS:
        st, x, k, reason, _, _ = lsqr(oracle, csr, csr_t, b, np.zeros(cols, dtype=dtype), it, 0.0, damp)
        sens = sensitivity(oracle, csr, csr_t, b, it, damp, x)
        scale = max(1.0, float(np.max(np.abs(x))))
        print(name, np.dtype(dtype).name, "damp", damp, it, "sensitivity", sens, "scale", scale)
        assert (st, k, reason) == (2, it, 0)
        assert sens <= SENSITIVITY_CAP * scale


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    names = [f"smm_hip_lsqr_{suf}" for suf in ("f32", "f64", "dev_f32", "dev_f64")]
    for name in names:
        assert re.search(r"\bint " + name + r"\(const smm_hip_csr\* a, const smm_hip_csr\* at,", header), name
    so = os.path.join(LIB, "libsmm_hip.so")
    if not os.path.exists(so):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    for lib in (so, os.path.join(LIB, "libsmm_hip_fma.so")):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, timeout=120).stdout
        for name in names:
            assert re.search(r" T " + name + r"$", exported, re.M), (lib, name)
    import sparse_matrix_math_amd as smm

    assert callable(smm.LSQR) and callable(smm.lsqr_dev)
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus LSQR(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps," in drop_in


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::LSQR<float> / <double> (two function pointers in the case) with the defaulted arguments; -Wall -Werror.  Without a GPU the call
    reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it; with one, SUCCESS by reason 2 and a small ||At r||."""
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double"}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip, int(words[8])) == (0, 0, 2), words
            assert float.fromhex(words[10]) <= (100 * 1e-3 if name == "float" else 10 * 1e-8)
        else:
            assert (status, hip) == (1, -3), words
