"""MINRES without a GPU: the test matrices are what tests/minres_cases.py says they are, the CPU restatement
(tests/minres_restatement.py, the definition the GPU loop is compared with) converges on them with a residual norm that never grows, an
exact solve of the unshifted operator as preconditioner saves steps, every fixed-pass case of tests/test_gpu_minres.py is well enough
conditioned to be compared, the new symbols are declared and exported, and tests/cpp/minres_case.cpp compiles against the drop-in
header with -Wall -Werror."""
import os
import re
import shutil
import subprocess

import minres_cases as cases
import numpy as np
import pytest
from minres_restatement import kernel_dot, minres, sensitivity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "minres_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
DTYPES = [np.float32, np.float64]
FIXED_ITS = (1, 3, 10)
SENSITIVITY_CAP = 1e-2  # of max(1, max|x_ref|): the cap of the fixed-pass rule (tests/test_gpu_cgs.py `allowed`)


def build_case(tmp_path):
    """the g++ line of tests/test_cgs_cpu.py"""
    exe = tmp_path / "minres_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def exact_apply(name):
    """M^-1 of the unshifted operator as a dense symmetric matrix: the best case an IC0 or AMG of it approaches"""
    inv = np.linalg.inv(cases.dense(cases.unshifted(name)))
    inv = (inv + inv.T) / 2
    return lambda r: inv @ r


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_matrices_are_symmetric_bit_for_bit(name, dtype):
    csr = cases.matrix(name, dtype)
    a = cases.dense(csr)
    assert csr[2].dtype == dtype and np.array_equal(a, a.T)
    start, pos, _ = csr
    assert all(np.all(np.diff(pos[start[r]:start[r + 1]]) > 0) for r in range(len(start) - 1))  # sorted, distinct columns


def test_inertia_and_the_zero_block():
    for name, negative in cases.NEGATIVE.items():
        ev = np.linalg.eigvalsh(cases.dense(cases.matrix(name)))
        assert int((ev < 0).sum()) == negative and int((ev > 0).sum()) == len(ev) - negative, name
    ev = np.linalg.eigvalsh(cases.dense(cases.matrix("shifted2d_16")))
    assert abs(float(np.min(np.abs(ev))) - 0.044) < 1e-3
    ev = np.linalg.eigvalsh(cases.dense(cases.matrix("shifted2d_12")))
    assert (ev < 0).any() and (ev > 0).any()
    assert np.all(np.linalg.eigvalsh(cases.dense(cases.matrix("spd"))) > 0)
    start, pos, _ = cases.matrix("saddle")
    rows = len(start) - 1
    assert rows == 168
    stored = [r in pos[start[r]:start[r + 1]] for r in range(rows)]
    assert all(stored[:144]) and not any(stored[144:])  # the (2,2) block is zero and not stored
    b = cases.dense(cases.matrix("saddle"))[144:, :144]
    assert np.linalg.matrix_rank(b) == 24 and np.all((b != 0).sum(axis=1) == 2) and np.all((b != 0).sum(axis=0) <= 1)


def test_kernel_dot_is_a_dot():
    """the partitioned sum against an accurate one, at lengths on both sides of a pack, a wave, a workgroup and a trip"""
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        for n in (1, 3, 64, 255, 257, 1024, 2049, 4099, 9001):
            a = rng.uniform(-1, 1, n).astype(dtype)
            b = rng.uniform(-1, 1, n).astype(dtype)
            exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
            bound = np.finfo(dtype).eps * float(np.dot(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64))) * 32
            for grid in (2048, max(1, min((n + 255) // 256, 2048))):
                assert abs(float(kernel_dot(a, b, grid)) - exact) <= bound, (dtype, n, grid)


@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_converges_and_phibar_never_grows(oracle, name):
    eps = 1e-8
    csr, b = cases.matrix(name), cases.rhs(name)
    history = []
    st, x, it, res = minres(oracle, csr, b, np.zeros(len(b)), -1, eps, history=history)
    r = b - cases.dense(csr) @ x
    rel = float(np.linalg.norm(r) / np.linalg.norm(b))
    print(name, "steps", it, "phibar^2", float(res), "true |r|", float(np.linalg.norm(r)), "relative", rel)
    assert st == 0 and 0 < it < len(b) and res <= eps * eps
    assert rel < 1e-7
    assert float(np.linalg.norm(r)) <= 10 * eps  # the condition tests/test_gpu_minres.py puts on the GPU's answer, met with room
    assert len(history) == it + 1 and all(history[k + 1] <= history[k] for k in range(it))


@pytest.mark.parametrize("name", cases.INDEFINITE)
def test_restatement_fp32_meets_the_gpu_test_conditions(oracle, name):
    eps = 1e-3
    csr, b = cases.matrix(name, np.float32), cases.rhs(name, np.float32)
    st, x, it, res = minres(oracle, csr, b, np.zeros(len(b), dtype=np.float32), -1, eps)
    r = b.astype(np.float64) - cases.dense(csr) @ x.astype(np.float64)
    print(name, "steps", it, "true |r|", float(np.linalg.norm(r)))
    assert st == 0 and float(np.linalg.norm(r)) <= 100 * eps


@pytest.mark.parametrize("name", ["shifted2d_16", "shifted2d_12"])
def test_exact_preconditioner_of_the_unshifted_operator_saves_steps(oracle, name):
    eps = 1e-8
    csr, b = cases.matrix(name), cases.rhs(name)
    zero = np.zeros(len(b))
    st0, _, plain, _ = minres(oracle, csr, b, zero, -1, eps)
    history = []
    st1, x, with_m, _ = minres(oracle, csr, b, zero, -1, eps, apply=exact_apply(name), history=history)
    print(name, "steps without / with M", plain, with_m, "true |r|", float(np.linalg.norm(b - cases.dense(csr) @ x)))
    assert st0 == st1 == 0 and with_m < plain
    assert all(history[k + 1] <= history[k] for k in range(with_m))
    assert float(np.linalg.norm(b - cases.dense(csr) @ x)) <= 1e-6 * float(np.linalg.norm(b))


def test_a_negative_definite_preconditioner_diverges_at_once(oracle):
    csr, b = cases.matrix("shifted2d_12"), cases.rhs("shifted2d_12")
    st, x, it, _ = minres(oracle, csr, b, np.zeros(len(b)), -1, 1e-8, apply=lambda r: -r)
    assert (st, it) == (1, 0) and not x.any()


def test_edges_of_the_restatement(oracle):
    csr, b = cases.matrix("shifted2d_12"), cases.rhs("shifted2d_12")
    zero = np.zeros(len(b))
    assert minres(oracle, csr, b, zero, 0, 1e-8)[::2] == (2, 0)
    st, x, it, res = minres(oracle, csr, b, zero, 5, 0.0)
    assert (st, it) == (2, 5) and res > 0  # phibar^2 > eps^2 = 0: MAX_ITERATIONS_REACHED by the status rule, at every fixed pass count
    xs = np.linalg.solve(cases.dense(csr), b)
    bb = oracle.spmv(csr, 0, None, xs)  # b := A xs in the oracle's arithmetic, so that xs is an exact start
    st, x, it, res = minres(oracle, csr, bb, xs, -1, 0.0)
    assert (st, it, float(res)) == (0, 0, 0.0) and np.array_equal(x, xs)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_fixed_pass_cases_are_well_conditioned(oracle, name, dtype):
    """the sensitivity of every fixed-pass case of the GPU test stays under the cap of its tolerance rule"""
    csr, b = cases.matrix(name, dtype), cases.rhs(name, dtype)
    for it in FIXED_ITS:
        st, x, k, _ = minres(oracle, csr, b, np.zeros(len(b), dtype=dtype), it, 0.0)
        sens = sensitivity(oracle, csr, b, it, x)
        scale = max(1.0, float(np.max(np.abs(x))))
        print(name, np.dtype(dtype).name, it, "sensitivity", sens, "scale", scale)
        assert k == it and st == 2
        assert sens <= SENSITIVITY_CAP * scale


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    names = [f"smm_hip_minres_{suf}" for suf in ("f32", "f64", "dev_f32", "dev_f64")]
    for name in names:
        assert re.search(r"\bint " + name + r"\(const smm_hip_csr\* a,", header), name
    so = os.path.join(LIB, "libsmm_hip.so")
    if not os.path.exists(so):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, timeout=120).stdout
    for name in names:
        assert re.search(r" T " + name + r"$", exported, re.M), name
    import sparse_matrix_math_amd as smm

    assert callable(smm.MINRES) and callable(smm.minres_dev)
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus MINRES(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps)" in drop_in


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::MINRES<float> / <double> (two function pointers in the case) and the preconditioned overload; -Wall -Werror.  Without a GPU the
    call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"float", "double"}
    for name, words in lines.items():
        status, hip = int(words[2]), int(words[4])
        if os.path.exists("/dev/kfd"):
            assert (status, hip) == (0, 0), words
            x = [float.fromhex(w) for w in words[6:9]]
            np.testing.assert_allclose(x, 1.0, rtol=1e-4 if name == "float" else 1e-6)
        else:
            assert (status, hip) == (1, -3), words
