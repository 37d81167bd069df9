"""MINRES on the GPU (csrc/smm_solvers_minres.hip) through the C ABI, against the CPU restatement of the loop that include/smm_hip.h
states (tests/minres_restatement.py): fixed passes, converged runs, the residual norm that never grows, the same bits twice,
preconditioners built on the unshifted operator, the refusals, the edges, every SpMV family, the device-pointer form on offset views,
the fma flavour and the drop-in C++ header.  The matrices are those of tests/minres_cases.py.

A fixed-pass run (eps = 0) stops at the pass limit with phibar^2 > eps^2, which the status rule of the contract calls
MAX_ITERATIONS_REACHED: that is what these tests expect of it, and what the restatement returns."""
import ctypes
import subprocess

import minres_cases as cases
import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from minres_restatement import minres, perturbed, sensitivity
from test_gpu_solvers import RTOL
from test_minres_cpu import build_case

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
SUCCESS, DIVERGED, MAX_ITERATIONS_REACHED = 0, 1, 2
CONVERGED = ("shifted2d_16", "shifted2d_16b", "shifted2d_12", "saddle")
EPS = {np.float64: 1e-8, np.float32: 1e-3}

_REF = {}


def system(name, dtype):
    key = ("system", name, np.dtype(dtype).name)
    if key not in _REF:
        _REF[key] = (cases.matrix(name, dtype), cases.rhs(name, dtype))
    return _REF[key]


def reference(oracle, tag, csr, b, it, apply=None):
    """(status, x, iterations, sensitivity) of the restatement after `it` fixed passes from x0 = 0, computed once per case"""
    key = ("fixed", tag, csr[2].dtype.name, it)
    if key not in _REF:
        st, x, k, _ = minres(oracle, csr, b, np.zeros(len(b), dtype=b.dtype), it, 0.0, apply)
        _REF[key] = (st, x, k, sensitivity(oracle, csr, b, it, x, apply))
    return _REF[key]


def converged(oracle, name, dtype):
    key = ("converged", name, np.dtype(dtype).name)
    if key not in _REF:
        csr, b = system(name, dtype)
        _REF[key] = minres(oracle, csr, b, np.zeros(len(b), dtype=dtype), -1, EPS[dtype])
    return _REF[key]


def allowed(x_ref, sens, dtype):
    """the tolerance rule of tests/test_gpu_cgs.py"""
    scale = max(1.0, float(np.max(np.abs(x_ref))))
    assert sens <= 1e-2 * scale, ("the restatement itself is too sensitive for this case", sens, scale)
    return max(RTOL[dtype] * scale, 4 * sens)


def make(smm, csr):
    rows = len(csr[0]) - 1
    return smm.CSRMatrix(rows, rows, *csr)


def worst(x, ref):
    return float(np.max(np.abs(x.astype(np.float64) - ref.astype(np.float64))))


def true_residual(csr, b, x):
    return float(np.linalg.norm(b.astype(np.float64) - cases.dense(csr) @ x.astype(np.float64)))


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("it", [1, 3, 10])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", cases.NAMES)
def test_fixed_passes_match_the_restatement(smm, oracle, name, dtype, it):
    csr, b = system(name, dtype)
    st_ref, x_ref, it_ref, sens = reference(oracle, name, csr, b, it)
    tol = allowed(x_ref, sens, dtype)
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.MINRES(make(smm, csr), b.copy(), x, it, 0.0, info=info)
    err = worst(x, x_ref)
    print(name, np.dtype(dtype).name, it, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert info["iterations"] == it_ref == it
    assert int(st) == st_ref == MAX_ITERATIONS_REACHED
    assert err <= tol
    assert info["resnorm2"] > 0


@pytest.mark.parametrize("name", CONVERGED)
def test_converged_fp64(smm, oracle, name):
    eps = EPS[np.float64]
    csr, b = system(name, np.float64)
    st_ref, _, it_ref, _ = converged(oracle, name, np.float64)
    x = np.zeros(len(b))
    info = {}
    st = smm.MINRES(make(smm, csr), b.copy(), x, -1, eps, info=info)
    res = true_residual(csr, b, x)
    print(name, "passes", info["iterations"], "restatement", it_ref, "true |r|", res, "phibar^2", info["resnorm2"])
    assert int(st) == st_ref == SUCCESS
    assert res <= 10 * eps
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    assert info["resnorm2"] <= eps * eps


@pytest.mark.parametrize("name", CONVERGED)
def test_converged_fp32(smm, oracle, name):
    """the pass count must lie inside the range of the restatement's unperturbed and three perturbed runs, widened by max(2, it_ref // 5)"""
    eps = EPS[np.float32]
    csr, b = system(name, np.float32)
    zero = np.zeros(len(b), dtype=np.float32)
    st_ref, _, it_ref, _ = converged(oracle, name, np.float32)
    counts = [it_ref] + [minres(oracle, csr, perturbed(b, seed), zero, -1, eps)[2] for seed in range(3)]
    x = zero.copy()
    info = {}
    st = smm.MINRES(make(smm, csr), b.copy(), x, -1, eps, info=info)
    res = true_residual(csr, b, x)
    print(name, "passes", info["iterations"], "restatement", counts, "true |r|", res)
    assert int(st) == st_ref == SUCCESS
    assert res <= 100 * eps
    slack = max(2, it_ref // 5)
    assert min(counts) - slack <= info["iterations"] <= max(counts) + slack, (info, counts)


def test_the_residual_never_grows(smm):
    csr, b = system("shifted2d_16", np.float64)
    A = make(smm, csr)
    seen = []
    for k in range(1, 13):
        x = np.zeros(len(b))
        info = {}
        smm.MINRES(A, b.copy(), x, k, 0.0, info=info)
        assert info["iterations"] == k
        seen.append(info["resnorm2"])
    print("phibar^2 by pass limit", seen)
    assert all(seen[k + 1] <= seen[k] for k in range(len(seen) - 1))
    assert seen[0] <= float(np.dot(b, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_same_bits_twice(smm, dtype):
    csr, b = system("shifted2d_16b", dtype)
    A = make(smm, csr)
    runs = []
    for _ in range(2):
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        st = smm.MINRES(A, b.copy(), x, -1, EPS[dtype], info=info)
        runs.append((int(st), info["iterations"], info["resnorm2"], x))
    assert runs[0][:3] == runs[1][:3] and runs[0][0] == SUCCESS
    np.testing.assert_array_equal(bits(runs[0][3]), bits(runs[1][3]))


PRECONDITIONED = {"IC0": {}, "FSAI": {}, "CHEBYSHEV": {}, "AMG": {}}


@pytest.mark.parametrize("kind", list(PRECONDITIONED))
def test_preconditioned_by_the_unshifted_operator(smm, oracle, kind):
    """A = L - I, M made on a handle of L: SUCCESS, a small true residual (loose: the stop test is in the M^-1-norm), fewer passes than
    without M, and three fixed passes against the restatement with the handle's own apply as the black box"""
    eps = EPS[np.float64]
    csr, b = system("shifted2d_16", np.float64)
    A = make(smm, csr)
    L = make(smm, cases.unshifted("shifted2d_16"))
    M = L.getPreconditioner(kind, **PRECONDITIONED[kind])
    info, plain = {}, {}
    x = np.zeros(len(b))
    st = smm.MINRES(A, b.copy(), x, -1, eps, M, info=info)
    x0 = np.zeros(len(b))
    st0 = smm.MINRES(A, b.copy(), x0, -1, eps, info=plain)
    res = true_residual(csr, b, x)
    print(kind, "passes", info["iterations"], "without M", plain["iterations"], "true |r|", res, "|b|", float(np.linalg.norm(b)))
    assert int(st) == int(st0) == SUCCESS
    assert res <= 1e-6 * float(np.linalg.norm(b))
    assert info["iterations"] < plain["iterations"]

    def apply(r):
        out = np.zeros_like(r)
        M.apply(np.ascontiguousarray(r), out)
        return out

    st_ref, x_ref, it_ref, sens = reference(oracle, "precond/" + kind, csr, b, 3, apply)
    tol = allowed(x_ref, sens, np.float64)
    x = np.zeros(len(b))
    st = smm.MINRES(A, b.copy(), x, 3, 0.0, M, info=info)
    err = worst(x, x_ref)
    print(kind, "3 passes: max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert int(st) == st_ref == MAX_ITERATIONS_REACHED and info["iterations"] == it_ref == 3
    assert err <= tol


def test_refusals(smm):
    lib = _lib.load()
    dtype = np.float64
    csr, b = system("shifted2d_16", dtype)
    n = len(b)
    A = make(smm, csr)
    L = make(smm, cases.unshifted("shifted2d_16"))
    L12 = make(smm, cases.unshifted("shifted2d_12"))
    L32 = make(smm, cases.unshifted("shifted2d_16", np.float32))
    P = smm.SolverPreconditioner
    offers = {
        "JACOBI": L.getPreconditioner(P.JACOBI),
        "ILU0": L.getPreconditioner(P.ILU0),
        "JSWEEP_SGS 2 / 3": L.getPreconditioner(P.JSWEEP_SGS, sweeps=(2, 3)),
        "another size": L12.getPreconditioner(P.IC0),
        "the other dtype": L32.getPreconditioner(P.IC0),
        "NONE": L.getPreconditioner(P.NONE),
    }
    for what, M in offers.items():
        x = np.full(n, 0.25)
        with pytest.raises(smm.SmmHipError) as e:
            smm.MINRES(A, b.copy(), x, 1, 0.0, M)
        message = lib.smm_hip_last_error().decode()
        print(what, "->", message)
        assert e.value.code == INVALID and message.startswith("minres:"), (what, message)
        assert np.all(x == 0.25), what
    # the same kinds are taken once they fit: JSWEEP_SGS with equal step counts
    x = np.zeros(n)
    smm.MINRES(A, b.copy(), x, 1, 0.0, L.getPreconditioner(P.JSWEEP_SGS, sweeps=(3, 3)))
    # a rectangular matrix, a null vector, a null matrix, a matrix of the other dtype
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2))
    with pytest.raises(smm.SmmHipError) as e:
        smm.MINRES(W, np.ones(2), np.zeros(2), 1, 0.0)
    assert e.value.code == INVALID and lib.smm_hip_last_error().decode().startswith("minres:")
    st_c, it_c = ctypes.c_int(), ctypes.c_int()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    x = np.zeros(n)
    assert lib.smm_hip_minres_f64(A._h, None, p(x), 1, 0.0, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("minres:")
    assert lib.smm_hip_minres_f64(A._h, p(x), None, 1, 0.0, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert lib.smm_hip_minres_f64(None, p(x), p(x), 1, 0.0, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("minres:")
    wrong = np.zeros(n, dtype=np.float32)
    assert lib.smm_hip_minres_f32(A._h, p(wrong), p(wrong), 1, 0.0, None, ctypes.byref(st_c), ctypes.byref(it_c), None) == INVALID
    assert lib.smm_hip_last_error().decode().startswith("minres:")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_edges(smm, oracle, dtype):
    csr, b = system("shifted2d_12", dtype)
    n = len(b)
    A = make(smm, csr)
    info = {}
    # an exact start: b := A xs in the arithmetic of the row-sequential SpMV, so that r1 = 0 bit for bit
    xs = np.linalg.solve(cases.dense(csr), b.astype(np.float64)).astype(dtype)
    bb = np.zeros(n, dtype=dtype)
    S = make(smm, csr)
    S.set_kernel(smm.SPMV_STREAM, 1)
    S.rMult(xs, bb)
    np.testing.assert_array_equal(bb, oracle.spmv(csr, 0, None, xs))
    x = xs.copy()
    st = smm.MINRES(S, bb.copy(), x, -1, 0.0, info=info)
    assert (int(st), info["iterations"], info["resnorm2"]) == (SUCCESS, 0, 0.0)
    np.testing.assert_array_equal(bits(x), bits(xs))
    # rows == 0: nothing is read or written through b / x
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    z = np.zeros(0, dtype=dtype)
    st = smm.MINRES(E, z, z, -1, 1e-6, info=info)
    assert (int(st), info["iterations"]) == (SUCCESS, 0)
    lib = _lib.load()
    suf = "f32" if dtype == np.float32 else "f64"
    st_c, it_c = ctypes.c_int(-1), ctypes.c_int(-1)
    assert getattr(lib, f"smm_hip_minres_{suf}")(E._h, None, None, -1, dtype(1e-6), None, ctypes.byref(st_c), ctypes.byref(it_c), None) == 0
    assert (st_c.value, it_c.value) == (SUCCESS, 0)
    # maxIterations == 0: no step, x untouched, the start's r.r
    x = np.full(n, 0.5, dtype=dtype)
    st = smm.MINRES(A, b.copy(), x, 0, EPS[dtype], info=info)
    assert (int(st), info["iterations"]) == (MAX_ITERATIONS_REACHED, 0) and np.all(x == 0.5) and info["resnorm2"] > 0
    # a non-zero start: the start is read from x
    x0 = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    st_ref, x_ref, it_ref, _ = minres(oracle, csr, b, x0, 3, 0.0)
    x = x0.copy()
    st = smm.MINRES(A, b.copy(), x, 3, 0.0, info=info)
    assert int(st) == st_ref and info["iterations"] == it_ref == 3
    assert worst(x, x_ref) <= RTOL[dtype] * max(1.0, float(np.max(np.abs(x_ref))))
    # the outputs are optional; maxIterations beyond rows is clamped to rows
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    x = np.zeros(n, dtype=dtype)
    bb = b.copy()
    assert getattr(lib, f"smm_hip_minres_{suf}")(A._h, p(bb), p(x), 3, dtype(0), None, None, None, None) == 0
    x = np.zeros(n, dtype=dtype)
    st = smm.MINRES(A, b.copy(), x, 10 * n, 0.0, info=info)
    assert info["iterations"] <= n and np.isfinite(x).all()


def test_a_negative_definite_preconditioner_diverges(smm):
    """M built on -L: r1.y < 0 at the start -- DIVERGED, no step, x finite and equal to its start.  CHEBYSHEV of -L cannot be built (its
    bounds are negative), so the handle is whichever of the other kinds MINRES takes that create accepts on -L."""
    csr, b = system("shifted2d_16", np.float64)
    n = len(b)
    A = make(smm, csr)
    start, pos, val = cases.unshifted("shifted2d_16")
    N = smm.CSRMatrix(n, n, start, pos, -val)
    P = smm.SolverPreconditioner
    M, made = None, None
    for kind, kw in ((P.JSWEEP_SGS, {"sweeps": (3, 3)}), (P.MULTICOLOR_SGS, {}), (P.AMG, {})):
        try:
            M, made = N.getPreconditioner(kind, **kw), kind
            break
        except smm.SmmHipError:
            continue
    assert M is not None, "no kind MINRES takes can be created on -L: this sub-case has to be dropped and the summary has to say so"
    r = np.random.default_rng(4).uniform(-1, 1, n)
    y = np.zeros(n)
    M.apply(r, y)
    print("negative definite M:", made.name, "r.M^-1 r", float(np.dot(r, y)))
    assert float(np.dot(r, y)) < 0
    x0 = np.random.default_rng(5).uniform(-1, 1, n)
    x = x0.copy()
    info = {}
    st = smm.MINRES(A, b.copy(), x, -1, 1e-8, M, info=info)
    assert int(st) == DIVERGED and info["iterations"] == 0
    assert np.isfinite(x).all()
    np.testing.assert_array_equal(bits(x), bits(x0))


FAMILIES = [("STREAM", 1), ("STREAM", 2), ("STREAM", 4), ("VECTOR", 4), ("PATTERN", 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_every_spmv_family(smm, oracle, dtype):
    it = 10
    csr, b = system("shifted2d_16", dtype)
    _, x_ref, _, sens = reference(oracle, "shifted2d_16", csr, b, it)
    tol = allowed(x_ref, sens, dtype)
    got = {}
    for family, lanes in FAMILIES:
        A = make(smm, csr)
        A.set_kernel(getattr(smm, "SPMV_" + family), lanes)
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        smm.MINRES(A, b.copy(), x, it, 0.0, info=info)
        assert info["iterations"] == it and A.get_kernel() == (getattr(smm, "SPMV_" + family), lanes)
        got[family, lanes] = x
        err = worst(x, x_ref)
        print(family, lanes, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol)
        assert err <= tol, (family, lanes)
    np.testing.assert_array_equal(bits(got["STREAM", 1]), bits(got["PATTERN", 1]))
    # the saddle matrix (no stored diagonal in its last rows) under STREAM only: its pattern has no blocks and more offsets than MASKS takes
    csr, b = system("saddle", dtype)
    _, x_ref, _, sens = reference(oracle, "saddle", csr, b, it)
    tol = allowed(x_ref, sens, dtype)
    for lanes in (1, 2, 4):
        A = make(smm, csr)
        A.set_kernel(smm.SPMV_STREAM, lanes)
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        smm.MINRES(A, b.copy(), x, it, 0.0, info=info)
        err = worst(x, x_ref)
        print("saddle STREAM", lanes, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol)
        assert info["iterations"] == it and err <= tol, lanes


@pytest.mark.parametrize("precondition", [False, True], ids=["plain", "ic0"])
def test_device_pointers_on_offset_views_and_another_stream(smm, oracle, precondition):
    """smm_hip_minres_dev_f64 on a stream of the caller's, b and x views at element alignment inside larger buffers with guard bands"""
    dtype, it = np.float64, 3
    csr, b = system("shifted2d_16", dtype)
    n = len(b)
    M = None
    apply = None
    if precondition:
        L = make(smm, cases.unshifted("shifted2d_16"))
        M = L.getPreconditioner("IC0")

        def apply(r):
            out = np.zeros_like(r)
            M.apply(np.ascontiguousarray(r), out)
            return out

    st_ref, x_ref, _, sens = reference(oracle, "views/" + ("ic0" if precondition else "plain"), csr, b, it, apply)
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved = snapshot(d_b)
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    st, k, res = host.minres_dev(A, d_b, d_x, it, 0.0, M, s.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == st_ref == MAX_ITERATIONS_REACHED and k == it and res > 0
    assert worst(d_x.cpu().numpy(), x_ref) <= allowed(x_ref, sens, dtype)
    assert_unchanged(d_b, saved, "b")
    assert_guards_intact(d_b, "b")
    assert_guards_intact(d_x, "x")


def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it) against the restatement over the fma oracle.  The
    element-wise lines of the restatement stay a*x+b in NumPy, so this flavour is compared by tolerance only."""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    dtype, it = np.float64, 3
    csr, b = system("saddle", dtype)
    n = len(b)
    st_ref, x_ref, _, sens = reference(oracle_fma, "fma/saddle", csr, b, it)
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    h = P()
    assert lib.smm_hip_csr_create_f64(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
    fn = lib.smm_hip_minres_f64
    fn.argtypes = [P, P, P, ctypes.c_int, ctypes.c_double, P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    st, k, res = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    x = np.zeros(n, dtype=dtype)
    assert fn(h, ptr(b.copy()), ptr(x), it, 0.0, None, ctypes.byref(st), ctypes.byref(k), ctypes.byref(res)) == 0, lib.smm_hip_last_error()
    lib.smm_hip_csr_destroy(h)
    assert st.value == st_ref == MAX_ITERATIONS_REACHED and k.value == it
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


def write_matrix(path, csr):
    start, pos, val = csr
    rows = len(start) - 1
    with open(path, "w") as f:
        f.write(f"{rows} {len(pos)}\n")
        for r in range(rows):
            for k in range(start[r], start[r + 1]):
                f.write(f"{r} {int(pos[k])} {float(val[k])!r}\n")


def test_cpp_dropin_case_on_the_gpu(smm, oracle, tmp_path):
    """tests/cpp/minres_case.cpp on shifted2d_12, fp64: SMM::MINRES without a preconditioner and with the IC0 of the unshifted operator;
    both SUCCESS, both near the Python binding's x of the same solve, and the preconditioned run in fewer passes."""
    eps = EPS[np.float64]
    csr, b = system("shifted2d_12", np.float64)
    x_py = np.zeros(len(b))
    info = {}
    assert int(smm.MINRES(make(smm, csr), b.copy(), x_py, -1, eps, info=info)) == SUCCESS
    write_matrix(tmp_path / "a.txt", csr)
    write_matrix(tmp_path / "l.txt", cases.unshifted("shifted2d_12"))
    np.savetxt(tmp_path / "b.txt", b, fmt="%.17g")
    np.savetxt(tmp_path / "x.txt", x_py, fmt="%.17g")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)] + [str(tmp_path / f) for f in ("a.txt", "l.txt", "b.txt", "x.txt")] + [repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = {ln.split()[0]: ln.split() for ln in r.stdout.splitlines()}
    assert set(lines) == {"plain", "ic0"}
    got = {k: (int(w[2]), int(w[4]), int(w[6]), float.fromhex(w[8])) for k, w in lines.items()}
    assert got["plain"][:3] == (SUCCESS, 0, info["iterations"]) and got["plain"][3] == 0.0  # the same library, the same solve: the same bits
    # both answers solve A x = b to about eps in a norm of their own; |A^-1| = 1 / 0.00596 = 168 for this matrix
    assert got["ic0"][:2] == (SUCCESS, 0) and 0 < got["ic0"][2] < got["plain"][2]
    assert got["ic0"][3] <= 168 * 1e-6 * float(np.linalg.norm(b))
