"""IDR(s) on the GPU (csrc/smm_solvers_idrs.hip) through the C ABI, against the CPU restatement (tests/idrs_restatement.py; the method
is an addition, so there are no goldens): fixed steps, converged runs, the library's own shadow space, right preconditioning, the edge
semantics, the frozen loop and determinism, the kernel families, the device-pointer form on offset views, the near-breakdown system of
DESIGN.md 3.4 and the drop-in C++ header.  Tolerances: the `allowed` rule of tests/test_gpu_cgs.py with RTOL of tests/test_gpu_solvers.py."""
import subprocess

import numpy as np
import pytest
import torch
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from idrs_helpers import FIXED, NEAR_EPS, SEED, build_case, matrix, near_breakdown, reference, shadow_space
from idrs_restatement import idrs, raw_shadow
from test_gpu_cgs import allowed, make, worst
from test_gpu_gmres import oracle_apply

from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def padded(n):
    return max(64, (n + 63) // 64 * 64)


@pytest.mark.parametrize("mname,s,dtype,it", FIXED, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_fixed_steps_match_the_restatement(smm, oracle, mname, s, dtype, it):
    csr, b = matrix(mname, dtype)
    st_ref, x_ref, it_ref, sens, P = reference(oracle, mname, csr, b, it, s)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.IDRs(A, b.copy(), x, it, 0.0, s, P=P, info=info)
    err = worst(x, x_ref)
    print(mname, s, np.dtype(dtype).name, it, "max|x - ref|", err, "allowed", tol, "sensitivity", sens)
    assert int(st) == st_ref == 2 and info["iterations"] == it_ref == it
    assert err <= tol
    assert info["resnorm2"] >= 0


@pytest.mark.parametrize("s", [1, 4, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("mname", ["poisson2d_32", "convdiff3d_12"])
def test_converged(smm, oracle, mname, dtype, s):
    eps = 1e-6 if dtype == np.float64 else 1e-3
    csr, b = matrix(mname, dtype)
    zero = np.zeros(len(b), dtype=dtype)
    P = shadow_space(oracle, len(b), s, dtype)
    st_ref, _, it_ref, _ = idrs(oracle, csr, b, zero, -1, eps, s, P)
    A = make(smm, csr)
    x = zero.copy()
    info = {}
    st = smm.IDRs(A, b.copy(), x, -1, eps, s, P=P, info=info)
    print(mname, np.dtype(dtype).name, s, "SpMVs", info["iterations"], "restatement", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))), "r.r", info["resnorm2"])
    assert int(st) == st_ref == 0
    assert info["resnorm2"] <= dtype(eps) * dtype(eps)
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    if mname == "poisson2d_32":
        assert float(np.max(np.abs(x.astype(np.float64) - 1))) <= 55 * eps  # |A^-1| = 55 (tests/test_cgs_cpu.py)
    else:
        np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_the_librarys_own_shadow_space(smm, oracle, dtype):
    """In fp64, s = 1 after undoing the scale is the hash bit for bit (the division and the product each move a value by 2^-53 of itself,
    the hash's grid is 2^-24: rounding to the grid undoes both; in fp32 the grid is the rounding unit itself, so that check is not clean
    there).  In both dtypes the finished P equals the restatement's to 64 u and is orthonormal; a solve that generates P from a seed
    equals, bit for bit, the solve given that P; two seeds give different iterates."""
    csr, b = matrix("convdiff3d_12", dtype)
    n, s = len(b), 8
    ld = padded(n)
    u = float(np.finfo(dtype).eps)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    if dtype == np.float64:
        d_one = torch.zeros(ld, dtype=tdt, device="cuda")
        host.idrs_shadow_dev(n, 1, SEED, d_one, ld, dtype)
        raw = raw_shadow(n, 1, SEED, np.float64)[0]
        undone = d_one.cpu().numpy()[:n] * np.sqrt(np.sum(raw * raw))
        np.testing.assert_array_equal(np.round(undone * 2.0 ** 24), raw * 2.0 ** 24)
    d_P = torch.zeros((s, ld), dtype=tdt, device="cuda")
    host.idrs_shadow_dev(n, s, SEED, d_P, ld, dtype)
    P_gpu = d_P.cpu().numpy()[:, :n]
    P_ref = shadow_space(oracle, n, s, dtype)
    gap = float(np.max(np.abs(P_gpu.astype(np.float64) - P_ref.astype(np.float64))))
    gram = P_gpu.astype(np.float64) @ P_gpu.astype(np.float64).T
    print(np.dtype(dtype).name, "max|P - P_ref|", gap, "max|P^T P - I|", float(np.max(np.abs(gram - np.eye(s)))))
    assert gap <= 64 * u
    assert float(np.max(np.abs(gram - np.eye(s)))) <= 16 * u
    assert not d_P[:, n:].any()  # the padding is not written
    A = make(smm, csr)
    got = {}
    for name, kwargs in (("seed", dict(seed=SEED)), ("given", dict(P=P_gpu[:4].copy())), ("other", dict(seed=SEED + 1))):
        x = np.zeros(n, dtype=dtype)  # (the first four columns of the s = 8 space are the s = 4 space of that seed)
        info = {}
        st = smm.IDRs(A, b.copy(), x, 10, 0.0, 4, info=info, **kwargs)
        assert int(st) == 2 and info["iterations"] == 10
        got[name] = (x, info)
    np.testing.assert_array_equal(bits(got["seed"][0]), bits(got["given"][0]))
    assert got["seed"][1] == got["given"][1]
    assert not np.array_equal(got["seed"][0], got["other"][0])


@pytest.mark.parametrize("kind", ["JACOBI", "SYMMETRIC_GAUS_SEIDEL", "BLOCK_ILU0"])
def test_right_preconditioning(smm, oracle, kind):
    dtype, eps, s = np.float64, 1e-6, 4
    csr, b = matrix("convdiff3d_12", dtype)
    zero = np.zeros(len(b), dtype=dtype)
    A = make(smm, csr)
    M, apply = oracle_apply(smm, oracle, A, csr, getattr(smm.SolverPreconditioner, kind))
    info = {}
    for it in (3, 10):
        st_ref, x_ref, it_ref, sens, P = reference(oracle, "precond/" + kind, csr, b, it, s, apply)
        x = zero.copy()
        st = smm.IDRs(A, b.copy(), x, it, 0.0, s, M, P=P, info=info)
        err, tol = worst(x, x_ref), allowed(x_ref, sens, dtype)
        print(kind, it, "max|x - ref|", err, "allowed", tol)
        assert int(st) == st_ref == 2 and info["iterations"] == it_ref == it
        assert err <= tol
    P = shadow_space(oracle, len(b), s, dtype)
    st_ref, _, it_ref, _ = idrs(oracle, csr, b, zero, -1, eps, s, P, apply=apply)
    x = zero.copy()
    st = smm.IDRs(A, b.copy(), x, -1, eps, s, M, P=P, info=info)
    print(kind, "SpMVs", info["iterations"], "restatement", it_ref)
    assert int(st) == st_ref == 0 and info["resnorm2"] <= eps * eps
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_edge_semantics(smm, oracle, dtype):
    csr, b = matrix("poisson2d_32", dtype)
    rows = len(b)
    A = make(smm, csr)
    info = {}
    x = np.zeros(rows, dtype=dtype)
    st = smm.IDRs(A, b.copy(), x, 0, 1e-6, info=info)
    assert int(st) == 2 and info["iterations"] == 0 and not x.any()
    # -1 means rows: the converged run is the run capped at rows
    runs = []
    for maxit in (-1, rows):
        x = np.zeros(rows, dtype=dtype)
        st = smm.IDRs(A, b.copy(), x, maxit, 1e-3, info=info)
        runs.append((int(st), info["iterations"], x))
    assert runs[0][:2] == runs[1][:2] and runs[0][0] == 0 and np.array_equal(bits(runs[0][2]), bits(runs[1][2]))
    # an exact x0: no step, SUCCESS, x bit for bit
    x = np.ones(rows, dtype=dtype)
    st = smm.IDRs(A, b.copy(), x, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 0 and info["resnorm2"] == 0 and np.array_equal(x, np.ones(rows, dtype=dtype))
    # rows == 0
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    z = np.zeros(0, dtype=dtype)
    st = smm.IDRs(E, z, z, -1, 1e-6, info=info)
    assert int(st) == 0 and info["iterations"] == 0
    # s of 0 and 9; a matrix that is not square: INVALID, x untouched
    for s in (0, 9):
        x = np.full(rows, 7, dtype=dtype)
        with pytest.raises(smm.SmmHipError) as e:
            smm.IDRs(A, b.copy(), x, 1, 0.0, s)
        assert e.value.code == INVALID and np.all(x == 7)
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2, dtype=dtype))
    x = np.full(2, 7, dtype=dtype)
    with pytest.raises(smm.SmmHipError) as e:
        smm.IDRs(W, np.ones(2, dtype=dtype), x, 1, 0.0, 1)
    assert e.value.code == INVALID and np.all(x == 7)
    # ldP < rows with a P
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_v = torch.zeros(rows, dtype=tdt, device="cuda")
    with pytest.raises(smm.SmmHipError) as e:
        host.idrs_dev(A, d_v, d_v.clone(), 1, 0.0, 1, None, d_v.clone(), rows - 1)
    assert e.value.code == INVALID
    # the breakdown: the rotation [[0, 1], [-1, 0]], b = e1, s = 1, P = e1 makes M[0][0] = p . A r = 0 at the first step
    rot = (np.array([0, 1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([1, -1], dtype=dtype))
    e1 = np.array([1, 0], dtype=dtype)
    x = np.zeros(2, dtype=dtype)
    st = smm.IDRs(make(smm, rot), e1.copy(), x, -1, 1e-6, 1, P=e1.reshape(1, 2), info=info)
    assert int(st) == 1 and info["iterations"] == 0 and not x.any() and info["resnorm2"] == 1
    assert idrs(oracle, rot, e1, np.zeros(2, dtype=dtype), -1, 1e-6, 1, e1.reshape(1, 2))[::2] == (1, 0)


@pytest.mark.parametrize("s", [4, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_frozen_loop_and_determinism(smm, dtype, s):
    """The launches queued behind the raised flag must write nothing, and no sum depends on timing or on when the host looked: a converged
    run with maxIterations = -1, the same run with maxIterations = its step count (which queues nothing past the end) and a second
    identical run give the same bits of x and the same info."""
    eps = 1e-3 if dtype == np.float32 else 1e-6
    csr, b = matrix("poisson2d_32", dtype)
    A = make(smm, csr)
    runs = []
    for maxit in (-1, None, -1):
        x = np.zeros(len(b), dtype=dtype)
        info = {}
        st = smm.IDRs(A, b.copy(), x, runs[0][2]["iterations"] if maxit is None else maxit, eps, s, info=info)
        runs.append((int(st), x, info))
    st1, x1, info1 = runs[0]
    assert st1 == 0 and 4 < info1["iterations"] < len(b)
    for st, x, info in runs[1:]:
        assert st == 0 and info == info1
        np.testing.assert_array_equal(bits(x), bits(x1))


def test_pattern_family(smm, oracle):
    """convdiff3d(54) in fp64, as tests/test_gpu_gmres.py::test_pattern_family: the handle adopts PATTERN, then five steps on AUTO and five
    with STREAM forced at one lane per row"""
    dtype, s, it = np.float64, 4, 5
    csr = gen.convdiff3d(54, 0.3, dtype=dtype)
    b = gen.row_sums(csr[0], csr[2])
    n = len(b)
    _, x_ref, _, sens, P = reference(oracle, "family/convdiff3d_54", csr, b, it, s)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    info = {}
    smm.IDRs(A, b.copy(), np.zeros(n, dtype=dtype), 16, 1e30, s, info=info)
    assert info["iterations"] == 0
    assert A.get_kernel()[0] == smm.SPMV_PATTERN and A.pattern_info()[0] != 0
    got = {}
    x = np.zeros(n, dtype=dtype)
    st = smm.IDRs(A, b.copy(), x, it, 0.0, s, P=P, info=info)
    assert int(st) == 2 and info["iterations"] == it and A.get_kernel()[0] == smm.SPMV_PATTERN
    got["auto"] = x
    S = make(smm, csr)
    S.set_kernel(smm.SPMV_STREAM, 1)
    x = np.zeros(n, dtype=dtype)
    st = smm.IDRs(S, b.copy(), x, it, 0.0, s, P=P, info=info)
    assert int(st) == 2 and info["iterations"] == it and S.get_kernel() == (smm.SPMV_STREAM, 1)
    got["stream"] = x
    errs = {k: worst(v, x_ref) for k, v in got.items()}
    print("max|x - ref|", errs, "allowed", tol)
    assert errs["auto"] <= tol and errs["stream"] <= tol


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_stream_family_at_every_lane_setting(smm, oracle, lanes):
    dtype, s, it = np.float64, 4, 10
    csr, b = matrix("convdiff3d_12", dtype)
    _, x_ref, _, sens, P = reference(oracle, "convdiff3d_12", csr, b, it, s)
    A = make(smm, csr)
    A.set_kernel(smm.SPMV_STREAM, lanes)
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    st = smm.IDRs(A, b.copy(), x, it, 0.0, s, P=P, info=info)
    assert int(st) == 2 and info["iterations"] == it and A.get_kernel() == (smm.SPMV_STREAM, lanes)
    assert worst(x, x_ref) <= allowed(x_ref, sens, dtype)


def test_device_pointers_on_offset_views_and_another_stream(smm, oracle):
    """smm_hip_idrs_dev_f64 on a stream of the caller's; b, x and P are views at element alignment inside larger buffers with guard bands,
    P with a leading dimension above rows"""
    dtype, it, s = np.float64, 10, 4
    csr, b = matrix("convdiff3d_12", dtype)
    n = len(b)
    ldp = n + 3
    st_ref, x_ref, _, sens, P = reference(oracle, "convdiff3d_12", csr, b, it, s)
    wide = np.full((s, ldp), np.nan, dtype=dtype)
    wide[:, :n] = P
    d_b = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    d_P = carve_like(wide, fit(1, dtype), device="cuda:0")
    assert d_b.data_ptr() % 16 == 8 and d_x.data_ptr() % 16 == 8 and d_P.data_ptr() % 16 == 8
    d_csr = [torch.from_numpy(a).to("cuda:0") for a in csr]
    saved_b, saved_P = snapshot(d_b), snapshot(d_P)
    A = smm.CSRMatrix.from_device(n, n, d_csr[0], d_csr[1], d_csr[2], dtype)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    st, k, res = host.idrs_dev(A, d_b, d_x, it, 0.0, s, None, d_P, ldp, 0, stream.cuda_stream)
    torch.cuda.synchronize()
    assert int(st) == st_ref == 2 and k == it and res >= 0
    assert worst(d_x.cpu().numpy(), x_ref) <= allowed(x_ref, sens, dtype)
    assert_unchanged(d_b, saved_b, "b")
    assert_unchanged(d_P, saved_P, "P")
    for view, name in ((d_b, "b"), (d_x, "x"), (d_P, "P")):
        assert_guards_intact(view, name)


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
def test_near_breakdown_system(smm, oracle, jacobi):
    """convdiff3d(32, 0.3) in fp32 (where BiCGStab's rho holds no correct digit), s = 4; eps as tests/idrs_helpers.py
    NEAR_EPS explains"""
    eps = NEAR_EPS[jacobi]
    csr, b, P, _, it_ref, _ = near_breakdown(oracle, jacobi)
    A = make(smm, csr)
    M = A.getPreconditioner(smm.SolverPreconditioner.JACOBI) if jacobi else None
    x = np.zeros(len(b), dtype=np.float32)
    info = {}
    st = smm.IDRs(A, b.copy(), x, -1, eps, 4, M, P=P, info=info)
    print("jacobi" if jacobi else "plain", "SpMVs", info["iterations"], "restatement", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert np.isfinite(x).all() and int(st) == 0
    assert float(np.max(np.abs(x.astype(np.float64) - 1))) <= 100 * eps
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5), (info, it_ref)


def test_cpp_dropin_case_on_the_gpu(smm, oracle, tmp_path):
    """tests/cpp/idrs_case.cpp on convdiff3d_12 in fp64 (s = 4, the library's P from seed 0) agrees with the Python call to `allowed`"""
    eps, s = 1e-8, 4
    csr, b = matrix("convdiff3d_12", np.float64)
    start, pos, val = csr
    rows = len(b)
    path = tmp_path / "convdiff.txt"
    with open(path, "w") as f:
        f.write(f"{rows} {len(pos)}\n")
        for r in range(rows):
            for k in range(start[r], start[r + 1]):
                f.write(f"{r} {int(pos[k])} {float(val[k])!r}\n")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe), str(path), repr(eps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "status 0 hip 0", lines[0]
    x_cpp = np.array([float.fromhex(ln.split()[1]) for ln in lines[1:]])
    assert len(x_cpp) == rows
    x = np.zeros(rows)
    st = smm.IDRs(make(smm, csr), b.copy(), x, -1, eps, s)
    assert int(st) == 0
    # both are converged solutions of the same system by the same code: within 10 eps of x = 1 each, and of each other to `allowed`
    # with the sensitivity of a converged run taken as the residual bound |A^-1| eps <= 10 eps
    np.testing.assert_allclose(x_cpp, 1.0, rtol=10 * eps)
    assert worst(x_cpp, x) <= allowed(x, 10 * eps, np.float64)
