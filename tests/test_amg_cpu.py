"""The aggregation multigrid preconditioner without a GPU: the CPU restatement (tests/amg_restatement.py, the definition the device code
is compared with) against itself -- every row in one aggregate, roots more than two strong hops apart, the row sums of P, a symmetric
Galerkin operator, a symmetric cycle that at least halves ConjugateGradient's iteration count -- and the public surfaces."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from amg_restatement import (AmgRefused, aggregates, coarse_inverse, dense_apply, dense_of, hash32, hierarchy, make_apply, omega_of, operator_complexity,
                             roots, row_of, strength)
from chebyshev_restatement import pcg
from test_chebyshev_cpu import spd5
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "amg_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
ABI = ("smm_hip_precond_create_amg", "smm_hip_precond_amg_info", "smm_hip_precond_amg_level", "smm_hip_precond_amg_aggregates",
       "smm_hip_precond_amg_coarse_inverse_f32", "smm_hip_precond_amg_coarse_inverse_f64", "smm_hip_precond_amg_refresh")

_REF = {}


def build_case(tmp_path):
    """the g++ line of tests/gmres_helpers.py for tests/cpp/amg_case.cpp"""
    exe = tmp_path / "amg_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def case(name, dtype=np.float64):
    """(csr, keyword arguments of the hierarchy), the cases of the issue"""
    if name == "poisson2d_32":
        return gen_matrices(dtype)["poisson2d_32"], {}
    if name == "poisson2d_32_c48":
        return gen_matrices(dtype)["poisson2d_32"], {"coarse_rows": 48}
    if name == "stencil3d_12":
        return gen.stencil3d(12, 12, 12, dtype=dtype), {}
    if name == "convdiff3d_12":
        return gen_matrices(dtype)["convdiff3d_12"], {}
    if name == "convdiff3d_20":
        return gen.convdiff3d(20, 0.3, dtype=dtype), {}
    assert name == "spd5"
    return spd5(dtype), {}


CASES = ("poisson2d_32", "stencil3d_12", "convdiff3d_12", "convdiff3d_20", "spd5", "poisson2d_32_c48")


def levels_of(name, dtype=np.float64):
    key = (name, np.dtype(dtype).name)
    if key not in _REF:
        csr, kw = case(name, dtype)
        _REF[key] = (csr, hierarchy(csr, **kw))
    return _REF[key]


def test_hash_is_the_murmur3_finaliser():
    # fmix32 of 1, 2, 3 as the scalar statement computes them
    def scalar(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    got = hash32(np.arange(1000))
    assert [int(v) for v in got[:5]] == [scalar(i + 1) for i in range(5)]
    assert len(set(int(v) for v in got)) == 1000


@pytest.mark.parametrize("name", CASES)
def test_every_row_has_exactly_one_aggregate(name):
    csr, levels = levels_of(name)
    sizes = [len(v["A"][0]) - 1 for v in levels]
    print(name, "rows per level", sizes, "nnz", [len(v["A"][1]) for v in levels], "operator complexity", round(operator_complexity(levels), 3),
          "rounds", [v.get("rounds") for v in levels[:-1]], "phase-2 passes", [v.get("passes") for v in levels[:-1]], "left over", [v.get("left") for v in levels[:-1]])
    if name == "spd5":
        assert sizes == [5]
    if name in ("convdiff3d_20", "poisson2d_32_c48"):
        assert len(levels) == 3
    for l, lv in enumerate(levels[:-1]):
        n, n_c = sizes[l], lv["n_c"]
        agg = lv["agg"]
        assert agg.shape == (n,) and agg.min() == 0 and agg.max() == n_c - 1
        assert len(np.unique(agg)) == n_c == sizes[l + 1]  # no aggregate is empty
        roots_at = np.nonzero(lv["state"] == 2)[0]
        np.testing.assert_array_equal(agg[roots_at], np.arange(len(roots_at)))  # numbered in ascending row order
        assert 10 * n_c < 9 * n
    assert sizes[-1] <= 1024


@pytest.mark.parametrize("name", ("poisson2d_32", "stencil3d_12"))
def test_roots_are_more_than_two_strong_hops_apart(name):
    """on a symmetric strength graph no two roots share a strong neighbour or are strong neighbours; every non-root is within two hops of one"""
    csr, levels = levels_of(name)
    lv = levels[0]
    n = len(csr[0]) - 1
    G = np.zeros((n, n), dtype=bool)
    G[row_of(csr[0])[lv["strong"]], csr[1][lv["strong"]]] = True
    assert (G == G.T).all()
    G1 = G | np.eye(n, dtype=bool)
    reach = (G1.astype(np.int32) @ G1.astype(np.int32)) > 0  # within two hops
    is_root = lv["state"] == 2
    between = reach[np.ix_(is_root, is_root)]
    assert between.sum() == is_root.sum()  # only the diagonal
    assert reach[:, is_root].any(axis=1).all()  # maximal
    state, rounds = roots(csr, lv["strong"])
    assert rounds <= 12 and (state == lv["state"]).all()


@pytest.mark.parametrize("name", ("poisson2d_32", "convdiff3d_12"))
def test_row_sums_of_p(name):
    """sum_j P_ij = 1 - omega (row sum of D^-1 A), within rounding: a row of S T holds the row of S summed by aggregate"""
    csr, levels = levels_of(name)
    lv = levels[0]
    start, pos, val = csr
    A = dense_of(csr)
    want = 1.0 - omega_of(lv["lam"]) * (A.sum(axis=1) / np.diag(A))
    P = lv["P"]
    got = np.add.reduceat(P[2], P[0][:-1])
    mass = omega_of(lv["lam"]) * (np.abs(A).sum(axis=1) / np.abs(np.diag(A))) + 1.0
    slack = 16 * np.finfo(np.float64).eps * mass  # at most 8 entries in a row, each rounded three times
    assert np.all(np.abs(got - want) <= slack)


@pytest.mark.parametrize("name", ("poisson2d_32", "stencil3d_12", "poisson2d_32_c48"))
def test_galerkin_operator_is_symmetric(name):
    csr, levels = levels_of(name)
    for lv in levels[1:]:
        A1 = dense_of(lv["A"])
        asym = float(np.max(np.abs(A1 - A1.T)))
        print(name, len(A1), "asymmetry", asym, "largest entry", float(np.max(np.abs(A1))))
        assert asym <= 64 * np.finfo(np.float64).eps * float(np.max(np.abs(A1)))


def test_strength_threshold_halves_per_level():
    csr, _ = case("stencil3d_12")
    d = np.full(len(csr[0]) - 1, 6.0)
    assert strength(csr, d, 1.0 / 6.0).sum() == len(csr[1]) - len(d)  # 1 >= (1/36) 36: every off-diagonal entry, at equality
    assert strength(csr, d, 0.17).sum() == 0


def test_isolated_rows_stall():
    """a diagonal matrix: every row is its own root, n_c = n, the level does not shrink: dense only, or refused above 1024 rows"""
    def diag(n):
        return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(1.0, 2.0, n)
    levels = hierarchy(diag(300))
    assert len(levels) == 1 and "P" not in levels[0]
    csr = diag(300)
    st, _ = roots(csr, np.zeros(300, dtype=bool))
    assert (st == 2).all()
    assert aggregates(csr, np.zeros(300, dtype=bool), st)[1] == 300
    with pytest.raises(AmgRefused):
        hierarchy(diag(1025))


@pytest.mark.parametrize("name", ("poisson2d_32", "stencil3d_12"))
def test_cycle_is_symmetric_and_halves_cg(oracle, name):
    """b = A 1, eps 1e-8, fp64: the restated PCG with the restated cycle against the oracle's ConjugateGradient"""
    eps = 1e-8
    csr, levels = levels_of(name)
    fn = make_apply(oracle, levels, coarse_inverse(levels[-1]["A"]))
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-1, 1, (2, len(csr[0]) - 1))
    uMv, vMu = float(u @ fn(v)), float(v @ fn(u))
    assert abs(uMv - vMu) <= 1e-12 * abs(uMv)
    b = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(len(b))
    st_ref, _, it_ref, _ = oracle.cg(csr, b, zero, -1, eps)
    st, x, it, rr = pcg(oracle, csr, b, zero, -1, eps, fn)
    print(name, "iterations", it, "unpreconditioned", it_ref, "r.r", rr, "max|x - 1|", float(np.max(np.abs(x - 1))), "|uMv - vMu| / |uMv|", abs(uMv - vMu) / abs(uMv))
    assert st == st_ref == 0 and rr < eps * eps
    assert 0 < it <= it_ref // 2
    np.testing.assert_allclose(x, 1.0, rtol=100 * eps)


def test_dense_apply_is_the_inverse():
    csr, levels = levels_of("spd5")
    inv = coarse_inverse(csr)
    b = gen.row_sums(csr[0], csr[2])
    np.testing.assert_allclose(dense_apply(inv, b), 1.0, rtol=1e-14)
    big = np.random.default_rng(1).uniform(-1, 1, (130, 130))
    v = np.random.default_rng(2).uniform(-1, 1, 130)
    np.testing.assert_allclose(dense_apply(big, v), big @ v, atol=1e-13)


def test_public_surface():
    assert host.SolverPreconditioner.AMG == 8 and host.SolverPreconditioner["AMG"].value == 8
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in ABI:
            assert hasattr(lib, name), (name, fma)
            assert name in _lib.exported_symbols()
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    assert "#define SMM_PRECOND_AMG 8" in header
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, host.SolverPreconditioner.JACOBI, theta=0.1)  # refused before the handle is touched


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::AMGPreconditioner<float> / <double> through ConjugateGradient, BiCGStab and GMRES; -Wall -Werror.  Without a GPU every call
    reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
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
