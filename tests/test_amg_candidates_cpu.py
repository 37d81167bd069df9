"""The multigrid preconditioner with near-null-space candidates without a GPU: the CPU restatement (tests/amg_candidates_restatement.py,
the definition the device code is compared with) against itself -- orthonormal kept columns, T B_{l+1} = B_l, whole nodes, identity rows
for what was dropped, ConjugateGradient counts on elasticity that stay flat under refinement where the scalar hierarchy's double -- the
elasticity generators and the public surfaces."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from amg_candidates_restatement import DROP_TOL, LDS_ROWS, hierarchy, node_graph, thin_qr, wave_dot
from amg_restatement import coarse_inverse, dense_of, make_apply
from amg_restatement import hierarchy as scalar_hierarchy
from chebyshev_restatement import pcg

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "cpp", "amg_candidates_case.cpp")
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
ABI = tuple(f"smm_hip_precond_{name}_{suf}" for name in ("create_amg_candidates", "create_amg_candidates_dev", "amg_candidates") for suf in ("f32", "f64"))
COARSE_ROWS = 64  # every elasticity case below gets three levels
EPS = float(np.finfo(np.float64).eps)

_REF = {}


def build_case(tmp_path):
    """the g++ line of tests/test_amg_cpu.py for tests/cpp/amg_candidates_case.cpp"""
    exe = tmp_path / "amg_candidates_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def elasticity(name, dtype=np.float64):
    """(csr, B = the rigid body modes, dofs per node) of a named case, made once"""
    key = ("matrix", name, np.dtype(dtype).name)
    if key not in _REF:
        dims = tuple(int(v) for v in name.split("_")[1].split("x"))
        start, pos, val, coords = (gen.elasticity2d if len(dims) == 2 else gen.elasticity3d)(*dims, dtype=dtype)
        _REF[key] = ((start, pos, val), gen.rigid_body_modes(coords, dtype=dtype), len(dims))
    return _REF[key]


def with_lone_node(dtype=np.float64):
    """elasticity2d(6, 6) and one more node coupled to nothing: its aggregate has 2 rows for 3 candidates"""
    key = ("lone", np.dtype(dtype).name)
    if key not in _REF:
        start, pos, val, coords = gen.elasticity2d(6, 6, dtype=dtype)
        n = len(start) - 1
        start = np.concatenate([start, [start[-1] + 2, start[-1] + 4]]).astype(np.int32)
        pos = np.concatenate([pos, [n, n + 1, n, n + 1]]).astype(np.int32)
        val = np.concatenate([val, np.array([2.0, 0.5, 0.5, 3.0], dtype=dtype)])
        coords = np.concatenate([coords, [[9.0, 2.0]]])
        _REF[key] = ((start, pos, val), gen.rigid_body_modes(coords, dtype=dtype), 2)
    return _REF[key]


def levels_of(name, dtype=np.float64):
    key = ("levels", name, np.dtype(dtype).name)
    if key not in _REF:
        csr, B, b = elasticity(name, dtype)
        _REF[key] = hierarchy(csr, B, b, coarse_rows=COARSE_ROWS)
    return _REF[key]


def dense_rect(csr, cols):
    start, pos, val = csr
    out = np.zeros((len(start) - 1, cols))
    out[np.repeat(np.arange(len(start) - 1), np.diff(start)), pos] = val
    return out


CASES = ("e_16x16", "e_32x32", "e_48x16", "e_6x6x6")


# ---- the generators --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dofs", [("e_16x16", 544), ("e_32x32", 2112), ("e_48x16", 1632), ("e_6x6x6", 882), ("e_2x3x4", 120)])
def test_generators(name, dofs):
    csr, B, b = elasticity(name)
    start, pos, val = csr
    n = len(start) - 1
    assert n == dofs and B.shape == (n, 3 if b == 2 else 6)
    A = dense_rect(csr, n)
    assert (A == A.T).all()
    assert all((np.diff(pos[start[i]:start[i + 1]]) > 0).all() for i in range(n))
    w = np.linalg.eigvalsh(A)
    assert w[0] > 0  # clamped: positive definite
    # rigid body modes carry no strain: A B vanishes on every row whose elements touch no clamped node
    dims = tuple(int(v) for v in name.split("_")[1].split("x"))
    coords = (gen.elasticity2d if b == 2 else gen.elasticity3d)(*dims)[3]
    assert coords.shape == (n // b, b) and coords[:, 0].min() == 1.0
    free = np.repeat(coords[:, 0] > 1.0, b)
    assert np.max(np.abs(A @ B)[free]) <= 64 * EPS * np.max(np.abs(A)) * np.max(np.abs(B))
    assert np.max(np.abs(A @ B)[~free]) > 0.1


def test_generator_arguments():
    with pytest.raises(ValueError):
        gen.elasticity2d(4, 4, clamp="front")
    with pytest.raises(ValueError):
        gen.elasticity3d(0, 4, 4)
    with pytest.raises(ValueError):
        gen.rigid_body_modes(np.zeros((3, 4)))
    top = gen.elasticity2d(3, 5, clamp="top")
    assert len(top[0]) - 1 == 2 * 4 * 5 and top[3][:, 1].max() == 4.0
    assert gen.elasticity2d(3, 3, dtype=np.float32)[2].dtype == np.float32


# ---- the restatement against itself ----------------------------------------------------------------------------------------------
def test_wave_dot_is_a_function_of_the_length_alone():
    rng = np.random.default_rng(7)
    for m in (1, 2, 63, 64, 65, 200):
        x, y = rng.uniform(-1, 1, (2, m))
        assert abs(wave_dot(x, y) - float(x @ y)) <= m * EPS * float(np.abs(x) @ np.abs(y))
        assert wave_dot(x, y) == wave_dot(x.copy(), y.copy())
    z = np.zeros(5)
    assert wave_dot(z, z) == 0.0 and not np.signbit(wave_dot(-z, z))


@pytest.mark.parametrize("name", CASES)
def test_kept_columns_are_orthonormal_and_t_reproduces_b(name):
    """Q^T Q = I on the kept columns within the bound of modified Gram-Schmidt, 8 k eps cond(V) per aggregate (Bjorck 1967: the loss of
    orthogonality is of order eps cond(V)); T B_{l+1} = B_l within 8 k eps (|T| |B_{l+1}|) entry by entry (k products, each rounded a few
    times).  None of these cases drops a column."""
    levels = levels_of(name)
    assert len(levels) == 3
    for l, lv in enumerate(levels[:-1]):
        n, k = lv["B"].shape
        T = dense_rect(lv["T"], lv["n_c"])
        assert lv["dropped"] == 0 and lv["kept"].all()
        gram = T.T @ T
        worst = 0.0
        for a in range(lv["n_agg"]):
            V = lv["B"][lv["agg"] == a]
            cond = float(np.linalg.cond(V))
            err = float(np.max(np.abs(gram[a * k:(a + 1) * k, a * k:(a + 1) * k] - np.eye(k))))
            worst = max(worst, err / (EPS * cond))
            assert err <= 8 * k * EPS * cond, (l, a, err, cond)
        off = gram - np.kron(np.eye(lv["n_agg"]), np.ones((k, k))) * gram
        assert (off == 0).all()  # columns of different aggregates share no row
        B_next = levels[l + 1]["B"]
        assert B_next.shape == (lv["n_c"], k)
        assert np.all(np.abs(T @ B_next - lv["B"]) <= 8 * k * EPS * (np.abs(T) @ np.abs(B_next)))
        print(name, "level", l, "rows", n, "aggregates", lv["n_agg"], "|Q^T Q - I| / (eps cond)", worst)


@pytest.mark.parametrize("name", CASES)
def test_no_node_is_split(name):
    levels = levels_of(name)
    b0 = elasticity(name)[2]
    for l, lv in enumerate(levels[:-1]):
        b = b0 if l == 0 else lv["B"].shape[1]
        per_node = lv["agg"].reshape(-1, b)
        assert (per_node == per_node[:, :1]).all()
        assert len(np.unique(lv["agg"])) == lv["n_agg"] and lv["agg"].max() == lv["n_agg"] - 1
        assert lv["n_c"] == lv["n_agg"] * lv["B"].shape[1] == len(levels[l + 1]["A"][0]) - 1
        N = lv["N"]
        assert len(N[0]) - 1 == len(lv["agg"]) // b


def test_node_graph_holds_frobenius_norms():
    csr, _, b = elasticity("e_2x3x4")
    A = dense_rect(csr, len(csr[0]) - 1)
    N = dense_rect(node_graph(csr, b), (len(csr[0]) - 1) // b)
    nodes = len(N)
    want = np.sqrt((A.reshape(nodes, b, nodes, b) ** 2).sum(axis=(1, 3)))
    np.testing.assert_allclose(N, want, rtol=16 * EPS)
    assert ((N != 0) == (want != 0)).all()


def test_a_deficient_aggregate_yields_an_identity_row():
    csr, B, b = with_lone_node()
    n = len(csr[0]) - 1
    levels = hierarchy(csr, B, b, coarse_rows=8)
    lv = levels[0]
    a = int(lv["agg"][n - 1])
    assert (lv["agg"] == a).sum() == 2 and lv["dropped"] == 1  # the lone node is an aggregate of its own: 2 rows, 3 candidates
    k = 3
    assert list(lv["kept"][a * k:(a + 1) * k]) == [True, True, False]
    row = a * k + 2
    A1 = dense_of(levels[1]["A"])
    want = np.zeros(len(A1))
    want[row] = 1.0
    assert (A1[row] == want).all() and (A1[:, row] == want).all()
    assert (levels[1]["B"][row] == 0).all()
    T = dense_rect(lv["T"], lv["n_c"])
    assert (T[:, row] == 0).all() and (lv["T"][0][-2:] - lv["T"][0][-3:-1] == 2).all()
    # the dropped column was an exact combination of the other two: T B_1 still gives B_0 back
    assert np.all(np.abs(T @ levels[1]["B"] - B) <= 8 * k * EPS * np.maximum(np.abs(T) @ np.abs(levels[1]["B"]), np.abs(B)))
    for v in levels:
        assert (np.abs(np.diag(dense_of(v["A"]))) >= 1e-5).all()  # no level has a zero diagonal


def test_dependent_and_zero_columns_are_dropped():
    rng = np.random.default_rng(11)
    V = rng.uniform(-1, 1, (70, 5))
    V[:, 3] = V[:, 0]  # a duplicate
    V[:, 4] = 0.0
    Q, R, kept = thin_qr(V)
    assert list(kept) == [True, True, True, False, False]
    assert (Q[:, 3:] == 0).all() and (R[3:] == 0).all()
    assert abs(R[0, 3] - R[0, 0]) <= 70 * EPS * R[0, 0] and np.all(np.abs(R[1:3, 3]) <= 70 * EPS * R[0, 0]) and (R[:, 4] == 0).all()
    np.testing.assert_allclose(Q @ R, V, atol=32 * EPS)
    nearly = V[:, :2].copy()
    nearly[:, 1] = nearly[:, 0] * (1 + DROP_TOL)  # parallel: what is left after the projection is rounding, far below the tolerance
    assert list(thin_qr(nearly)[2]) == [True, False]
    apart = V[:, :2].copy()
    apart[:, 1] = apart[:, 0] + 4 * DROP_TOL * V[:, 2]  # independent by four times the tolerance: kept
    assert list(thin_qr(apart)[2]) == [True, True]
    assert LDS_ROWS == 256 and DROP_TOL == 2.0 ** -13


def counts(oracle, name):
    """(unpreconditioned, scalar hierarchy, rigid body modes) ConjugateGradient iterations to 1e-8 of b = A 1, made once"""
    key = ("counts", name)
    if key not in _REF:
        eps = 1e-8
        csr, B, b = elasticity(name)
        rhs = gen.row_sums(csr[0], csr[2])
        zero = np.zeros(len(rhs))
        st0, _, it0, _ = oracle.cg(csr, rhs, zero, -1, eps)
        out = [it0]
        for levels in (scalar_hierarchy(csr, coarse_rows=COARSE_ROWS), levels_of(name)):
            fn = make_apply(oracle, levels, coarse_inverse(levels[-1]["A"]))
            st, x, it, rr = pcg(oracle, csr, rhs, zero, -1, eps, fn)
            assert st == st0 == 0 and rr < eps * eps
            np.testing.assert_allclose(x, 1.0, rtol=1e-5)
            out.append(it)
        _REF[key] = tuple(out)
    return _REF[key]


@pytest.mark.parametrize("name", CASES)
def test_cg_counts_beat_the_scalar_hierarchy(oracle, name):
    """measured (none / candidates=None / rigid body modes): 16x16 149 / 24 / 14, 32x32 282 / 44 / 16, 48x16 301 / 46 / 17,
    6x6x6 92 / 25 / 14"""
    none, scalar, modes = counts(oracle, name)
    print(name, "iterations: none", none, "scalar hierarchy", scalar, "rigid body modes", modes)
    assert modes < scalar and modes < none


def test_cg_counts_stay_flat_under_refinement(oracle):
    _, scalar16, modes16 = counts(oracle, "e_16x16")
    _, scalar32, modes32 = counts(oracle, "e_32x32")
    assert modes32 - modes16 < scalar32 - scalar16


# ---- the public surfaces ---------------------------------------------------------------------------------------------------------
def test_public_surface():
    for fma in (False, True):
        lib = ctypes.CDLL(_lib.library_path(fma=fma))
        for name in ABI:
            assert hasattr(lib, name), (name, fma)
            assert name in _lib.exported_symbols()
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for line in ("#define SMM_AMG_MAX_CANDIDATES 6", "#define SMM_AMG_MAX_DOFS_PER_NODE 4", "#define SMM_AMG_DROP_TOL 0.0001220703125", "#define SMM_AMG_QR_LDS_ROWS 256"):
        assert line in header
    B = np.ones((4, 1))
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, host.SolverPreconditioner.JACOBI, candidates=B)  # refused before the handle is touched
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, "AMG", dofs_per_node=2)
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, "AMG", candidates=B, degree=3)
    assert hasattr(host.Preconditioner, "amg_candidates")


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::AMGPreconditioner<double> with candidates through ConjugateGradient; -Wall -Werror.  Without a GPU the call reports DIVERGED
    with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "small"
    status, hip = int(words[2]), int(words[4])
    if os.path.exists("/dev/kfd"):
        assert (status, hip) == (0, 0), words
        np.testing.assert_allclose([float.fromhex(w) for w in words[6:10]], 1.0, rtol=1e-8)
    else:
        assert (status, hip) == (1, -3), words
