"""The iterated triangular sweeps on the CPU (tests/jsweep_restatement.py) against the oracle's exact sweeps: exact at levels - 1 steps,
not yet at levels - 2, symmetric at equal counts, fewer solver iterations than without a preconditioner; the ABI surface.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from jsweep_restatement import IC0, ILU0, SGS, apply, bicgstab, exact, factor, levels, make_apply, pcg, split

from sparse_matrix_math_amd import _lib, host
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
CASE = os.path.join(ROOT, "tests", "cpp", "jsweep_case.cpp")
DTYPES = [np.float32, np.float64]
BASES = (SGS, ILU0, IC0)
NEW_SYMBOLS = ("smm_hip_precond_create_jsweep", "smm_hip_precond_jsweep_info", "smm_hip_precond_jsweep_set_sweeps", "smm_hip_precond_jsweep_refresh")
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_CACHE = {}


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def chain(n, dtype, diag=2.0):
    """the n-row tridiagonal chain (-1 beside the diagonal): n dependency levels in either sweep.  With 2 on the diagonal (the 1-D
    Laplacian) the ILU0 / IC0 factors couple a row to its neighbour with a weight that tends to 1, with 1 on the diagonal SGS does: a
    change in one row reaches the far end undamped, so a truncated sweep cannot have settled on the exact bits early (with a dominant
    diagonal it does: 4 / -1 reaches the exact fp32 result after some twenty steps)"""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.concatenate([np.full(n - 1, -1.0), np.full(n, diag), np.full(n - 1, -1.0)])
    order = np.lexsort((cols, rows))
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=start[1:])
    return start, cols[order].astype(np.int32), vals[order].astype(dtype)


def arrow(n, dtype):
    """a diagonal plus a full last row and a full last column: rows of one level beside an (n - 1)-entry row; symmetric positive definite"""
    start = np.zeros(n + 1, dtype=np.int32)
    start[1:n] = 2 * np.arange(1, n)
    start[n] = 2 * (n - 1) + n
    pos = np.empty(start[n], dtype=np.int32)
    val = np.empty(start[n], dtype=dtype)
    pos[0:2 * (n - 1):2] = np.arange(n - 1)
    pos[1:2 * (n - 1):2] = n - 1
    val[0:2 * (n - 1):2] = 3.0 + (np.arange(n - 1) % 5) / 8
    val[1:2 * (n - 1):2] = -1.0 / (1 + np.arange(n - 1) % 7)
    pos[2 * (n - 1):] = np.arange(n)
    val[2 * (n - 1):-1] = val[1:2 * (n - 1):2]
    val[-1] = n
    return start, pos, val


def from_dense(dense, dtype):
    start = np.zeros(len(dense) + 1, dtype=np.int32)
    np.cumsum((dense != 0).sum(axis=1), out=start[1:])
    return start, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(dtype)


def cross(n, dtype):
    """a diagonal plus a full first and a full last row and column; symmetric, dominant diagonal.  The last row's n - 1 lower entries and
    the first row's n - 1 upper entries are more than a wavefront stages (512), every other wavefront holds 64 or so: rows walked from
    global memory and rows walked from LDS inside one workgroup, in both triangles"""
    j = np.arange(n)
    dense = np.diag(3.0 + (j % 5) / 8)
    dense[0, :] = dense[:, 0] = -1.0 / (1 + j % 7)
    dense[n - 1, :] = dense[:, n - 1] = -1.0 / (1 + j % 5)
    dense[0, 0] = dense[n - 1, n - 1] = n
    return from_dense(dense, dtype)


def band(n, width, dtype):
    """`width` sub- and super-diagonals, symmetric, dominant diagonal: with width 10 a wavefront's 64 rows hold some 640 entries of either
    triangle -- every full wavefront walks from global memory, the last, partial one from LDS; n dependency levels"""
    i, j = np.indices((n, n))
    dist = np.abs(i - j)
    dense = np.where((dist > 0) & (dist <= width), -1.0 / (1 + dist % 3), 0.0)
    dense[np.arange(n), np.arange(n)] = 2.0 * width + 5
    return from_dense(dense, dtype)


def wave_entries(csr):
    """per triangle the entries each wavefront of 64 consecutive rows holds"""
    lo, up, _ = split(csr[0], csr[1])
    n = len(csr[0]) - 1
    return [np.add.reduceat((idx >= 0).sum(axis=1), np.arange(0, n, 64)) for idx in (lo, up)]


def ragged(dtype):
    """random_rows with a dominant diagonal, every fifth row cut down to its diagonal alone"""
    start, pos, val = gen.random_rows(200, 200, 1, 9, seed=7, dtype=dtype, diag_dominant=True)
    keep = np.ones(len(pos), dtype=bool)
    rowof = np.repeat(np.arange(200), np.diff(start))
    keep[(rowof % 5 == 0) & (pos != rowof)] = False
    s2 = np.zeros(201, dtype=np.int32)
    np.cumsum(np.bincount(rowof[keep], minlength=200), out=s2[1:])
    return s2, np.ascontiguousarray(pos[keep]), np.ascontiguousarray(val[keep])


def js_matrix(name, dtype):
    """the matrices of the apply comparisons, made once per dtype"""
    key = (name, np.dtype(dtype).name)
    if key not in _CACHE:
        csr = {"poisson2d_9x7": lambda: gen.poisson2d(9, 7, dtype=dtype), "convdiff3d_5": lambda: gen.convdiff3d(5, 0.3, dtype=dtype),
               "chain_65": lambda: chain(65, dtype), "chain_65_sgs": lambda: chain(65, dtype, 1.0), "arrow_300": lambda: arrow(300, dtype), "cross_700": lambda: cross(700, dtype), "band10_300": lambda: band(300, 10, dtype), "ragged_200": lambda: ragged(dtype),
               "one": lambda: (np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([2.5], dtype=dtype)),
               "none": lambda: (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)),
               "poisson2d_5": lambda: gen.poisson2d(5, dtype=dtype), "poisson2d_24": lambda: gen.poisson2d(24, dtype=dtype),
               "poisson2d_32": lambda: gen.poisson2d(32, dtype=dtype), "convdiff3d_10": lambda: gen.convdiff3d(10, 0.3, dtype=dtype),
               "convdiff3d_12": lambda: gen.convdiff3d(12, 0.3, dtype=dtype)}[name]()
        _CACHE[key] = tuple(np.ascontiguousarray(a) for a in csr)
    return _CACHE[key]


NAMES = ("poisson2d_9x7", "convdiff3d_5", "chain_65", "arrow_300", "cross_700", "band10_300", "ragged_200", "one", "none")
SPD = ("poisson2d_9x7", "chain_65", "arrow_300", "cross_700", "band10_300", "one", "none")  # IC0 needs a symmetric positive definite matrix
CASES = [(n, b) for n in NAMES for b in BASES if b != IC0 or n in SPD]


def chain_for(base):
    """the chain on which that base's sweeps carry a change undamped (chain's docstring)"""
    return "chain_65_sgs" if base == SGS else "chain_65"


def rhs_of(n, dtype):
    return np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)


def test_the_test_matrices_are_what_they_claim():
    assert levels(*js_matrix("chain_65", np.float64)[:2]) == (65, 65)
    assert levels(*js_matrix("arrow_300", np.float64)[:2]) == (2, 2)
    assert levels(*js_matrix("none", np.float64)[:2]) == (0, 0) and levels(*js_matrix("one", np.float64)[:2]) == (1, 1)
    start, pos, _ = js_matrix("ragged_200", np.float64)
    assert (np.diff(start)[::5] == 1).all() and np.diff(start).max() > 4
    assert np.diff(js_matrix("arrow_300", np.float64)[0]).max() == 300
    # the kernel stages up to 512 entries of a wavefront's 64 rows through LDS and walks longer ranges from global memory: both paths, in
    # both triangles, inside one 256-row workgroup
    for name in ("cross_700", "band10_300"):
        for counts in wave_entries(js_matrix(name, np.float64)):
            assert counts.max() > 512 and counts.min() <= 512, (name, counts)
    lo, up = wave_entries(js_matrix("cross_700", np.float64))
    assert lo[10] > 512 and lo[8] <= 512 and lo[9] <= 512 and up[0] > 512 and up[1] <= 512  # workgroups of rows 512 .. 699 and 0 .. 255
    assert levels(*js_matrix("cross_700", np.float64)[:2]) == (3, 3) and levels(*js_matrix("band10_300", np.float64)[:2]) == (300, 300)
    assert max(c.max() for n in ("poisson2d_9x7", "convdiff3d_5", "chain_65", "arrow_300", "ragged_200") for c in wave_entries(js_matrix(n, np.float64))) <= 512


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,base", CASES)
def test_exact_at_levels_minus_one(oracle, name, base, dtype):
    """after k steps every row of level <= k holds the exact sweep's bits: levels - 1 steps give the oracle's sequential sweeps"""
    csr = js_matrix(name, dtype)
    n = len(csr[0]) - 1
    f = factor(oracle, csr, base)
    lo, up = levels(csr[0], csr[1])
    r = rhs_of(n, dtype)
    z = apply(csr[0], csr[1], f, base, max(1, lo - 1), max(1, up - 1), r)
    np.testing.assert_array_equal(bits(z), bits(exact(oracle, csr, base, f, r)))
    z = apply(csr[0], csr[1], f, base, lo + 2, up + 3, r)  # and it stays there
    np.testing.assert_array_equal(bits(z), bits(exact(oracle, csr, base, f, r)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
def test_truncation_is_really_applied(oracle, base, dtype):
    """the 65-row chain with a right-hand side of ones at levels - 2 = 63 steps: the deepest row is not final yet"""
    csr = js_matrix(chain_for(base), dtype)
    f = factor(oracle, csr, base)
    r = np.ones(65, dtype=dtype)
    want = exact(oracle, csr, base, f, r)
    np.testing.assert_array_equal(bits(apply(csr[0], csr[1], f, base, 64, 64, r)), bits(want))
    short = apply(csr[0], csr[1], f, base, 63, 64, r)
    assert not np.array_equal(bits(short), bits(want))
    assert not np.array_equal(bits(apply(csr[0], csr[1], f, base, 64, 63, r)), bits(want))


@pytest.mark.parametrize("base", (SGS, IC0))
def test_symmetric_at_equal_counts(oracle, base):
    """the operator applied to the unit vectors of poisson2d(5) equals its transpose to rounding; with unequal counts it does not"""
    csr = js_matrix("poisson2d_5", np.float64)
    n = 25
    fn = make_apply(oracle, csr, base, 3, 3)
    op = np.stack([fn(e) for e in np.eye(n)], axis=1)
    assert np.max(np.abs(op - op.T)) <= 8 * np.finfo(np.float64).eps * np.max(np.abs(op))
    assert np.all(np.linalg.eigvalsh((op + op.T) / 2) > 0)
    fn = make_apply(oracle, csr, base, 1, 4)
    op = np.stack([fn(e) for e in np.eye(n)], axis=1)
    assert np.max(np.abs(op - op.T)) > 1e-4 * np.max(np.abs(op))


@pytest.mark.parametrize("name,base,solver", [("convdiff3d_12", ILU0, "bicgstab"), ("convdiff3d_12", SGS, "bicgstab"), ("poisson2d_32", IC0, "cg"),
                                              ("poisson2d_32", SGS, "cg")])
def test_three_sweeps_need_fewer_iterations_than_none(oracle, name, base, solver):
    """fp64 to 1e-8: strictly fewer iterations than without a preconditioner (a condition, not a tuned bound)"""
    csr = js_matrix(name, np.float64)
    b = gen.row_sums(csr[0], csr[2])
    zero = np.zeros(len(b))
    loop = pcg if solver == "cg" else bicgstab
    st0, _, it0, _ = loop(oracle, csr, b, zero, -1, 1e-8, lambda r: r.copy())
    st, x, it, _ = loop(oracle, csr, b, zero, -1, 1e-8, make_apply(oracle, csr, base, 3, 3))
    print(name, base, solver, "iterations", it, "without a preconditioner", it0)
    assert st == st0 == 0 and it < it0
    np.testing.assert_allclose(x, 1.0, atol=1e-5)


def test_abi_surface():
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols()
    lib = _lib.load()
    assert len(lib.smm_hip_precond_create_jsweep.argtypes) == 5 and len(lib.smm_hip_precond_jsweep_info.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for line in ("#define SMM_PRECOND_JSWEEP_SGS 14", "#define SMM_PRECOND_JSWEEP_ILU0 15", "#define SMM_PRECOND_JSWEEP_IC0 16", "#define SMM_JSWEEP_DEFAULT_SWEEPS 3",
                 "#define SMM_JSWEEP_MAX_SWEEPS 1024"):
        assert line in header
    P = host.SolverPreconditioner
    assert (int(P.JSWEEP_SGS), int(P.JSWEEP_ILU0), int(P.JSWEEP_IC0)) == (14, 15, 16)
    for name in ("jsweep_info", "jsweep_set_sweeps", "jsweep_refresh"):
        assert callable(getattr(host.Preconditioner, name))
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, P.ILU0, sweeps=3)  # refused before the handle is touched
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, "JSWEEP_ILU0", sweeps=3, power=2)


def build_case(tmp_path):
    """the g++ line of tests/test_multicolor_cpu.py::build_case for tests/cpp/jsweep_case.cpp"""
    exe = tmp_path / "jsweep_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::JacobiSweepPreconditioner<T> through BiCGStab and ConjugateGradient, info / setSweeps / refresh; -Wall -Werror.  Without a GPU
    every call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 10
    if not os.path.exists("/dev/kfd"):
        for ln in lines:
            if "-exact" in ln:
                assert ln.endswith("same 0 one_step_same 0") and f"hip {_lib.SMM_HIP_ERR_NO_DEVICE}" in ln
            else:
                assert f"status 1 hip {_lib.SMM_HIP_ERR_NO_DEVICE}" in ln
