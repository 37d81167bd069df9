"""The multicolour reordering on the CPU (tests/multicolor_restatement.py): every colouring is proper, the colours are contiguous after the
permutation, the permuted matrix has as many dependency levels as colours, its row sums are those of the matrix, the restated loops
converge; the ABI surface and the drop-in C++ case.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from chebyshev_restatement import bicgstab, pcg
from multicolor_restatement import IC0, ILU0, SGS, bounds, color, is_proper, keys, make_apply, permutation, permute, setup, splitmix64
from test_chebyshev_cpu import spd5
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib, host
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
CASE = os.path.join(ROOT, "tests", "cpp", "multicolor_case.cpp")
NAMES = ("poisson2d_32", "convdiff3d_12", "convdiff3d_20", "banded_2000", "random_500", "dense70_in_200", "spd5", "one")
SYMMETRIC = ("poisson2d_32", "convdiff3d_12", "convdiff3d_20", "banded_2000", "dense70_in_200", "spd5", "one")
NEW_SYMBOLS = ("smm_hip_csr_color", "smm_hip_csr_color_dev", "smm_hip_csr_permute_create", "smm_hip_csr_permute_create_dev", "smm_hip_csr_permute_refresh_f32",
               "smm_hip_csr_permute_refresh_f64", "smm_hip_precond_create_multicolor", "smm_hip_precond_multicolor_refresh", "smm_hip_precond_multicolor_info",
               "smm_hip_precond_multicolor_perm", "smm_hip_precond_multicolor_matrix")

_CACHE = {}


def dense_block(dtype, n=200, first=40, size=70):
    """the identity with a dense, diagonally dominant size x size block at rows first .. first + size: that many colours"""
    rng = np.random.default_rng(11)
    dense = np.eye(n)
    blk = rng.uniform(-1, 1, (size, size))
    blk = (blk + blk.T) / 2
    blk[np.arange(size), np.arange(size)] = size + 1.0
    dense[first:first + size, first:first + size] = blk
    start = np.zeros(n + 1, dtype=np.int32)
    np.cumsum((dense != 0).sum(axis=1), out=start[1:])
    pos = np.nonzero(dense)[1].astype(np.int32)
    return start, pos, dense[dense != 0].astype(dtype)


def mc_matrix(name, dtype):
    """the matrices of the issue, made once per dtype"""
    key = (name, np.dtype(dtype).name)
    if key not in _CACHE:
        if name == "convdiff3d_20":
            csr = gen.convdiff3d(20, 0.3, dtype=dtype)
        elif name == "random_500":
            csr = gen.random_rows(500, 500, 3, 12, seed=3, dtype=dtype, diag_dominant=True)
        elif name == "dense70_in_200":
            csr = dense_block(dtype)
        elif name == "spd5":
            csr = spd5(dtype)
        elif name == "one":
            csr = (np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([2.5], dtype=dtype))
        else:
            csr = gen_matrices(dtype)[name]
        _CACHE[key] = tuple(np.ascontiguousarray(a) for a in csr)
    return _CACHE[key]


def colored(name):
    key = ("color", name)
    if key not in _CACHE:
        _CACHE[key] = color(mc_matrix(name, np.float64))
    return _CACHE[key]


def test_keys_are_splitmix64():
    """the published test vector of splitmix64 seeded with 0 (its first output), and no ties among the first 2^16 keys"""
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    assert len(set(keys(1 << 16))) == 1 << 16


@pytest.mark.parametrize("name", NAMES)
def test_colouring_is_proper_and_contiguous(name):
    csr = mc_matrix(name, np.float64)
    colors, ncolors = colored(name)
    n = len(colors)
    print(name, "rows", n, "colours", ncolors, "sizes", np.bincount(colors)[:12])
    assert colors.min() >= 0 and is_proper(csr, colors)
    assert set(colors.tolist()) == set(range(ncolors))  # greedy leaves no colour unused
    perm = permutation(colors)
    assert sorted(perm.tolist()) == list(range(n))
    bnd = bounds(colors, ncolors)
    assert bnd[0] == 0 and bnd[-1] == n
    for c in range(ncolors):
        rows = perm[bnd[c]:bnd[c + 1]]
        assert (colors[rows] == c).all() and (np.diff(rows) > 0).all()  # contiguous, original index ascending inside a colour
    # rows of one colour do not reference each other in B
    bstart, bpos, _ = permute(csr, perm)
    rowof = np.repeat(np.arange(n), np.diff(bstart))
    color_of_new = colors[perm]
    off = rowof != bpos
    assert not np.any(color_of_new[rowof[off]] == color_of_new[bpos[off]])
    assert all((np.diff(bpos[bstart[i]:bstart[i + 1]]) > 0).all() for i in range(n))


def test_the_pattern_of_random_rows_is_not_symmetric():
    start, pos, _ = mc_matrix("random_500", np.float64)
    stored = set(zip(np.repeat(np.arange(500), np.diff(start)).tolist(), pos.tolist()))
    assert any((j, i) not in stored for i, j in stored)


def test_dense_block_needs_more_than_64_colours():
    assert colored("dense70_in_200")[1] == 70
    assert colored("one")[1] == 1


@pytest.mark.parametrize("name", NAMES)
def test_levels_of_the_permuted_matrix(oracle, name):
    """the oracle's level count on B (both sweeps, one block, no cut): ncolors for a symmetric pattern -- a row of colour c has a neighbour
    of every smaller colour --, never more"""
    csr = mc_matrix(name, np.float64)
    colors, ncolors = colored(name)
    bcsr = permute(csr, permutation(colors))
    n = len(colors)
    _, deepest = oracle.block_level_cut(bcsr, np.array([0, n], dtype=np.int32), 0)
    _, natural = oracle.block_level_cut(csr, np.array([0, n], dtype=np.int32), 0)
    print(name, "levels natural", natural, "multicolour", deepest, "colours", ncolors)
    assert deepest <= ncolors
    if name in SYMMETRIC:
        assert deepest == ncolors


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", ("convdiff3d_12", "random_500", "dense70_in_200"))
def test_row_sums_of_the_permuted_matrix(oracle, name, dtype):
    """B (P x) = P (A x): every row holds the same products, so the exact sums agree bit for bit and the oracle's sequential sums agree up to
    the summation order (one rounding per entry)"""
    csr = mc_matrix(name, dtype)
    perm = permutation(colored(name)[0])
    bcsr = permute(csr, perm)
    n = len(perm)
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(dtype)
    px = np.ascontiguousarray(x[perm])
    for i in range(n):
        r = perm[i]
        a = sorted((csr[2][csr[0][r]:csr[0][r + 1]].astype(np.float64) * x[csr[1][csr[0][r]:csr[0][r + 1]]].astype(np.float64)).tolist())
        b = sorted((bcsr[2][bcsr[0][i]:bcsr[0][i + 1]].astype(np.float64) * px[bcsr[1][bcsr[0][i]:bcsr[0][i + 1]]].astype(np.float64)).tolist())
        assert a == b and math.fsum(a) == math.fsum(b)
    got = oracle.spmv(bcsr, 0, None, px).astype(np.float64)
    want = oracle.spmv(csr, 0, None, x)[perm].astype(np.float64)
    length = np.diff(bcsr[0])
    mag = oracle.spmv((bcsr[0], bcsr[1], np.abs(bcsr[2])), 0, None, np.abs(px)).astype(np.float64)
    assert np.all(np.abs(got - want) <= 2 * length * np.finfo(dtype).eps * mag)


@pytest.mark.parametrize("name,base,solver", [("poisson2d_32", IC0, "cg"), ("poisson2d_32", SGS, "cg"), ("banded_2000", IC0, "cg"), ("convdiff3d_12", SGS, "bicgstab"),
                                              ("convdiff3d_12", ILU0, "bicgstab"), ("random_500", ILU0, "bicgstab"), ("dense70_in_200", SGS, "bicgstab"),
                                              ("spd5", IC0, "cg"), ("one", SGS, "cg")])
def test_restated_loops_converge(oracle, name, base, solver):
    csr = mc_matrix(name, np.float64)
    b = gen.row_sums(csr[0], csr[2])
    fn = make_apply(oracle, csr, base)
    zero = np.zeros(len(b))
    loop = pcg if solver == "cg" else bicgstab
    st, x, it, _ = loop(oracle, csr, b, zero, -1, 1e-8, fn)
    print(name, base, solver, "iterations", it, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == 0 and it <= len(b)
    np.testing.assert_allclose(x, 1.0, atol=1e-5)


def test_a_callers_colouring_is_honoured(oracle):
    """red-black on the 5-point grid: two colours, and another preconditioner than the greedy colouring's"""
    csr = mc_matrix("poisson2d_32", np.float64)
    i = np.arange(32 * 32)
    redblack = ((i // 32 + i % 32) % 2).astype(np.int32)
    assert is_proper(csr, redblack)
    _, ncolors, perm, _, _ = setup(oracle, csr, SGS, redblack)
    assert ncolors == 2 and (np.diff(perm[:512]) > 0).all()
    r = np.random.default_rng(4).uniform(-1, 1, 1024)
    assert not np.array_equal(make_apply(oracle, csr, SGS, redblack)(r), make_apply(oracle, csr, SGS)(r))


def test_abi_surface():
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols()
    lib = _lib.load()
    assert len(lib.smm_hip_csr_permute_create.argtypes) == 5 and len(lib.smm_hip_precond_create_multicolor.argtypes) == 5
    header = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for line in ("#define SMM_PRECOND_MULTICOLOR_SGS 9", "#define SMM_PRECOND_MULTICOLOR_ILU0 10", "#define SMM_PRECOND_MULTICOLOR_IC0 11"):
        assert line in header
    P = host.SolverPreconditioner
    assert (int(P.MULTICOLOR_SGS), int(P.MULTICOLOR_ILU0), int(P.MULTICOLOR_IC0)) == (9, 10, 11)
    for name in ("color", "permute", "permute_refresh"):
        assert callable(getattr(host.CSRMatrix, name))
    for name in ("multicolor_info", "multicolor_perm", "multicolor_matrix", "multicolor_refresh"):
        assert callable(getattr(host.Preconditioner, name))
    with pytest.raises(ValueError):
        host.CSRMatrix.getPreconditioner(None, P.JACOBI, colors=[0, 1])  # refused before the handle is touched


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_colouring_without_gpu():
    import sparse_matrix_math_amd as smm

    with pytest.raises(smm.SmmHipError) as e:
        smm.CSRMatrix(5, 5, *spd5(np.float64))
    assert e.value.code == _lib.SMM_HIP_ERR_NO_DEVICE


def build_case(tmp_path):
    """the g++ line of tests/gmres_helpers.py for tests/cpp/multicolor_case.cpp"""
    exe = tmp_path / "multicolor_case"
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}",
           "-o", str(exe), CASE, f"-L{LIB}", "-lsmm_hip", f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_cpp_case_compiles_against_the_dropin_header(tmp_path):
    """SMM::MulticolorPreconditioner<T, Base> through BiCGStab and ConjugateGradient, SMM::color / permute / permuteRefresh; -Wall -Werror.
    Without a GPU every call reports DIVERGED with SMM_HIP_ERR_NO_DEVICE beside it."""
    if not os.path.exists(os.path.join(LIB, "libsmm_hip.so")):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 10
    if not os.path.exists("/dev/kfd"):
        for ln in lines:
            if "-permute" in ln:
                assert ln.endswith("same 0") and f"hip {_lib.SMM_HIP_ERR_NO_DEVICE}" in ln
            else:
                assert f"status 1 hip {_lib.SMM_HIP_ERR_NO_DEVICE}" in ln
