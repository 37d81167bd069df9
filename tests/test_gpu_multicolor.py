"""The multicolour reordering on the GPU (csrc/smm_color.hip, csrc/smm_precond_mc.hip) through the C ABI, against its CPU restatement
(tests/multicolor_restatement.py): the colours, the permutation and the permuted matrix exactly, the applies and the factors bit for bit,
the solvers by the fixed-pass tolerance rule of tests/test_gpu_cgs.py, a caller's colouring, refresh, the refusals, the fma flavour and
the drop-in C++ header."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch
from chebyshev_restatement import bicgstab, pcg, sensitivity
from device_views import assert_guards_intact, assert_unchanged, carve_like, fit, snapshot
from gmres_restatement import gmres
from gmres_restatement import sensitivity as gmres_sensitivity
from multicolor_restatement import IC0, ILU0, SGS, bounds, color, make_apply, permutation, permute, setup
from test_gpu_cgs import allowed, make, worst
from test_multicolor_cpu import NAMES, build_case, mc_matrix
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID, PRECOND = -1, -4  # SMM_HIP_ERR_INVALID, SMM_HIP_ERR_PRECOND
BASES = (SGS, ILU0, IC0)
KIND = {SGS: "MULTICOLOR_SGS", ILU0: "MULTICOLOR_ILU0", IC0: "MULTICOLOR_IC0"}
SPD = ("poisson2d_32", "convdiff3d_20", "banded_2000", "dense70_in_200", "spd5", "one")  # IC0 needs a symmetric positive definite matrix
ids = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731

_REF = {}


def cached(key, compute):
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def spd_matrix(name, dtype):
    """the matrix of that name; for IC0 the convection-diffusion ones are replaced by their symmetric part's stand-in, the Laplacian"""
    if name == "convdiff3d_20":
        return cached(("poisson3d_20", np.dtype(dtype).name), lambda: gen.poisson3d(20, dtype=dtype))
    return mc_matrix(name, dtype)


def case(name, base, dtype):
    return spd_matrix(name, dtype) if base == IC0 else mc_matrix(name, dtype)


def restated_setup(oracle, tag, name, base, dtype, colors=None, ckey=None):
    return cached(("setup", tag, name, base, np.dtype(dtype).name, ckey), lambda: setup(oracle, case(name, base, dtype), base, colors))


def rhs_of(n, dtype):
    return np.random.default_rng(5).uniform(-1, 1, n).astype(dtype)


def redblack(nx, ny):
    i = np.arange(nx * ny)
    return ((i // nx + i % nx) % 2).astype(np.int32)


def code_of(call):
    with pytest.raises(_lib.SmmHipError) as e:
        call()
    return e.value.code


# ---- colouring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_colours_bounds_and_permutation_equal_the_restatement(smm, name, dtype):
    csr = mc_matrix(name, dtype)
    colors_ref, ncolors_ref = cached(("color", name), lambda: color(mc_matrix(name, np.float64)))
    A = make(smm, csr)
    colors, ncolors = A.color()
    print(name, np.dtype(dtype).name, "colours", ncolors, "restated", ncolors_ref)
    assert ncolors == ncolors_ref
    np.testing.assert_array_equal(colors, colors_ref)
    M = A.getPreconditioner("MULTICOLOR_SGS")
    n, bnd = M.multicolor_info()
    assert n == ncolors_ref and M.levels() == (ncolors_ref, ncolors_ref)
    np.testing.assert_array_equal(bnd, bounds(colors_ref, ncolors_ref))
    np.testing.assert_array_equal(M.multicolor_perm(), permutation(colors_ref))
    d_colors = carve_like(np.full(len(colors), -7, dtype=np.int32), 1, device="cuda:0")
    assert A.color_dev(d_colors) == ncolors_ref
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_colors.cpu().numpy(), colors_ref)
    assert_guards_intact(d_colors, "colors")


# ---- permutation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_permute_equals_numpy_bit_for_bit(smm, name, dtype):
    csr = mc_matrix(name, dtype)
    n = len(csr[0]) - 1
    A = make(smm, csr)
    for perm in (permutation(cached(("color", name), lambda: color(mc_matrix(name, np.float64)))[0]), np.random.default_rng(9).permutation(n).astype(np.int32)):
        want = permute(csr, perm)
        B = A.permute(perm)
        start, pos = B.get_pattern()
        np.testing.assert_array_equal(start, want[0])
        np.testing.assert_array_equal(pos, want[1])
        np.testing.assert_array_equal(bits(B.get_values()), bits(want[2]))
    # the matrix multicolor_matrix lends is that matrix
    M = A.getPreconditioner("MULTICOLOR_SGS")
    Bm = M.multicolor_matrix()
    want = permute(csr, M.multicolor_perm())
    np.testing.assert_array_equal(Bm.get_pattern()[1], want[1])
    np.testing.assert_array_equal(bits(Bm.get_values()), bits(want[2]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_permute_refresh_follows_value_edits(smm, dtype):
    csr = mc_matrix("convdiff3d_12", dtype)
    n = len(csr[0]) - 1
    perm = np.random.default_rng(3).permutation(n).astype(np.int32)
    A = make(smm, csr)
    B = A.permute(perm)
    A.scale(0.375)
    B.permute_refresh(A)
    np.testing.assert_array_equal(bits(B.get_values()), bits(A.permute(perm).get_values()))
    rows = np.array([0, 5, n - 1, 7], dtype=np.int32)
    assert A.update_entries(rows, rows, np.array([9.5, -3.25, 77.0, 0.125], dtype=dtype)).all()
    B.permute_refresh(A)
    fresh = permute((csr[0], csr[1], A.get_values()), perm)
    np.testing.assert_array_equal(bits(B.get_values()), bits(fresh[2]))
    # a matrix with the source's pattern serves as well; y = B (P x) follows
    twin = make(smm, (csr[0], csr[1], (csr[2] * dtype(2)).astype(dtype)))
    B.permute_refresh(twin)
    np.testing.assert_array_equal(bits(B.get_values()), bits(permute((csr[0], csr[1], (csr[2] * dtype(2)).astype(dtype)), perm)[2]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_permute_refusals(smm, dtype):
    csr = mc_matrix("spd5", dtype)
    A = make(smm, csr)
    good = np.array([4, 2, 0, 1, 3], dtype=np.int32)
    B = A.permute(good)
    before = B.get_values().copy()
    for bad in ([0, 1, 2, 3, 5], [0, 1, 2, 3, -1], [0, 1, 2, 2, 4], [0, 1, 2, 3], [0, 1, 2, 3, 4, 0]):
        assert code_of(lambda: A.permute(np.array(bad, dtype=np.int32))) == INVALID
    W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
    assert code_of(lambda: W.permute(np.array([0, 1], dtype=np.int32))) == INVALID
    assert code_of(lambda: W.color()) == INVALID
    # refresh: a handle of foreign origin, another shape, another pattern, the other dtype
    assert code_of(lambda: A.permute_refresh(B)) == INVALID
    assert code_of(lambda: A.transpose().permute_refresh(A)) == INVALID
    assert code_of(lambda: B.transpose_refresh(A)) == INVALID
    assert code_of(lambda: B.permute_refresh(make(smm, mc_matrix("one", dtype)))) == INVALID
    assert not np.array_equal(B.get_pattern()[1], csr[1])
    assert code_of(lambda: B.permute_refresh(B)) == INVALID  # the shape and entry count of the source, another pattern
    odt = np.float32 if dtype == np.float64 else np.float64
    assert code_of(lambda: B.permute_refresh(make(smm, mc_matrix("spd5", odt)))) == INVALID
    np.testing.assert_array_equal(bits(B.get_values()), bits(before))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_permute_device_pointers_on_offset_views(smm, dtype):
    csr = mc_matrix("random_500", dtype)
    n = len(csr[0]) - 1
    perm = np.random.default_rng(12).permutation(n).astype(np.int32)
    A = make(smm, csr)
    for residue in (1, 3):
        d_perm = carve_like(perm, residue, device="cuda:0")
        saved = snapshot(d_perm)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        B = A.permute_dev(d_perm, n, s.cuda_stream)
        torch.cuda.synchronize()
        want = permute(csr, perm)
        np.testing.assert_array_equal(B.get_pattern()[0], want[0])
        np.testing.assert_array_equal(B.get_pattern()[1], want[1])
        np.testing.assert_array_equal(bits(B.get_values()), bits(want[2]))
        assert_unchanged(d_perm, saved, "perm")
        assert_guards_intact(d_perm, "perm")
    bad = perm.copy()
    bad[17] = bad[18]
    assert code_of(lambda: A.permute_dev(carve_like(bad, 1, device="cuda:0"), n)) == INVALID
    assert code_of(lambda: A.permute_dev(carve_like(perm, 1, device="cuda:0"), n - 1)) == INVALID


# ---- apply and factors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,base", [(n, b) for n in NAMES for b in BASES if b != IC0 or n in SPD])
def test_apply_and_factor_bit_for_bit(smm, oracle, name, base, dtype):
    csr = case(name, base, dtype)
    _, ncolors, perm, bcsr, f = restated_setup(oracle, "plain", name, base, dtype)
    n = len(perm)
    r = rhs_of(n, dtype)
    z_ref = cached(("apply", "plain", name, base, np.dtype(dtype).name), lambda: make_apply(oracle, csr, base)(r))
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    assert M.multicolor_info()[0] == ncolors
    z = np.full(n, np.nan, dtype=dtype)
    saved = r.copy()
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(z_ref))
    np.testing.assert_array_equal(bits(r), bits(saved))
    if base != SGS:
        np.testing.assert_array_equal(bits(M.values()), bits(f))
    assert code_of(lambda: M.apply(r, r)) == INVALID  # rhs aliases x: refused like the exact kinds (ref:1667)
    np.testing.assert_array_equal(bits(r), bits(saved))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("nx,ny", [(32, 64), (45, 45), (41, 50), (33, 62)])
def test_colour_sizes_around_the_chain_limit(smm, oracle, nx, ny, base, dtype):
    """red-black on nx x ny grids: colours of 1024 / 1024, 1013 / 1012, 1025 / 1025 and 1023 / 1023 rows -- at, below and above the 1024
    rows up to which colours are chained inside one workgroup, and off the 256-row workgroups of the large-colour launch"""
    csr = cached(("grid", nx, ny, np.dtype(dtype).name), lambda: gen.poisson2d(nx, ny, dtype=dtype))
    colors = redblack(nx, ny)
    n = nx * ny
    r = rhs_of(n, dtype)
    z_ref = make_apply(oracle, csr, base, colors)(r)
    M = make(smm, csr).getPreconditioner(KIND[base], colors=colors)
    ncolors, bnd = M.multicolor_info()
    assert ncolors == 2 and bnd.tolist() == [0, (n + 1) // 2, n]
    z = np.full(n, np.nan, dtype=dtype)
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(z_ref))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
def test_apply_device_pointers_on_offset_views_and_another_stream(smm, oracle, base, dtype):
    name = "convdiff3d_20"
    csr = case(name, base, dtype)
    n = len(csr[0]) - 1
    r = rhs_of(n, dtype)
    z_ref = cached(("apply", "plain", name, base, np.dtype(dtype).name), lambda: make_apply(oracle, csr, base)(r))
    M = make(smm, csr).getPreconditioner(KIND[base])
    d_r = carve_like(r, fit(1, dtype), device="cuda:0")
    d_z = carve_like(np.zeros(n, dtype=dtype), fit(3, dtype), device="cuda:0")
    saved = snapshot(d_r)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    M.apply_dev(d_r, d_z, s.cuda_stream)
    M.take_error(s.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(d_z.cpu().numpy()), bits(z_ref))
    assert_unchanged(d_r, saved, "rhs")
    assert_guards_intact(d_r, "rhs")
    assert_guards_intact(d_z, "x")


# ---- solvers -----------------------------------------------------------------------------------------------------------------
def restated(oracle, solver, name, base, dtype, it, eps):
    """(status, x, iterations, sensitivity or None) of the restated loop, made once"""
    def compute():
        csr = case(name, base, dtype)
        b = gen.row_sums(csr[0], csr[2])
        fn = make_apply(oracle, csr, base)
        zero = np.zeros(len(b), dtype=dtype)
        if solver == "cg":
            solve = lambda bb: pcg(oracle, csr, bb, zero, it, eps, fn)  # noqa: E731
        elif solver == "bicgstab":
            solve = lambda bb: bicgstab(oracle, csr, bb, zero, it, eps, fn)  # noqa: E731
        else:
            solve = lambda bb: gmres(oracle, csr, bb, zero, it, eps, 30, fn)  # noqa: E731
        st, x, k, _ = solve(b)
        sens = None
        if eps == 0.0:
            sens = gmres_sensitivity(oracle, csr, b, it, 30, x, fn) if solver == "gmres" else sensitivity(lambda bb: solve(bb)[1], b, x)
        return st, x, k, sens
    return cached(("solve", solver, name, base, np.dtype(dtype).name, it, eps), compute)


def run(smm, solver, A, b, it, eps, M, dtype):
    x = np.zeros(len(b), dtype=dtype)
    info = {}
    if solver == "cg":
        st = smm.ConjugateGradient(A, b, np.zeros(len(b), dtype=dtype), x, it, eps, M, info=info)
    elif solver == "bicgstab":
        st = smm.BiCGStab(A, b.copy(), x, it, eps, M, info=info)
    else:
        st = smm.GMRES(A, b.copy(), x, it, eps, 30, M, info=info)
    return int(st), x, info


SOLVES = [("bicgstab", "convdiff3d_12", SGS), ("bicgstab", "convdiff3d_12", ILU0), ("bicgstab", "random_500", ILU0), ("gmres", "convdiff3d_12", ILU0),
          ("cg", "poisson2d_32", IC0), ("cg", "poisson2d_32", SGS), ("cg", "banded_2000", IC0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name,base", SOLVES)
def test_fixed_steps_match_the_restated_loops(smm, oracle, solver, name, base, dtype):
    """the fixed-pass rule of tests/test_gpu_cgs.py: 5 passes with eps = 0 against the restated loop, within `allowed`"""
    it = 5
    csr = case(name, base, dtype)
    b = gen.row_sums(csr[0], csr[2])
    st_ref, x_ref, it_ref, sens = restated(oracle, solver, name, base, dtype, it, 0.0)
    tol = allowed(x_ref, sens, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    st, x, info = run(smm, solver, A, b, it, 0.0, M, dtype)
    err = worst(x, x_ref)
    print(solver, name, base, np.dtype(dtype).name, "max|x - ref|", err, "allowed", tol, "sensitivity", sens, info)
    assert st == st_ref and info["iterations"] == it_ref == it
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("solver,name,base", [("bicgstab", "convdiff3d_20", SGS), ("bicgstab", "convdiff3d_20", ILU0), ("gmres", "convdiff3d_20", SGS),
                                              ("cg", "poisson2d_32", IC0), ("cg", "poisson2d_32", SGS)])
def test_converged_runs(smm, oracle, solver, name, base, dtype):
    """SUCCESS, and the restated loop's iteration count within that rule's slack, max(2, ref // 5)"""
    eps = 1e-8 if dtype == np.float64 else 1e-3
    csr = case(name, base, dtype)
    b = gen.row_sums(csr[0], csr[2])
    st_ref, _, it_ref, _ = restated(oracle, solver, name, base, dtype, -1, eps)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    st, x, info = run(smm, solver, A, b, -1, eps, M, dtype)
    print(solver, name, base, np.dtype(dtype).name, "iterations", info["iterations"], "restated", it_ref, "max|x - 1|", float(np.max(np.abs(x - 1))))
    assert st == st_ref == 0
    assert abs(info["iterations"] - it_ref) <= max(2, it_ref // 5)


def test_refinement_takes_the_kinds(smm):
    """the refinement driver hands M32 to its inner solver: BiCGStab + MULTICOLOR_ILU0 and CG + MULTICOLOR_IC0 on the fp32 copy"""
    for name, inner, kind in (("convdiff3d_12", "BICGSTAB", "MULTICOLOR_ILU0"), ("poisson2d_32", "CG", "MULTICOLOR_IC0")):
        csr = mc_matrix(name, np.float64)
        b = gen.row_sums(csr[0], csr[2])
        A = make(smm, csr)
        A32 = A.astype(np.float32)
        M32 = A32.getPreconditioner(kind)
        x = np.zeros(len(b))
        info = {}
        st = smm.IterativeRefinement(A, b, x, 1e-10, inner=inner, a32=A32, M=M32, info=info)
        print(name, inner, kind, info)
        assert int(st) == 0
        np.testing.assert_allclose(x, 1.0, atol=1e-8)


# ---- a caller's colouring, refresh -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_a_callers_colouring(smm, oracle, dtype):
    csr = mc_matrix("poisson2d_32", dtype)
    colors = redblack(32, 32)
    r = rhs_of(1024, dtype)
    A = make(smm, csr)
    for base in BASES:
        M = A.getPreconditioner(KIND[base], colors=colors)
        ncolors, bnd = M.multicolor_info()
        assert ncolors == 2 and bnd.tolist() == [0, 512, 1024] and M.levels() == (2, 2)
        np.testing.assert_array_equal(M.multicolor_perm(), permutation(colors))
        z = np.zeros(1024, dtype=dtype)
        M.apply(r, z)
        np.testing.assert_array_equal(bits(z), bits(make_apply(oracle, csr, base, colors)(r)))
    # not a colouring: two neighbours share a colour; a colour out of range; a wrong count
    bad = colors.copy()
    bad[1] = bad[0]
    assert code_of(lambda: A.getPreconditioner("MULTICOLOR_SGS", colors=bad)) == INVALID
    for v in (-1, 1024):
        bad = colors.copy()
        bad[100] = v
        assert code_of(lambda: A.getPreconditioner("MULTICOLOR_ILU0", colors=bad)) == INVALID
    assert code_of(lambda: A.getPreconditioner("MULTICOLOR_SGS", colors=colors[:-1])) == INVALID
    # colours nobody holds are empty levels: 0 and 5 instead of 0 and 1
    sparse = (colors * 5).astype(np.int32)
    M = A.getPreconditioner("MULTICOLOR_SGS", colors=sparse)
    assert M.multicolor_info()[1].tolist() == [0, 512, 512, 512, 512, 512, 1024]
    z = np.zeros(1024, dtype=dtype)
    M.apply(r, z)
    np.testing.assert_array_equal(bits(z), bits(make_apply(oracle, csr, SGS, colors)(r)))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("base", BASES)
def test_refresh_after_a_value_edit(smm, base, dtype):
    """a handle is a snapshot: the old apply until refreshed, then bit for bit a newly created handle"""
    name = "poisson2d_32" if base == IC0 else "convdiff3d_12"
    csr = mc_matrix(name, dtype)
    n = len(csr[0]) - 1
    r = rhs_of(n, dtype)
    A = make(smm, csr)
    M = A.getPreconditioner(KIND[base])
    old = np.zeros(n, dtype=dtype)
    M.apply(r, old)
    A.scale(1.75)
    d = np.arange(0, n, 3, dtype=np.int32)
    assert A.update_entries(d, d, np.full(len(d), 0.5, dtype=dtype), add=True).all()
    stale = np.zeros(n, dtype=dtype)
    M.apply(r, stale)
    np.testing.assert_array_equal(bits(stale), bits(old))
    M.multicolor_refresh()
    fresh = A.getPreconditioner(KIND[base])
    z, z_fresh = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    M.apply(r, z)
    fresh.apply(r, z_fresh)
    np.testing.assert_array_equal(bits(z), bits(z_fresh))
    assert not np.array_equal(bits(z), bits(old))
    if base != SGS:
        np.testing.assert_array_equal(bits(M.values()), bits(fresh.values()))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals(smm, dtype):
    start, pos, val = mc_matrix("spd5", dtype)
    P = smm.SolverPreconditioner
    A = make(smm, (start, pos, val))
    b = gen.row_sums(start, val)
    # the structural failures of the exact kinds, with their codes: a missing diagonal, an empty row; SGS: a stored zero and |d| < 1e-5
    assert pos[start[3] + 1] == 3
    for kind, exact in ((P.MULTICOLOR_SGS, P.SYMMETRIC_GAUS_SEIDEL), (P.MULTICOLOR_ILU0, P.ILU0), (P.MULTICOLOR_IC0, P.IC0)):
        keep = np.ones(len(pos), dtype=bool)
        keep[start[3] + 1] = False
        s2 = start.copy()
        s2[4:] -= 1
        assert code_of(lambda: make(smm, (s2, pos[keep], val[keep])).getPreconditioner(kind)) == code_of(lambda: make(smm, (s2, pos[keep], val[keep])).getPreconditioner(exact)) == PRECOND
        ragged = gen_matrices(dtype)["ragged_300"]
        assert code_of(lambda: make(smm, ragged).getPreconditioner(kind)) == code_of(lambda: make(smm, ragged).getPreconditioner(exact)) == PRECOND
        W = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=dtype))
        assert code_of(lambda: W.getPreconditioner(kind)) == INVALID
    for tiny in (0.0, 1e-6):
        v = val.copy()
        v[start[3] + 1] = tiny
        assert code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(P.MULTICOLOR_SGS)) == PRECOND
        assert code_of(lambda: make(smm, (start, pos, v)).getPreconditioner(P.SYMMETRIC_GAUS_SEIDEL)) == PRECOND
    # solvers: the batched and row-partitioned entry points, apply_spmv, the kinds a solver does not take, a foreign matrix; nothing written
    S, I, C = (A.getPreconditioner(k) for k in (P.MULTICOLOR_SGS, P.MULTICOLOR_ILU0, P.MULTICOLOR_IC0))
    x = np.full(5, 0.25, dtype=dtype)
    keep_x = x.copy()
    B2 = np.stack([b, b], axis=1).copy()
    X2 = np.full_like(B2, 0.25)
    for M in (S, I, C):
        assert code_of(lambda: smm.BiCGStabBatch(A, B2, X2, 5, 1e-6, M)) == INVALID
        assert code_of(lambda: M.apply_spmv(b, x)) == INVALID
        assert code_of(lambda: smm.BiCGStab(make(smm, (start, pos, val)), b.copy(), x, 5, 1e-6, M)) == INVALID
    assert code_of(lambda: smm.BiCGStab(A, b.copy(), x, 5, 1e-6, C)) == INVALID
    assert code_of(lambda: smm.GMRES(A, b.copy(), x, 5, 1e-6, 30, C)) == INVALID
    assert code_of(lambda: smm.ConjugateGradient(A, b, x, x, 5, 1e-6, I)) == INVALID
    np.testing.assert_array_equal(bits(x), bits(keep_x))
    np.testing.assert_array_equal(bits(X2), bits(np.full_like(B2, 0.25)))
    d_v = carve_like(b, fit(1, dtype), device="cuda:0")
    d_x = carve_like(keep_x, fit(1, dtype), device="cuda:0")
    saved = snapshot(d_x)
    assert code_of(lambda: S.apply_spmv_dev(d_v, d_x)) == INVALID
    torch.cuda.synchronize()
    assert_unchanged(d_x, saved, "x")
    J = A.getPreconditioner(P.JACOBI)
    for call in (J.multicolor_info, J.multicolor_perm, J.multicolor_matrix, J.multicolor_refresh):
        assert code_of(call) == INVALID
    # the same handles still solve
    tol = 1e-6 if dtype == np.float64 else 1e-4
    for M in (S, C):
        x = np.zeros(5, dtype=dtype)
        assert int(smm.ConjugateGradient(A, b, x, x, -1, tol, M)) == 0
        np.testing.assert_allclose(x, 1.0, rtol=1e-3)


def test_row_partitioned_solver_refuses_the_kinds(smm):
    from sparse_matrix_math_amd import distributed as dist

    csr = mc_matrix("convdiff3d_12", np.float64)
    n = len(csr[0]) - 1
    comm = dist.NativeComm.single()
    tens = [torch.tensor(a, device="cuda:0") for a in csr]
    D = dist.NativeDistMatrix(comm, n, [0, n], tens[0], tens[1], tens[2], np.float64)
    b = torch.tensor(gen.row_sums(csr[0], csr[2]), device="cuda:0")
    x = torch.full((n,), 0.25, dtype=torch.float64, device="cuda:0")
    for kind in (smm.SolverPreconditioner.MULTICOLOR_SGS, smm.SolverPreconditioner.MULTICOLOR_ILU0):
        D.set_precond(kind)
        assert code_of(lambda: D.bicgstab(b, x, 5, 1e-8)) == INVALID
    torch.cuda.synchronize()
    assert bool((x == 0.25).all())
    D.close()
    comm.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_no_rows(smm, dtype):
    E = smm.CSRMatrix(0, 0, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    assert E.color()[1] == 0
    M = E.getPreconditioner("MULTICOLOR_ILU0")
    assert M.multicolor_info()[0] == 0 and M.levels() == (0, 0)
    z = np.zeros(0, dtype=dtype)
    M.apply(z, z)
    assert E.permute(np.zeros(0, dtype=np.int32)).nnz == 0


# ---- flavour and drop-in -----------------------------------------------------------------------------------------------------
def test_fma_flavour(oracle_fma):
    """libsmm_hip_fma.so (loaded as tests/test_gpu_fma_flavour.py loads it): the sweeps use fma() there, and so do the fma oracle's, so
    the three applies are bit for bit in this flavour too"""
    _lib._share_hip_runtime_with_torch()
    lib = ctypes.CDLL(_lib.library_path(fma=True))
    lib.smm_hip_last_error.restype = ctypes.c_char_p
    assert lib.smm_hip_uses_std_fma() == 1
    assert lib.smm_hip_init(0) == 0, lib.smm_hip_last_error()
    P = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(P)  # noqa: E731
    lib.smm_hip_precond_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(P)]
    lib.smm_hip_precond_destroy.argtypes = [P]
    lib.smm_hip_csr_destroy.argtypes = [P]
    for dtype, suf in ((np.float32, "f32"), (np.float64, "f64")):
        for base, kind, name in ((SGS, 9, "convdiff3d_12"), (ILU0, 10, "convdiff3d_12"), (IC0, 11, "poisson2d_32")):
            csr = mc_matrix(name, dtype)
            n = len(csr[0]) - 1
            r = rhs_of(n, dtype)
            z_ref = make_apply(oracle_fma, csr, base)(r)
            h, m = P(), P()
            create = getattr(lib, f"smm_hip_csr_create_{suf}")
            create.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.POINTER(P)]
            assert create(n, n, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ctypes.byref(h)) == 0
            assert lib.smm_hip_precond_create(h, kind, ctypes.byref(m)) == 0, lib.smm_hip_last_error()
            z = np.zeros(n, dtype=dtype)
            apply = getattr(lib, f"smm_hip_precond_apply_{suf}")
            apply.argtypes = [P, P, P]
            assert apply(m, ptr(r), ptr(z)) == 0, lib.smm_hip_last_error()
            lib.smm_hip_precond_destroy(m)
            lib.smm_hip_csr_destroy(h)
            np.testing.assert_array_equal(bits(z), bits(z_ref))


def test_cpp_dropin_case_on_the_gpu(tmp_path):
    """tests/cpp/multicolor_case.cpp: SMM::MulticolorPreconditioner in BiCGStab and ConjugateGradient on the 6 x 6 generated matrix ends
    with SUCCESS at x = 1 with 2 colours (a path graph), and SMM::permute with the inverse permutation gives the matrix back bit for bit"""
    exe = build_case(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 10
    for ln in lines:
        words = ln.split()
        if "-permute" in words[0]:
            assert words[1:] == ["hip", "0", "colors", "2", "same", "1"], ln
            continue
        assert words[1:7] == ["status", "0", "hip", "0", "colors", "2"], ln
        x = np.array([float.fromhex(w) for w in words[8:]])
        np.testing.assert_allclose(x, 1.0, atol=1e-3 if words[0].startswith("float") else 1e-5)
