"""The generalised lobpcg (A x = lambda B x) without a GPU: the CPU restatement (tests/lobpcg_gen_restatement.py, the definition the GPU
loop is compared with) meets on every case of tests/lobpcg_gen_cases.py every bound that tests/test_gpu_lobpcg_gen.py puts on the GPU's
answer, against a dense reference that is numpy alone; its counts and edge paths are what the contract says; the mass generators agree
with an element-by-element assembly written here; the new symbols are declared, exported and bound; and the argument checks answer
SMM_HIP_ERR_INVALID before a device is asked for."""
import ctypes
import itertools
import os
import re
import subprocess

import lobpcg_gen_cases as cases
import lobpcg_restatement as standard
import numpy as np
import pytest
from lobpcg_gen_restatement import DIVERGED, LARGEST, SMALLEST, SUCCESS, b_orthonormalise, lobpcg
from lobpcg_restatement import start_block

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
WHICH = {"LA": LARGEST, "SA": SMALLEST}
NEW_SYMBOLS = [f"smm_hip_{base}_{suf}" for base in ("lobpcg_gen", "lobpcg_gen_dev", "multi_block_axpy_bases_dev", "multi_rotate_bases_dev") for suf in ("f32", "f64")]
_ID = lambda v: v.__name__ if isinstance(v, type) else str(v)  # noqa: E731


def working(name, dtype):
    a, b = cases.pair(name, dtype)
    return cases.dense(a).astype(dtype), cases.dense(b).astype(dtype)


def test_the_case_list():
    assert len(cases.combos()) == 13
    assert all(3 * k <= cases.ROWS[name] and k <= standard.MAX_K for name, _, k in cases.combos())
    np.testing.assert_allclose(cases.exact("chain_60"), cases.chain_analytic(), rtol=1e-12)  # the dense reference against the closed form
    for name in cases.ROWS:
        a, b = (cases.dense(m) for m in cases.pair(name))
        assert a.shape == b.shape == (cases.ROWS[name],) * 2 and np.array_equal(a, a.T) and np.array_equal(b, b.T) and np.linalg.eigvalsh(b)[0] > 0
    ev = cases.exact("square_16x16")
    assert abs(ev[1] - ev[2]) <= 1e-12 and abs(ev[4] - ev[5]) <= 1e-12 and ev[6] - ev[5] >= 0.02  # two double values among six, a clean cut


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,which,k", cases.combos(), ids=_ID)
def test_restatement_meets_the_gpu_bounds(name, which, k, dtype):
    """against the dense reference: the bounds of tests/test_gpu_lobpcg_gen.py as ratios, all <= 1; at most 500 iterations, half the
    cap; the orthonormality ratio stays under ORTH_WORST, from which the GPU test takes its bound; bmatvecs counted"""
    tol = cases.TOL[np.dtype(dtype)]
    eps = float(np.finfo(dtype).eps)
    lam = cases.exact(name)
    norm = float(np.max(np.abs(lam)))
    a, b = working(name, dtype)
    history = []
    r = lobpcg(a, k, WHICH[which], cases.MAX_ITERATIONS, tol, B=b, history=history)
    w, X = r["w"].astype(np.float64), r["X"].astype(np.float64)
    a64, b64 = (cases.dense(m) for m in cases.pair(name))
    BX = b64 @ X
    err = float(np.max(np.abs(w - cases.wanted(lam, which, k)))) / (10 * tol * norm)
    res = float(np.max(np.linalg.norm(a64 @ X - BX * w, axis=0) / np.linalg.norm(BX, axis=0))) / (10 * tol * norm)
    orth = float(np.max(np.abs(X.T @ BX - np.eye(k)))) / eps
    print(name, which, k, np.dtype(dtype).name, "iterations", r["iterations"], "err / (10 tol |lambda|)", err, "true residual / (10 tol |lambda| |Bx|)", res,
          "max|X^T B X - I| / eps", orth, "bmatvecs", r["bmatvecs"])
    assert r["status"] == SUCCESS and r["nconv"] == k
    assert err <= 1 and res <= 1
    assert r["iterations"] <= 500 and len(history) == r["iterations"]
    assert r["bmatvecs"] == 2 * k - 1 + sum(history) and r["matvecs"] == k + sum(history) and r["applies"] == 0
    assert orth <= cases.ORTH_WORST[np.dtype(dtype)]
    assert np.all(np.diff(w) <= 0) if which == "LA" else np.all(np.diff(w) >= 0)


def test_restatement_edges():
    a, b = working("chain_60", np.float64)
    for dtype in DTYPES:  # B = None is the standard loop, bit for bit
        a_t = a.astype(dtype)
        one, two = lobpcg(a_t, 3, SMALLEST, 1000, cases.TOL[np.dtype(dtype)]), standard.lobpcg(a_t, 3, SMALLEST, 1000, cases.TOL[np.dtype(dtype)])
        assert one["bmatvecs"] == 0 and one["status"] == two["status"] == SUCCESS
        assert all(np.array_equal(one[key], two[key]) for key in ("w", "X", "residuals")) and all(one[key] == two[key] for key in ("iterations", "matvecs", "nconv"))
    # B = -I: the first w . q is negative -- DIVERGED at the start, nothing returned
    r = lobpcg(a, 3, SMALLEST, 10, 1e-10, B=-np.eye(60))
    assert r["status"] == DIVERGED and r["w"] is None and r["X"] is None and b_orthonormalise(start_block(60, 3, 0, np.float64), -np.eye(60)) is None
    # B = A: every start block spans eigenvectors of the value 1 -- converged at iteration 0
    for dtype in DTYPES:
        a_t = a.astype(dtype)
        r = lobpcg(a_t, 3, SMALLEST, 10, cases.TOL[np.dtype(dtype)], B=a_t)
        assert r["status"] == SUCCESS and r["iterations"] == 0 and r["bmatvecs"] == 5 and r["matvecs"] == 3
        assert float(np.max(np.abs(r["w"].astype(np.float64) - 1.0))) <= 4 * float(np.finfo(dtype).eps)
    # X0 = the hash start gives the bits of X0 = None; a start block of rank below k is DIVERGED
    X0 = start_block(60, 3, 0, np.float64)
    one, two = lobpcg(a, 3, SMALLEST, 1000, 1e-10, B=b), lobpcg(a, 3, SMALLEST, 1000, 1e-10, B=b, X0=X0)
    assert np.array_equal(one["X"], two["X"]) and np.array_equal(one["w"], two["w"])
    X0[:, 2] = X0[:, 0]
    assert lobpcg(a, 3, SMALLEST, 1000, 1e-10, B=b, X0=X0)["status"] == DIVERGED
    bad = b.copy()
    bad[0, 0] = np.nan
    assert lobpcg(a, 2, SMALLEST, 5, 1e-10, B=bad)["status"] == DIVERGED


def ic0(a):
    """the incomplete Cholesky factor on the pattern of a's lower triangle (a stand-in for the library's IC0, in numpy)"""
    n = a.shape[0]
    L = np.tril(a).astype(np.float64)
    pattern = L != 0
    for c in range(n):
        L[c, c] = np.sqrt(L[c, c])
        below = np.nonzero(pattern[c + 1:, c])[0] + c + 1
        L[below, c] /= L[c, c]
        for j in below:
            rows = below[(below >= j) & pattern[below, j]]
            L[rows, j] -= L[rows, c] * L[j, c]
    return L


def test_a_preconditioner_of_a_cuts_the_iteration_count():
    """diag_33x29, SA, k = 4, fp64: with the IC0 of A the restatement takes strictly fewer iterations than without -- the condition
    tests/test_gpu_lobpcg_gen.py asserts of the library's SGS and IC0"""
    a, b = working("diag_33x29", np.float64)
    L = ic0(a)
    Minv = np.linalg.inv(L @ L.T)
    lam = cases.exact("diag_33x29")
    plain = lobpcg(a, 4, SMALLEST, cases.MAX_ITERATIONS, 1e-10, B=b)
    with_m = lobpcg(a, 4, SMALLEST, cases.MAX_ITERATIONS, 1e-10, B=b, M=lambda v: Minv @ v)
    print("iterations", plain["iterations"], "with IC0", with_m["iterations"])
    assert plain["status"] == with_m["status"] == SUCCESS and with_m["iterations"] < plain["iterations"]
    assert with_m["applies"] == with_m["matvecs"] - 4 == with_m["bmatvecs"] - 7
    assert float(np.max(np.abs(with_m["w"] - lam[:4]))) <= 10 * 1e-10 * float(lam[-1])


def assembled_mass(cells, clamp_axis, clamp_low, rho):
    """element by element, by 2-point Gauss quadrature of N_i N_j on the unit cell: exact for the products of Q1 shape functions"""
    dim = len(cells)
    nodes = [c + 1 for c in cells]
    number, count = {}, 0
    for node in itertools.product(*[range(m) for m in nodes[::-1]]):  # x fastest
        node = node[::-1]
        if node[clamp_axis] != (0 if clamp_low else cells[clamp_axis]):
            number[node] = count
            count += 1
    out = np.zeros((count * dim, count * dim))
    g = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)
    corners = list(itertools.product((0, 1), repeat=dim))
    element = np.zeros((len(corners), len(corners)))
    for point in itertools.product(g, repeat=dim):
        shape = np.array([np.prod([x if bit else 1.0 - x for bit, x in zip(corner, point)]) for corner in corners])
        element += rho * np.outer(shape, shape) / 2 ** dim
    for cell in itertools.product(*[range(c) for c in cells]):
        for i, ci in enumerate(corners):
            for j, cj in enumerate(corners):
                ni, nj = tuple(np.add(cell, ci)), tuple(np.add(cell, cj))
                if ni in number and nj in number:
                    for comp in range(dim):
                        out[number[ni] * dim + comp, number[nj] * dim + comp] += element[i, j]
    return out


@pytest.mark.parametrize("cells,clamp,rho", [((5, 3), "left", 1.0), ((3, 4), "top", 2.5), ((2, 3, 2), "left", 1.0), ((3, 2, 2), "back", 0.5)], ids=_ID)
def test_mass_generators(cells, clamp, rho):
    axis, low = {"left": (0, True), "top": (1, False), "back": (2, False)}[clamp]
    make, stiffness = (gen.mass2d, gen.elasticity2d) if len(cells) == 2 else (gen.mass3d, gen.elasticity3d)
    for dtype in DTYPES:
        start, pos, val = make(*cells, clamp=clamp, rho=rho, dtype=dtype)
        rows = len(start) - 1
        m = cases.dense((start, pos, val))
        assert val.dtype == dtype and start.dtype == pos.dtype == np.int32 and rows == len(stiffness(*cells, clamp=clamp)[0]) - 1
        assert all(np.all(np.diff(pos[start[r]:start[r + 1]]) > 0) for r in range(rows)) and np.all(val != 0)
        assert np.array_equal(m, m.T) and np.linalg.eigvalsh(m)[0] > 0
        want = assembled_mass(cells, axis, low, rho)
        assert float(np.max(np.abs(m - want))) <= 8 * float(np.finfo(dtype).eps) * float(np.max(want))
    with pytest.raises(ValueError):
        gen.mass2d(3, 3, clamp="front")


def test_exports_and_wrappers():
    """what the parent of this feature does not have"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smm_hip.h")).read(), flags=re.S)
    so = _lib.library_path()
    if not os.path.exists(so):
        pytest.fail("libsmm_hip.so not built (build() makes it)")
    for fma in (False, True):
        exported = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path(fma=fma)], capture_output=True, text=True, timeout=120).stdout
        for name in NEW_SYMBOLS:
            assert re.search(r" T " + name + r"$", exported, re.M), (name, fma)
            assert name in _lib.exported_symbols()
            assert f"{name}(" in text
    assert "#define SMM_LOBPCG_MAX_BASES 3" in text
    lib = _lib.load()
    assert len(lib.smm_hip_lobpcg_gen_f32.argtypes) == 20 and len(lib.smm_hip_lobpcg_gen_dev_f64.argtypes) == 21
    assert len(lib.smm_hip_multi_block_axpy_bases_dev_f64.argtypes) == 11 and len(lib.smm_hip_multi_rotate_bases_dev_f32.argtypes) == 9
    assert lib.smm_hip_lobpcg_gen_f32.argtypes[5] is ctypes.c_float and lib.smm_hip_lobpcg_gen_dev_f64.argtypes[5] is ctypes.c_double
    import sparse_matrix_math_amd as smm

    for name in ("lobpcg_gen_dev", "multi_block_axpy_bases_dev", "multi_rotate_bases_dev"):
        assert callable(getattr(smm, name))
    assert smm.LOBPCG_MAX_BASES == 3
    assert smm.LobpcgGenInfo._fields == smm.LobpcgInfo._fields + ("bmatvecs",)
    drop_in = open(os.path.join(ROOT, "include", "smm_hip", "sparse_matrix_math.h")).read()
    assert "inline SolverStatus lobpcg(const CSRMatrix<T>& a, const CSRMatrix<T>& b, int k, int which, T* eigenvalues," in drop_in


def test_argument_checks_answer_before_a_device_is_asked_for():
    """SMM_HIP_ERR_INVALID with a message that starts with the entry point's name, on a machine with or without a GPU, outputs untouched.
    (Every check that needs a matrix handle needs a device to make one: tests/test_gpu_lobpcg_gen.py has those.)"""
    lib = _lib.load()
    P = ctypes.c_void_p
    w = np.full(4, 7.0)
    ints = [ctypes.c_int(-5) for _ in range(6)]
    refs = [ctypes.byref(i) for i in ints]
    assert lib.smm_hip_lobpcg_gen_f64(None, None, 2, 1, 10, 0.0, None, None, 0, 0, w.ctypes.data_as(P), None, 0, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    assert lib.smm_hip_lobpcg_gen_dev_f32(None, None, 2, 1, 10, 0.0, None, None, 0, 0, None, None, 0, None, None, *refs) == _lib.SMM_HIP_ERR_INVALID
    assert lib.smm_hip_last_error().decode().startswith("lobpcg:")
    assert np.all(w == 7.0) and all(i.value == -5 for i in ints)

    def array(*items):
        return (P * len(items))(*items)

    # never dereferenced: the checks come first.  Columns of 64 elements, ld 64, fp64: a block of 4 columns is 2048 bytes
    v = [1 << 20, 2 << 20, 3 << 20]
    ww = [4 << 20, 5 << 20, 6 << 20]
    h = P(7 << 20)
    y = np.ones(16)
    yp = y.ctypes.data_as(P)
    axpy, rot = lib.smm_hip_multi_block_axpy_bases_dev_f64, lib.smm_hip_multi_rotate_bases_dev_f64
    refused_axpy = [(-1, 4, 4, 3, array(*v), 64, h, 4, array(*ww), 64), (64, 0, 4, 3, array(*v), 64, h, 4, array(*ww), 64), (64, 4, 0, 3, array(*v), 64, h, 4, array(*ww), 64),
                    (64, 25, 4, 3, array(*v), 64, h, 25, array(*ww), 64), (64, 4, 25, 3, array(*v), 64, h, 4, array(*ww), 64), (64, 4, 4, 3, array(*v), 63, h, 4, array(*ww), 64),
                    (64, 4, 4, 3, array(*v), 64, h, 4, array(*ww), 63), (64, 4, 4, 3, array(*v), 64, h, 3, array(*ww), 64), (64, 4, 4, 3, array(*v), 64, None, 4, array(*ww), 64),
                    (64, 4, 4, 0, array(*v), 64, h, 4, array(*ww), 64), (64, 4, 4, 4, array(*v, 8 << 20), 64, h, 4, array(*ww, 9 << 20), 64),
                    (64, 4, 4, 3, None, 64, h, 4, array(*ww), 64), (64, 4, 4, 3, array(*v), 64, h, 4, None, 64),
                    (64, 4, 4, 3, array(v[0], None, v[2]), 64, h, 4, array(*ww), 64), (64, 4, 4, 3, array(*v), 64, h, 4, array(ww[0], ww[1], None), 64),
                    (64, 4, 4, 3, array(*v), 64, h, 4, array(ww[0], ww[1], v[0]), 64),             # W[2] is V[0]
                    (64, 4, 4, 2, array(v[0], v[1]), 64, h, 4, array(ww[0], v[1] + 2040), 64),     # W[1] begins in V[1]'s last element
                    (64, 4, 4, 2, array(v[0], ww[0] + 2040), 64, h, 4, array(ww[0], ww[1]), 64)]   # V[1] begins in W[0]'s last element
    for args in refused_axpy:
        assert axpy(*args, None) == _lib.SMM_HIP_ERR_INVALID, args[:4]
        assert lib.smm_hip_last_error().decode().startswith("multi_block_axpy_bases:")
    refused_rot = [(-1, 4, 4, 3, array(*v), 64, yp, 4), (64, 4, 0, 3, array(*v), 64, yp, 4), (64, 3, 4, 3, array(*v), 64, yp, 4), (64, 65, 4, 3, array(*v), 64, yp, 65),
                   (64, 4, 4, 3, array(*v), 63, yp, 4), (64, 4, 4, 3, array(*v), 64, yp, 3), (64, 4, 4, 3, array(*v), 64, None, 4), (64, 4, 4, 0, array(*v), 64, yp, 4),
                   (64, 4, 4, 4, array(*v, 8 << 20), 64, yp, 4), (64, 4, 4, 3, None, 64, yp, 4), (64, 4, 4, 3, array(v[0], v[1], None), 64, yp, 4)]
    for args in refused_rot:
        assert rot(*args, None) == _lib.SMM_HIP_ERR_INVALID, args[:4]
        assert lib.smm_hip_last_error().decode().startswith("multi_rotate_bases:")
    # nothing to do: no device either
    assert axpy(0, 4, 4, 3, array(*v), 64, h, 4, array(*ww), 64, None) == _lib.SMM_HIP_OK
    assert rot(0, 4, 4, 3, array(*v), 64, yp, 4, None) == _lib.SMM_HIP_OK
