"""BiCGStab's CPU restatement (tests/bicgstab_restatement.py, the definition the long-run audit of the GPU drivers is compared with)
without a GPU: with the sequential sum it is oracle.bicgstab bit for bit, and in fp32 every member of the ensemble of summation orders
stays finite and converges on the convection-diffusion systems on which a GPU loop was once recorded to return NaN
(profiles/r05/resident_fp32_diag.txt).  The recorded fixture of oracle/gen_golden_v5.py is checked against a re-run of its smallest
cases."""
import numpy as np
import pytest
from bicgstab_restatement import bicgstab, dot_chunked, dot_variants

from oracle.gen_golden_v5 import CASES, EPS, MAXIT, case_inputs, case_tag, load_golden, run_case
from oracle.oracle import PRECOND_JACOBI, PRECOND_NONE
from sparse_matrix_math_amd import generators as gen


@pytest.mark.parametrize("precond", ["none", "jacobi"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("grid", [16, 24])
def test_sequential_restatement_is_the_oracle_bit_for_bit(oracle, grid, dtype, precond):
    csr = gen.convdiff3d(grid, 0.3, dtype=dtype)
    b = gen.row_sums(csr[0], csr[2])
    x0 = np.zeros(len(b), dtype=dtype)
    diag = oracle.jacobi_setup(csr)[1] if precond == "jacobi" else None
    ocode = (PRECOND_JACOBI, diag) if precond == "jacobi" else (PRECOND_NONE, None)
    for maxit, eps in ((1, 1e-30), (3, 1e-30), (6, 1e-30), (40, 1e-30), (-1, 1e-4 if dtype == np.float32 else 1e-9)):
        st_o, x_o, it_o, res_o = oracle.bicgstab(csr, b, x0, maxit, eps, *ocode)
        st, x, it, res, hist = bicgstab(oracle, csr, b, x0, maxit, eps, diag=diag, keep_x=True)
        assert (st, it) == (st_o, it_o), (maxit, st, it, st_o, it_o)
        assert res.dtype == dtype and float(res) == res_o
        assert x.dtype == dtype and np.array_equal(x, x_o)
        assert all(len(hist[f]) == it for f in ("rho", "alpha", "omega", "beta", "resnorm", "xnorm", "x"))
        assert hist["resnorm"][-1] == res and np.array_equal(hist["x"][-1], x)
        if maxit == -1:
            assert 6 < it < len(b) and res <= eps  # it left by the residual test


def test_chunked_sum_is_the_sequential_one_per_chunk(oracle):
    """the partition itself: one chunk is the oracle's dot; 512-row chunks are the oracle's dot of every chunk, added in order"""
    rng = np.random.default_rng(11)
    for dtype in (np.float32, np.float64):
        a, b = rng.uniform(-1, 1, 1300).astype(dtype), rng.uniform(-1, 1, 1300).astype(dtype)
        assert dot_chunked(a, b, chunk=4096) == oracle.dot(a, b)
        total = dtype(0)
        for lo in range(0, 1300, 512):
            total = dtype(total + oracle.dot(a[lo:lo + 512].copy(), b[lo:lo + 512].copy()))
        assert dot_chunked(a, b) == total


@pytest.mark.parametrize("grid,precond", CASES)
def test_fp32_ensemble_stays_finite_and_converges(oracle, grid, precond):
    """convdiff3d(grid, 0.3), b = row sums, x0 = 0, eps = 1e-2: no summation order produces a NaN or stalls.  (A member that did would be
    a CPU reproduction of the recorded GPU NaN.)"""
    csr, b, diag = case_inputs(oracle, grid, precond, np.float32)
    for name, dot in dot_variants(oracle).items():
        st, x, it, res, hist = bicgstab(oracle, csr, b, np.zeros(len(b), dtype=np.float32), MAXIT, EPS, diag=diag, dot=dot)
        print(grid, precond, name, "iterations", it, "res", float(res), "max|x - 1|", float(np.max(np.abs(x - 1))), "largest resnorm", float(hist["resnorm"].max()))
        for f in ("rho", "alpha", "omega", "beta", "resnorm", "xnorm"):
            assert np.isfinite(hist[f]).all(), (name, f, int(np.argmin(np.isfinite(hist[f]))) + 1)
        assert st == 0 and it < MAXIT and res <= EPS, (name, it, float(res))
        assert np.isfinite(x).all() and float(np.max(np.abs(x - 1))) <= 5e-2, name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("precond", ["none", "jacobi"])
def test_fixture_is_what_the_generator_records(oracle, precond, dtype):
    """grid 32 re-run here: every recorded scalar bit for bit.  The 48^3 and 64^3 cases are NOT re-run (half a minute of CPU): that the
    generator reproduces them rests on running oracle/gen_golden_v5.py itself"""
    g = load_golden()
    tag = case_tag(32, precond, dtype)
    rec = run_case(oracle, 32, precond, dtype)
    keys = sorted(k for k in g.files if k.startswith(tag + "/"))
    assert keys == sorted(f"{tag}/{k}" for k in rec)
    for k, v in rec.items():
        np.testing.assert_array_equal(g[f"{tag}/{k}"], v, err_msg=k)


@pytest.mark.parametrize("grid,precond", CASES)
def test_rho_is_at_the_rounding_level(grid, precond):
    """What the fp32 runs have in common with the GPU's NaN (tests/test_gpu_bicgstab_long.py, KNOWN_NAN), read from the fixture: from
    iteration 20 on rho_k = r_(k-1) . r0 is typically no larger than a few u ||r_(k-1)|| ||r0|| in every ensemble member -- the size of the
    rounding error of the dot product itself (and, for the fp64-accumulating member, of the rounding of r's entries) -- so rho and
    alpha = rho / (ap . r0) hold no correct digit and an exactly zero sum is one rounding pattern among many.  32 u: five bits above the
    unit roundoff; a rho that carried information would sit orders of magnitude higher (rho_1 / (||r0|| ||r0||) = 1)."""
    g = load_golden()
    tag = case_tag(grid, precond, np.float32)
    u = float(np.finfo(np.float32).eps)
    for name in ("sequential", "pairwise", "fp64acc", "chunked"):
        rho, res = g[f"{tag}/{name}/rho"].astype(np.float64), g[f"{tag}/{name}/resnorm"].astype(np.float64)
        rel = np.abs(rho[1:]) / (res[:-1] * np.sqrt(rho[0]))  # rho_1 = r0 . r0
        print(grid, precond, name, "median |rho| / (||r|| ||r0||) from k = 20:", float(np.median(rel[18:])) / u, "u")
        assert np.median(rel[18:]) <= 32 * u, name
        assert np.all(rho != 0), name  # ... and no CPU member happens to hit the zero
