"""The PATTERN family's sweep kernel (smm_spmv_sweep.hip): the slots kernel's copy walked offset-major, up to R 64-row waves per hardware
wave held open in registers.  Forced on (smm_hip_csr_pattern_slots(m, 3)) it must give the tile kernel's bits for every operation at every
compiled R, keep them across value edits, fall back when the copy is refused, and solve like the tile kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 3
SWEEP, SLOTS, TILE = "spmvPatternSweepKernel", "spmvPatternSlotsKernel", "spmvPatternTileKernel"
ROWS_OPEN = (8, 16, 32)  # every compiled R


@pytest.fixture(autouse=True)
def default_rows_open():
    yield
    host.set_pattern_sweep_rows(0)


def handles(smm, csr, lanes, modes=(0, 3)):
    """handles of one matrix on the PATTERN family at `lanes`: by default (tile kernel, sweep kernel)"""
    n = len(csr[0]) - 1
    out = []
    for mode in modes:
        A = smm.CSRMatrix(n, n, *csr)
        A.set_kernel(PATTERN, lanes)
        A.pattern_slots(mode)
        out.append(A)
    return out


def spmv(A, x, lhs=None, op=0):
    out = np.zeros(len(x), dtype=x.dtype)
    if op == 0:
        A.rMult(x, out)
    elif op == 1:
        A.rMultAdd(lhs, x, out)
    else:
        A.rMultSub(lhs, x, out)
    return out


# (rows, offsets per side, largest offset).  At most 16384 rows, so that the analysis samples every row and takes the row masks.
#   200: fewer rows than one workgroup block (4 waves)
#   7_777, 3_001: not multiples of 64; far diagonals enter and leave inside the matrix, so masks change inside a super-block and
#     non-uniform waves occur
#   16_001: 251 waves over 8 groups of 32: the last group's super-block is partly empty (27 waves), hardware waves own 0 or 1 wave
#   16_384: whole waves only
CASES = [(200, 5, 40), (7_777, 25, 300), (3_001, 30, 2000), (16_001, 25, 4096), (16_384, 25, 1000)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("rows_open", ROWS_OPEN)
def test_sweep_bits_equal_tile_kernel(smm, dtype, lanes, rows_open):
    host.set_pattern_sweep_rows(rows_open)
    rng = np.random.default_rng(11)
    for n, k, maxoff in CASES:
        csr = gen.banded_random_spd(n, k, 0x5EED + n, maxoff, dtype=dtype)
        T, S = handles(smm, csr, lanes)
        x = rng.uniform(-1, 1, n).astype(dtype)
        lhs = rng.uniform(-1, 1, n).astype(dtype)
        for op in (0, 1, 2):
            want = spmv(T, x, lhs, op)
            got = spmv(S, x, lhs, op)
            np.testing.assert_array_equal(got, want, err_msg=f"n {n} op {op}")
        assert T.pattern_info()[0] == 1  # the row masks
        assert T.kernel_desc()[0] == TILE
        name, nbytes = S.kernel_desc()
        assert name == SWEEP and nbytes > 0
        S.pattern_slots(1)
        assert S.kernel_desc() == (SLOTS, nbytes)  # the same copy, the same bytes
        np.testing.assert_array_equal(spmv(S, x), spmv(T, x))


def blocks_check(args, **env):
    """tools/lab/sweep_blocks_check.py in a process of its own (the variables in `env` are read once per process)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lab", "sweep_blocks_check.py"), *args], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "sweep blocks check: ALL OK" in r.stdout, r.stdout[-3000:]
    return r.stdout


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sweep_many_super_blocks(dtype):
    """Matrices generated on the device, one workgroup per CU (SMM_HIP_PATTERN_SWEEP_WGS=1: 32 CUs x 4 = 128 hardware waves per XCD group
    whatever the registers of the variant).  2^21 rows are 4096 waves per group: every hardware wave holds all R waves open, in 1 / 2 / 4
    super-blocks at R = 32 / 16 / 8.  2_300_017 rows are 4493 waves per group: 2 / 3 / 5 super-blocks whose hardware waves hold 18 / 12 / 8
    waves (R = 32: slots 18..31 stay empty), the last hardware waves of a block short or empty, the last wave of the matrix partial.  The
    diagonals enter and leave over the first and last 2^18 rows, so masks change inside super-blocks."""
    out = blocks_check(["--dtype", dtype, "--rows-open", "8,16,32", "--rows", "2097152,2300017"], SMM_HIP_PATTERN_SWEEP_WGS="1")
    assert out.count("ok rows") == 6, out


def test_sweep_shipped_block():
    """The configuration AUTO ships (fp32, R = 16, three workgroups per CU: 384 hardware waves per XCD group, 6144 waves per super-block) at
    3_145_728 rows -- one super-block per group, every hardware wave holding all 16 waves -- and at 6_400_017 rows: 12 501 waves per
    group in three super-blocks of 4167, 11 waves per hardware wave, the last ones short or empty."""
    out = blocks_check(["--dtype", "f32", "--rows-open", "16", "--rows", "3145728,6400017"])
    assert out.count("ok rows") == 2, out


def test_sweep_selected_by_the_environment():
    """SMM_HIP_PATTERN_SLOTS=3 with the handle's own mode left at -1: the sweep kernel runs (and is named by kernel_desc), with the tile
    kernel's bits; =1 keeps the slots kernel"""
    out = blocks_check(["--env-mode", "--rows", "16001,7777"], SMM_HIP_PATTERN_SLOTS="3")
    assert out.count("spmvPatternSweepKernel SMM_HIP_PATTERN_SLOTS=3") == 2, out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lab", "sweep_blocks_check.py"), "--env-mode", "--rows", "16001"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, SMM_HIP_PATTERN_SLOTS="1"))
    assert r.returncode == 1 and "spmvPatternSlotsKernel ran" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows_open", ROWS_OPEN)
def test_sweep_in_place_and_fused_dots(smm, dtype, rows_open):
    host.set_pattern_sweep_rows(rows_open)
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 5, 4096, dtype=dtype)
    T, S = handles(smm, csr, 2)
    dev = torch.device("cuda")
    td = torch.float32 if dtype == np.float32 else torch.float64
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.rand(n, generator=g, dtype=td).to(dev) - 0.5
    lhs = torch.rand(n, generator=g, dtype=td).to(dev)
    w1 = torch.rand(n, generator=g, dtype=td).to(dev)
    res = {}
    for name, A in (("tile", T), ("sweep", S)):
        buf = lhs.clone()
        A.spmv_dev(2, buf, x, buf)  # rMultSub with out == lhs
        torch.cuda.synchronize()
        res[name, "inplace"] = buf.cpu().numpy()
        P = host.partials_count()
        for mode in (1, 2):
            sums = []
            for _ in range(2):
                out = torch.zeros(n, dtype=td, device=dev)
                parts = torch.zeros(2 * P, dtype=td, device=dev)
                A.spmv_fused_dev(0, None, x, out, mode, w1, parts)
                torch.cuda.synchronize()
                sums.append(parts.cpu().numpy())
                res[name, "out", mode] = out.cpu().numpy()
            np.testing.assert_array_equal(sums[0], sums[1])  # the same partials at every launch
            res[name, "dots", mode] = sums[0].reshape(2, P).astype(np.float64).sum(axis=1)
            fins = []
            for _ in range(2):
                fin = torch.zeros(host.finish_len(), dtype=td, device=dev)
                out = torch.zeros(n, dtype=td, device=dev)
                A.spmv_fused_dev(0, None, x, out, mode, w1, fin, finish=True)
                torch.cuda.synchronize()
                o = host.finish_totals_offset()
                fins.append(fin[o:o + 2].cpu().numpy())
                res[name, "out_finish", mode] = out.cpu().numpy()
            np.testing.assert_array_equal(fins[0], fins[1])
            res[name, "finish", mode] = fins[0]
    assert S.kernel_desc()[0] == SWEEP
    np.testing.assert_array_equal(res["sweep", "inplace"], res["tile", "inplace"])
    tol = 1e-4 if dtype == np.float32 else 1e-11
    for mode in (1, 2):
        np.testing.assert_array_equal(res["sweep", "out", mode], res["tile", "out", mode])
        np.testing.assert_array_equal(res["sweep", "out_finish", mode], res["tile", "out", mode])
        np.testing.assert_allclose(res["sweep", "dots", mode], res["tile", "dots", mode], rtol=tol)
        cnt = 2 if mode == 2 else 1  # totals: out.w1 (mode 1); out.out, out.w1 (mode 2)
        np.testing.assert_allclose(res["sweep", "finish", mode][:cnt].astype(np.float64), res["sweep", "dots", mode][:cnt], rtol=tol)
        np.testing.assert_allclose(res["sweep", "finish", mode][:cnt].astype(np.float64), res["tile", "finish", mode][:cnt].astype(np.float64), rtol=tol)


@pytest.mark.parametrize("rows_open", ROWS_OPEN)
def test_sweep_propagates_inf_and_nan(smm, rows_open):
    host.set_pattern_sweep_rows(rows_open)
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 9, 4096, dtype=np.float32)
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(np.float32)
    x[[5, 700, 10_000, 15_990]] = [np.inf, np.nan, -np.inf, np.nan]
    T, S = handles(smm, csr, 2)
    want = spmv(T, x)
    got = spmv(S, x)
    assert S.kernel_desc()[0] == SWEEP
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(got, want)
    # and in values[]: a row's Inf or NaN entry reaches that row alone
    vals = csr[2].copy()
    vals[[3, 40_000, 400_000, len(vals) - 2]] = [np.nan, np.inf, -np.inf, np.nan]
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
    T, S = handles(smm, (csr[0], csr[1], vals), 2)
    want = spmv(T, x)
    got = spmv(S, x)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).sum() >= n - 4
    np.testing.assert_array_equal(got, want)


def test_sweep_follows_every_edit(smm):
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 13, 4096, dtype=np.float32)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    _, S = handles(smm, csr, 2)
    _, O = handles(smm, gen.banded_random_spd(n, 25, 13, 4096, dtype=np.float32), 2)
    spmv(S, x)  # the copy is built
    assert S.kernel_desc()[0] == SWEEP
    rows = np.repeat(np.arange(n), np.diff(csr[0]))

    def check(what):
        F = smm.CSRMatrix(n, n, csr[0], csr[1], S.get_values())
        F.set_kernel(PATTERN, 2)
        F.pattern_slots(3)
        np.testing.assert_array_equal(spmv(S, x), spmv(F, x), err_msg=what)
        F.pattern_slots(0)
        np.testing.assert_array_equal(spmv(S, x), spmv(F, x), err_msg=what + " (tile kernel)")

    S.scale(1.5)
    check("scale")
    S.inplaceAdd(O)
    check("inplaceAdd")
    S.inplaceSubtract(O)
    check("inplaceSubtract")
    pick = rng.integers(0, len(rows), 500)
    S.update_entries(rows[pick], csr[1][pick], rng.uniform(-2, 2, 500).astype(np.float32))
    check("update_entries")
    S.update_entries(rows[pick], csr[1][pick], rng.uniform(-2, 2, 500).astype(np.float32), add=True)
    check("update_entries add")
    S.updateEntry(int(rows[7]), int(csr[1][7]), 3.25)
    check("updateEntry")
    S.set_values(rng.uniform(-1, 1, len(rows)).astype(np.float32))
    check("set_values")
    S.zeroValues()
    check("zeroValues")
    assert not spmv(S, x).any()


def test_sweep_fallback_when_refused(smm):
    """Without the copy (mode 2 on a matrix with few uniform waves, mode 0) the tile kernel runs, with its bits; mode 2 on a matrix
    too small for a full super-block keeps the slots kernel; mode 3 forces the copy as mode 1 does"""
    n = 64 * 250
    few = gen.banded_random_spd(n, 25, 21, 12_000, dtype=np.float32)  # most waves see a diagonal enter or leave
    many = gen.banded_random_spd(n, 25, 21, 40, dtype=np.float32)  # two waves of 250 do
    x = np.random.default_rng(8).uniform(-1, 1, n).astype(np.float32)
    for csr, expect in ((few, TILE), (many, SLOTS)):
        T, A = handles(smm, csr, 2)
        A.pattern_slots(2)
        got = spmv(A, x)
        assert A.kernel_desc()[0] == expect
        np.testing.assert_array_equal(got, spmv(T, x))
        A.pattern_slots(3)  # forced: the copy is built whatever the share of uniform waves; most rows of `few` come from CSR
        np.testing.assert_array_equal(spmv(A, x), got)
        assert A.kernel_desc()[0] == SWEEP
        A.pattern_slots(0)
        assert A.kernel_desc()[0] == TILE
        np.testing.assert_array_equal(spmv(A, x), got)
    # where the slots kernel does not apply (one lane per row) the mode changes nothing
    T, A = handles(smm, many, 1)
    np.testing.assert_array_equal(spmv(A, x), spmv(T, x))
    assert A.kernel_desc()[0] == T.kernel_desc()[0] != SWEEP


@pytest.mark.parametrize("precond", [None, "JACOBI"])
def test_sweep_bicgstab_agrees_with_tile_kernel(smm, precond):
    """(with JACOBI the division by the diagonal is folded into the SpMV's row operation: the divisor ops run through the sweep kernel)"""
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 0x5EED, 8192, dtype=np.float32)
    b = np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)
    res = {}
    for mode in (0, 3):
        A = smm.CSRMatrix(n, n, *csr)
        A.set_kernel(PATTERN, 2)
        A.pattern_slots(mode)
        M = A.getPreconditioner(smm.SolverPreconditioner.JACOBI) if precond else None
        x = np.zeros(n, dtype=np.float32)
        info = {}
        st = smm.BiCGStab(A, b, x, 200, 1e-6, M=M, info=info)
        res[mode] = (int(st), info.get("iterations"), x)
        assert A.kernel_desc()[0] == (SWEEP if mode else TILE)
    assert res[0][0] == res[3][0] == 0  # SUCCESS: the loop stopped early on its device-side done flag
    assert abs(res[0][1] - res[3][1]) <= 2
    np.testing.assert_allclose(res[3][2], res[0][2], rtol=0, atol=1e-4 * np.abs(res[0][2]).max())
