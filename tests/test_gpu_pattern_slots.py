"""The PATTERN family's slots kernel (smm_spmv_slots.hip): the values of every uniform 64-row wave read from a wave-sliced copy, the
other waves from CSR.  Forced on (smm_hip_csr_pattern_slots(m, 1)) it must give the tile kernel's bits for every operation, keep them
across value edits, fall back when the copy is refused, and solve like the tile kernel."""
import numpy as np
import pytest
import torch

from sparse_matrix_math_amd import generators as gen
from sparse_matrix_math_amd import host

pytestmark = pytest.mark.gpu
PATTERN = 3
SLOTS, TILE = "spmvPatternSlotsKernel", "spmvPatternTileKernel"


def handles(smm, csr, lanes):
    """(tile kernel, slots kernel) handles of one matrix, both on the PATTERN family at `lanes`"""
    n = len(csr[0]) - 1
    out = []
    for mode in (0, 1):
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


# banded matrices whose far diagonals enter and leave inside the matrix (non-uniform waves), row counts not multiples of 64; at most
# 16384 rows, so that the analysis samples every row and takes the row masks
CASES = [(16_001, 25, 4096), (7_777, 25, 300), (3_001, 30, 2000)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lanes", [2, 4])
def test_slots_bits_equal_tile_kernel(smm, dtype, lanes):
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
        assert name == SLOTS and nbytes > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slots_in_place_and_fused_dots(smm, dtype):
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
    for name, A in (("tile", T), ("slots", S)):
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
            fin = torch.zeros(host.finish_len(), dtype=td, device=dev)
            out = torch.zeros(n, dtype=td, device=dev)
            A.spmv_fused_dev(0, None, x, out, mode, w1, fin, finish=True)
            torch.cuda.synchronize()
            o = host.finish_totals_offset()
            res[name, "finish", mode] = fin[o:o + 2].cpu().numpy()
    np.testing.assert_array_equal(res["slots", "inplace"], res["tile", "inplace"])
    tol = 1e-4 if dtype == np.float32 else 1e-11
    for mode in (1, 2):
        np.testing.assert_array_equal(res["slots", "out", mode], res["tile", "out", mode])
        np.testing.assert_allclose(res["slots", "dots", mode], res["tile", "dots", mode], rtol=tol)
        cnt = 2 if mode == 2 else 1  # totals: out.w1 (mode 1); out.out, out.w1 (mode 2)
        np.testing.assert_allclose(res["slots", "finish", mode][:cnt].astype(np.float64), res["slots", "dots", mode][:cnt], rtol=tol)


def test_slots_propagate_inf_and_nan(smm):
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 9, 4096, dtype=np.float32)
    T, S = handles(smm, csr, 2)
    x = np.random.default_rng(2).uniform(-1, 1, n).astype(np.float32)
    x[[5, 700, 10_000, 15_990]] = [np.inf, np.nan, -np.inf, np.nan]
    want = spmv(T, x)
    got = spmv(S, x)
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(got, want)


def test_slots_follow_every_edit(smm):
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 13, 4096, dtype=np.float32)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    _, S = handles(smm, csr, 2)
    _, O = handles(smm, gen.banded_random_spd(n, 25, 13, 4096, dtype=np.float32), 2)
    spmv(S, x)  # the copy is built
    assert S.kernel_desc()[0] == SLOTS
    rows = np.repeat(np.arange(n), np.diff(csr[0]))

    def check(what):
        F = smm.CSRMatrix(n, n, csr[0], csr[1], S.get_values())
        F.set_kernel(PATTERN, 2)
        F.pattern_slots(1)
        np.testing.assert_array_equal(spmv(S, x), spmv(F, x), err_msg=what)

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


def test_slots_fallback_when_refused(smm):
    """AUTO's rule (mode 2 on a set kernel): a matrix with few uniform waves keeps the tile kernel, with its bits"""
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
        A.pattern_slots(0)
        assert A.kernel_desc()[0] == TILE
        np.testing.assert_array_equal(spmv(A, x), got)


@pytest.mark.parametrize("precond", [None, "JACOBI"])
def test_slots_bicgstab_agrees_with_tile_kernel(smm, precond):
    n = 16_001
    csr = gen.banded_random_spd(n, 25, 0x5EED, 8192, dtype=np.float32)
    b = np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)
    res = {}
    for mode in (0, 1):
        A = smm.CSRMatrix(n, n, *csr)
        A.set_kernel(PATTERN, 2)
        A.pattern_slots(mode)
        M = A.getPreconditioner(smm.SolverPreconditioner.JACOBI) if precond else None
        x = np.zeros(n, dtype=np.float32)
        info = {}
        st = smm.BiCGStab(A, b, x, 200, 1e-6, M=M, info=info)
        res[mode] = (int(st), info.get("iterations"), x)
        assert A.kernel_desc()[0] == (SLOTS if mode else TILE)
    assert res[0][0] == res[1][0] == 0  # SUCCESS: the loop stopped early on its device-side done flag
    assert abs(res[0][1] - res[1][1]) <= 2
    np.testing.assert_allclose(res[1][2], res[0][2], rtol=0, atol=1e-4 * np.abs(res[0][2]).max())
