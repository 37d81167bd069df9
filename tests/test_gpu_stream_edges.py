"""spmvStreamKernel<T, L> and spmvTileKernel<T, L, G> (csrc/smm_spmv.hip) at the edges of the tile cut and in every instantiation, against
the oracle by the rules of tests/test_gpu_spmv.py: bit-identical at one lane per row, else |out - ref| <= bound(csr, x, dtype, lhs).

The cases (tests/stream_cases.py; tests/test_stream_cases_cpu.py asserts that each holds its edge and that at least 60 % of its rows sit in
staged tiles) are sized for tiles of 1021 entries, so the tests pin SMM_HIP_STREAM_NV=1.  The device's cut is checked without a new ABI:
tile_info() after the first SpMV must equal (tiles, cap_nnz, max_rows, tile_kernel) of the restated cut.  The environment is changed with
monkeypatch before a handle is created (these switches are read at every ask); SMM_HIP_STREAM_VARIANT is latched once per process, so the
two kernels it alone reaches run in a fresh child, tests/stream_variant_worker.py.

Instantiations launched here, per dtype: the pipelined kernel at L = 1, 8, 16, 32, 64 (in process) and L = 2, 4 (child, variant 0); the TILE
kernel at L = 2, 4 x G = 4 .. 16 (in process) and L = 1 x G = 4 .. 16 (child, variant 1).  Run with -s to see each (kernel, dtype, L, G)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import stream_cases as sc
from test_gpu_spmv import bound

from oracle.oracle import OP_ASSIGN

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("SMM_HIP_STREAM_NV", "SMM_HIP_TILE_BATCH", "SMM_HIP_XCD_CHUNK_TILES", "SMM_HIP_SPMV_FAMILY", "SMM_HIP_SPMV_LANES")


@pytest.fixture(autouse=True)
def tiles_of_1021(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SMM_HIP_STREAM_NV", "1")


def handle(smm, prob, lanes):
    A = smm.CSRMatrix(prob["rows"], prob["cols"], *prob["csr"])
    A.set_kernel(sc.STREAM, lanes)
    assert A.get_kernel() == (sc.STREAM, lanes)
    return A


def run_and_check(smm, oracle, prob, lanes, geometry, what, forced_batch=None):
    """a fresh handle: the three operations and rMultSub in place against the oracle, tile_info() behind the first SpMV against the restated cut"""
    A = handle(smm, prob, lanes)
    seen = []
    outs = sc.run_ops(A, prob, after_first=lambda: seen.append(A.tile_info()))
    tiles = sc.cut_rows(prob["csr"][0], geometry[0], geometry[1])
    assert seen[0] == (len(tiles) - 1, *geometry), what
    assert A.tile_info() == seen[0] and A.get_kernel() == (sc.STREAM, lanes)
    assert sc.mismatches(outs, sc.references(oracle, prob), prob, lanes, bound) == [], what
    print("launched:", "tile" if geometry[2] else "stream", prob["x"].dtype.name, lanes,
          sc.tile_batch(prob["csr"][0], lanes, forced_batch) if geometry[2] else "-", what)
    return A, outs


@pytest.mark.parametrize("lanes", sc.LANES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cases_by_lane_count(smm, oracle, dtype, lanes):
    """edges, seams and few on the default kernel of every lane count: the pipelined kernel at 1, 8, 16, 32 and 64 lanes, the TILE kernel at 2, 4"""
    geometry = sc.expected_geometry(lanes, None, 1, dtype)
    assert geometry[0] == sc.CAP_NNZ and geometry[2] == (1 if lanes in (2, 4) else 0)
    for name in ("edges", "seams-multiple", "seams-odd", "few"):
        A, _ = run_and_check(smm, oracle, sc.problem(name, dtype, geometry), lanes, geometry, (name, lanes))
        if name == "few":
            assert A.tile_info()[0] == 3  # a grid of 3 workgroups: nGroups == 3


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_batch_sweep_gives_the_same_bits(smm, oracle, monkeypatch, dtype, lanes):
    """spmvTileKernel<T, L, 4 .. 16>: G changes how a piece is walked, not the order of its sum"""
    geometry = sc.expected_geometry(lanes, None, 1, dtype)
    for name in ("batch", "edges"):
        prob = sc.problem(name, dtype, geometry, lanes=lanes)
        first = None
        for g in range(4, 17):
            monkeypatch.setenv("SMM_HIP_TILE_BATCH", str(g))
            _, outs = run_and_check(smm, oracle, prob, lanes, geometry, (name, lanes, g), forced_batch=g)
            first = first or outs
            for op, out in outs.items():
                np.testing.assert_array_equal(out, first[op], err_msg=f"{name} {op} batch {g} against batch 4")


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_sweep(smm, oracle, monkeypatch, dtype, lanes):
    """SMM_HIP_STREAM_NV: at one lane per row (pipelined kernel, as many passes as its registers hold) the outputs are the oracle's bits whatever
    the cut; at 2 lanes (TILE kernel) 1 .. 7, the last clipped to CAP_MAX -- tile_info() must show the capacity streamCap computes"""
    values = range(1, 8) if lanes == 2 else range(1, 5) if dtype == np.float32 else range(1, 3)
    built_for = sc.expected_geometry(lanes, None, 1, dtype)
    caps = []
    for nv in values:
        monkeypatch.setenv("SMM_HIP_STREAM_NV", str(nv))
        geometry = sc.expected_geometry(lanes, None, nv, dtype)
        caps.append(geometry[0])
        for name in ("edges", "seams-odd"):
            run_and_check(smm, oracle, sc.problem(name, dtype, built_for), lanes, geometry, (name, lanes, nv))
    if lanes == 2:
        assert caps == ([1021, 2045, 3069, 4093, 5117, 6141, 6553] if dtype == np.float32 else [1021, 2045, 3069, 4093, 4361, 4361, 4361])
    else:
        assert caps == [1024 * nv - 3 for nv in values]


@pytest.mark.parametrize("lanes", [1, 2, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_xcd_chunk_tiles_gives_the_same_bits(smm, oracle, monkeypatch, dtype, lanes):
    """tiles dealt to the workgroup groups 1, 3 or 5 at a time, round-robin, with a tile count that is no multiple: the same outputs, bit for bit,
    as with one contiguous share each"""
    geometry = sc.expected_geometry(lanes, None, 1, dtype)
    for name, prob, values in (("few", sc.problem("few", dtype, geometry, tiles=11), (1, 3)), ("seams-odd", sc.problem("seams-odd", dtype), (5,))):
        monkeypatch.delenv("SMM_HIP_XCD_CHUNK_TILES", raising=False)
        A, base = run_and_check(smm, oracle, prob, lanes, geometry, (name, lanes))
        assert name != "few" or A.tile_info()[0] == 11  # (11 tiles in chunks of 3: the last chunk is short, groups 4 .. 7 get nothing)
        for chunk in values:
            monkeypatch.setenv("SMM_HIP_XCD_CHUNK_TILES", str(chunk))
            _, outs = run_and_check(smm, oracle, prob, lanes, geometry, (name, lanes, chunk))
            for op, out in outs.items():
                np.testing.assert_array_equal(out, base[op], err_msg=f"{name} {op} chunk {chunk}")


@pytest.mark.parametrize("lanes", [1, 2, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_dots_on_a_grid_below_the_partials_count(smm, oracle, dtype, lanes):
    """3 and a few dozen workgroups: the epilogue clears the partial slots no workgroup owns (a buffer prefilled with NaN comes back finite) and
    the in-launch finish, launched twice, leaves the totals; tolerances of test_headline_kernel_against_oracle_at_scale"""
    import torch

    dev = torch.device("cuda:0")
    td = torch.float32 if dtype == np.float32 else torch.float64
    stream = torch.cuda.current_stream().cuda_stream
    P = smm.host.partials_count()
    geometry = sc.expected_geometry(lanes, None, 1, dtype)
    for name in ("few", "edges"):
        prob = sc.problem(name, dtype, geometry)
        n = prob["rows"]
        A = handle(smm, prob, lanes)
        ref = sc.references(oracle, prob)["rMult"]
        ref64, lhs64 = ref.astype(np.float64), prob["lhs"].astype(np.float64)
        want_oo, want_ow = float(ref64 @ ref64), float(ref64 @ lhs64)
        tol = 4 * n * np.finfo(dtype).eps
        dx, dw = torch.from_numpy(prob["x"]).to(dev), torch.from_numpy(prob["lhs"]).to(dev)
        dout = torch.empty(n, dtype=td, device=dev)
        for mode in (1, 2):
            parts = torch.full((2 * P,), float("nan"), dtype=td, device=dev)
            A.spmv_fused_dev(OP_ASSIGN, None, dx, dout, mode, dw, parts, stream)
            fin = torch.zeros(smm.host.finish_len(), dtype=td, device=dev)
            for _ in range(2):  # twice: the arrival counter must be back at zero for the second launch
                A.spmv_fused_dev(OP_ASSIGN, None, dx, dout, mode, dw, fin, stream, finish=True)
            torch.cuda.synchronize()
            tiles = A.tile_info()[0]
            assert 0 < tiles < P and (name != "few" or tiles == 3)  # fewer workgroups than slots: the rest must be cleared
            assert sc.mismatches({"rMult": dout.cpu().numpy()}, {"rMult": ref}, prob, lanes, bound) == [], (name, mode)
            sums = parts.cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(sums[:mode * P])), (name, mode, int(np.flatnonzero(~np.isfinite(sums[:mode * P]))[0]))
            off = smm.host.finish_totals_offset()
            totals = fin.cpu().numpy()
            got, want = ((sums[:P].sum(),), (want_ow,)) if mode == 1 else ((sums[:P].sum(), sums[P:].sum()), (want_oo, want_ow))
            for i, (g, w) in enumerate(zip(got, want)):
                scale = float(np.abs(ref64 * (ref64 if (mode == 2 and i == 0) else lhs64)).sum())
                assert abs(g - w) <= tol * scale, (name, mode, i, g, w)
                assert abs(float(totals[off + i]) - w) <= tol * scale, (name, mode, i, totals[off + i], w)
                # the finished total is the sum of the same partials in the fixed order of the separate summing kernel
                assert abs(float(totals[off + i]) - g) <= 2048 * np.finfo(dtype).eps * scale


def run_worker(variant, *args):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["SMM_HIP_STREAM_VARIANT"] = str(variant)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "stream_variant_worker.py"), str(variant), *args], cwd=os.path.dirname(HERE), env=env,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("STREAM_VARIANT_WORKER ")]
    assert len(lines) == 1, proc.stdout[-2000:] + proc.stderr[-2000:]
    rep = json.loads(lines[0][len("STREAM_VARIANT_WORKER "):])
    assert rep["variant"] == variant
    assert rep["n_failures"] == 0, "\n".join(rep["failures"]) + "\n" + proc.stderr[-2000:]
    print("launched:", sorted({tuple("-" if v is None else v for v in row) for row in rep["launched"]}))
    return rep


def test_tile_kernel_with_one_lane_per_row_in_a_fresh_process():
    """SMM_HIP_STREAM_VARIANT=1: spmvTileKernel<T, 1, 4 .. 16>, bit-identical to the oracle"""
    rep = run_worker(1)
    cases = 4
    assert rep["checks"] == 2 * cases * 13 * 4  # dtypes x cases x batch values x (three operations and the one in place)
    assert {tuple(row) for row in rep["launched"]} == {("tile", dn, 1, g) for dn in ("float32", "float64") for g in range(4, 17)}


def test_pipelined_kernel_with_pieces_in_one_wave_in_a_fresh_process(smm, oracle, tmp_path):
    """SMM_HIP_STREAM_VARIANT=0: spmvStreamKernel<T, 2> and <T, 4> within the bound, and on the rows both kernels stage bit-identical to the TILE
    kernel's outputs at the same lane count, computed here"""
    defaults = {}
    for dtype in DTYPES:
        for lanes in (2, 4):
            pipelined = sc.expected_geometry(lanes, 0, 1, dtype)  # the child's `edges` is the pipelined kernel's
            geometry = sc.expected_geometry(lanes, None, 1, dtype)
            assert geometry[2] == 1 and pipelined[:2] == geometry[:2]
            for name in ("edges", "batch", "seams-multiple", "seams-odd"):
                prob = sc.problem(name, dtype, pipelined, lanes=lanes)
                _, outs = run_and_check(smm, oracle, prob, lanes, geometry, (name, lanes))
                for op, out in outs.items():
                    defaults[f"{name}/{np.dtype(dtype).name}/{lanes}/{op}"] = out
    path = str(tmp_path / "tile_kernel_outputs.npz")
    np.savez(path, **defaults)
    rep = run_worker(0, path)
    assert rep["checks"] == 2 * 2 * 4 * (4 + 4)  # dtypes x lane counts x cases x (outputs against the oracle + against the TILE kernel)
    assert rep["compared_rows"] > 0.6 * sum(sc.problem(name, np.float32, sc.expected_geometry(lanes, 0, 1, np.float32), lanes=lanes)["rows"]
                                            for lanes in (2, 4) for name in ("edges", "batch", "seams-multiple", "seams-odd")) * 2
    assert {tuple(row) for row in rep["launched"]} == {("stream", dn, lanes, None) for dn in ("float32", "float64") for lanes in (2, 4)}
