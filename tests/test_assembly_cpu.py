"""Assembling a CSRMatrix from triplets (smm_hip_assembly_*): the CPU side.  The boundary declares and exports the entry points, nothing
is computed without a GPU, and `assemble_model` below -- the rule of include/smm_hip.h in numpy: a stable sort of the (row, col) keys,
then every run of equal keys summed left to right in the value dtype, the first contribution taken as it is -- reproduces the arrays the
reference's own TripletMatrix -> CSRMatrix produced (tests/golden/reference_outputs_v1.npz).  tests/test_gpu_assembly.py compares the
device against this model bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from sparse_matrix_math_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = ("mesh1e1", "mesh1em1", "mesh1em6")
ENTRY_POINTS = ["smm_hip_assembly_create", "smm_hip_assembly_create_dev", "smm_hip_assembly_info", "smm_hip_assembly_pattern", "smm_hip_assembly_destroy"] + [
    f"smm_hip_assembly_{base}_{suf}" for base in ("csr_create", "csr_create_dev", "refill", "refill_dev") for suf in ("f32", "f64")]


def assemble_model(rows, cols, row_idx, col_idx, values):
    """(start, positions, values, first_active_start, longest_run) of the list of triplets: TripletMatrix::addEntry in list order
    (ref:606-618) followed by CSRMatrix::fillArrays (ref:1606-1641)"""
    row_idx = np.asarray(row_idx, dtype=np.int64)
    col_idx = np.asarray(col_idx, dtype=np.int64)
    values = np.asarray(values)
    assert row_idx.shape == col_idx.shape == values.shape
    assert ((row_idx >= 0) & (row_idx < rows) & (col_idx >= 0) & (col_idx < cols)).all()
    n = row_idx.size
    key = (row_idx << 32) | col_idx
    order = np.argsort(key, kind="stable")  # list order inside a run of equal keys
    skey = key[order]
    svals = values[order]
    run_begin = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]])) if n else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([run_begin, [n]]))
    out = svals[run_begin].copy()  # the first contribution as it is
    active = np.flatnonzero(lens > 1)
    step = 1
    while active.size:
        out[active] = out[active] + svals[run_begin[active] + step]  # one rounding per further contribution, in the value dtype
        step += 1
        active = active[lens[active] > step]
    hrow = skey[run_begin] >> 32
    start = np.zeros(rows + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(hrow, minlength=rows)[:rows]) if rows else 0
    positions = (skey[run_begin] & 0xFFFFFFFF).astype(np.int32)
    nonempty = np.flatnonzero(start[1:] != 0)
    first_active = int(nonempty[0]) if nonempty.size else rows  # ref:1619-1628
    return start, positions, out.astype(values.dtype, copy=False), first_active, int(lens.max()) if n else 0


def csr_to_triplets(start, positions, values):
    rows = np.repeat(np.arange(len(start) - 1, dtype=np.int32), np.diff(start))
    return rows, np.asarray(positions, dtype=np.int32), np.asarray(values)


def header_text():
    import re

    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smm_hip.h")).read(), flags=re.S)


def test_header_declares_and_both_libraries_export_the_entry_points():
    text = header_text()
    lib = _lib.load()
    fma = ctypes.CDLL(_lib.library_path(fma=True))
    for name in ENTRY_POINTS:
        assert f"{name}(" in text, f"{name} not declared in include/smm_hip.h"
        assert hasattr(lib, name), f"{name} not exported by libsmm_hip.so"
        assert hasattr(fma, name), f"{name} not exported by libsmm_hip_fma.so"
        assert name in _lib.exported_symbols()
    assert "typedef struct smm_hip_assembly smm_hip_assembly;" in text


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_assembly_without_gpu():
    import sparse_matrix_math_amd as smm

    with pytest.raises(smm.SmmHipError) as e:
        smm.AssemblyPlan(3, 3, [0, 1, 2], [0, 1, 2])
    assert e.value.code == _lib.SMM_HIP_ERR_NO_DEVICE
    with pytest.raises(smm.SmmHipError) as e:
        smm.CSRMatrix.from_triplets(3, 3, [0, 1, 2], [0, 1, 2], np.ones(3))
    assert e.value.code == _lib.SMM_HIP_ERR_NO_DEVICE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("asset", ASSETS)
def test_model_reproduces_the_reference_triplet_to_csr(golden, asset, dtype):
    """the entries of each asset fed as triplets in a seeded random order: the three arrays of the reference, bit for bit"""
    start, pos, val = (golden[f"asset/{asset}/{k}"] for k in ("start", "positions", "values"))
    val = val.astype(dtype)
    n = len(start) - 1
    r, c, v = csr_to_triplets(start, pos, val)
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(r.size)
        s2, p2, v2, first, longest = assemble_model(n, n, r[p], c[p], v[p])
        np.testing.assert_array_equal(s2, start)
        np.testing.assert_array_equal(p2, pos)
        assert v2.dtype == np.dtype(dtype) and v2.tobytes() == val.tobytes()
        assert first == 0 and longest == 1


def test_model_follows_list_order():
    """repeated pairs: addEntry's running sum in LIST order, the first contribution as it is"""
    f = np.float32
    r = np.array([2, 0, 2, 2, 0, 2], dtype=np.int32)
    c = np.array([1, 3, 1, 1, 3, 0], dtype=np.int32)
    v = np.array([1e8, -0.0, 1.0, -1e8, 0.5, -0.0], dtype=f)
    start, pos, val, first, longest = assemble_model(4, 5, r, c, v)
    assert start.tolist() == [0, 1, 1, 3, 3] and pos.tolist() == [3, 0, 1] and first == 0 and longest == 3
    want = np.array([f(-0.0) + f(0.5), f(-0.0), (f(1e8) + f(1.0)) + f(-1e8)], dtype=f)
    assert val.tobytes() == want.tobytes()
    assert np.signbit(val[1]) and val[2] == 0.0  # a lone -0.0 stays -0.0; 1e8 + 1 rounds to 1e8 in fp32: list order, not sorted order
    # empty list, leading empty rows
    s, p, w, first, longest = assemble_model(3, 2, [], [], np.zeros(0, dtype=f))
    assert s.tolist() == [0, 0, 0, 0] and p.size == 0 and w.size == 0 and first == 3 and longest == 0
    s, p, w, first, longest = assemble_model(5, 2, [3], [1], np.ones(1, dtype=f))
    assert s.tolist() == [0, 0, 0, 0, 1, 1] and first == 3
