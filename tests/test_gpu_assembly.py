"""A CSRMatrix assembled from triplets on the device (smm_hip_assembly_*, csrc/smm_assembly.hip), through the C ABI / the Python mirror.
The pattern must be the reference's fillArrays result and the values those of its addEntry calls IN LIST ORDER, bit for bit: compared
with the reference's own arrays (golden assets) and with the numpy model of tests/test_assembly_cpu.py, which that file pins to them.  A
refill must leave the handle multiplying exactly like a fresh handle made from the expected values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen
from test_assembly_cpu import ASSETS, assemble_model, csr_to_triplets
from test_gpu_csr_update import CONFIGS, small_matrices, spmv, try_kernel

pytestmark = pytest.mark.gpu
VECTOR, STREAM, PATTERN = 1, 2, 3
NONE, MASKS, CODES, CONST = 0, 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def split_triplets(csr, rng, dtype, max_parts=6):
    """every entry split into 1 .. max_parts contributions whose magnitudes spread over 16 binades (they add up to the entry, to
    rounding), the whole list shuffled; returns (rows, cols, contributions, parts per entry)"""
    r, c, v = csr_to_triplets(*csr)
    parts = rng.integers(1, max_parts + 1, r.size)
    owner = np.repeat(np.arange(r.size), parts)
    mag = np.exp2(rng.uniform(-8, 8, owner.size)) * rng.choice([-1.0, 1.0], owner.size)
    w = (v[owner].astype(np.float64) * mag).astype(dtype)
    first = np.concatenate([[0], np.cumsum(parts)[:-1]])
    isfirst = np.zeros(owner.size, dtype=bool)
    isfirst[first] = True
    rest = np.add.reduceat(np.where(isfirst, 0.0, w.astype(np.float64)), first)
    w[first] = (v.astype(np.float64) - rest).astype(dtype)
    p = rng.permutation(owner.size)
    return r[owner][p], c[owner][p], w[p], parts


def check_against_model(smm, rows, cols, r, c, v, first_active=None):
    start, pos, val, first, longest = assemble_model(rows, cols, r, c, v)
    plan = smm.AssemblyPlan(rows, cols, r, c)
    assert (plan.rows, plan.cols, plan.n, plan.nnz, plan.longest_run) == (rows, cols, len(r), len(pos), longest)
    s2, p2 = plan.pattern()
    np.testing.assert_array_equal(s2, start)
    np.testing.assert_array_equal(p2, pos)
    A = plan.assemble(v)
    assert (A.rows, A.cols, A.nnz, A.first_active_start) == (rows, cols, len(pos), first)
    if first_active is not None:
        assert first == first_active
    assert same_bits(A.get_values(), val)
    return plan, A, (start, pos, val)


def bicgstab(smm, A, b, iters):
    x = np.zeros(A.rows, dtype=A.dtype)
    info = {}
    st = smm.BiCGStab(A, b, x, iters, 1e-30, info=info)
    return int(st), info["iterations"], x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("asset", ASSETS)
def test_golden_assets_from_shuffled_triplets(smm, golden, asset, dtype):
    start, pos, val = (golden[f"asset/{asset}/{k}"] for k in ("start", "positions", "values"))
    val = val.astype(dtype)
    n = len(start) - 1
    r, c, v = csr_to_triplets(start, pos, val)
    p = np.random.default_rng(17).permutation(r.size)
    plan = smm.AssemblyPlan(n, n, r[p], c[p])
    s2, p2 = plan.pattern()
    np.testing.assert_array_equal(s2, start)
    np.testing.assert_array_equal(p2, pos)
    assert plan.nnz == plan.n == pos.size and plan.longest_run == 1
    A = plan.assemble(v[p])
    assert same_bits(A.get_values(), val) and A.first_active_start == 0
    F = smm.CSRMatrix(n, n, start, pos, val)
    A.set_kernel(STREAM, 1)
    F.set_kernel(STREAM, 1)
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    assert same_bits(spmv(A, x, dtype), spmv(F, x, dtype))
    b = spmv(F, np.ones(n, dtype=dtype), dtype)
    sa, sf = bicgstab(smm, A, b, 12), bicgstab(smm, F, b, 12)
    assert sa[:2] == sf[:2] and same_bits(sa[2], sf[2])
    # the one-call form
    B = smm.CSRMatrix.from_triplets(n, n, r[p], c[p], v[p])
    assert same_bits(B.get_values(), val) and B.nnz == pos.size


def generated(dtype):
    return {
        "poisson2d": gen.poisson2d(150, 130, dtype=dtype),
        "convdiff3d": gen.convdiff3d_varying(18, dtype=dtype),
        "dictionary": gen.banded_random_spd(6000, 32, 0x5EED, 2500, dtype=dtype),
    }


@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_matrices_split_contributions_follow_list_order(smm, dtype):
    encodings = {"poisson2d": MASKS, "convdiff3d": MASKS, "dictionary": CODES}  # (the summed splits no longer give constant diagonals)
    for name, csr in generated(dtype).items():
        rng = np.random.default_rng(3)
        n = len(csr[0]) - 1
        r, c, w, parts = split_triplets(csr, rng, dtype)
        # what keeps this honest: the same contributions summed in sorted-value order give other bits for >= 1 % of the split entries
        o = np.argsort(w, kind="stable")
        in_list_order = assemble_model(n, n, r, c, w)[2]
        in_value_order = assemble_model(n, n, r[o], c[o], w[o])[2]
        differs = in_list_order.view(np.uint8).reshape(len(parts), -1) != in_value_order.view(np.uint8).reshape(len(parts), -1)
        fraction = differs.any(axis=1)[parts > 1].mean()
        print(f"{name} {np.dtype(dtype).name}: {fraction:.3f} of the split entries depend on the order")
        assert fraction >= 0.01, (name, fraction)
        plan, A, (start, pos, val) = check_against_model(smm, n, n, r, c, w)
        np.testing.assert_array_equal(start, csr[0])
        np.testing.assert_array_equal(pos, csr[1])
        assert plan.longest_run == parts.max()
        F = smm.CSRMatrix(n, n, start, pos, val)
        x = rng.uniform(-1, 1, n).astype(dtype)
        for fam, lanes in [(STREAM, 1), (PATTERN, 1)]:
            assert try_kernel(A, fam, lanes) and try_kernel(F, fam, lanes)
            assert same_bits(spmv(A, x, dtype), spmv(F, x, dtype)), (name, fam)
        assert A.pattern_info()[0] == encodings[name] and A.pattern_info() == F.pattern_info()
        assert A.hasSameNonZeroPattern(F)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(smm, dtype):
    rng = np.random.default_rng(5)
    none = np.zeros(0, dtype=np.int32)
    # no triplets at all
    plan, A, _ = check_against_model(smm, 4, 3, none, none, np.zeros(0, dtype=dtype), first_active=4)
    y = np.full(4, 7, dtype=dtype)
    A.rMult(np.ones(3, dtype=dtype), y)
    assert not y.any()
    plan.refill(A, np.zeros(0, dtype=dtype))
    check_against_model(smm, 0, 0, none, none, np.zeros(0, dtype=dtype), first_active=0)
    # empty rows at both ends, rectangular, repeated pairs
    r = np.array([4, 2, 3, 2, 4, 2, 3], dtype=np.int32)
    c = np.array([0, 2, 1, 2, 0, 0, 1], dtype=np.int32)
    v = rng.uniform(-1, 1, r.size).astype(dtype)
    plan, A, csr = check_against_model(smm, 7, 3, r, c, v, first_active=2)
    assert csr[0].tolist() == [0, 0, 0, 2, 3, 4, 4, 4] and plan.longest_run == 2
    F = smm.CSRMatrix(7, 3, *csr)
    x = rng.uniform(-1, 1, 3).astype(dtype)
    assert same_bits(spmv(A, x, dtype), spmv(F, x, dtype))
    check_against_model(smm, 3, 9, [0, 2, 0], [8, 8, 0], rng.uniform(-1, 1, 3).astype(dtype), first_active=0)
    # one entry carrying a run of 5000 contributions of mixed magnitudes, among ordinary ones
    csr = gen.poisson2d(20, dtype=dtype)
    r, c, v = csr_to_triplets(*csr)
    big = np.exp2(rng.uniform(-10, 10, 5000)) * rng.choice([-1.0, 1.0], 5000)
    r = np.concatenate([r, np.full(5000, 7, dtype=np.int32)])
    c = np.concatenate([c, np.full(5000, 8, dtype=np.int32)])
    v = np.concatenate([v, big.astype(dtype)])
    p = rng.permutation(r.size)
    plan, A, _ = check_against_model(smm, 400, 400, r[p], c[p], v[p])
    assert plan.longest_run == 5001 and plan.nnz == csr[1].size  # (7, 8) is a stored entry of the 20 x 20 grid
    # a list without repeated pairs keeps only the permutation
    csr = gen.random_rows(300, 200, 0, 9, seed=4, dtype=dtype, empty_every=5)
    r, c, v = csr_to_triplets(*csr)
    p = rng.permutation(r.size)
    plan, A, got = check_against_model(smm, 300, 200, r[p], c[p], v[p])
    assert plan.n == plan.nnz and plan.longest_run == 1 and same_bits(got[2], csr[2])
    # a lone -0.0 stays -0.0; -0.0 + -0.0 too; -0.0 + 0.0 is +0.0
    v = np.array([-0.0, -0.0, -0.0, -0.0, 0.0], dtype=dtype)
    plan, A, got = check_against_model(smm, 2, 2, [0, 1, 1, 0, 0], [0, 1, 1, 1, 1], v)
    assert np.signbit(A.get_values()).tolist() == [True, False, True]


OUT_OF_RANGE = [("row < 0", -1, 0), ("row >= rows", 6, 0), ("col < 0", 0, -3), ("col >= cols", 0, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_entries_are_refused_by_index(smm, dtype):
    import torch

    rng = np.random.default_rng(2)
    rows, cols, n = 6, 5, 1000
    for what, br, bc in OUT_OF_RANGE:
        r = rng.integers(0, rows, n).astype(np.int32)
        c = rng.integers(0, cols, n).astype(np.int32)
        good = (r.copy(), c.copy())
        for at in (977, 613):  # two offenders: the FIRST list index is named
            r[at], c[at] = br, bc
        with pytest.raises(smm.SmmHipError) as e:
            smm.AssemblyPlan(rows, cols, r, c)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID and "entry 613 " in str(e.value), (what, str(e.value))
        dr, dc = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
        with pytest.raises(smm.SmmHipError) as e:
            smm.AssemblyPlan.from_device(rows, cols, n, dr, dc, torch.cuda.current_stream().cuda_stream)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID and "entry 613 " in str(e.value), (what, str(e.value))
        check_against_model(smm, rows, cols, good[0], good[1], rng.uniform(-1, 1, n).astype(dtype))  # a correct call succeeds afterwards
    with pytest.raises(smm.SmmHipError) as e:
        smm.AssemblyPlan(0, 0, [0], [0])  # rows == 0: every entry is out of range
    assert e.value.code == _lib.SMM_HIP_ERR_INVALID and "entry 0 " in str(e.value)
    h = ctypes.c_void_p()
    st = _lib.load().smm_hip_assembly_create(4, 4, (1 << 31), None, None, ctypes.byref(h))  # refused before any array is looked at
    assert st == _lib.SMM_HIP_ERR_INVALID and not h.value and b"32-bit limit" in _lib.load().smm_hip_last_error()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refill_refuses_foreign_matrices_and_the_other_dtype(smm, dtype):
    rng = np.random.default_rng(6)
    csr = gen.poisson2d(12, dtype=dtype)
    n = len(csr[0]) - 1
    r, c, v = csr_to_triplets(*csr)
    plan, A, _ = check_against_model(smm, n, n, r, c, v)
    other = smm.AssemblyPlan(n, n, r, c)  # the same list, another plan
    newv = rng.uniform(-1, 1, v.size).astype(dtype)
    for foreign in (smm.CSRMatrix(n, n, *csr), other.assemble(v)):
        with pytest.raises(smm.SmmHipError) as e:
            plan.refill(foreign, newv)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID
        assert same_bits(foreign.get_values(), csr[2])
    odt = np.float64 if dtype == np.float32 else np.float32
    suf = "f64" if dtype == np.float32 else "f32"
    wrong = newv.astype(odt)
    st = getattr(_lib.load(), f"smm_hip_assembly_refill_{suf}")(plan._h, A._h, wrong.ctypes.data_as(ctypes.c_void_p), 0)
    assert st == _lib.SMM_HIP_ERR_INVALID
    suf = "f32" if dtype == np.float32 else "f64"
    st = getattr(_lib.load(), f"smm_hip_assembly_refill_{suf}")(plan._h, A._h, newv.ctypes.data_as(ctypes.c_void_p), 2)  # unknown mode
    assert st == _lib.SMM_HIP_ERR_INVALID
    assert same_bits(A.get_values(), csr[2])
    plan.refill(A, newv)  # ... and the plan's own matrix takes it, also once the plan that made `foreign` is gone
    assert same_bits(A.get_values(), newv)
    plan.close()
    x = rng.uniform(-1, 1, n).astype(dtype)
    assert same_bits(spmv(A, x, dtype), spmv(smm.CSRMatrix(n, n, csr[0], csr[1], newv), x, dtype))  # the matrix outlives its plan


def test_refused_allocation_then_retry(smm):
    lib = _lib.load()
    rng = np.random.default_rng(8)
    csr = gen.poisson2d(40, dtype=np.float32)
    n = len(csr[0]) - 1
    r, c, w, _ = split_triplets(csr, rng, np.float32)
    try:
        lib.smm_hip_debug_fail_next_alloc(1)
        with pytest.raises(smm.SmmHipError) as e:
            smm.AssemblyPlan(n, n, r, c)
        assert e.value.code == _lib.SMM_HIP_ERR_NOMEM
        lib.smm_hip_debug_fail_next_alloc(8 * r.size)  # the keys of the sort, after the plan's first array: half-way through the symbolic pass
        with pytest.raises(smm.SmmHipError) as e:
            smm.AssemblyPlan(n, n, r, c)
        assert e.value.code == _lib.SMM_HIP_ERR_NOMEM
        plan = smm.AssemblyPlan(n, n, r, c)
        lib.smm_hip_debug_fail_next_alloc(1)
        with pytest.raises(smm.SmmHipError) as e:
            plan.assemble(w)
        assert e.value.code == _lib.SMM_HIP_ERR_NOMEM
        A = plan.assemble(w)
        lib.smm_hip_debug_fail_next_alloc(1)
        with pytest.raises(smm.SmmHipError) as e:
            plan.refill(A, w, add=True)
        assert e.value.code == _lib.SMM_HIP_ERR_NOMEM
    finally:
        lib.smm_hip_debug_fail_next_alloc(0)
    want = assemble_model(n, n, r, c, w)[2]
    assert same_bits(A.get_values(), want)  # the refused refill changed nothing
    plan.refill(A, w, add=True)
    assert same_bits(A.get_values(), want + want)


@pytest.mark.parametrize("analysed", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_refill_equals_a_fresh_handle(smm, oracle, dtype, analysed):
    rng = np.random.default_rng(12)
    for name, csr in small_matrices(dtype).items():
        n = len(csr[0]) - 1
        r, c, w1, _ = split_triplets(csr, rng, dtype, max_parts=4)
        plan = smm.AssemblyPlan(n, n, r, c)
        A = plan.assemble(w1)
        start, pos = plan.pattern()
        x = rng.uniform(-1, 1, n).astype(dtype)
        if analysed:
            assert try_kernel(A, PATTERN, 1), name
            A.set_kernel(0, 0)
        spmv(A, x, dtype)  # the first SpMV
        w2 = (w1 * rng.uniform(0.5, 2.0, w1.size)).astype(dtype)
        w3 = rng.permutation(w1)
        set_values = assemble_model(n, n, r, c, w2)[2]
        add_values = set_values + assemble_model(n, n, r, c, w3)[2]  # one rounding
        for add, w, want in ((False, w2, set_values), (True, w3, add_values)):
            tiles, enc_before = A.tile_info(), A.pattern_info()  # (the second round: after the PATTERN analysis in any case)
            assert enc_before[0] != CONST and (enc_before[0] != NONE or not (analysed or add))
            plan.refill(A, w, add=add)
            assert same_bits(A.get_values(), want), (name, add)
            assert A.tile_info() == tiles and A.pattern_info() == enc_before, (name, add)
            ecsr = (start, pos, want)
            F = smm.CSRMatrix(n, n, *ecsr)
            for fam, lanes in CONFIGS:
                assert try_kernel(A, fam, lanes) and try_kernel(F, fam, lanes), (name, add, fam, lanes)
                got = spmv(A, x, dtype)
                assert same_bits(got, spmv(F, x, dtype)), f"{name} add={add} {fam}/{lanes}"
                if lanes == 1:
                    np.testing.assert_array_equal(got, oracle.spmv(ecsr, 0, None, x), err_msg=f"{name} add={add} {fam}/1 oracle")
            A.set_kernel(0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refill_and_the_constant_diagonal_encoding(smm, dtype):
    rng = np.random.default_rng(13)
    csr = gen.poisson2d(120, dtype=dtype)
    n = len(csr[0]) - 1
    r, c, v = csr_to_triplets(*csr)
    p = rng.permutation(r.size)
    r, c, v = r[p], c[p], v[p]
    plan = smm.AssemblyPlan(n, n, r, c)
    A = plan.assemble(v)
    A.set_kernel(PATTERN, 1)
    assert A.pattern_info() == (CONST, 5)
    x = rng.uniform(-1, 1, n).astype(dtype)
    plan.refill(A, (v * dtype(-2.5)).astype(dtype))  # constant diagonals again: re-verified, stays
    assert A.pattern_info() == (CONST, 5)
    F = smm.CSRMatrix(n, n, csr[0], csr[1], csr[2] * dtype(-2.5))
    F.set_kernel(PATTERN, 1)
    assert same_bits(spmv(A, x, dtype), spmv(F, x, dtype))
    plan.refill(A, v, add=True)  # -2.5 v + v on every diagonal
    assert A.pattern_info() == (CONST, 5)
    w = rng.uniform(-1, 1, v.size).astype(dtype)
    plan.refill(A, w)  # varying values: drops to the masks with values read
    assert A.pattern_info() == (MASKS, 5)
    want = assemble_model(n, n, r, c, w)[2]
    F = smm.CSRMatrix(n, n, csr[0], csr[1], want)
    F.set_kernel(PATTERN, 1)
    assert same_bits(spmv(A, x, dtype), spmv(F, x, dtype))
    # solvers after a refill: the single-launch BiCGStab's slot-major copy follows
    previous = smm.host.bicgstab_resident(-1)
    try:
        csr = gen.convdiff3d_varying(24, dtype=dtype)
        n = len(csr[0]) - 1
        r, c, w1, _ = split_triplets(csr, rng, dtype, max_parts=3)
        plan = smm.AssemblyPlan(n, n, r, c)
        b = rng.uniform(-1, 1, n).astype(dtype)
        w2 = (w1 * dtype(0.75)).astype(dtype)
        want = assemble_model(n, n, r, c, w2)[2]
        for resident in (False, True):
            smm.host.bicgstab_resident(2 if resident else 0)
            A = plan.assemble(w1)
            A.set_kernel(PATTERN, 1)
            bicgstab(smm, A, b, 40)
            plan.refill(A, w2)
            F = smm.CSRMatrix(n, n, csr[0], csr[1], want)
            F.set_kernel(PATTERN, 1)
            sa, sf = bicgstab(smm, A, b, 40), bicgstab(smm, F, b, 40)
            assert sa[:2] == sf[:2] and same_bits(sa[2], sf[2]), resident
    finally:
        smm.host.bicgstab_resident(previous)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_forms_on_a_side_stream(smm, dtype):
    import torch

    rng = np.random.default_rng(14)
    dev = torch.device("cuda:0")
    csr = gen.convdiff3d_varying(18, dtype=dtype)
    n = len(csr[0]) - 1
    r, c, w1, _ = split_triplets(csr, rng, dtype)
    w2 = rng.permutation(w1)
    host_plan = smm.AssemblyPlan(n, n, r, c)
    H = host_plan.assemble(w1)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        dr, dc = torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)
        d1, d2 = torch.from_numpy(w1).to(dev), torch.from_numpy(w2).to(dev)
        plan = smm.AssemblyPlan.from_device(n, n, r.size, dr, dc, side.cuda_stream)
        dr.fill_(-7)  # the index arrays are not needed after the call
        dc.fill_(-7)
        A = plan.assemble_dev(d1, dtype, side.cuda_stream)
        side.synchronize()
        assert (plan.n, plan.nnz, plan.longest_run) == (host_plan.n, host_plan.nnz, host_plan.longest_run)
        for a, b in zip(plan.pattern(), host_plan.pattern()):
            np.testing.assert_array_equal(a, b)
        assert same_bits(A.get_values(), H.get_values()) and A.first_active_start == H.first_active_start
        plan.refill_dev(A, d2, False, side.cuda_stream)
        plan.refill_dev(A, d1, True, side.cuda_stream)
        side.synchronize()
        host_plan.refill(H, w2)
        host_plan.refill(H, w1, add=True)
        assert same_bits(A.get_values(), H.get_values())
        x = rng.uniform(-1, 1, n).astype(dtype)
        assert same_bits(spmv(A, x, dtype), spmv(H, x, dtype))


def test_full_size_benchmark_matrix_from_shuffled_triplets(smm):
    """the 10 M-row benchmark matrix (BASELINE config 3, fp32) expanded to 485 M triplets on the device, shuffled, assembled"""
    import torch

    from sparse_matrix_math_amd import host

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n, k, seed, mo = 10_000_000, 25, 0x5EED, 1 << 20
    nnz = host.gen_banded_nnz(n, k, seed, mo)
    d_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_pos = torch.empty(nnz, dtype=torch.int32, device=dev)
    d_val = torch.empty(nnz, dtype=torch.float32, device=dev)
    host.gen_banded_dev(n, k, seed, mo, d_start, d_pos, d_val, np.float32, stream)
    counts = (d_start[1:] - d_start[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), counts, output_size=nnz)
    perm = torch.randperm(nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    r, c, v = rows[perm], d_pos[perm], d_val[perm]
    del rows, perm, counts
    plan = smm.AssemblyPlan.from_device(n, n, nnz, r, c, stream)
    assert plan.nnz == nnz == 484552446 and plan.n == nnz and plan.longest_run == 1
    A = plan.assemble_dev(v, np.float32, stream)
    torch.cuda.synchronize()
    del r, c
    assert A.nnz == nnz and A.first_active_start == 0
    start, pos = plan.pattern()
    assert torch.equal(torch.from_numpy(start), d_start.cpu())
    assert torch.equal(torch.from_numpy(pos), d_pos.cpu())
    del start, pos
    assert torch.equal(torch.from_numpy(A.get_values()), d_val.cpu())
    G = smm.CSRMatrix.from_device(n, n, d_start, d_pos, d_val, np.float32)
    b = torch.rand(n, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) + 0.5
    xs = []
    for M in (A, G):
        x = torch.zeros_like(b)
        status, iters, res = host.bicgstab_dev(M, b, x, 20, 0.0, None, stream)
        assert iters == 20 and np.isfinite(res)
        xs.append(x)
    assert torch.equal(xs[0], xs[1])
    plan.refill_dev(A, v, True, stream)  # values + values: exact
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(A.get_values()), (d_val + d_val).cpu())


def test_dropin_header_assembly(tmp_path):
    """tests/cpp/assembly_case.cpp: SMM::AssemblyPlan + CSRMatrix::init(plan, values) / assemble against a TripletMatrix-built twin"""
    lib = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
    exe = tmp_path / "assembly_case"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "assembly_case.cpp"), f"-L{lib}", "-lsmm_hip", f"-Wl,-rpath,{lib}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1] == "OK", r.stdout[-2000:]
