"""Editing a matrix's values on the device (smm_hip_csr_scale / axpy / zero / update_entries / set_values / values_changed,
csrc/smm_csr_update.hip).  After every edit the handle must multiply and solve exactly like a FRESH handle made from the edited arrays
(forced to the same kernel family and lanes), and at one lane like the reference's row loop (the oracle); the value-dependent state
(constant-diagonal encoding, the single-launch BiCGStab's slot-major values) must follow the edit and nothing pattern-shaped may change."""
import os
import subprocess

import numpy as np
import pytest

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
VECTOR, STREAM, PATTERN = 1, 2, 3
NONE, MASKS, CODES, CONST = 0, 1, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_matrices(dtype):
    return {
        "poisson2d": gen.poisson2d(150, 130, dtype=dtype),  # CONST
        "convdiff3d": gen.convdiff3d_varying(18, dtype=dtype),  # MASKS (diagonals vary)
        "banded": gen.banded_random_spd(20_000, 5, 7, 100, dtype=dtype),  # masks, STREAM by default
        "dictionary": gen.banded_random_spd(6000, 32, 0x5EED, 2500, dtype=dtype),  # 65 offsets: CODES
    }


ENCODINGS = {"poisson2d": CONST, "convdiff3d": MASKS, "banded": MASKS, "dictionary": CODES}
CONFIGS = [(STREAM, 1), (STREAM, 4), (VECTOR, 2), (PATTERN, 1), (PATTERN, 2)]


def entry_index(csr, r, c):
    start, pos, _ = csr
    if r < 0 or r >= len(start) - 1 or c < 0:
        return -1
    lo, hi = start[r], start[r + 1]
    k = lo + np.searchsorted(pos[lo:hi], c)
    return int(k) if k < hi and pos[k] == c else -1


def apply_entries(csr, rows, cols, vals, add):
    """the reference's updateEntry / addEntry one after another"""
    v = csr[2].copy()
    found = np.zeros(len(rows), dtype=bool)
    for i, (r, c, x) in enumerate(zip(rows, cols, vals)):
        k = entry_index(csr, int(r), int(c))
        if k >= 0:
            v[k] = v[k] + x if add else x
            found[i] = True
    return v


def batch(csr, rng, dtype, n=300):
    """entries that are stored, repeated ones, missing ones and out-of-range ones"""
    start, pos, _ = csr
    rows = len(start) - 1
    rr = rng.integers(0, rows, n)
    ks = np.array([rng.integers(start[r], start[r + 1]) if start[r + 1] > start[r] else -1 for r in rr])
    cc = np.where(ks >= 0, pos[np.maximum(ks, 0)], 0).astype(np.int64)
    cc[::7] = rng.integers(0, rows, len(cc[::7]))  # mostly not stored
    rr = np.concatenate([rr, rr[:40], [-1, rows, 0, 3], rr[:5]])
    cc = np.concatenate([cc, cc[:40], [0, 0, -2, rows + 5], cc[:5]])
    vals = rng.uniform(-2, 2, len(rr)).astype(dtype)
    return rr.astype(np.int32), cc.astype(np.int32), vals


def edited_values(name, csr, rng, dtype):
    """(edit name, function(A, B) applying it to handle A, the numpy values after it)"""
    v = csr[2]
    other = (v * dtype(0.3)).astype(dtype) if name == "poisson2d" else rng.uniform(-1, 1, v.size).astype(dtype)
    rr, cc, bv = batch(csr, rng, dtype)
    newv = rng.uniform(-1, 1, v.size).astype(dtype)
    return other, [
        ("scale", lambda A, B: A.__imul__(1.7), v * dtype(1.7)),
        ("axpy+1", lambda A, B: A.inplaceAdd(B), v + other),
        ("axpy-1", lambda A, B: A.inplaceSubtract(B), v - other),
        ("axpy0.25", lambda A, B: A.axpy(0.25, B), v + dtype(0.25) * other),
        ("zero", lambda A, B: A.zeroValues(), np.zeros_like(v)),
        ("set-entries", lambda A, B: A.update_entries(rr, cc, bv), apply_entries(csr, rr, cc, bv, False)),
        ("add-entries", lambda A, B: A.update_entries(rr, cc, bv, add=True), apply_entries(csr, rr, cc, bv, True)),
        ("set-values", lambda A, B: A.set_values(newv), newv),
    ]


def spmv(A, x, dtype):
    y = np.empty(A.rows, dtype=dtype)
    A.rMult(x, y)
    return y


def try_kernel(A, fam, lanes):
    try:
        A.set_kernel(fam, lanes)
        return True
    except _lib.SmmHipError:
        return False


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_edit_equals_a_fresh_handle(smm, oracle, dtype):
    rng = np.random.default_rng(11)
    for name, csr in small_matrices(dtype).items():
        n = len(csr[0]) - 1
        x = rng.uniform(-1, 1, n).astype(dtype)
        other, edits = edited_values(name, csr, rng, dtype)
        B = smm.CSRMatrix(n, n, csr[0], csr[1], other)
        for edit, fn, want in edits:
            A = smm.CSRMatrix(n, n, *csr)
            pattern_ok = try_kernel(A, PATTERN, 1)  # analysed before the edit (CONST where it applies)
            assert pattern_ok and A.pattern_info()[0] == ENCODINGS[name], (name, A.pattern_info())
            A.set_kernel(0, 0)
            spmv(A, x, dtype)  # the first SpMV
            tiles = A.tile_info()
            enc_before = A.pattern_info()
            fn(A, B)
            np.testing.assert_array_equal(A.get_values(), want, err_msg=f"{name} {edit}")
            assert A.tile_info() == tiles
            enc = A.pattern_info()
            assert enc[1] == enc_before[1] and (enc[0] == enc_before[0] or (enc_before[0] == CONST and enc[0] == MASKS)), (name, edit, enc_before, enc)
            ecsr = (csr[0], csr[1], want)
            F = smm.CSRMatrix(n, n, *ecsr)
            for fam, lanes in CONFIGS:
                if fam == PATTERN and not pattern_ok:
                    continue
                assert try_kernel(A, fam, lanes) and try_kernel(F, fam, lanes), (name, edit, fam, lanes)
                got = spmv(A, x, dtype)
                np.testing.assert_array_equal(got, spmv(F, x, dtype), err_msg=f"{name} {edit} {fam}/{lanes}")
                if lanes == 1:
                    np.testing.assert_array_equal(got, oracle.spmv(ecsr, 0, None, x), err_msg=f"{name} {edit} {fam}/1 oracle")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_values_changed_on_device_arrays(smm, oracle, dtype):
    import torch

    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    for name, csr in small_matrices(dtype).items():
        n = len(csr[0]) - 1
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in csr]
        A = smm.CSRMatrix.from_device(n, n, d[0], d[1], d[2], dtype)
        pattern_ok = try_kernel(A, PATTERN, 1)
        x = rng.uniform(-1, 1, n).astype(dtype)
        spmv(A, x, dtype)
        newv = csr[2].copy()
        newv[::3] *= dtype(-2)
        stream = torch.cuda.current_stream().cuda_stream
        d[2].copy_(torch.from_numpy(newv).to(dev))
        A.values_changed(stream)
        ecsr = (csr[0], csr[1], newv)
        F = smm.CSRMatrix(n, n, *ecsr)
        for fam, lanes in [(STREAM, 1), (PATTERN, 1)] if pattern_ok else [(STREAM, 1)]:
            assert try_kernel(A, fam, lanes) and try_kernel(F, fam, lanes)
            got = spmv(A, x, dtype)
            np.testing.assert_array_equal(got, spmv(F, x, dtype), err_msg=name)
            np.testing.assert_array_equal(got, oracle.spmv(ecsr, 0, None, x), err_msg=name)
        # the edit calls write the caller's array
        A.scale(2.0)
        np.testing.assert_array_equal(d[2].cpu().numpy(), newv * dtype(2))


@pytest.fixture
def march_rows(smm):
    smm.host.set_march_min_rows(1 << 21, 1 << 21)
    yield
    smm.host.set_march_min_rows(-1, -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["march7", "march27"])
def test_march_kernels_after_edits(smm, oracle, march_rows, dtype, kind):
    """grid matrices served by the 2.5-D kernels: an exact CONST edit keeps the march kernel, an entry edit demotes to values read"""
    rng = np.random.default_rng(9)
    csr = gen.stencil3d(128, 128, 128, dtype=dtype) if kind == "march7" else gen.stencil3d_wide(128, 128, 128, 27, dtype=dtype)
    n = len(csr[0]) - 1
    x = rng.uniform(-1, 1, n).astype(dtype)
    A = smm.CSRMatrix(n, n, *csr)
    A.set_kernel(PATTERN, 1)
    assert A.pattern_info()[0] == CONST
    kernel = A.kernel_desc()[0]
    assert kernel == ("spmvPatternConstMarchKernel" if kind == "march7" else "spmvPatternConstMarch3Kernel")
    spmv(A, x, dtype)
    A *= 0.5
    v = csr[2] * dtype(0.5)
    assert A.pattern_info()[0] == CONST and A.kernel_desc()[0] == kernel
    np.testing.assert_array_equal(spmv(A, x, dtype), oracle.spmv((csr[0], csr[1], v), 0, None, x))
    rr, cc, bv = np.array([n // 2, 7], dtype=np.int32), np.array([n // 2, 7], dtype=np.int32), np.array([9.5, -3], dtype=dtype)
    found = A.update_entries(rr, cc, bv)
    assert found.all()
    v = apply_entries((csr[0], csr[1], v), rr, cc, bv, False)
    assert A.pattern_info()[0] == MASKS
    ecsr = (csr[0], csr[1], v)
    got = spmv(A, x, dtype)
    np.testing.assert_array_equal(got, oracle.spmv(ecsr, 0, None, x))
    F = smm.CSRMatrix(n, n, *ecsr)
    F.set_kernel(PATTERN, 1)
    np.testing.assert_array_equal(got, spmv(F, x, dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_encoding_after_edits(smm, dtype):
    csr = gen.poisson2d(120, dtype=dtype)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    B = smm.CSRMatrix(n, n, csr[0], csr[1], csr[2] * dtype(3))
    A.set_kernel(PATTERN, 1)
    B.set_kernel(PATTERN, 1)
    assert A.pattern_info() == (CONST, 5)
    tiles = A.tile_info()
    A *= -2.5
    assert A.pattern_info() == (CONST, 5)
    A.inplaceAdd(B)
    assert A.pattern_info() == (CONST, 5)
    A.zeroValues()
    assert A.pattern_info() == (CONST, 5)
    A.set_values(csr[2])  # constant again: re-verified, stays
    assert A.pattern_info() == (CONST, 5)
    assert A.updateEntry(60, 61, 0.125)  # one diagonal broken at one row
    assert A.pattern_info() == (MASKS, 5)
    assert A.tile_info() == tiles
    assert not A.updateEntry(0, 50, 1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_solvers_after_edits(smm, dtype):
    rng = np.random.default_rng(4)
    cases = {"poisson2d": gen.poisson2d(96, dtype=dtype), "convdiff3d": gen.convdiff3d_varying(24, dtype=dtype)}
    previous = smm.host.bicgstab_resident(-1)
    try:
        for name, csr in cases.items():
            n = len(csr[0]) - 1
            b = rng.uniform(-1, 1, n).astype(dtype)
            diag = np.array([entry_index(csr, i, i) for i in range(n)])
            rr = np.arange(0, n, 17, dtype=np.int32)
            bv = (csr[2][diag[rr]] * dtype(1.5)).astype(dtype)
            v = apply_entries(csr, rr, rr, bv, False) * dtype(0.75)
            ecsr = (csr[0], csr[1], v)

            def solve(A, which, resident):
                smm.host.bicgstab_resident(2 if resident else 0)
                x = np.zeros(n, dtype=dtype)
                info = {}
                if which == "cg":
                    st = smm.ConjugateGradient(A, b, x, x, 60, 1e-30, info=info)
                else:
                    st = smm.BiCGStab(A, b, x, 40, 1e-30, info=info)
                return int(st), info["iterations"], x

            for which, resident in (("cg", False), ("bicgstab", False), ("bicgstab", True)):
                if which == "cg" and name != "poisson2d":
                    continue
                A = smm.CSRMatrix(n, n, *csr)
                A.set_kernel(PATTERN, 1)
                solve(A, which, resident)  # (the single-launch form builds its slot-major values here)
                A.update_entries(rr, rr, bv)
                A *= 0.75
                F = smm.CSRMatrix(n, n, *ecsr)
                F.set_kernel(PATTERN, 1)
                st, it, x = solve(A, which, resident)
                st2, it2, x2 = solve(F, which, resident)
                assert (st, it) == (st2, it2), (name, which, resident)
                np.testing.assert_array_equal(x, x2, err_msg=f"{name} {which} resident={resident}")
    finally:
        smm.host.bicgstab_resident(previous)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_preconditioners_after_edits(smm, dtype):
    rng = np.random.default_rng(8)
    P = smm.SolverPreconditioner
    csr = gen.poisson2d(80, dtype=dtype)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    A.set_kernel(PATTERN, 1)
    assert A.pattern_info()[0] == CONST
    sgs = A.getPreconditioner(P.SYMMETRIC_GAUS_SEIDEL)
    ilu = A.getPreconditioner(P.ILU0)
    blk = A.getPreconditioner(P.BLOCK_ILU0)
    ilu_vals, blk_vals = ilu.values(), blk.values()
    rr = np.arange(0, n, 5, dtype=np.int32)
    bv = np.full(rr.size, 5.5, dtype=dtype)
    A.update_entries(rr, rr, bv)  # diagonal no longer constant: CONST -> MASKS (the buffer the block one-launch form read stays valid)
    assert A.pattern_info()[0] == MASKS
    ecsr = (csr[0], csr[1], apply_entries(csr, rr, rr, bv, False))
    F = smm.CSRMatrix(n, n, *ecsr)
    r = rng.uniform(-1, 1, n).astype(dtype)
    x1, x2 = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    sgs.apply(r, x1)
    F.getPreconditioner(P.SYMMETRIC_GAUS_SEIDEL).apply(r, x2)
    np.testing.assert_array_equal(x1, x2)  # SGS follows A
    np.testing.assert_array_equal(ilu.values(), ilu_vals)  # snapshots
    np.testing.assert_array_equal(blk.values(), blk_vals)
    Av = spmv(F, r, dtype)
    y1, y2 = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    blk.apply_spmv(r, y1)  # M^-1 (A v) in one launch, A in its CURRENT encoding
    blk.apply(Av, y2)
    np.testing.assert_array_equal(y1, y2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_error_paths(smm, oracle, dtype):
    csr = gen.poisson2d(30, dtype=dtype)
    n = len(csr[0]) - 1
    A = smm.CSRMatrix(n, n, *csr)
    pos = csr[1].copy()
    assert pos[2] == 30
    pos[2] = 29  # same rows, cols, nnz and start[]: one column differs
    B = smm.CSRMatrix(n, n, csr[0], pos, csr[2])
    assert not A.hasSameNonZeroPattern(B) and A.hasSameNonZeroPattern(A)
    for _ in range(2):  # (the second time from the cached verdict)
        with pytest.raises(smm.SmmHipError) as e:
            A.inplaceAdd(B)
        assert e.value.code == _lib.SMM_HIP_ERR_INVALID
    np.testing.assert_array_equal(A.get_values(), csr[2])
    odt = np.float64 if dtype == np.float32 else np.float32
    C = smm.CSRMatrix(n, n, csr[0], csr[1], csr[2].astype(odt))
    with pytest.raises(smm.SmmHipError) as e:
        A.inplaceSubtract(C)
    assert e.value.code == _lib.SMM_HIP_ERR_INVALID
    np.testing.assert_array_equal(A.get_values(), csr[2])
    with pytest.raises(ValueError):
        A.set_values(csr[2][:-1])  # too short
    # empty matrix, and one with empty rows
    E = smm.CSRMatrix(4, 4, np.zeros(5, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype))
    E *= 3.0
    E.zeroValues()
    E.inplaceAdd(E)
    assert not E.updateEntry(0, 0, 1.0)
    E.set_values(np.zeros(0, dtype=dtype))
    assert E.get_values().size == 0
    rcsr = gen.random_rows(500, 500, 0, 6, seed=3, dtype=dtype, empty_every=4)
    R = smm.CSRMatrix(500, 500, *rcsr)
    rng = np.random.default_rng(2)
    rr, cc, bv = batch(rcsr, rng, dtype, 100)
    found = R.update_entries(rr, cc, bv, add=True)
    want = apply_entries(rcsr, rr, cc, bv, True)
    np.testing.assert_array_equal(R.get_values(), want)
    assert found.tolist() == [entry_index(rcsr, int(r), int(c)) >= 0 for r, c in zip(rr, cc)]
    x = rng.uniform(-1, 1, 500).astype(dtype)
    np.testing.assert_array_equal(spmv(R, x, dtype), oracle.spmv((rcsr[0], rcsr[1], want), 0, None, x))


def test_dropin_header_edits_through_the_device(tmp_path):
    """tests/cpp/mutators_case.cpp through the drop-in header WITH a device mirror: every edit after rMult goes through the GPU, the printout
    (host reads after device-side bulk edits included) must equal the host-only run, and the edited matrix multiplies like a fresh one"""
    lib = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
    exe = tmp_path / "mutators_dropin"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "mutators_case.cpp"), f"-L{lib}", "-lsmm_hip", f"-Wl,-rpath,{lib}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    outs = {}
    for mirror in ("0", "1"):
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, SMM_CASE_MIRROR=mirror))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[mirror] = r
    assert outs["1"].stdout == outs["0"].stdout
    fresh = [ln for ln in outs["1"].stderr.splitlines() if ln.startswith("fresh ")]
    assert len(fresh) == 8 and all(ln.endswith(" 1") for ln in fresh), outs["1"].stderr[-2000:]


def test_dropin_single_entry_edits_reach_a_preconditioner_made_before(tmp_path):
    """updateEntry / addEntry / setValue on a matrix with a device mirror are queued; an SGSPreconditioner made before them (it reads A at
    every apply) must see them at its next apply -- bit for bit an SGS made from a fresh matrix with the edited arrays"""
    lib = os.path.join(ROOT, "sparse_matrix_math_amd", "lib")
    exe = tmp_path / "precond_edit_case"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'include', 'smm_hip')}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "precond_edit_case.cpp"), f"-L{lib}", "-lsmm_hip", f"-Wl,-rpath,{lib}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    checks = [ln for ln in lines if ln.startswith("sgs ")]
    assert len(checks) == 10 and all(ln.endswith(" 1") for ln in checks), r.stdout
    assert lines[-1] == "status 0", r.stdout
