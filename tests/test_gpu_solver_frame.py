"""The host frame the Krylov drivers share (csrc/smm_solver_host.h), through the C ABI on poisson2d_32 (1024 rows) in both dtypes: what
every solver entry point does with bad arguments, and with a device allocation that is refused before or inside its device loop
(smm_hip_debug_fail_next_alloc: a host-side refusal, nothing faults).  Both tests pin behaviour the solvers had before they shared a
frame."""
import ctypes

import numpy as np
import pytest
import torch
from test_oracle import gen_matrices

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
OK, INVALID, NOMEM = _lib.SMM_HIP_OK, _lib.SMM_HIP_ERR_INVALID, _lib.SMM_HIP_ERR_NOMEM
K = 2  # columns of the batched solvers' blocks
PASSES = 10  # eps = 0: every solve makes exactly this many passes
NPART = 2048  # partial-sum slots (csrc/smm_internal.h)

HOST = ["cg", "bicgstab", "bicgstab_functor", "bicgsymmetric", "cgs", "bicg", "gmres", "cg_batch", "bicgstab_batch"]
DEV = ["cg", "bicgstab", "cgs", "bicg", "gmres", "cg_batch", "bicgstab_batch"]
# no register-resident path: a refusal inside the device driver always reaches the caller
NO_RESIDENT = {"bicgsymmetric", "cgs", "bicg", "gmres", "cg_batch", "bicgstab_batch"}
ENTRIES = [(n, False) for n in HOST] + [(n, True) for n in DEV]
ENTRY_IDS = [n + ("_dev" if d else "") for n, d in ENTRIES]


def suffix(dtype):
    return "f32" if dtype == np.float32 else "f64"


def bits(x):
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


class Outputs:
    def __init__(self, dtype):
        ct = ctypes.c_float if dtype == np.float32 else ctypes.c_double
        self.status, self.iterations, self.res = (ctypes.c_int * K)(), (ctypes.c_int * K)(), (ct * K)()

    def key(self):
        return list(self.status), list(self.iterations)


def solve(lib, name, dev, dtype, a, b, x0, x, out, apply_fn=None):
    """one call of smm_hip_<name>[_dev]_<suffix>; a / b / x0 / x: what goes into those arguments (None: a null pointer)"""
    stream = [None] if dev else []
    tail = [out.status, out.iterations, out.res]
    args = {
        "cg": [a, b, x0, x, PASSES, 0.0, None] + stream + tail,
        "bicgstab": [a, b, x, PASSES, 0.0, None] + stream + tail,
        "bicgstab_functor": [a, b, x, PASSES, 0.0, apply_fn, None] + tail,
        "bicgsymmetric": [a, b, x, PASSES, 0.0] + tail[:2],
        "cgs": [a, b, x, PASSES, 0.0] + stream + tail,
        "bicg": [a, None, b, x, PASSES, 0.0] + stream + tail,
        "gmres": [a, b, x, PASSES, 0.0, 30, None] + stream + tail,
        "cg_batch": [a, K, b, x0, x, PASSES, 0.0] + stream + tail,
        "bicgstab_batch": [a, K, b, x, PASSES, 0.0, None] + stream + tail,
    }[name]
    return getattr(lib, f"smm_hip_{name}{'_dev' if dev else ''}_{suffix(dtype)}")(*args)


def identity_apply(lib, dtype, rows):
    """M = I as the caller's host functor of smm_hip_bicgstab_functor_*"""
    nbytes = rows * np.dtype(dtype).itemsize

    def apply(user, rhs, x):
        ctypes.memmove(x, rhs, nbytes)
        return 0

    return getattr(lib, f"smm_hip_bicgstab_functor_{suffix(dtype)}").apply_type(apply)


def vectors(name, dtype, b1):
    """b, x0, x of one solve: n elements, or interleaved n x K blocks for the batched solvers (column 1 = half of column 0)"""
    if name.endswith("_batch"):
        b = np.ascontiguousarray(np.stack([b1, 0.5 * b1], axis=1).astype(dtype)).reshape(-1)
    else:
        b = b1.copy()
    return b, np.zeros_like(b), np.zeros_like(b)


def hptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def case(smm):
    made = {}
    for dtype in DTYPES:
        csr = gen_matrices(dtype)["poisson2d_32"]
        rows = len(csr[0]) - 1
        wide = smm.CSRMatrix(2, 3, np.array([0, 1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.ones(2, dtype=dtype))
        made[np.dtype(dtype).name] = (smm.CSRMatrix(rows, rows, *csr), wide, gen.row_sums(csr[0], csr[2]))
    return made


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name,dev", ENTRIES, ids=ENTRY_IDS)
def test_bad_arguments(smm, case, name, dev, dtype):
    """a null matrix, a matrix of the other dtype, a 2 x 3 matrix, a null b, a null x: SMM_HIP_ERR_INVALID, the caller's x untouched,
    the message names the solver (the functor form reports as bicgstab, whose loop it runs)"""
    lib = _lib.load()
    A, wide, b1 = case[np.dtype(dtype).name]
    other = case["float64" if dtype == np.float32 else "float32"][0]
    apply_fn = identity_apply(lib, dtype, len(b1))
    b, x0, x = vectors(name, dtype, b1)
    x[:] = 0.25
    if dev:
        keep = (torch.from_numpy(b).cuda(), torch.from_numpy(x0).cuda(), torch.from_numpy(x).cuda())
        pb, px0, px = (t.data_ptr() for t in keep)
        read_x = lambda: keep[2].cpu().numpy()  # noqa: E731
    else:
        pb, px0, px = hptr(b), hptr(x0), hptr(x)
        read_x = lambda: x  # noqa: E731
    before = bits(x).copy()
    prefix = ("bicgstab" if name == "bicgstab_functor" else name) + ":"
    bad = {"null matrix": (None, pb, px0, px), "other dtype": (other._h, pb, px0, px), "2 x 3": (wide._h, pb, px0, px),
           "null b": (A._h, None, px0, px), "null x": (A._h, pb, px0, None)}
    for what, (a, cb, cx0, cx) in bad.items():
        rc = solve(lib, name, dev, dtype, a, cb, cx0, cx, Outputs(dtype), apply_fn)
        message = lib.smm_hip_last_error().decode()
        assert rc == INVALID, (what, rc, message)
        assert message.startswith(prefix), (what, message)
        np.testing.assert_array_equal(bits(read_x()), before, err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("name", HOST)
def test_refused_allocation(smm, case, name, dtype):
    """(a) the wrapper's first staging buffer is refused: SMM_HIP_ERR_NOMEM, x untouched.  (b) the refusal lands on the partial-sum
    buffers (2 * NPART elements: more than any vector or block of this case), inside the device driver with the copies in already
    queued: SMM_HIP_ERR_NOMEM and x untouched, or -- where a register-resident path served the solve and never asked -- the clean
    solve's bits.  After either, a clean solve gives the bits, counts and status of the solve made before any injection."""
    lib = _lib.load()
    A, _, b1 = case[np.dtype(dtype).name]
    rows, itemsize = len(b1), np.dtype(dtype).itemsize
    apply_fn = identity_apply(lib, dtype, rows)

    def run():
        b, x0, x = vectors(name, dtype, b1)
        x[:] = 0.25
        x0[:] = 0.25
        out = Outputs(dtype)
        rc = solve(lib, name, False, dtype, A._h, hptr(b), hptr(x0), hptr(x), out, apply_fn)
        return rc, x, out.key()

    rc, x_clean, key_clean = run()
    assert rc == OK, lib.smm_hip_last_error()
    assert all(k == PASSES for k in key_clean[1][:K if name.endswith("_batch") else 1]), key_clean
    untouched = np.full_like(x_clean, 0.25)
    for what, threshold in (("a", rows * itemsize), ("b", 2 * NPART * itemsize)):
        try:
            _lib.check(lib.smm_hip_debug_fail_next_alloc(threshold))
            rc, x, key = run()
        finally:
            _lib.check(lib.smm_hip_debug_fail_next_alloc(0))
        print(name, np.dtype(dtype).name, "case", what, "->", rc)
        if what == "a" or name in NO_RESIDENT:
            assert rc == NOMEM, (what, rc, lib.smm_hip_last_error())
        if rc == NOMEM:
            np.testing.assert_array_equal(bits(x), bits(untouched), err_msg=what)
        else:
            assert rc == OK and key == key_clean, (what, rc, key, key_clean)
            np.testing.assert_array_equal(bits(x), bits(x_clean), err_msg=what)
        rc, x, key = run()
        assert rc == OK and key == key_clean, (what, rc, key, key_clean)
        np.testing.assert_array_equal(bits(x), bits(x_clean), err_msg="clean solve after case " + what)
