"""The two dense kernels of GMRES's Gram-Schmidt (csrc/smm_solvers_gmres.hip) through the device-pointer ABI: smm_hip_multi_dot_dev_*
against NumPy in float64 within n * eps * sum |v_i w| (the bound of tests/test_gpu_spmv.py), smm_hip_multi_axpy_dev_* bit for bit against
the sequential NumPy nest in the matrix dtype (default a*x+b flavour), both on aligned arrays, on a padded leading dimension whose
padding is NaN, and on views at odd element alignment between guard bands."""
import ctypes

import numpy as np
import pytest
import torch
from device_views import address, assert_guards_intact, assert_unchanged, carve, carve_like, fit, snapshot

from sparse_matrix_math_amd import _lib, host

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
INVALID = -1  # SMM_HIP_ERR_INVALID
DEV = "cuda:0"
SMALL = [(n, k) for n in (1, 63, 257, 4099) for k in (1, 2, 8, 9, 31, 65)]
# A lane of the 16-byte path holds two packs per trip, so one trip of 2048 workgroups covers 2048 * 2048 elements in fp32 and half that
# in fp64.  With the leading dimension rounded up to 64 ("padded64", the layout of the solver's basis) the 16-byte path runs, and
#   2048 * 256 + 3     fits the grid in one trip;
#   2048 * 2048 + 3    is exactly one trip in fp32 (plus the odd tail) and two trips and one pack in fp64;
#   2048 * 2048 + 4099 takes a second trip in fp32 as well (two full workgroups, then the tail).
# With ld = n ("tight") every n here is odd, so the columns are only element-aligned and both kernels take one element per lane: that
# path strides over the grid from 2048 * 256 elements.
LARGE = [(2048 * 256 + 3, 1), (2048 * 256 + 3, 9), (2048 * 2048 + 3, 2), (2048 * 2048 + 4099, 2)]
LAYOUTS = ["tight", "padded64"]
_DATA = {}


def data(n, k, dtype):
    """(V as k rows of n -- column i of the basis is V[i] --, w, coefficients), made once per shape"""
    key = (n, k, np.dtype(dtype).name)
    if key not in _DATA:
        rng = np.random.default_rng(n * 131 + k)
        _DATA[key] = (rng.uniform(-1, 1, (k, n)).astype(dtype), rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, k).astype(dtype))
    return _DATA[key]


def dot_reference(V, w):
    V64, w64 = V.astype(np.float64), w.astype(np.float64)
    return V64 @ w64, np.abs(V64 * w64).sum(axis=1)


def axpy_reference(V, coef, w):
    """the sequential nest: acc = w; acc = c_i * v_i + acc for i ascending, every operation rounded once in the matrix dtype"""
    acc = w.copy()
    for i in range(len(coef)):
        t = coef[i] * V[i]
        acc = t + acc
    return acc


def padded(V, ld, fill):
    k, n = V.shape
    out = np.full((k, ld), fill, dtype=V.dtype)
    out[:, :n] = V
    return out


def basis(V, layout):
    """(the device copy of V, its leading dimension): "tight" is ld = n; "padded64" rounds ld up to 64 elements, as the solver's basis
    does, and fills what lies between n and ld with NaN"""
    n = V.shape[1]
    if layout == "tight":
        return torch.from_numpy(V).to(DEV), n
    ld = (n + 63) // 64 * 64
    d_V = torch.from_numpy(padded(V, ld, np.nan)).to(DEV)
    assert d_V.data_ptr() % 16 == 0
    return d_V, ld


def check_dot(out, V, w, dtype):
    exact, mag = dot_reference(V, w)
    n = V.shape[1]
    err = np.abs(out.astype(np.float64) - exact)
    bound = n * np.finfo(dtype).eps * mag + np.finfo(dtype).tiny
    print("multi_dot", V.shape, np.dtype(dtype).name, "worst error / bound", float(np.max(err / bound)))
    assert np.all(err <= bound), (V.shape, err, bound)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k", SMALL + LARGE)
def test_multi_dot(smm, n, k, dtype, layout):
    V, w, _ = data(n, k, dtype)
    d_V, ld = basis(V, layout)
    d_w = torch.from_numpy(w).to(DEV)
    d_out = torch.full((k,), float("nan"), dtype=d_w.dtype, device=DEV)
    host.multi_dot_dev(n, k, d_V, ld, d_w, d_out, dtype)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    check_dot(out, V, w, dtype)
    host.multi_dot_dev(n, k, d_V, ld, d_w, d_out, dtype)  # the same bits again: fixed order, no atomics
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint8), out.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k,ld", [(257, 9, 320), (4099, 31, 4160), (63, 2, 67)])
def test_multi_dot_padding_is_never_read_into_a_result(smm, n, k, ld, dtype):
    """ld > n with NaN between the columns (ld = 67 also breaks the columns' 16-byte alignment)"""
    V, w, _ = data(n, k, dtype)
    d_V = torch.from_numpy(padded(V, ld, np.nan)).to(DEV)
    d_w = torch.from_numpy(w).to(DEV)
    d_out = torch.zeros(k, dtype=d_w.dtype, device=DEV)
    host.multi_dot_dev(n, k, d_V, ld, d_w, d_out, dtype)
    torch.cuda.synchronize()
    check_dot(d_out.cpu().numpy(), V, w, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k", [(4099, 9), (2048 * 256 + 3, 2)])
def test_multi_dot_on_offset_views(smm, n, k, dtype):
    """V, w and the result carved at odd element alignment, guard bands around each"""
    V, w, _ = data(n, k, dtype)
    d_V = carve_like(V, fit(1, dtype), device=DEV)
    d_w = carve_like(w, fit(3, dtype), device=DEV)
    d_out = carve(k, dtype, fit(1, dtype), device=DEV)
    assert address(d_V) % 16 != 0 and address(d_w) % 16 != 0
    saved = snapshot(d_V), snapshot(d_w)
    host.multi_dot_dev(n, k, d_V, n, d_w, d_out, dtype)
    torch.cuda.synchronize()
    check_dot(d_out.cpu().numpy(), V, w, dtype)
    assert_unchanged(d_V, saved[0], "V")
    assert_unchanged(d_w, saved[1], "w")
    for t, name in ((d_V, "V"), (d_w, "w"), (d_out, "out")):
        assert_guards_intact(t, name)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k", SMALL + LARGE)
def test_multi_axpy_bit_identical(smm, n, k, dtype, layout):
    if smm.uses_std_fma():
        pytest.fail("this test states the default a*x+b flavour; the loaded library is the fma flavour")
    V, w, coef = data(n, k, dtype)
    ref = axpy_reference(V, coef, w)
    d_V, ld = basis(V, layout)
    before = d_V.clone()
    d_c = torch.from_numpy(coef).to(DEV)
    # out of place
    d_w = torch.from_numpy(w).to(DEV)
    d_out = torch.full((n,), float("nan"), dtype=d_w.dtype, device=DEV)
    host.multi_axpy_dev(n, k, d_V, ld, d_c, d_w, d_out, dtype)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    np.testing.assert_array_equal(d_w.cpu().numpy().view(np.uint8), w.view(np.uint8))
    # in place
    host.multi_axpy_dev(n, k, d_V, ld, d_c, d_w, d_w, dtype)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_w.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    assert torch.equal(d_V.view(torch.uint8), before.view(torch.uint8))
    np.testing.assert_array_equal(d_c.cpu().numpy().view(np.uint8), coef.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k,ld", [(257, 9, 320), (4099, 31, 4160), (63, 2, 67)])
def test_multi_axpy_padding(smm, n, k, ld, dtype):
    V, w, coef = data(n, k, dtype)
    ref = axpy_reference(V, coef, w)
    d_V = torch.from_numpy(padded(V, ld, np.nan)).to(DEV)
    d_c, d_w = torch.from_numpy(coef).to(DEV), torch.from_numpy(w).to(DEV)
    before = d_V.clone()
    host.multi_axpy_dev(n, k, d_V, ld, d_c, d_w, d_w, dtype)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_w.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    assert torch.equal(d_V.view(torch.uint8), before.view(torch.uint8))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("n,k", [(4099, 9), (2048 * 256 + 3, 2)])
def test_multi_axpy_on_offset_views(smm, n, k, dtype, inplace):
    V, w, coef = data(n, k, dtype)
    ref = axpy_reference(V, coef, w)
    d_V = carve_like(V, fit(3, dtype), device=DEV)
    d_w = carve_like(w, fit(1, dtype), device=DEV)
    d_c = carve_like(coef, fit(1, dtype), device=DEV)
    d_out = d_w if inplace else carve(n, dtype, fit(3, dtype), device=DEV)
    saved = snapshot(d_V), snapshot(d_c), snapshot(d_w)
    host.multi_axpy_dev(n, k, d_V, n, d_c, d_w, d_out, dtype)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    assert_unchanged(d_V, saved[0], "V")
    assert_unchanged(d_c, saved[1], "coef")
    if not inplace:
        assert_unchanged(d_w, saved[2], "w")
    for t, name in ((d_V, "V"), (d_w, "w"), (d_c, "coef"), (d_out, "out")):
        assert_guards_intact(t, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_bad_arguments(smm, dtype):
    lib = _lib.load()
    suf = "f32" if dtype == np.float32 else "f64"
    dot, axpy = getattr(lib, f"smm_hip_multi_dot_dev_{suf}"), getattr(lib, f"smm_hip_multi_axpy_dev_{suf}")
    n = 100
    V, w, coef = data(n, 66, dtype)
    d_V, d_w, d_c = (torch.from_numpy(a).to(DEV) for a in (V, w, coef))
    d_out = torch.zeros(66, dtype=d_w.dtype, device=DEV)
    d_o = torch.full((n,), 7.0, dtype=d_w.dtype, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for k in (0, 66, -1):
        assert dot(n, k, p(d_V), n, p(d_w), p(d_out), None) == INVALID
        assert axpy(n, k, p(d_V), n, p(d_c), p(d_w), p(d_o), None) == INVALID
    assert dot(n, 2, None, n, p(d_w), p(d_out), None) == INVALID
    assert dot(n, 2, p(d_V), n, None, p(d_out), None) == INVALID
    assert dot(n, 2, p(d_V), n, p(d_w), None, None) == INVALID
    assert axpy(n, 2, None, n, p(d_c), p(d_w), p(d_o), None) == INVALID
    assert axpy(n, 2, p(d_V), n, None, p(d_w), p(d_o), None) == INVALID
    assert axpy(n, 2, p(d_V), n, p(d_c), None, p(d_o), None) == INVALID
    assert axpy(n, 2, p(d_V), n, p(d_c), p(d_w), None, None) == INVALID
    assert dot(-1, 2, p(d_V), n, p(d_w), p(d_out), None) == INVALID
    assert dot(n, 2, p(d_V), n - 1, p(d_w), p(d_out), None) == INVALID  # ld < n
    torch.cuda.synchronize()
    assert float(d_out.abs().max()) == 0 and float((d_o - 7).abs().max()) == 0  # nothing was written
    # n == 0: every product is an empty sum
    assert dot(0, 3, None, 0, None, p(d_out), None) == 0
    assert axpy(0, 3, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert float(d_out[:3].abs().max()) == 0
