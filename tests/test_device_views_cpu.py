"""tests/device_views.py on CPU tensors: every residue is reached, a write just outside the array is reported with its place, an untouched
buffer passes."""
import numpy as np
import pytest
import torch
from device_views import GUARD, address, assert_guards_intact, assert_unchanged, carve, carve_like, fit, residues, snapshot

TYPES = [np.int32, np.float32, np.float64]


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", [0, 1, 5, 1023])
def test_every_residue_is_reached(dtype, n):
    size = np.dtype(dtype).itemsize
    assert residues(dtype) == tuple(range(16 // size))
    for r in residues(dtype):
        v = carve(n, dtype, r)
        assert v.numel() == n and address(v) % 16 == r * size and (n == 0 or v.data_ptr() == address(v))
        meta = v._carved
        assert meta["buf"].numel() == n + 2 * GUARD + 4
        assert GUARD <= meta["begin"] < GUARD + 4 and meta["buf"].numel() - meta["begin"] - n >= GUARD
        assert_guards_intact(v)
    with pytest.raises(ValueError):
        carve(n, dtype, 16 // size)
    assert fit(3, dtype) == 3 % (16 // size) and fit(2, dtype) == 2 % (16 // size)


@pytest.mark.parametrize("dtype", TYPES)
def test_guard_fill(dtype):
    v = carve(7, dtype, 1)
    buf = v._carved["buf"]
    if np.dtype(dtype).kind == "f":
        assert bool(torch.isnan(buf).all())  # a read past either end shows as NaN in a result
    else:
        assert not buf.any()
        w = carve(7, dtype, 1, fill=41)  # a valid column / nnz: a read past the end stays a harmless index
        assert bool((w._carved["buf"] == 41).all())
    v.fill_(3)
    assert_guards_intact(v)  # writing the array itself is no violation


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("where", ["before", "after", "last"])
def test_a_planted_write_is_reported(dtype, where):
    n = 37
    for r in residues(dtype):
        v = carve(n, dtype, r)
        buf, begin = v._carved["buf"], v._carved["begin"]
        index, offset = {"before": (begin - 1, -1), "after": (begin + n, n), "last": (buf.numel() - 1, buf.numel() - 1 - begin)}[where]
        buf[index] = 5
        with pytest.raises(AssertionError, match=rf"offset {offset} relative"):
            assert_guards_intact(v)


def test_a_changed_nan_payload_is_reported():
    """byte for byte: another NaN in a NaN guard is a write"""
    v = carve(4, np.float32, 2)
    bits = v._carved["buf"].view(torch.int32)
    bits[v._carved["begin"] + 4] ^= 1
    assert bool(torch.isnan(v._carved["buf"]).all())
    with pytest.raises(AssertionError, match="offset 4 relative"):
        assert_guards_intact(v)


@pytest.mark.parametrize("dtype", TYPES)
def test_carve_like_and_assert_unchanged(dtype):
    a = (np.arange(24) - 5).astype(dtype).reshape(8, 3)
    v = carve_like(a, 1)
    assert tuple(v.shape) == (8, 3) and v.data_ptr() % 16 == np.dtype(dtype).itemsize
    np.testing.assert_array_equal(v.numpy(), a)
    saved = snapshot(v)
    assert_unchanged(v, saved)
    assert_guards_intact(v)
    v[2, 1] = 99
    with pytest.raises(AssertionError, match="element 7 changed"):
        assert_unchanged(v, saved, "a")
    assert_guards_intact(v)
