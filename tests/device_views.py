"""Offset views with guard bands for the tests of the device-pointer ABI.

carve() hands out an array that sits INSIDE a larger torch buffer, at a chosen distance from a 16-byte boundary, with a band of known
content on either side.  A kernel that needs more alignment than the element's own reads or writes the wrong place; a kernel that runs
past either end of an array changes a band, and assert_guards_intact() names the first changed element relative to the array.  Works on
CPU tensors too (tests/test_device_views_cpu.py)."""
import numpy as np
import torch

GUARD = 1024
SPARE = 4  # elements of slack so that every residue can be reached
_INT_OF_SIZE = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
             np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def torch_dtype(dtype):
    return dtype if isinstance(dtype, torch.dtype) else _TORCH_OF[np.dtype(dtype)]


def residues(dtype):
    """the residues a type of at least 4 bytes can take: 0..3 for 4-byte elements, 0..1 for 8-byte ones"""
    return tuple(range(16 // torch.empty(0, dtype=torch_dtype(dtype)).element_size()))


def fit(residue, dtype):
    """a residue stated for 4-byte elements, folded into the range of `dtype` (3 -> 1 for 8-byte elements)"""
    return residue % len(residues(dtype))


def _bits(t):
    """the same memory as integers: NaN payloads and signed zeros compare bit for bit"""
    return t.view(_INT_OF_SIZE[t.element_size()])


def carve(n, dtype, residue, guard=GUARD, fill=None, device="cpu"):
    """A view of n elements of one buffer of n + 2 * guard + 4 elements with view.data_ptr() % 16 == residue * itemsize.  The whole
    buffer -- the view as well -- starts out as `fill`: NaN for floating types and 0 for integers when not given (callers pass a valid
    column for positions[] and nnz for start[], so that a read past the end can never become an out-of-range gather)."""
    td = torch_dtype(dtype)
    if fill is None:
        fill = float("nan") if td.is_floating_point else 0
    buf = torch.full((n + 2 * guard + SPARE,), fill, dtype=td, device=device)
    size = buf.element_size()
    per16 = max(16 // size, 1)
    if not 0 <= residue < min(per16, SPARE):
        raise ValueError(f"residue {residue} is out of range for {td}")
    assert buf.data_ptr() % size == 0
    here = (buf.data_ptr() // size + guard) % per16
    begin = guard + (residue - here) % per16
    assert begin - guard < SPARE, "the allocation is not 16-byte aligned by more than the spare elements cover"
    view = buf[begin:begin + n]
    assert address_of(buf, begin) % 16 == residue * size and view.numel() == n
    assert n == 0 or view.data_ptr() == address_of(buf, begin)
    return _attach(view, buf, begin, n)


def address_of(buf, begin):
    return buf.data_ptr() + begin * buf.element_size()


def address(view):
    """the device (or host) address of a carved view's first element -- also for n == 0, where torch reports no address of its own"""
    return address_of(view._carved["buf"], view._carved["begin"])


def _attach(view, buf, begin, n):
    bits = _bits(buf)
    view._carved = {"buf": buf, "begin": begin, "n": n, "front": bits[:begin].clone(), "back": bits[begin + n:].clone()}
    return view


def carve_like(array, residue, guard=GUARD, fill=None, device="cpu"):
    """carve() filled with a numpy array (any shape, C order): the returned view has the array's shape"""
    array = np.ascontiguousarray(array)
    flat = carve(array.size, array.dtype, residue, guard, fill, device)
    flat.copy_(torch.from_numpy(array.reshape(-1)))
    if array.ndim == 1:
        return flat
    meta = flat._carved
    shaped = flat.view(array.shape)
    shaped._carved = meta
    return shaped


def snapshot(view):
    """the present bits of an array, for assert_unchanged"""
    return _bits(view.reshape(-1)).clone()


def _first_difference(now, saved):
    diff = torch.nonzero(now != saved)
    return int(diff[0]) if diff.numel() else -1


def assert_unchanged(view, saved, name="array"):
    """an input still holds the bits of its snapshot()"""
    at = _first_difference(_bits(view.reshape(-1)), saved)
    assert at < 0, f"{name}: element {at} changed"


def assert_guards_intact(view, name="array"):
    """both guard bands of a carved view hold their first bits; the failure names the first changed element as an offset from the
    array's first element (negative: before it; >= n: after its end)"""
    meta = view._carved
    bits = _bits(meta["buf"])
    begin, n = meta["begin"], meta["n"]
    at = _first_difference(bits[:begin], meta["front"])
    assert at < 0, f"{name}: guard changed at offset {at - begin} relative to the array (before its first element)"
    at = _first_difference(bits[begin + n:], meta["back"])
    assert at < 0, f"{name}: guard changed at offset {n + at} relative to the array of {n} elements (past its end)"
