"""Host-side mirror of the reference's public API for the hot path, on top of the C ABI (include/smm_hip.h).

Names, argument order and error behaviour follow include/sparse_matrix_math.h of vasil-pashov/sparse_matrix_math:
CSRMatrix.rMult / rMultAdd / rMultSub (ref:1501-1515), getPreconditioner (ref:1643-1651), ConjugateGradient
(ref:2316-2398, IC0 overload ref:2414-2505), BiCGStab (ref:2191-2303), BiCGSymmetric (ref:2021-2102), ConjugateGradientSquared
(ref:2104-2178), SolverStatus
(ref:2010-2014), SolverPreconditioner (ref:1002-1006).  Vectors are numpy arrays in host memory, like the
reference's raw T* arguments; the `*_dev` helpers take device pointers (ints or objects with .data_ptr()) for
callers that keep their data in HBM (bench.py, the multi-GPU driver).

Everything here runs on the GPU through libsmm_hip.so.  There is no CPU implementation in this package.
"""
import collections
import ctypes
import enum

import numpy as np

from . import _lib
from ._lib import check


class SolverStatus(enum.IntEnum):  # ref:2010-2014
    SUCCESS = 0
    DIVERGED = 1
    MAX_ITERATIONS_REACHED = 2


class SolverPreconditioner(enum.IntEnum):
    """ref:1002-1006 has NONE, SYMMETRIC_GAUS_SEIDEL (sic) and ILU0; JACOBI, IC0 and the BLOCK_ forms (ILU0 / SGS of the
    block-diagonal part of A, one wavefront per block) are additions, and so is CHEBYSHEV (a polynomial in D^-1 A: SpMVs and
    element-wise passes only), AMG (smoothed-aggregation multigrid, a symmetric V-cycle) and the MULTICOLOR_ forms (SGS / ILU0 / IC0 of the
    matrix renumbered colour by colour: a handful of dependent levels per sweep) and FSAI / SPAI (approximate inverses that are sparse
    matrices themselves: an apply is one or two SpMVs) and the JSWEEP_ forms (the exact SGS / ILU0 / IC0 factor in the natural numbering,
    each triangular solve replaced by a fixed number of Jacobi steps: no dependent levels at all).  Values are the SMM_PRECOND_* codes of
    the C ABI."""
    NONE = 0
    JACOBI = 1
    ILU0 = 2
    SYMMETRIC_GAUS_SEIDEL = 3
    IC0 = 4
    BLOCK_ILU0 = 5
    BLOCK_SGS = 6
    CHEBYSHEV = 7
    AMG = 8
    MULTICOLOR_SGS = 9
    MULTICOLOR_ILU0 = 10
    MULTICOLOR_IC0 = 11
    FSAI = 12
    SPAI = 13
    JSWEEP_SGS = 14
    JSWEEP_ILU0 = 15
    JSWEEP_IC0 = 16


OP_ASSIGN, OP_ADD, OP_SUB = 0, 1, 2
MAX_RHS = 8  # SMM_HIP_MAX_RHS: the most right-hand sides one block holds
SPMV_AUTO, SPMV_VECTOR, SPMV_STREAM, SPMV_PATTERN, SPMV_BLOCKS, SPMV_LONGROWS = 0, 1, 2, 3, 4, 5
SWEEP_AUTO, SWEEP_LEVELS, SWEEP_SYNCFREE, SWEEP_SYNCFREE_XCD = 0, 1, 2, 3
CHEB_BOUND_GERSHGORIN, CHEB_BOUND_POWER, CHEB_BOUND_USER = 0, 1, 2  # SMM_CHEB_BOUND_*: where a Chebyshev preconditioner's bounds come from
_MULTICOLOR_BASE = {SolverPreconditioner.MULTICOLOR_SGS: SolverPreconditioner.SYMMETRIC_GAUS_SEIDEL, SolverPreconditioner.MULTICOLOR_ILU0: SolverPreconditioner.ILU0,
                    SolverPreconditioner.MULTICOLOR_IC0: SolverPreconditioner.IC0}
_JSWEEP_BASE = {SolverPreconditioner.JSWEEP_SGS: SolverPreconditioner.SYMMETRIC_GAUS_SEIDEL, SolverPreconditioner.JSWEEP_ILU0: SolverPreconditioner.ILU0,
                SolverPreconditioner.JSWEEP_IC0: SolverPreconditioner.IC0}
_AINV_KINDS = (SolverPreconditioner.FSAI, SolverPreconditioner.SPAI)
_CHEB_BOUNDS = {"GERSHGORIN": CHEB_BOUND_GERSHGORIN, "POWER": CHEB_BOUND_POWER, "USER": CHEB_BOUND_USER}

_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
_CT = {"f32": ctypes.c_float, "f64": ctypes.c_double}


def _suffix(dtype):
    try:
        return _SUFFIX[np.dtype(dtype)]
    except KeyError:
        raise TypeError(f"only float32 and float64 are supported (the reference's float/double), got {dtype}")


def _fn(base, suf):
    return getattr(_lib.load(), f"{base}_{suf}")


def _host(a, dtype, name, n=None, writable=False):
    if not isinstance(a, np.ndarray) or a.dtype != np.dtype(dtype) or not a.flags.c_contiguous:
        raise TypeError(f"{name} must be a C-contiguous numpy array of {np.dtype(dtype)}")
    if writable and not a.flags.writeable:
        raise TypeError(f"{name} must be writable")
    if n is not None and a.size < n:
        raise ValueError(f"{name} has {a.size} elements, needs {n}")
    return a.ctypes.data_as(ctypes.c_void_p)


def _dptr(t):
    """device pointer from an int, None, or anything with .data_ptr() (torch tensors)"""
    if t is None:
        return ctypes.c_void_p(0)
    if hasattr(t, "data_ptr"):
        return ctypes.c_void_p(t.data_ptr())
    return ctypes.c_void_p(int(t))


def _block(a, dtype, name, rows, k=None, writable=False):
    """an interleaved block of right-hand sides: a C-contiguous (rows, k) array of `dtype`, 1 <= k <= MAX_RHS (k given: exactly that
    many columns).  Checked here, before the library is touched.  Returns (pointer, k)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.dtype(dtype) or a.ndim != 2 or not a.flags.c_contiguous:
        raise TypeError(f"{name} must be a C-contiguous (n, k) numpy array of {np.dtype(dtype)}")
    if writable and not a.flags.writeable:
        raise TypeError(f"{name} must be writable")
    if not 1 <= a.shape[1] <= MAX_RHS:
        raise ValueError(f"{name} has {a.shape[1]} columns, a block holds 1 .. {MAX_RHS}")
    if k is not None and a.shape[1] != k:
        raise ValueError(f"{name} has {a.shape[1]} columns, the other blocks have {k}")
    if a.shape[0] != rows:
        raise ValueError(f"{name} has {a.shape[0]} rows, needs {rows}")
    return a.ctypes.data_as(ctypes.c_void_p), a.shape[1]


def init(device=0):
    check(_lib.load().smm_hip_init(int(device)))


def device_info():
    name = ctypes.create_string_buffer(256)
    cus = ctypes.c_int()
    mem = ctypes.c_size_t()
    check(_lib.load().smm_hip_device_info(name, 256, ctypes.byref(cus), ctypes.byref(mem)))
    return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}


def partials_count():
    return _lib.load().smm_hip_partials_count()


def finish_len():
    return _lib.load().smm_hip_finish_len()


def finish_totals_offset():
    return _lib.load().smm_hip_finish_totals_offset()


def uses_std_fma():
    return bool(_lib.load().smm_hip_uses_std_fma())


def synchronize(stream=None):
    check(_lib.load().smm_hip_stream_synchronize(_dptr(stream)))


def profile_enable(on=True):
    check(_lib.load().smm_hip_profile_enable(1 if on else 0))


def profile_read(reset=True):
    """(summed SpMV kernel milliseconds, launches) measured with HIP events on the launch stream"""
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    check(_lib.load().smm_hip_profile_read(ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0))
    return ms.value, n.value


def set_march_min_rows(const_diagonals_rows=-1, values_read_rows=-1):
    """from how many rows grid-shaped matrices run the 2.5-D kernels (-1: the default); applies to matrices analysed afterwards"""
    check(_lib.load().smm_hip_set_march_min_rows(int(const_diagonals_rows), int(values_read_rows)))


def set_pattern_sweep_rows(rows_open=0):
    """how many 64-row waves a hardware wave of the PATTERN sweep kernel holds open: 8, 16, 32 (0: the default); same bits at each"""
    check(_lib.load().smm_hip_set_pattern_sweep_rows(int(rows_open)))


def profile_read_waits(reset=True):
    """(exposed ms, exchanges): what the halo exchanges of the row-partitioned SpMVs cost BEYOND the local block that ran beside them"""
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    check(_lib.load().smm_hip_profile_read_waits(ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0))
    return ms.value, n.value


class Preconditioner:
    """`int apply(const T* rhs, T* x) const` (ref:1173-1235).  Created by CSRMatrix.getPreconditioner."""

    def __init__(self, matrix, kind, block_rows=None, level_cap=None, partition=None, chebyshev=None, amg=None, colors=None, power=None, sweeps=None,
                 candidates=None):
        self.matrix = matrix  # keeps the matrix alive (the reference holds a const CSRMatrix&)
        self.kind = SolverPreconditioner(kind)
        self._h = ctypes.c_void_p()
        if chebyshev is not None:  # (degree, bound mode, eig_ratio, power_steps, lambda_min, lambda_max): CHEBYSHEV with chosen parameters
            degree, bound, ratio, steps, lmin, lmax = chebyshev
            check(_lib.load().smm_hip_precond_create_chebyshev(matrix._h, int(degree), int(bound), float(ratio), int(steps), float(lmin), float(lmax),
                                                               ctypes.byref(self._h)))
        elif candidates is not None:  # (B, dofs_per_node, stream) + amg: AMG with near-null-space candidates
            B, dofs_per_node, stream = candidates
            theta, max_levels, coarse_rows, smooth_degree, ratio = amg
            rest = (int(dofs_per_node), float(theta), int(max_levels), int(coarse_rows), int(smooth_degree), float(ratio))
            if hasattr(B, "data_ptr"):  # a device tensor (n, k) with strides (1, n) -- e.g. the transpose of a contiguous (k, n) one --, or (n,)
                shape, stride = tuple(B.shape), tuple(B.stride())
                if not (len(shape) == 1 or (len(shape) == 2 and (shape[1] == 1 or stride[1] == shape[0]) and (shape[0] <= 1 or stride[0] == 1))):
                    raise TypeError("candidates on the device must be column-major: shape (n, k) with strides (1, n)")
                if shape[0] != matrix.rows or _SUFFIX.get(np.dtype(str(B.dtype).replace("torch.", ""))) != matrix._suf:
                    raise ValueError(f"candidates must have {matrix.rows} rows and the matrix dtype")
                k = 1 if len(shape) == 1 else shape[1]
                check(_fn("smm_hip_precond_create_amg_candidates_dev", matrix._suf)(matrix._h, _dptr(B), k, *rest, _dptr(stream), ctypes.byref(self._h)))
            else:
                B = np.asarray(B)
                B = B.reshape(-1, 1) if B.ndim == 1 else B
                if B.ndim != 2 or B.shape[0] != matrix.rows:
                    raise ValueError(f"candidates must have {matrix.rows} rows, got {B.shape[0]}")
                B = np.asfortranarray(B, dtype=matrix.dtype)
                check(_fn("smm_hip_precond_create_amg_candidates", matrix._suf)(matrix._h, B.ctypes.data_as(ctypes.c_void_p), B.shape[1], *rest, ctypes.byref(self._h)))
        elif amg is not None:  # (theta, max_levels, coarse_rows, smooth_degree, eig_ratio): AMG with chosen parameters
            theta, max_levels, coarse_rows, smooth_degree, ratio = amg
            check(_lib.load().smm_hip_precond_create_amg(matrix._h, float(theta), int(max_levels), int(coarse_rows), int(smooth_degree), float(ratio), ctypes.byref(self._h)))
        elif sweeps is not None:  # JSWEEP_ kinds with chosen step counts (lower, upper); 0 = the default
            check(_lib.load().smm_hip_precond_create_jsweep(matrix._h, int(_JSWEEP_BASE[self.kind]), int(sweeps[0]), int(sweeps[1]), ctypes.byref(self._h)))
        elif power is not None:  # FSAI / SPAI on the pattern of the power-th structural power of the matrix
            check(_lib.load().smm_hip_precond_create_ainv(matrix._h, int(kind), int(power), ctypes.byref(self._h)))
        elif colors is not None:  # MULTICOLOR_ kinds with the caller's colouring (one colour per row)
            colors = np.ascontiguousarray(colors, dtype=np.int32)
            check(_lib.load().smm_hip_precond_create_multicolor(matrix._h, int(_MULTICOLOR_BASE[self.kind]), _host(colors, np.int32, "colors"), colors.size,
                                                                ctypes.byref(self._h)))
        elif block_rows is None and level_cap is None and partition is None:
            check(_lib.load().smm_hip_precond_create(matrix._h, int(kind), ctypes.byref(self._h)))
        elif level_cap is None and partition is None:  # BLOCK_ILU0 / BLOCK_SGS with a chosen block size
            check(_lib.load().smm_hip_precond_create_block(matrix._h, int(kind), int(block_rows), ctypes.byref(self._h)))
        else:  # ... a chosen level cut (0 = none; None / -1 = the default) and partition (None / 0 = auto, 1 = contiguous rows, 2 = grid bricks)
            check(_lib.load().smm_hip_precond_create_block_ex(matrix._h, int(kind), int(block_rows or 0), -1 if level_cap is None else int(level_cap),
                                                               int(partition or 0), ctypes.byref(self._h)))

    def block_record_bytes(self):
        """BLOCK_ kinds: bytes one apply reads per row besides the vectors: (lower-sweep record, upper-sweep record, row-order entries)"""
        v = [ctypes.c_int() for _ in range(3)]
        check(_lib.load().smm_hip_precond_block_record_bytes(self._h, *[ctypes.byref(c) for c in v]))
        return tuple(c.value for c in v)

    def block_rows(self):
        """BLOCK_ kinds: (the rows block by block -- order[bounds[b] : bounds[b+1]] are block b's rows, the identity for contiguous
        blocks --, the brick's extent along the grid axes or (0, 0, 0))"""
        n = self.matrix.rows
        order = np.zeros(n, dtype=np.int32)
        brick = (ctypes.c_int * 3)()
        check(_lib.load().smm_hip_precond_block_rows(self._h, order.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(brick, ctypes.c_void_p)))
        return order, tuple(brick)

    def level_cap(self):
        """BLOCK_ kinds: the level cut this handle was built with (0 = none)"""
        c = ctypes.c_int()
        check(_lib.load().smm_hip_precond_block_level_cap(self._h, ctypes.byref(c)))
        return c.value

    def block_bounds(self):
        """BLOCK_ kinds: the nblocks + 1 row numbers at which the rows were cut"""
        n = ctypes.c_int()
        check(_lib.load().smm_hip_precond_block_count(self._h, ctypes.byref(n)))
        out = np.zeros(n.value + 1, dtype=np.int32)
        check(_lib.load().smm_hip_precond_block_bounds(self._h, out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out

    def apply(self, rhs, x):
        suf = self.matrix._suf
        n = self.matrix.rows
        check(_fn("smm_hip_precond_apply", suf)(self._h, _host(rhs, self.matrix.dtype, "rhs", n), _host(x, self.matrix.dtype, "x", n, True)))
        return 0

    def apply_dev(self, d_rhs, d_x, stream=None):
        check(_fn("smm_hip_precond_apply_dev", self.matrix._suf)(self._h, _dptr(d_rhs), _dptr(d_x), _dptr(stream)))

    def apply_spmv(self, v, x):
        """x = M^-1 (A v) (ref:2234-2235); the BLOCK_ kinds form A v inside the apply's launch"""
        suf = self.matrix._suf
        n = self.matrix.rows
        check(_fn("smm_hip_precond_apply_spmv", suf)(self._h, _host(v, self.matrix.dtype, "v", n), _host(x, self.matrix.dtype, "x", n, True)))
        return 0

    def apply_spmv_dev(self, d_v, d_x, stream=None):
        check(_fn("smm_hip_precond_apply_spmv_dev", self.matrix._suf)(self._h, _dptr(d_v), _dptr(d_x), _dptr(stream)))

    def take_error(self, stream=None):
        """synchronises `stream`; raises when a triangular sweep applied on it failed to finish (apply_dev cannot report it)"""
        check(_lib.load().smm_hip_precond_take_error(self._h, _dptr(stream)))

    def chebyshev_info(self):
        """CHEBYSHEV: {degree, bound (CHEB_BOUND_*), lambda_min, lambda_max} as the handle keeps them"""
        degree, bound, lmin, lmax = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        check(_lib.load().smm_hip_precond_chebyshev_info(self._h, ctypes.byref(degree), ctypes.byref(bound), ctypes.byref(lmin), ctypes.byref(lmax)))
        return {"degree": degree.value, "bound": bound.value, "lambda_min": lmin.value, "lambda_max": lmax.value}

    def amg_info(self):
        """AMG: {levels, rows (per level), nnz (per level), operator_complexity = sum nnz(A_l) / nnz(A_0)}"""
        levels, oc = ctypes.c_int(), ctypes.c_double()
        rows, nnz = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32)
        check(_lib.load().smm_hip_precond_amg_info(self._h, ctypes.byref(levels), _host(rows, np.int32, "rows"), _host(nnz, np.int32, "nnz"), 16, ctypes.byref(oc)))
        return {"levels": levels.value, "rows": [int(v) for v in rows[:levels.value]], "nnz": [int(v) for v in nnz[:levels.value]], "operator_complexity": oc.value}

    def amg_level(self, level):
        """AMG: (A_l, P_l, R_l) as CSRMatrix objects around handles this preconditioner OWNS (they live as long as it does and closing them
        does nothing); P_l and R_l are None on the coarsest level"""
        hs = [ctypes.c_void_p() for _ in range(3)]
        check(_lib.load().smm_hip_precond_amg_level(self._h, int(level), *(ctypes.byref(h) for h in hs)))
        out = []
        for h in hs:
            if not h:
                out.append(None)
                continue
            m = CSRMatrix._adopt(h, self.matrix.dtype)
            m._borrowed = True
            m._keep = self
            out.append(m)
        return tuple(out)

    def amg_aggregates(self, level):
        """AMG: the aggregate number of every row of level `level` (the coarsest level has none: SmmHipError)"""
        info = self.amg_info()
        if not 0 <= int(level) < info["levels"]:
            raise ValueError(f"level {level} of {info['levels']}")
        agg = np.empty(info["rows"][int(level)], dtype=np.int32)
        check(_lib.load().smm_hip_precond_amg_aggregates(self._h, int(level), _host(agg, np.int32, "agg"), len(agg)))
        return agg

    def amg_coarse_inverse(self):
        """AMG: the dense inverse of the coarsest matrix, n_L x n_L in the matrix dtype"""
        n = self.amg_info()["rows"][-1]
        out = np.empty((n, n), dtype=self.matrix.dtype)
        check(_fn("smm_hip_precond_amg_coarse_inverse", self.matrix._suf)(self._h, _host(out, self.matrix.dtype, "out"), n * n))
        return out

    def amg_candidates(self, level):
        """AMG created with candidates: {B: B_l of level `level` (n_l, k), dropped: the columns of T_l with no entries (the coarse dofs
        that became identity rows), T: T_l as a CSRMatrix this preconditioner owns (None on the coarsest level)}"""
        info = self.amg_info()
        if not 0 <= int(level) < info["levels"]:
            raise ValueError(f"level {level} of {info['levels']}")
        fn = _fn("smm_hip_precond_amg_candidates", self.matrix._suf)
        k, dropped, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
        check(fn(self._h, int(level), ctypes.c_void_p(0), 0, ctypes.byref(k), ctypes.byref(dropped), ctypes.byref(t)))
        B = np.empty((info["rows"][int(level)], k.value), dtype=self.matrix.dtype, order="F")
        check(fn(self._h, int(level), B.ctypes.data_as(ctypes.c_void_p), B.size, None, None, None))
        T = None
        if t:
            T = CSRMatrix._adopt(t, self.matrix.dtype)
            T._borrowed = True
            T._keep = self
        return {"B": B, "dropped": dropped.value, "T": T}

    def amg_refresh(self):
        """AMG: keep every aggregate and pattern, redo the values from the matrix's present values (after a value edit).  Synchronous."""
        check(_lib.load().smm_hip_precond_amg_refresh(self._h))

    def multicolor_info(self):
        """MULTICOLOR_ kinds: (ncolors, the ncolors + 1 row bounds of the colours in the permuted matrix)"""
        n = ctypes.c_int()
        check(_lib.load().smm_hip_precond_multicolor_info(self._h, ctypes.byref(n), ctypes.c_void_p(0), 0))
        bounds = np.zeros(n.value + 1, dtype=np.int32)
        check(_lib.load().smm_hip_precond_multicolor_info(self._h, ctypes.byref(n), _host(bounds, np.int32, "bounds"), bounds.size))
        return n.value, bounds

    def multicolor_perm(self):
        """MULTICOLOR_ kinds: perm[] -- row i of the permuted matrix is row perm[i] of the matrix"""
        perm = np.zeros(self.matrix.rows, dtype=np.int32)
        check(_lib.load().smm_hip_precond_multicolor_perm(self._h, _host(perm, np.int32, "perm"), perm.size))
        return perm

    def multicolor_matrix(self):
        """MULTICOLOR_ kinds: B = P A Pᵀ as a CSRMatrix around a handle this preconditioner OWNS (closing it does nothing)"""
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_precond_multicolor_matrix(self._h, ctypes.byref(h)))
        m = CSRMatrix._adopt(h, self.matrix.dtype)
        m._borrowed = True
        m._keep = self
        return m

    def multicolor_refresh(self):
        """MULTICOLOR_ kinds: keep the colouring, redo the permuted values and the factor from the matrix's present values.  Synchronous."""
        check(_lib.load().smm_hip_precond_multicolor_refresh(self._h))

    def ainv_info(self):
        """FSAI / SPAI: {power, max_row (the longest row of the pattern), nnz (the entries of G / M)}"""
        power, max_row, nnz = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        check(_lib.load().smm_hip_precond_ainv_info(self._h, ctypes.byref(power), ctypes.byref(max_row), ctypes.byref(nnz)))
        return {"power": power.value, "max_row": max_row.value, "nnz": int(nnz.value)}

    def ainv_matrix(self):
        """FSAI: (G, Gt); SPAI: (M, None) -- CSRMatrix objects around handles this preconditioner OWNS (closing them does nothing)"""
        hs = [ctypes.c_void_p(), ctypes.c_void_p()]
        check(_lib.load().smm_hip_precond_ainv_matrix(self._h, ctypes.byref(hs[0]), ctypes.byref(hs[1])))
        out = []
        for h in hs:
            if not h:
                out.append(None)
                continue
            m = CSRMatrix._adopt(h, self.matrix.dtype)
            m._borrowed = True
            m._keep = self
            out.append(m)
        return tuple(out)

    def ainv_refresh(self):
        """FSAI / SPAI: keep every pattern, redo the values from the matrix's present values (after a value edit).  Synchronous."""
        check(_lib.load().smm_hip_precond_ainv_refresh(self._h))

    def jsweep_info(self):
        """JSWEEP_ kinds: {base (the exact kind), sweeps_lower, sweeps_upper, levels_lower, levels_upper}; sweeps of levels - 1 make the
        apply the exact kind's bit for bit"""
        v = [ctypes.c_int() for _ in range(5)]
        check(_lib.load().smm_hip_precond_jsweep_info(self._h, *[ctypes.byref(c) for c in v]))
        return {"base": SolverPreconditioner(v[0].value), "sweeps_lower": v[1].value, "sweeps_upper": v[2].value, "levels_lower": v[3].value,
                "levels_upper": v[4].value}

    def jsweep_set_sweeps(self, lower, upper=None):
        """JSWEEP_ kinds: change the step counts (upper None: the same as lower), no rebuild"""
        check(_lib.load().smm_hip_precond_jsweep_set_sweeps(self._h, int(lower), int(lower if upper is None else upper)))

    def jsweep_refresh(self):
        """JSWEEP_ kinds: keep the pattern and its split, redo the factor and the triangles' values from the matrix's present values.  Synchronous."""
        check(_lib.load().smm_hip_precond_jsweep_refresh(self._h))

    def values(self):
        """factor values: diag (JACOBI, CHEBYSHEV, AMG) or the ILU0 / IC0 / BLOCK_ILU0 values on A's pattern (MULTICOLOR_ILU0 / _IC0: on
        the permuted matrix's pattern); FSAI / SPAI: the values of G / M on their own pattern (ainv_matrix)"""
        count = self.matrix.rows if self.kind in (SolverPreconditioner.JACOBI, SolverPreconditioner.CHEBYSHEV, SolverPreconditioner.AMG) else self.matrix.nnz
        if self.kind in _AINV_KINDS:
            count = self.ainv_info()["nnz"]
        out = np.empty(count, dtype=self.matrix.dtype)
        check(_fn("smm_hip_precond_values", self.matrix._suf)(self._h, _host(out, self.matrix.dtype, "out"), count))
        return out

    def set_sweep(self, mode):
        """SWEEP_AUTO / SWEEP_LEVELS / SWEEP_SYNCFREE: how the triangular sweeps are launched (same numbers either way)"""
        check(_lib.load().smm_hip_precond_set_sweep(self._h, int(mode)))

    def levels(self):
        kind, lo, up = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(_lib.load().smm_hip_precond_info(self._h, ctypes.byref(kind), ctypes.byref(lo), ctypes.byref(up)))
        return lo.value, up.value

    def close(self):
        if self._h:
            _lib.load().smm_hip_precond_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CSRMatrix:
    """Device-resident CSRMatrix<T> with the reference's layout (ref:1243-1259): values[nnz], positions[nnz]
    (ascending per row), start[rows+1]."""

    def __init__(self, rows, cols, start, positions, values):
        values = np.ascontiguousarray(values)
        self.dtype = values.dtype
        self._suf = _suffix(self.dtype)
        start = np.ascontiguousarray(start, dtype=np.int32)
        positions = np.ascontiguousarray(positions, dtype=np.int32)
        if start.size != rows + 1:
            raise ValueError("start must have rows+1 entries")
        if positions.size < start[-1] or values.size < start[-1]:
            raise ValueError("positions/values shorter than start[rows]")
        self._h = ctypes.c_void_p()
        self._keep = None
        check(_fn("smm_hip_csr_create", self._suf)(int(rows), int(cols), _host(start, np.int32, "start"), _host(positions, np.int32, "positions"),
                                                   _host(values, self.dtype, "values"), ctypes.byref(self._h)))
        self._read_info()

    @classmethod
    def from_device(cls, rows, cols, d_start, d_positions, d_values, dtype):
        """Wrap arrays already in HBM (no copy).  The arrays are kept referenced by the returned object."""
        self = cls.__new__(cls)
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(self.dtype)
        self._h = ctypes.c_void_p()
        self._keep = (d_start, d_positions, d_values)
        check(_fn("smm_hip_csr_create_dev", self._suf)(int(rows), int(cols), _dptr(d_start), _dptr(d_positions), _dptr(d_values), ctypes.byref(self._h)))
        self._read_info()
        return self

    @classmethod
    def from_triplets(cls, rows, cols, row_idx, col_idx, values):
        """The reference's TripletMatrix + CSRMatrix(triplet) in one call, assembled on the device: repeated (row, col) pairs add up in
        list order.  The plan is created and dropped; keep an AssemblyPlan to assemble the same list of pairs again."""
        plan = AssemblyPlan(rows, cols, row_idx, col_idx)
        try:
            return plan.assemble(values)
        finally:
            plan.close()

    @classmethod
    def _adopt(cls, handle, dtype):
        self = cls.__new__(cls)
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(self.dtype)
        self._h = handle
        self._keep = None
        self._read_info()
        return self

    def _read_info(self):
        r, c, n, d, f = (ctypes.c_int() for _ in range(5))
        check(_lib.load().smm_hip_csr_info(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(n), ctypes.byref(d), ctypes.byref(f)))
        self.rows, self.cols, self.nnz, self.first_active_start = r.value, c.value, n.value, f.value

    # reference getters (ref:1351-1364)
    def getDenseRowCount(self):
        return self.rows

    def getDenseColCount(self):
        return self.cols

    def getNonZeroCount(self):
        return self.nnz

    def set_kernel(self, family=SPMV_AUTO, lanes_per_row=0):
        check(_lib.load().smm_hip_csr_set_kernel(self._h, int(family), int(lanes_per_row)))

    def get_kernel(self):
        fam, lanes = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().smm_hip_csr_get_kernel(self._h, ctypes.byref(fam), ctypes.byref(lanes)))
        return fam.value, lanes.value

    def autotune(self):
        check(_lib.load().smm_hip_csr_autotune(self._h))
        return self.get_kernel()

    def _spmv(self, op, lhs, mult, out):
        fn = _fn("smm_hip_spmv", self._suf)
        plhs = _host(lhs, self.dtype, "lhs", self.rows) if op != OP_ASSIGN else ctypes.c_void_p(0)
        check(fn(self._h, op, plhs, _host(mult, self.dtype, "mult", self.cols), _host(out, self.dtype, "out", self.rows, True)))

    def rMult(self, mult, res):  # ref:1501-1505
        self._spmv(OP_ASSIGN, None, mult, res)

    def rMultAdd(self, lhs, mult, out):  # ref:1507-1510
        self._spmv(OP_ADD, lhs, mult, out)

    def rMultSub(self, lhs, mult, out):  # ref:1512-1515
        self._spmv(OP_SUB, lhs, mult, out)

    def spmv_dev(self, op, d_lhs, d_x, d_out, stream=None):
        check(_fn("smm_hip_spmv_dev", self._suf)(self._h, int(op), _dptr(d_lhs), _dptr(d_x), _dptr(d_out), _dptr(stream)))

    # ---- several right-hand sides at once (smm_hip.h "CSR SpMM"): X is (cols, k), Lhs / Out are (rows, k), C-contiguous, k <= MAX_RHS.
    # Additions: the reference multiplies by one vector.  Column j of Out is what rMult / rMultAdd / rMultSub give for column j alone.
    def _spmm(self, op, lhs, mult, out):
        pout, k = _block(out, self.dtype, "Out", self.rows, None, True)
        px, _ = _block(mult, self.dtype, "X", self.cols, k)
        plhs = _block(lhs, self.dtype, "Lhs", self.rows, k)[0] if op != OP_ASSIGN else ctypes.c_void_p(0)
        check(_fn("smm_hip_spmm", self._suf)(self._h, op, k, plhs, px, pout))

    def rMultBlock(self, X, Out):
        self._spmm(OP_ASSIGN, None, X, Out)

    def rMultAddBlock(self, Lhs, X, Out):
        self._spmm(OP_ADD, Lhs, X, Out)

    def rMultSubBlock(self, Lhs, X, Out):
        self._spmm(OP_SUB, Lhs, X, Out)

    def spmm_dev(self, op, k, d_lhs, d_x, d_out, stream=None):
        check(_fn("smm_hip_spmm_dev", self._suf)(self._h, int(op), int(k), _dptr(d_lhs), _dptr(d_x), _dptr(d_out), _dptr(stream)))

    def tile_info(self):
        """(tiles, nonzeros per tile, rows per tile, 1 if spmvTileKernel serves the launches) of the STREAM family's tile table"""
        v = [ctypes.c_int() for _ in range(4)]
        check(_lib.load().smm_hip_csr_tile_info(self._h, *[ctypes.byref(c) for c in v]))
        return tuple(c.value for c in v)

    def pattern_info(self):
        """(encoding, distinct offsets) of the PATTERN family for this matrix: encoding 0 none / not analysed, 1 row masks, 2 entry
        codes, 3 row masks + constant diagonals (no values[] read)"""
        enc, k = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().smm_hip_csr_pattern_info(self._h, ctypes.byref(enc), ctypes.byref(k)))
        return enc.value, k.value

    def find_blocks(self, block_size=0):
        """the BLOCKS family's analysis (every entry checked on the device): block_size 2, 3 or 4 tests that size, 0 tries 4, 3, 2 and
        keeps the first that fits.  Returns the size kept by this call, 0 when the matrix does not fit (not an error)."""
        found = ctypes.c_int()
        check(_lib.load().smm_hip_csr_find_blocks(self._h, int(block_size), ctypes.byref(found)))
        return found.value

    def blocks_info(self):
        """(block size, blocks, most entries a row may hold at that size) of the kept BLOCKS analysis; (0, 0, 0) without one"""
        b, n, cap = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
        check(_lib.load().smm_hip_csr_blocks_info(self._h, ctypes.byref(b), ctypes.byref(n), ctypes.byref(cap)))
        return b.value, n.value, cap.value

    def longrows_configure(self, split_len=0, segment_len=0):
        """the LONGROWS family's two lengths (0 = the default of either; SmmHipError outside the ranges include/smm_hip.h states): rows of
        more than split_len entries are cut into segments of segment_len.  Replaces a kept analysis at once; without one the lengths are
        kept for the analysis set_kernel(SPMV_LONGROWS) runs."""
        check(_lib.load().smm_hip_csr_longrows_configure(self._h, int(split_len), int(segment_len)))

    def longrows_info(self):
        """(split_len, segment_len, long rows, segments) of the kept LONGROWS analysis; (0, 0, 0, 0) without one"""
        s, g, n, segs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        check(_lib.load().smm_hip_csr_longrows_info(self._h, ctypes.byref(s), ctypes.byref(g), ctypes.byref(n), ctypes.byref(segs)))
        return s.value, g.value, n.value, segs.value

    def kernel_desc(self):
        """(kernel name without template arguments, bytes one launch of it moves by ITS data layout) for the next SpMV of this matrix"""
        buf = ctypes.create_string_buffer(64)
        nbytes = ctypes.c_longlong()
        check(_lib.load().smm_hip_csr_kernel_desc(self._h, buf, 64, ctypes.byref(nbytes)))
        return buf.value.decode(), nbytes.value

    def pattern_allow_const(self, allow):
        """False: a matrix with constant diagonals keeps reading values[] (measurements); same bits either way"""
        check(_lib.load().smm_hip_csr_pattern_allow_const(self._h, 1 if allow else 0))

    def pattern_slots(self, mode):
        """the PATTERN slots kernel: -1 AUTO (default), 0 off, 1 wherever it applies, 2 AUTO's rules also on a kernel set with set_kernel,
        3 wherever it applies and walked by the sweep kernel; same bits as the tile kernel"""
        check(_lib.load().smm_hip_csr_pattern_slots(self._h, int(mode)))

    # ---- editing the values on the device (the pattern stays; smm_hip.h "editing the VALUES of a matrix") ----
    # The reference's names (ref:1525-1604) return once the edit is done on the GPU; the batch / bulk forms below take an optional
    # stream and are then only enqueued on it.  Preconditioners made before an edit: SGS follows it, the other kinds are snapshots.
    def _edited(self, stream):
        if stream is None:
            synchronize(None)

    def scale(self, alpha, stream=None):
        check(_fn("smm_hip_csr_scale", self._suf)(self._h, float(alpha), _dptr(stream)))
        self._edited(stream)

    def axpy(self, alpha, other, stream=None):
        """values += alpha * other.values (same pattern and dtype, else SmmHipError with SMM_HIP_ERR_INVALID and nothing changed)"""
        check(_fn("smm_hip_csr_axpy", self._suf)(self._h, float(alpha), other._h, _dptr(stream)))
        self._edited(stream)

    def zero(self, stream=None):
        check(_fn("smm_hip_csr_zero", self._suf)(self._h, _dptr(stream)))
        self._edited(stream)

    def __imul__(self, alpha):  # ref:1525-1531
        self.scale(alpha)
        return self

    def inplaceAdd(self, other):  # ref:1533-1540
        self.axpy(1.0, other)

    def inplaceSubtract(self, other):  # ref:1542-1549
        self.axpy(-1.0, other)

    def zeroValues(self):  # ref:1591-1594
        self.zero()

    def hasSameNonZeroPattern(self, other):  # ref:1366-1385
        same = ctypes.c_int()
        check(_lib.load().smm_hip_csr_same_pattern(self._h, other._h, ctypes.byref(same)))
        return bool(same.value)

    def update_entries(self, rows, cols, vals, add=False):
        """Apply (rows[i], cols[i], vals[i]) in one device pass as if one after another (SET, or ADD with add=True); returns the bool
        mask of the entries that are stored (the others changed nothing)"""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=self.dtype)
        n = rows.size
        if cols.size != n or vals.size != n:
            raise ValueError("rows, cols and vals must have the same length")
        found = np.zeros(n, dtype=np.uint8)
        check(_fn("smm_hip_csr_update_entries", self._suf)(self._h, n, _host(rows, np.int32, "rows"), _host(cols, np.int32, "cols"), _host(vals, self.dtype, "vals"),
                                                          1 if add else 0, _host(found, np.uint8, "found")))
        return found.astype(bool)

    def update_entries_dev(self, n, d_rows, d_cols, d_vals, add=False, d_found=None, stream=None):
        check(_fn("smm_hip_csr_update_entries_dev", self._suf)(self._h, int(n), _dptr(d_rows), _dptr(d_cols), _dptr(d_vals), 1 if add else 0, _dptr(d_found),
                                                              _dptr(stream)))
        self._edited(stream)

    def updateEntry(self, row, col, value):  # ref:1572-1580
        return bool(self.update_entries([row], [col], [value])[0])

    def addEntry(self, row, col, value):  # ref:1596-1604
        return bool(self.update_entries([row], [col], [value], add=True)[0])

    def set_values(self, values):
        """replace all nnz values from a host array (only values[] is uploaded)"""
        values = np.ascontiguousarray(values, dtype=self.dtype)
        check(_fn("smm_hip_csr_set_values", self._suf)(self._h, _host(values, self.dtype, "values", self.nnz)))

    def set_values_dev(self, d_values, stream=None):
        check(_fn("smm_hip_csr_set_values_dev", self._suf)(self._h, _dptr(d_values), _dptr(stream)))
        self._edited(stream)

    def get_values(self):
        out = np.empty(self.nnz, dtype=self.dtype)
        check(_fn("smm_hip_csr_get_values", self._suf)(self._h, _host(out, self.dtype, "out")))
        return out

    def values_changed(self, stream=None):
        """from_device matrices: the caller has written d_values itself (ordered before this call on `stream`)"""
        check(_fn("smm_hip_csr_values_changed", self._suf)(self._h, _dptr(stream)))
        self._edited(stream)

    # ---- the transpose, built on the device (smm_hip.h "the TRANSPOSE of a matrix") ----
    def transpose(self, stream=None):
        """Aᵀ as a new CSRMatrix that owns its arrays and does not need this one afterwards: row j holds column j's entries, source rows
        ascending; values bit for bit.  May synchronise `stream`."""
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_transpose_create(self._h, _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def norm2(self, tol=1e-6, at=None):
        """||A||_2, the largest singular value: svds(self, 1)[1][0] without the vectors (needs min(rows, cols) >= 3).  tol is svds's:
        the residual estimate relative to the value itself.  RuntimeError when the solve does not report SUCCESS."""
        _, s, _, info = svds(self, 1, tol=tol, at=at, vectors=False)
        if info.status != SolverStatus.SUCCESS:
            raise RuntimeError(f"norm2: svds ended with {info.status.name} after {info.restarts} restarts")
        return float(s[0])

    def transpose_refresh(self, A, stream=None):
        """called on a matrix made by transpose(): take over the present values of A (the source, or a matrix with its pattern) in one
        gather pass -- a value edit of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) for any other pair."""
        check(_fn("smm_hip_csr_transpose_refresh", self._suf)(self._h, A._h, _dptr(stream)))
        self._edited(stream)

    # ---- colouring and symmetric permutation, on the device (smm_hip.h "a COLOURING of the rows and the SYMMETRIC PERMUTATION") ----
    def color(self):
        """(colors[rows], ncolors): greedy colouring of the adjacency graph in descending splitmix64(row + 1) order; no stored
        off-diagonal entry joins two rows of one colour"""
        colors = np.zeros(self.rows, dtype=np.int32)
        n = ctypes.c_int()
        check(_lib.load().smm_hip_csr_color(self._h, _host(colors, np.int32, "colors"), colors.size, ctypes.byref(n)))
        return colors, n.value

    def color_dev(self, d_colors, stream=None):
        """the same into an int32 device array of `rows` entries; returns ncolors"""
        n = ctypes.c_int()
        check(_lib.load().smm_hip_csr_color_dev(self._h, _dptr(d_colors), self.rows, _dptr(stream), ctypes.byref(n)))
        return n.value

    def permute(self, perm, stream=None):
        """P A Pᵀ as a new CSRMatrix that owns its arrays: row i is this matrix's row perm[i], entry (i, j) its (perm[i], perm[j]); columns
        ascend, values bit for bit.  SmmHipError (SMM_HIP_ERR_INVALID) when perm is not a permutation of 0 .. rows - 1."""
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_permute_create(self._h, _host(perm, np.int32, "perm"), perm.size, _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def permute_dev(self, d_perm, count, stream=None):
        """permute() with perm[] in an int32 device array of `count` entries"""
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_permute_create_dev(self._h, _dptr(d_perm), int(count), _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def permute_refresh(self, A, stream=None):
        """called on a matrix made by permute(): take over the present values of A (the source, or a matrix with its pattern) in one
        gather pass -- a value edit of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) for any other pair."""
        check(_fn("smm_hip_csr_permute_refresh", self._suf)(self._h, A._h, _dptr(stream)))
        self._edited(stream)

    # ---- bandwidth-reducing ordering, on the device (smm_hip.h "a BANDWIDTH-REDUCING ORDERING") ----
    def rcm(self, reverse=True):
        """(perm[rows], info): the reverse Cuthill-McKee ordering of the adjacency graph (reverse=False: Cuthill-McKee); perm[i] is the
        row that becomes row i, so B = A.permute(perm) has its entries near the diagonal.  info: components, levels, bandwidth_before,
        bandwidth_after.  One host round trip per level of every breadth-first search: long thin graphs are slow."""
        perm = np.zeros(self.rows, dtype=np.int32)
        comps, levels = ctypes.c_int(), ctypes.c_int()
        before, after = ctypes.c_longlong(), ctypes.c_longlong()
        check(_lib.load().smm_hip_csr_rcm(self._h, _host(perm, np.int32, "perm"), perm.size, 1 if reverse else 0, ctypes.byref(comps), ctypes.byref(levels),
                                          ctypes.byref(before), ctypes.byref(after)))
        return perm, {"components": comps.value, "levels": levels.value, "bandwidth_before": before.value, "bandwidth_after": after.value}

    def rcm_dev(self, d_perm, reverse=True, stream=None):
        """the same into an int32 device array of `rows` entries, on `stream` (synchronised); returns info"""
        comps, levels = ctypes.c_int(), ctypes.c_int()
        before, after = ctypes.c_longlong(), ctypes.c_longlong()
        check(_lib.load().smm_hip_csr_rcm_dev(self._h, _dptr(d_perm), self.rows, 1 if reverse else 0, _dptr(stream), ctypes.byref(comps), ctypes.byref(levels),
                                              ctypes.byref(before), ctypes.byref(after)))
        return {"components": comps.value, "levels": levels.value, "bandwidth_before": before.value, "bandwidth_after": after.value}

    def bandwidth(self):
        """(max |i - j| over the stored entries, the number of distinct j - i)"""
        width, offsets = ctypes.c_longlong(), ctypes.c_longlong()
        check(_lib.load().smm_hip_csr_bandwidth(self._h, ctypes.byref(width), ctypes.byref(offsets)))
        return width.value, offsets.value

    def isSymmetric(self):
        """(pattern, values): the pattern equals the transpose's; in addition every value equals its mirror image by IEEE == (a NaN never
        does).  (False, False) for a matrix that is not square."""
        p, v = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().smm_hip_csr_is_symmetric(self._h, ctypes.byref(p), ctypes.byref(v)))
        return bool(p.value), bool(v.value)

    def get_pattern(self):
        """(start[rows + 1], positions[nnz]) copied from the device"""
        start = np.empty(self.rows + 1, dtype=np.int32)
        positions = np.empty(self.nnz, dtype=np.int32)
        check(_lib.load().smm_hip_csr_get_pattern(self._h, _host(start, np.int32, "start"), _host(positions, np.int32, "positions")))
        return start, positions

    # ---- the product of two matrices, built on the device (smm_hip.h "the PRODUCT C = A B") ----
    def multiply(self, B, stream=None):
        """self B as a new CSRMatrix that owns its arrays: the structural product (nothing dropped by value), columns ascending; every
        entry is the row sum of rMult over this matrix's entries in stored order, bit for bit.  Synchronises `stream`."""
        if not isinstance(B, CSRMatrix):
            raise TypeError("multiply needs a CSRMatrix")
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_multiply_create(self._h, B._h, _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def __matmul__(self, B):
        if not isinstance(B, CSRMatrix):
            return NotImplemented
        return self.multiply(B)

    def multiply_into(self, A, B, stream=None):
        """the numeric phase alone: this matrix's values become those of A B on ITS pattern (+0.0 where no product lands) -- a value edit
        of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) when a product falls on an entry this matrix does not store.
        Synchronises `stream`."""
        check(_fn("smm_hip_csr_multiply_into", self._suf)(self._h, A._h, B._h, _dptr(stream)))
        self._edited(stream)

    # ---- the sum of two matrices with any two patterns, built on the device (smm_hip.h "the SUM C = alpha A + beta B") ----
    def add(self, B, alpha=1, beta=1, stream=None):
        """alpha self + beta B as a new CSRMatrix that owns its arrays: the union of the two patterns (nothing dropped by value), columns
        ascending; u = alpha a, v = beta b, the entry u + v, u or v -- the bits of the assembly of self's scaled triplets followed by B's.
        Both matrices must hold strictly ascending columns in every row (SmmHipError otherwise).  Synchronises `stream`."""
        if not isinstance(B, CSRMatrix):
            raise TypeError("add needs a CSRMatrix")
        h = ctypes.c_void_p()
        check(_fn("smm_hip_csr_add_create", self._suf)(self._h, float(alpha), B._h, float(beta), _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def __add__(self, B):
        if not isinstance(B, CSRMatrix):
            return NotImplemented
        return self.add(B)

    def __sub__(self, B):
        if not isinstance(B, CSRMatrix):
            return NotImplemented
        return self.add(B, 1, -1)

    def add_into(self, A, B, alpha=1, beta=1, stream=None):
        """the numeric phase alone: this matrix's values become those of alpha A + beta B on ITS pattern (+0.0 where neither stores an
        entry) -- a value edit of this matrix, which may itself be A, B or both (A <- A + sigma D in place).  SmmHipError
        (SMM_HIP_ERR_INVALID, nothing changed) when A or B stores an entry this matrix does not.  Synchronises `stream`."""
        check(_fn("smm_hip_csr_add_into", self._suf)(self._h, A._h, float(alpha), B._h, float(beta), _dptr(stream)))
        self._edited(stream)

    # ---- composing and slicing on the device (smm_hip.h "COMPOSING and SLICING matrices"); bmat / hstack / vstack are module functions ----
    def block_refresh(self, blocks, coef=None, stream=None):
        """called on a matrix made by bmat(): the numeric phase alone into the kept pattern, from the present values of `blocks` (the table
        of bmat: same None slots, same shapes and entry counts; that the patterns are those of then is the caller's contract) -- a value
        edit of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) otherwise."""
        p, q, table, pcoef, _ = _block_table(blocks, coef, self.dtype)
        check(_fn("smm_hip_csr_block_refresh", self._suf)(self._h, p, q, table, pcoef, _dptr(stream)))
        self._edited(stream)

    def submatrix(self, rows=None, cols=None, stream=None):
        """the rows `rows` (any order, repeats allowed) restricted to the columns `cols` (strictly ascending) as a new CSRMatrix that owns
        its arrays; values bit for bit.  Each of the two is None (all), a slice with step 1 (with two slices or a slice and None: the range
        form, no index list) or an integer array.  SmmHipError (SMM_HIP_ERR_INVALID) naming the first offending position for an index
        outside the matrix or columns that do not ascend strictly.  Synchronises `stream`."""
        h = ctypes.c_void_p()
        lib = _lib.load()
        rows, cols = _index_arg(rows, self.rows, "rows"), _index_arg(cols, self.cols, "cols")
        if isinstance(rows, tuple) and isinstance(cols, tuple):  # two ranges: no index list
            check(lib.smm_hip_csr_submatrix_range_create(self._h, rows[0], rows[1], cols[0], cols[1], _dptr(stream), ctypes.byref(h)))
            return CSRMatrix._adopt(h, self.dtype)
        if isinstance(rows, tuple):  # a range beside an index list: all of them is NULL, anything else is written out
            rows = None if rows == (0, self.rows) else np.arange(rows[0], rows[1], dtype=np.int32)
        if isinstance(cols, tuple):
            cols = None if cols == (0, self.cols) else np.arange(cols[0], cols[1], dtype=np.int32)
        pr = _host(rows, np.int32, "rows") if rows is not None else ctypes.c_void_p(0)
        pc = _host(cols, np.int32, "cols") if cols is not None else ctypes.c_void_p(0)
        check(lib.smm_hip_csr_submatrix_create(self._h, pr, 0 if rows is None else rows.size, pc, 0 if cols is None else cols.size, _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def submatrix_dev(self, d_rows, nr, d_cols, nc, stream=None):
        """submatrix() with the index lists in int32 device arrays of nr / nc entries (None: all rows / all columns)"""
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_submatrix_create_dev(self._h, _dptr(d_rows), int(nr), _dptr(d_cols), int(nc), _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, self.dtype)

    def submatrix_refresh(self, A, stream=None):
        """called on a matrix made by submatrix(): take over the present values of A (the source, or a matrix with its pattern) in one
        gather pass -- a value edit of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) for a matrix of another shape or
        entry count."""
        check(_fn("smm_hip_csr_submatrix_refresh", self._suf)(self._h, A._h, _dptr(stream)))
        self._edited(stream)

    def diagonal(self, return_missing=False):
        """the diagonal as a vector of min(rows, cols) elements, 0 where no diagonal entry is stored; with return_missing also how many
        are not stored"""
        out = np.zeros(min(self.rows, self.cols), dtype=self.dtype)
        missing = ctypes.c_int()
        check(_fn("smm_hip_csr_diagonal", self._suf)(self._h, _host(out, self.dtype, "out"), ctypes.byref(missing)))
        return (out, missing.value) if return_missing else out

    def diagonal_dev(self, d_out, d_missing=None, stream=None):
        """the same into a device array of min(rows, cols) elements; d_missing: an int32 on the device for the count, or None"""
        check(_fn("smm_hip_csr_diagonal_dev", self._suf)(self._h, _dptr(d_out), _dptr(d_missing), _dptr(stream)))

    def scale_rows_cols(self, r=None, c=None):
        """v_ij <- (r_i v_ij) c_j in place, two roundings in this order; r has `rows` elements, c `cols`; None skips the factor"""
        r = None if r is None else np.ascontiguousarray(r, dtype=self.dtype)
        c = None if c is None else np.ascontiguousarray(c, dtype=self.dtype)
        pr = _host(r, self.dtype, "r", self.rows) if r is not None else ctypes.c_void_p(0)
        pc = _host(c, self.dtype, "c", self.cols) if c is not None else ctypes.c_void_p(0)
        check(_fn("smm_hip_csr_scale_rows_cols", self._suf)(self._h, pr, pc))

    def scale_rows_cols_dev(self, d_r=None, d_c=None, stream=None):
        """the same with the vectors in device memory, enqueued on `stream`"""
        check(_fn("smm_hip_csr_scale_rows_cols_dev", self._suf)(self._h, _dptr(d_r), _dptr(d_c), _dptr(stream)))
        self._edited(stream)

    # ---- the other precision, converted on the device (smm_hip.h "a matrix in the OTHER PRECISION") ----
    def astype(self, dtype, stream=None):
        """this matrix with values of `dtype` (float32 / float64) as a new CSRMatrix that owns its arrays: float64 -> float32 rounds to
        nearest even (the bits of numpy's astype), float32 -> float64 is exact, the same dtype is a copy.  A finite value outside fp32's
        range raises SmmHipError (SMM_HIP_ERR_INVALID) naming the entry; underflow is allowed.  Synchronises `stream`."""
        dtype = np.dtype(dtype)
        code = 0 if _suffix(dtype) == "f32" else 1  # SMM_DTYPE_F32 / SMM_DTYPE_F64
        h = ctypes.c_void_p()
        check(_lib.load().smm_hip_csr_convert_create(self._h, code, _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, dtype)

    def convert_refresh(self, src, stream=None):
        """take over the present values of `src` (same rows, cols and nnz; that the patterns agree is the caller's contract), converted to
        this matrix's dtype -- a value edit of this matrix.  SmmHipError (SMM_HIP_ERR_INVALID, nothing changed) for another shape, for
        src being this matrix, or for a value outside fp32's range."""
        check(_lib.load().smm_hip_csr_convert_refresh(self._h, src._h, _dptr(stream)))
        self._edited(stream)

    def spmv_fused_dev(self, op, d_lhs, d_x, d_out, dot_mode, d_w1, d_partials, stream=None, finish=False):
        """SpMV with the dot products of the fresh out[] in its epilogue (dot_mode 1: out.w1; 2: out.out and out.w1).  finish=False:
        d_partials receives 2 x partials_count() per-workgroup sums; finish=True: d_partials is a finishing buffer of finish_len()
        elements (zeroed once) and the totals land at finish_totals_offset() + {0, 1}"""
        name = "smm_hip_spmv_fused_finish_dev" if finish else "smm_hip_spmv_fused_dev"
        check(_fn(name, self._suf)(self._h, int(op), _dptr(d_lhs), _dptr(d_x), _dptr(d_out), int(dot_mode), _dptr(d_w1), _dptr(d_partials), _dptr(stream)))

    def getPreconditioner(self, kind, block_rows=None, level_cap=None, partition=None, degree=None, bound=None, eig_ratio=None, power_steps=None,
                          lambda_min=None, lambda_max=None, theta=None, max_levels=None, coarse_rows=None, smooth_degree=None, colors=None, power=None, sweeps=None,
                          candidates=None, dofs_per_node=None, stream=None):
        """ref:1643-1651.  kind: a SolverPreconditioner or its name ("CHEBYSHEV").  block_rows / level_cap / partition: BLOCK_ kinds only;
        degree (3) / bound ("GERSHGORIN", "POWER", "USER" or a CHEB_BOUND_* code) / eig_ratio (30) / power_steps (10) / lambda_min /
        lambda_max (USER): CHEBYSHEV only; theta (0.08) / max_levels (10) / coarse_rows (256) / smooth_degree (2) and eig_ratio (30): AMG only.
        colors (one per row; None = CSRMatrix.color's): MULTICOLOR_ kinds only; power (1 .. 4; 1): FSAI / SPAI only;
        sweeps (an int, or a (lower, upper) pair; 1 .. 1024; 3): JSWEEP_ kinds only.  None = the default.
        candidates (AMG only): the near-null space B, (n, k) with 1 <= k <= 6 -- a numpy array, or a column-major device tensor in use on
        `stream` --, with dofs_per_node (1 .. 4; 1) rows per node: smoothed aggregation for vector-valued problems, e.g.
        generators.rigid_body_modes(coords) for elasticity.  None: the scalar hierarchy, as always."""
        if isinstance(kind, str):
            kind = SolverPreconditioner[kind]
        if candidates is not None or dofs_per_node is not None:
            if SolverPreconditioner(kind) != SolverPreconditioner.AMG or candidates is None:
                raise ValueError("candidates / dofs_per_node belong to the AMG preconditioner, and dofs_per_node needs candidates")
            if any(v is not None for v in (block_rows, level_cap, partition, degree, bound, power_steps, lambda_min, lambda_max, colors, power, sweeps)):
                raise ValueError("the AMG preconditioner takes theta / max_levels / coarse_rows / smooth_degree / eig_ratio only")
            return Preconditioner(self, kind, candidates=(candidates, 1 if dofs_per_node is None else dofs_per_node, stream),
                                  amg=(0.08 if theta is None else theta, 10 if max_levels is None else max_levels, 256 if coarse_rows is None else coarse_rows,
                                       2 if smooth_degree is None else smooth_degree, 30.0 if eig_ratio is None else eig_ratio))
        if sweeps is not None:
            if SolverPreconditioner(kind) not in _JSWEEP_BASE:
                raise ValueError("sweeps belongs to the JSWEEP_ preconditioners")
            if any(v is not None for v in (block_rows, level_cap, partition, degree, bound, eig_ratio, power_steps, lambda_min, lambda_max, theta, max_levels,
                                           coarse_rows, smooth_degree, colors, power)):
                raise ValueError("the JSWEEP_ preconditioners take sweeps only")
            lower, upper = (sweeps, sweeps) if isinstance(sweeps, (int, np.integer)) else sweeps
            return Preconditioner(self, kind, sweeps=(int(lower), int(upper)))
        if power is not None:
            if SolverPreconditioner(kind) not in _AINV_KINDS:
                raise ValueError("power belongs to the FSAI / SPAI preconditioners")
            if any(v is not None for v in (block_rows, level_cap, partition, degree, bound, eig_ratio, power_steps, lambda_min, lambda_max, theta, max_levels,
                                           coarse_rows, smooth_degree, colors)):
                raise ValueError("the FSAI / SPAI preconditioners take power only")
            return Preconditioner(self, kind, power=power)
        if colors is not None:
            if SolverPreconditioner(kind) not in _MULTICOLOR_BASE:
                raise ValueError("colors belongs to the MULTICOLOR_ preconditioners")
            return Preconditioner(self, kind, colors=colors)
        amg = (theta, max_levels, coarse_rows, smooth_degree)
        if any(v is not None for v in amg) or (eig_ratio is not None and SolverPreconditioner(kind) == SolverPreconditioner.AMG):
            if SolverPreconditioner(kind) != SolverPreconditioner.AMG:
                raise ValueError("theta / max_levels / coarse_rows / smooth_degree belong to the AMG preconditioner")
            if any(v is not None for v in (degree, bound, power_steps, lambda_min, lambda_max)):
                raise ValueError("degree / bound / power_steps / lambda_min / lambda_max belong to the CHEBYSHEV preconditioner")
            return Preconditioner(self, kind, amg=(0.08 if theta is None else theta, 10 if max_levels is None else max_levels, 256 if coarse_rows is None else coarse_rows,
                                                   2 if smooth_degree is None else smooth_degree, 30.0 if eig_ratio is None else eig_ratio))
        cheb = (degree, bound, eig_ratio, power_steps, lambda_min, lambda_max)
        if any(v is not None for v in cheb):
            if SolverPreconditioner(kind) != SolverPreconditioner.CHEBYSHEV:
                raise ValueError("degree / bound / eig_ratio / power_steps / lambda_min / lambda_max belong to the CHEBYSHEV preconditioner")
            if isinstance(bound, str):
                bound = _CHEB_BOUNDS[bound.upper()]
            cheb = (3 if degree is None else degree, CHEB_BOUND_GERSHGORIN if bound is None else bound, 30.0 if eig_ratio is None else eig_ratio,
                    10 if power_steps is None else power_steps, 0.0 if lambda_min is None else lambda_min, 0.0 if lambda_max is None else lambda_max)
            return Preconditioner(self, kind, chebyshev=cheb)
        return Preconditioner(self, kind, block_rows, level_cap, partition)

    def close(self):
        if self._h and getattr(self, "_borrowed", False):  # a level of a multigrid preconditioner, a multicolour one's matrix: that handle owns it
            self._h = ctypes.c_void_p()
        if self._h:
            _lib.load().smm_hip_csr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _index_arg(v, n, name):
    """None -> the range (0, n); a slice with step 1 -> the range (lo, hi); anything else -> a contiguous int32 array"""
    if v is None:
        return 0, n
    if isinstance(v, slice):
        lo, hi, step = v.indices(n)
        if step != 1:
            raise ValueError(f"{name}: a slice must have step 1 (pass an integer array for anything else)")
        return lo, max(lo, hi)
    a = np.ascontiguousarray(v, dtype=np.int32)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    return a


def _block_table(blocks, coef, dtype=None):
    """(p, q, the row-major handle table, the coefficient array or NULL, dtype) of a rectangular nested list of CSRMatrix / None"""
    rows = [list(r) for r in blocks]
    p, q = len(rows), len(rows[0]) if rows else 0
    if p < 1 or q < 1 or any(len(r) != q for r in rows):
        raise ValueError("blocks must be a rectangular table of at least one row and one column")
    flat = [b for r in rows for b in r]
    for b in flat:
        if b is not None and not isinstance(b, CSRMatrix):
            raise TypeError("a block is a CSRMatrix or None")
        if b is not None and dtype is None:
            dtype = b.dtype
    if dtype is None:
        raise ValueError("a table of None blocks has no element type")
    table = (ctypes.c_void_p * (p * q))(*[None if b is None else b._h for b in flat])
    pcoef = ctypes.c_void_p(0)
    if coef is not None:
        coef = np.ascontiguousarray(coef, dtype=dtype).reshape(-1)
        if coef.size != p * q:
            raise ValueError(f"coef has {coef.size} elements, the table has {p * q} slots")
        pcoef = _host(coef, dtype, "coef")
    return p, q, table, pcoef, np.dtype(dtype)


def _sizes(v, n, name):
    if v is None:
        return None, ctypes.c_void_p(0)
    a = np.ascontiguousarray([-1 if x is None else x for x in v], dtype=np.int32)
    if a.size != n:
        raise ValueError(f"{name} has {a.size} entries, the table has {n}")
    return a, _host(a, np.int32, name)


def bmat(blocks, coef=None, row_sizes=None, col_sizes=None, dtype=None, stream=None):
    """The block matrix of a rectangular nested list of CSRMatrix / None (a zero block), built on the device (smm_hip.h "COMPOSING and
    SLICING matrices") as a new CSRMatrix that owns its arrays: bmat([[H, Bt], [B, None]]).  coef: None or one scalar per slot (the
    entries of a slot become coef * v, one rounding; 1 copies the bits, 0 keeps stored zeros).  row_sizes / col_sizes: the heights /
    widths, needed only for a block row / column of None alone (None entries elsewhere).  dtype: needed only for a table of None alone.
    At most 64 slots.  Synchronises `stream`."""
    p, q, table, pcoef, dtype = _block_table(blocks, coef, dtype)
    keep_r, pr = _sizes(row_sizes, p, "row_sizes")
    keep_c, pc = _sizes(col_sizes, q, "col_sizes")
    h = ctypes.c_void_p()
    check(_fn("smm_hip_csr_block_create", _suffix(dtype))(p, q, table, pcoef, pr, pc, _dptr(stream), ctypes.byref(h)))
    return CSRMatrix._adopt(h, dtype)


def hstack(blocks, coef=None, stream=None):
    """[A, B, ...] side by side: bmat([blocks])"""
    return bmat([list(blocks)], coef, stream=stream)


def vstack(blocks, coef=None, stream=None):
    """[A; B; ...] one above the other: bmat([[A], [B], ...])"""
    return bmat([[b] for b in blocks], coef, stream=stream)


class AssemblyPlan:
    """The symbolic half of assembling a CSRMatrix from triplets on the device (smm_hip.h "assembling a matrix from TRIPLETS"): one list
    of (row, col) pairs sorted once; assemble / refill then turn a list of values -- values[i] belongs to pair i -- into the matrix's
    values with one gather-and-sum pass.  Repeated pairs add up in list order, bit for bit like the reference's addEntry (ref:606-618).
    A pair outside the matrix raises SmmHipError (SMM_HIP_ERR_INVALID) naming its list index."""

    def __init__(self, rows, cols, row_idx, col_idx):
        row_idx = np.ascontiguousarray(row_idx, dtype=np.int32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.int32)
        if row_idx.ndim != 1 or row_idx.shape != col_idx.shape:
            raise ValueError("row_idx and col_idx must be one-dimensional and of the same length")
        self._h = ctypes.c_void_p()
        check(_lib.load().smm_hip_assembly_create(int(rows), int(cols), row_idx.size, _host(row_idx, np.int32, "row_idx"), _host(col_idx, np.int32, "col_idx"),
                                                  ctypes.byref(self._h)))
        self._read_info()

    @classmethod
    def from_device(cls, rows, cols, n, d_row_idx, d_col_idx, stream=None):
        """n pairs in int32 device arrays (only read, not needed after the call); may synchronise `stream`"""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        check(_lib.load().smm_hip_assembly_create_dev(int(rows), int(cols), int(n), _dptr(d_row_idx), _dptr(d_col_idx), _dptr(stream), ctypes.byref(self._h)))
        self._read_info()
        return self

    def _read_info(self):
        r, c, z, l = (ctypes.c_int() for _ in range(4))
        n = ctypes.c_longlong()
        check(_lib.load().smm_hip_assembly_info(self._h, ctypes.byref(r), ctypes.byref(c), ctypes.byref(n), ctypes.byref(z), ctypes.byref(l)))
        self.rows, self.cols, self.n, self.nnz, self.longest_run = r.value, c.value, n.value, z.value, l.value

    def pattern(self):
        """(start[rows + 1], positions[nnz]) as the reference's fillArrays leaves them"""
        start = np.empty(self.rows + 1, dtype=np.int32)
        positions = np.empty(self.nnz, dtype=np.int32)
        check(_lib.load().smm_hip_assembly_pattern(self._h, _host(start, np.int32, "start"), _host(positions, np.int32, "positions")))
        return start, positions

    def _values(self, values, dtype=None):
        values = np.ascontiguousarray(values) if dtype is None else np.ascontiguousarray(values, dtype=dtype)
        if values.ndim != 1 or values.size != self.n:
            raise ValueError(f"values must hold one number per pair of the list ({self.n})")
        return values

    def assemble(self, values):
        """a new CSRMatrix of values.dtype that owns its arrays (it does not need the plan afterwards, except for refill)"""
        values = self._values(values)
        suf = _suffix(values.dtype)
        h = ctypes.c_void_p()
        check(_fn("smm_hip_assembly_csr_create", suf)(self._h, _host(values, values.dtype, "values"), ctypes.byref(h)))
        return CSRMatrix._adopt(h, values.dtype)

    def assemble_dev(self, d_values, dtype, stream=None):
        h = ctypes.c_void_p()
        check(_fn("smm_hip_assembly_csr_create_dev", _suffix(dtype))(self._h, _dptr(d_values), _dptr(stream), ctypes.byref(h)))
        return CSRMatrix._adopt(h, dtype)

    def refill(self, A, values, add=False):
        """new values for a matrix this plan created: those of assemble(values), or added to the present ones (add=True)"""
        values = self._values(values, A.dtype)
        check(_fn("smm_hip_assembly_refill", A._suf)(self._h, A._h, _host(values, A.dtype, "values"), 1 if add else 0))

    def refill_dev(self, A, d_values, add=False, stream=None):
        check(_fn("smm_hip_assembly_refill_dev", A._suf)(self._h, A._h, _dptr(d_values), 1 if add else 0, _dptr(stream)))
        A._edited(stream)

    def close(self):
        if self._h:
            _lib.load().smm_hip_assembly_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dot(a, b):
    """Vector<T>::operator* (ref:305-328)"""
    suf = _suffix(a.dtype)
    out = _CT[suf]()
    n = a.size
    check(_fn("smm_hip_dot", suf)(n, _host(a, a.dtype, "a"), _host(b, a.dtype, "b", n), ctypes.byref(out)))
    return a.dtype.type(out.value)


def dot_dev(n, d_a, d_b, d_result, dtype, stream=None):
    check(_fn("smm_hip_dot_dev", _suffix(dtype))(int(n), _dptr(d_a), _dptr(d_b), _dptr(d_result), _dptr(stream)))


def axpy_dev(n, a, d_x, d_y, d_out, dtype, stream=None):
    """out[i] = a * x[i] + y[i] on device pointers (the update loops of ref:2245-2274); out may alias x or y"""
    check(_fn("smm_hip_axpy_dev", _suffix(dtype))(int(n), float(a), _dptr(d_x), _dptr(d_y), _dptr(d_out), _dptr(stream)))


def _mh(M):
    return M._h if M is not None else ctypes.c_void_p(0)


def ConjugateGradient(a, b, x0, x, maxIterations, eps, M=None, info=None):
    """ref:2316-2398 (M = IC0 preconditioner: ref:2414-2505; a CHEBYSHEV preconditioner runs the same loop).  x may be x0.  Returns SolverStatus; `info`, when a
    dict, receives iterations and resnorm2."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_cg", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x0, a.dtype, "x0", a.rows), _host(x, a.dtype, "x", a.rows, True),
                                 int(maxIterations), a.dtype.type(eps), _mh(M), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def BiCGStab(a, b, x, maxIterations, eps, M=None, info=None):
    """ref:2191-2303.  x is the initial guess and receives the result."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_bicgstab", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                       a.dtype.type(eps), _mh(M), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm=res.value)
    return SolverStatus(st.value)


def _batch_out(suf):
    return (ctypes.c_int * MAX_RHS)(), (ctypes.c_int * MAX_RHS)(), (_CT[suf] * MAX_RHS)()


def _batch_result(k, st, it, res, info, resname, dtype):
    if info is not None:
        info.update({"iterations": np.array(it[:k], dtype=np.int32), resname: np.array(res[:k], dtype=dtype)})
    return [SolverStatus(v) for v in st[:k]]


def BiCGStabBatch(a, B, X, maxIterations, eps, M=None, info=None):
    """BiCGStab (ref:2191-2303) for the k columns of B at once -- an addition: B and X are C-contiguous (n, k) arrays, k <= MAX_RHS; X
    holds the initial guesses and receives the results.  M: None or a NONE / JACOBI / JSWEEP_SGS / JSWEEP_ILU0 preconditioner.  Column j is solved as BiCGStab
    solves it alone (its own iteration count, status and NaN behaviour).  Returns a list of k SolverStatus; `info`, when a dict,
    receives `iterations` and `resnorm` as arrays of length k."""
    suf = a._suf
    pb, k = _block(B, a.dtype, "B", a.rows)
    px, _ = _block(X, a.dtype, "X", a.rows, k, True)
    st, it, res = _batch_out(suf)
    check(_fn("smm_hip_bicgstab_batch", suf)(a._h, k, pb, px, int(maxIterations), a.dtype.type(eps), _mh(M), st, it, res))
    return _batch_result(k, st, it, res, info, "resnorm", a.dtype)


def ConjugateGradientBatch(a, B, X0, X, maxIterations, eps, info=None):
    """ConjugateGradient (ref:2316-2398) for the k columns of B at once -- an addition: B, X0 and X are C-contiguous (n, k) arrays,
    k <= MAX_RHS; X may be X0.  A column whose first residual already passes reports 0 iterations and is not written.  Returns a list
    of k SolverStatus; `info`, when a dict, receives `iterations` and `resnorm2` as arrays of length k."""
    suf = a._suf
    pb, k = _block(B, a.dtype, "B", a.rows)
    px0, _ = _block(X0, a.dtype, "X0", a.rows, k)
    px, _ = _block(X, a.dtype, "X", a.rows, k, True)
    st, it, res = _batch_out(suf)
    check(_fn("smm_hip_cg_batch", suf)(a._h, k, pb, px0, px, int(maxIterations), a.dtype.type(eps), st, it, res))
    return _batch_result(k, st, it, res, info, "resnorm2", a.dtype)


def bicgstab_batch_dev(a, k, d_b, d_x, maxIterations, eps, M=None, stream=None):
    """device-pointer BiCGStabBatch; returns ([SolverStatus] * k, iterations[k], resnorm[k]).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)  # (the library checks the range: SMM_HIP_ERR_INVALID)
    st, it, res = _batch_out(suf)
    check(_fn("smm_hip_bicgstab_batch_dev", suf)(a._h, k, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _mh(M), _dptr(stream), st, it, res))
    return [SolverStatus(v) for v in st[:k]], np.array(it[:k], dtype=np.int32), np.array(res[:k], dtype=a.dtype)


def cg_batch_dev(a, k, d_b, d_x0, d_x, maxIterations, eps, stream=None):
    """device-pointer ConjugateGradientBatch; returns ([SolverStatus] * k, iterations[k], resnorm2[k]).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)  # (the library checks the range: SMM_HIP_ERR_INVALID)
    st, it, res = _batch_out(suf)
    check(_fn("smm_hip_cg_batch_dev", suf)(a._h, k, _dptr(d_b), _dptr(d_x0), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _dptr(stream), st, it, res))
    return [SolverStatus(v) for v in st[:k]], np.array(it[:k], dtype=np.int32), np.array(res[:k], dtype=a.dtype)


def BiCGSymmetric(a, b, x, maxIterations, eps, info=None):
    """ref:2021-2102"""
    suf = a._suf
    st, it = ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_bicgsymmetric", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                            a.dtype.type(eps), ctypes.byref(st), ctypes.byref(it)))
    if info is not None:
        info.update(iterations=it.value)
    return SolverStatus(st.value)


def ConjugateGradientSquared(a, b, x, maxIterations, eps, info=None):
    """ref:2104-2178 with `residualSquared` declared before the `do` (the one repair, include/smm_hip.h).  For general matrices; x is the
    initial guess and receives the result.  The body always runs once; no breakdown test: a zero ap.r0 or rr0 leaves Inf / NaN in x.
    `info`, when a dict, receives iterations and resnorm2 (the last r.r)."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_cgs", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                  a.dtype.type(eps), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def cgs_dev(a, d_b, d_x, maxIterations, eps, stream=None):
    """device-pointer ConjugateGradientSquared; returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_cgs_dev", suf)(a._h, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _dptr(stream), ctypes.byref(st),
                                      ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


def GMRES(a, b, x, maxIterations, eps, restart=30, M=None, info=None):
    """Restarted GMRES(restart) with right preconditioning -- an addition (include/smm_hip.h states the loop).  For general matrices; x
    is the initial guess and receives the result; maxIterations < 0 means rows, with no other clamp.  M: None or any preconditioner
    BiCGStab accepts.  `info`, when a dict, receives iterations (Arnoldi steps) and resnorm2 (the last r.r)."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_gmres", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                    a.dtype.type(eps), int(restart), _mh(M), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def gmres_dev(a, d_b, d_x, maxIterations, eps, restart=30, M=None, stream=None):
    """device-pointer GMRES; returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_gmres_dev", suf)(a._h, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), int(restart), _mh(M), _dptr(stream),
                                        ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


def MINRES(a, b, x, maxIterations, eps, M=None, info=None):
    """MINRES with a symmetric positive definite preconditioner -- an addition (include/smm_hip.h states the loop).  For symmetric
    matrices, indefinite ones included; x is the initial guess and receives the result; maxIterations == -1 means rows, otherwise it is
    clamped to rows.  M: None or a preconditioner of a kind ConjugateGradient takes, created on a positive definite matrix of the same size
    (it need not be `a`).  `info`, when a dict, receives iterations and resnorm2 (the last phibar^2: the squared residual norm, in the
    M^-1-norm when M is given)."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_minres", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                     a.dtype.type(eps), _mh(M), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def minres_dev(a, d_b, d_x, maxIterations, eps, M=None, stream=None):
    """device-pointer MINRES; returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_minres_dev", suf)(a._h, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _mh(M), _dptr(stream),
                                         ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


IDRS_MAX_S = 8  # SMM_IDRS_MAX_S


def IDRs(a, b, x, maxIterations, eps, s=4, M=None, seed=0, P=None, info=None):
    """IDR(s), biorthogonal form, with right preconditioning -- an addition (include/smm_hip.h states the loop).  For general matrices; x
    is the initial guess and receives the result; maxIterations < 0 means rows, with no other clamp; 1 <= s <= IDRS_MAX_S.  M: None or any
    preconditioner GMRES accepts.  P: None (the library generates the shadow space from `seed`) or an (s, rows) array, row i the i-th
    shadow vector, used as given -- b, x and P are then staged through torch tensors on the current device and the device-pointer form
    runs.  `info`, when a dict, receives iterations (SpMVs) and resnorm2 (the last r.r)."""
    suf = a._suf
    if P is None:
        st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
        check(_fn("smm_hip_idrs", suf)(a._h, _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                       a.dtype.type(eps), int(s), _mh(M), int(seed), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
        status, iterations, resnorm2 = SolverStatus(st.value), it.value, res.value
    else:
        import torch

        _host(b, a.dtype, "b", a.rows)
        _host(x, a.dtype, "x", a.rows, True)
        P = np.asarray(P)
        if P.dtype != a.dtype or P.ndim != 2 or P.shape[1] != a.rows:
            raise TypeError(f"P must be an (s, rows) array of {a.dtype}")
        if P.shape[0] != int(s):
            raise ValueError(f"P has {P.shape[0]} shadow vectors, s is {int(s)}")
        ld = max(64, (a.rows + 63) // 64 * 64)  # the library's own layout: every column 16-byte aligned
        d_P = torch.zeros((P.shape[0], ld), dtype=torch.from_numpy(P[:0]).dtype, device="cuda")
        d_P[:, : a.rows] = torch.from_numpy(np.ascontiguousarray(P))
        d_b = torch.from_numpy(b[: a.rows]).cuda()
        d_x = torch.from_numpy(x[: a.rows]).cuda()
        torch.cuda.synchronize()
        status, iterations, resnorm2 = idrs_dev(a, d_b, d_x, maxIterations, eps, s, M, d_P, ld, seed)
        x[: a.rows] = d_x.cpu().numpy()
    if info is not None:
        info.update(iterations=iterations, resnorm2=resnorm2)
    return status


def idrs_dev(a, d_b, d_x, maxIterations, eps, s=4, M=None, d_P=None, ldP=0, seed=0, stream=None):
    """device-pointer IDR(s); d_P: None (generated from `seed`) or s columns of `rows` elements, column i at d_P + i * ldP, read only.
    Returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_idrs_dev", suf)(a._h, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), int(s), _mh(M), _dptr(d_P), int(ldP), int(seed),
                                       _dptr(stream), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


def idrs_shadow_dev(n, s, seed, d_P, ld, dtype, stream=None):
    """fills d_P (s columns of n elements of `dtype`, column i at d_P + i * ld) with the shadow space the library generates from `seed`:
    the hash of include/smm_hip.h made orthonormal.  Synchronises `stream`."""
    check(_fn("smm_hip_idrs_shadow_dev", _suffix(dtype))(int(n), int(s), int(seed), _dptr(d_P), int(ld), _dptr(stream)))


REFINE_INNER_CG, REFINE_INNER_BICGSTAB, REFINE_INNER_GMRES = 0, 1, 2
_REFINE_INNER = {"CG": REFINE_INNER_CG, "BICGSTAB": REFINE_INNER_BICGSTAB, "GMRES": REFINE_INNER_GMRES}


def _refine_inner(inner):
    return _REFINE_INNER[inner.upper()] if isinstance(inner, str) else int(inner)


def IterativeRefinement(a, b, x, eps, inner="CG", a32=None, M=None, maxOuter=20, maxInner=-1, innerEps=1e-4, restart=30, info=None):
    """Mixed-precision iterative refinement -- an addition (include/smm_hip.h states the loop): an fp64 answer from fp32 solves.  `a` is a
    float64 CSRMatrix, b and x float64 vectors (x is the initial guess and receives the result); every outer step takes the true fp64
    residual, solves for a correction in fp32 with `inner` ("CG", "BICGSTAB", "GMRES" or a REFINE_INNER_* code) on a32 and accepts it only
    if the true residual falls.  a32: a.astype(np.float32), kept by callers that solve more than once; None converts for this call (M
    must be None then).  M: None or a preconditioner of a32 of a kind the inner solver takes.  A rejected step or an error leaves x bit
    for bit.  Returns SolverStatus; `info`, when a dict, receives outer_iterations, inner_iterations and resnorm2 (the true ||b - A x||^2)."""
    st, outer, it, res = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    check(_lib.load().smm_hip_refine_f64(a._h, _mh(a32), _host(b, np.float64, "b", a.rows), _host(x, np.float64, "x", a.rows, True), _refine_inner(inner),
                                         int(maxOuter), int(maxInner), float(eps), float(innerEps), int(restart), _mh(M), ctypes.byref(st), ctypes.byref(outer),
                                         ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(outer_iterations=outer.value, inner_iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def refine_dev(a, d_b, d_x, eps, inner="CG", a32=None, M=None, maxOuter=20, maxInner=-1, innerEps=1e-4, restart=30, stream=None):
    """device-pointer IterativeRefinement; returns (SolverStatus, outer_iterations, inner_iterations, resnorm2).  Synchronises `stream`."""
    st, outer, it, res = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    check(_lib.load().smm_hip_refine_dev_f64(a._h, _mh(a32), _dptr(d_b), _dptr(d_x), _refine_inner(inner), int(maxOuter), int(maxInner), float(eps),
                                             float(innerEps), int(restart), _mh(M), _dptr(stream), ctypes.byref(st), ctypes.byref(outer), ctypes.byref(it),
                                             ctypes.byref(res)))
    return SolverStatus(st.value), outer.value, it.value, res.value


def multi_dot_dev(n, k, d_V, ld, d_w, d_out, dtype, stream=None):
    """d_out[i] = v_i . w for the k columns of V (column i at d_V + i * ld) on device pointers; asynchronous"""
    check(_fn("smm_hip_multi_dot_dev", _suffix(dtype))(int(n), int(k), _dptr(d_V), int(ld), _dptr(d_w), _dptr(d_out), _dptr(stream)))


def multi_axpy_dev(n, k, d_V, ld, d_coef, d_w, d_out, dtype, stream=None):
    """d_out = d_w + sum_i d_coef[i] v_i, i ascending through _smm_fma, on device pointers; d_out may alias d_w; asynchronous"""
    check(_fn("smm_hip_multi_axpy_dev", _suffix(dtype))(int(n), int(k), _dptr(d_V), int(ld), _dptr(d_coef), _dptr(d_w), _dptr(d_out), _dptr(stream)))


def multi_rotate_dev(n, m, l, d_V, ld, Y, dtype, stream=None):
    """V[:, :l] = V[:, :m] @ Y in place on a device pointer (m columns of n elements, column i at d_V + i * ld); Y: an (m, l) HOST array
    of `dtype`.  Each output is formed j ascending through _smm_fma; the columns l .. m-1 keep their bits.  Synchronises `stream`."""
    Y = np.asarray(Y)
    if Y.dtype != np.dtype(dtype) or Y.shape != (int(m), int(l)):
        raise TypeError(f"Y must be an ({m}, {l}) array of {np.dtype(dtype)}")
    Yf = np.asfortranarray(Y)  # element (i, c) at i + c * m
    check(_fn("smm_hip_multi_rotate_dev", _suffix(dtype))(int(n), int(m), int(l), _dptr(d_V), int(ld), Yf.ctypes.data_as(ctypes.c_void_p), int(m), _dptr(stream)))


EIGSH_LARGEST, EIGSH_SMALLEST = 0, 1  # SMM_EIGSH_LARGEST, SMM_EIGSH_SMALLEST
EIGSH_MAX_NCV = 64  # SMM_EIGSH_MAX_NCV
_EIGSH_WHICH = {"LA": EIGSH_LARGEST, "SA": EIGSH_SMALLEST}
EigshInfo = collections.namedtuple("EigshInfo", "residuals nconv restarts matvecs status")


def _eigsh_which(which):
    if isinstance(which, str):
        try:
            return _EIGSH_WHICH[which.upper()]
        except KeyError:
            raise ValueError(f"which must be 'LA' (largest algebraic) or 'SA' (smallest algebraic), got {which!r}")
    return int(which)


def eigsh(a, k=6, which="LA", ncv=None, tol=0.0, max_restarts=300, v0=None, seed=0, return_eigenvectors=True):
    """The k algebraically largest ("LA") or smallest ("SA") eigenvalues of the symmetric CSRMatrix `a`, with their eigenvectors, by
    thick-restart Lanczos on the device -- an addition (include/smm_hip.h states the algorithm).  ncv: basis columns, k + 2 <= ncv <=
    min(rows, EIGSH_MAX_NCV); None means min(rows, max(2k + 1, 20)).  tol <= 0 means the machine epsilon of the dtype; the test is
    rho_i <= tol * max|theta|.  v0: a start vector, or None for the hash vector of `seed`.  Returns (w, X, info), or (w, info) with
    return_eigenvectors=False: w in the order of `which` (descending for "LA", ascending for "SA"), X of shape (rows, k) with the
    eigenvectors in its columns, info an EigshInfo(residuals, nconv, restarts, matvecs, status).  When status is not SUCCESS the pairs are
    the best available.  No shift-invert, no interior eigenvalues, and not preconditioned: lobpcg is."""
    suf = a._suf
    k = int(k)
    w = np.zeros(max(k, 0), dtype=a.dtype)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    X = np.zeros((max(k, 0), a.rows), dtype=a.dtype) if return_eigenvectors else None  # row i: eigenvector i (column-major (rows, k))
    nconv, restarts, matvecs, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_eigsh", suf)(a._h, k, _eigsh_which(which), 0 if ncv is None else int(ncv), int(max_restarts), a.dtype.type(tol),
                                    None if v0 is None else _host(v0, a.dtype, "v0", a.rows), int(seed), w.ctypes.data_as(ctypes.c_void_p),
                                    None if X is None else X.ctypes.data_as(ctypes.c_void_p), a.rows, res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv),
                                    ctypes.byref(restarts), ctypes.byref(matvecs), ctypes.byref(st)))
    info = EigshInfo(res, nconv.value, restarts.value, matvecs.value, SolverStatus(st.value))
    return (w, X.T, info) if return_eigenvectors else (w, info)


def eigsh_dev(a, k, which, d_w, d_X, ldx, ncv=None, tol=0.0, max_restarts=300, d_v0=None, seed=0, stream=None):
    """device-pointer eigsh: d_w receives the k eigenvalues, d_X (may be None) eigenvector i at d_X + i * ldx; d_v0: None or a start
    vector on the device.  Returns an EigshInfo (residuals: a host array).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    nconv, restarts, matvecs, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_eigsh_dev", suf)(a._h, k, _eigsh_which(which), 0 if ncv is None else int(ncv), int(max_restarts), a.dtype.type(tol), _dptr(d_v0), int(seed),
                                        _dptr(d_w), _dptr(d_X), int(ldx), _dptr(stream), res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv),
                                        ctypes.byref(restarts), ctypes.byref(matvecs), ctypes.byref(st)))
    return EigshInfo(res, nconv.value, restarts.value, matvecs.value, SolverStatus(st.value))


SVDS_MAX_NCV = 64  # SMM_SVDS_MAX_NCV
SvdsInfo = collections.namedtuple("SvdsInfo", "residuals nconv restarts matvecs status")


def svds(a, k=6, ncv=0, tol=0.0, max_restarts=300, v0=None, seed=0, at=None, vectors=True):
    """The k largest singular values of the CSRMatrix `a` (any shape), with their left and right singular vectors, by thick-restart
    Golub-Kahan-Lanczos bidiagonalisation on the device -- an addition (include/smm_hip.h states the algorithm).  It works on `a` and
    its transpose, never on their product.  ncv: basis columns, k + 2 <= ncv <= min(rows, cols, SVDS_MAX_NCV); 0 means
    min(rows, cols, max(2k + 1, 20)).  tol <= 0 means the machine epsilon of the dtype; the test is rho_i <= tol * sigma_0.  v0: a start
    vector of a.cols elements, or None for the hash vector of `seed`.  at=None builds a transpose for the duration of the solve,
    at=a.transpose() keeps one, at=a asserts symmetry (square matrices only); that `at` is the transpose is trusted.  Returns
    (U, s, V, info): s descending, U of shape (rows, k) and V of shape (cols, k) with the vectors in their columns -- both None with
    vectors=False --, info an SvdsInfo(residuals, nconv, restarts, matvecs, status).  When status is not SUCCESS the triplets are the best
    available.  Not the smallest singular values, no shift, no block method."""
    suf = a._suf
    k = int(k)
    s = np.zeros(max(k, 0), dtype=a.dtype)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    U = np.zeros((max(k, 0), a.rows), dtype=a.dtype) if vectors else None  # row i: left vector i (column-major (rows, k))
    V = np.zeros((max(k, 0), a.cols), dtype=a.dtype) if vectors else None
    nconv, restarts, matvecs, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_svds", suf)(a._h, _mh(at), k, int(ncv or 0), int(max_restarts), a.dtype.type(tol), None if v0 is None else _host(v0, a.dtype, "v0", a.cols),
                                   int(seed), s.ctypes.data_as(ctypes.c_void_p), None if U is None else U.ctypes.data_as(ctypes.c_void_p), a.rows,
                                   None if V is None else V.ctypes.data_as(ctypes.c_void_p), a.cols, res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv),
                                   ctypes.byref(restarts), ctypes.byref(matvecs), ctypes.byref(st)))
    info = SvdsInfo(res, nconv.value, restarts.value, matvecs.value, SolverStatus(st.value))
    return (U.T, s, V.T, info) if vectors else (None, s, None, info)


def svds_dev(a, k, d_s, d_U, ldu, d_V, ldv, ncv=0, tol=0.0, max_restarts=300, d_v0=None, seed=0, at=None, stream=None):
    """device-pointer svds: d_s receives the k singular values, d_U (may be None) left vector i at d_U + i * ldu, d_V (may be None) right
    vector i at d_V + i * ldv; d_v0: None or a start vector of a.cols elements on the device.  Returns an SvdsInfo (residuals: a host
    array).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    nconv, restarts, matvecs, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_svds_dev", suf)(a._h, _mh(at), k, int(ncv or 0), int(max_restarts), a.dtype.type(tol), _dptr(d_v0), int(seed), _dptr(d_s), _dptr(d_U), int(ldu),
                                       _dptr(d_V), int(ldv), _dptr(stream), res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv), ctypes.byref(restarts),
                                       ctypes.byref(matvecs), ctypes.byref(st)))
    return SvdsInfo(res, nconv.value, restarts.value, matvecs.value, SolverStatus(st.value))


LOBPCG_MAX_K, LOBPCG_MAX_BASIS = 8, 24  # SMM_LOBPCG_MAX_K, SMM_LOBPCG_MAX_BASIS
LOBPCG_MAX_BASES = 3  # SMM_LOBPCG_MAX_BASES
LobpcgInfo = collections.namedtuple("LobpcgInfo", "residuals nconv iterations matvecs applies status")
LobpcgGenInfo = collections.namedtuple("LobpcgGenInfo", LobpcgInfo._fields + ("bmatvecs",))


def lobpcg(a, k=4, which="SA", M=None, X0=None, tol=0.0, max_iterations=1000, seed=0, return_eigenvectors=True, B=None):
    """The k algebraically smallest ("SA") or largest ("LA") eigenvalues of the symmetric CSRMatrix `a`, with their eigenvectors, by
    LOBPCG on the device -- the preconditioned block method, an addition (include/smm_hip.h states the loop).  1 <= k <= LOBPCG_MAX_K
    with 3k <= rows.  M: None or a symmetric positive definite preconditioner (any kind ConjugateGradient takes, or JACOBI or SGS) of a matrix of the same
    size, which need not be `a`: a shifted L - sigma I takes the preconditioner of L; with "LA" an M is legal but seldom useful.  X0:
    None for the hash columns of `seed`, or a (rows, k) start block.  tol <= 0 means the machine epsilon of the dtype; column j has
    converged when ||A x_j - theta_j x_j|| <= tol * max|theta|.  Returns (w, X, info), or (w, info) with return_eigenvectors=False: w in
    the order of `which`, X of shape (rows, k), info a LobpcgInfo(residuals, nconv, iterations, matvecs, applies, status).  When status
    is MAX_ITERATIONS_REACHED the pairs are the best available; when it is DIVERGED they are not written.
    B: None, or a symmetric positive definite CSRMatrix of the same size and dtype: the GENERALISED problem A x = lambda B x (K x =
    lambda M x with a mass matrix: the vibration modes).  Column j has then converged when ||A x_j - theta_j B x_j|| <= tol *
    max|theta| * ||B x_j||, X is B-orthonormal (X^T B X = I), M still approximates A^-1, and info is a LobpcgGenInfo: LobpcgInfo's
    fields and bmatvecs, the products with B."""
    suf = a._suf
    k = int(k)
    w = np.zeros(max(k, 0), dtype=a.dtype)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    X = np.zeros((max(k, 0), a.rows), dtype=a.dtype) if return_eigenvectors else None  # row j: eigenvector j (column-major (rows, k))
    start = None
    if X0 is not None:
        X0 = np.asarray(X0)
        if X0.dtype != a.dtype or X0.shape != (a.rows, k):
            raise TypeError(f"X0 must be a ({a.rows}, {k}) array of {a.dtype}")
        start = np.ascontiguousarray(X0.T)  # row j: start column j
    nconv, its, matvecs, bmatvecs, applies, st = (ctypes.c_int() for _ in range(6))
    head = (k, _eigsh_which(which), int(max_iterations), a.dtype.type(tol), _mh(M), None if start is None else start.ctypes.data_as(ctypes.c_void_p), a.rows, int(seed),
            w.ctypes.data_as(ctypes.c_void_p), None if X is None else X.ctypes.data_as(ctypes.c_void_p), a.rows, res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv),
            ctypes.byref(its), ctypes.byref(matvecs))
    if B is None:
        check(_fn("smm_hip_lobpcg", suf)(a._h, *head, ctypes.byref(applies), ctypes.byref(st)))
        info = LobpcgInfo(res, nconv.value, its.value, matvecs.value, applies.value, SolverStatus(st.value))
    else:
        check(_fn("smm_hip_lobpcg_gen", suf)(a._h, B._h, *head, ctypes.byref(bmatvecs), ctypes.byref(applies), ctypes.byref(st)))
        info = LobpcgGenInfo(res, nconv.value, its.value, matvecs.value, applies.value, SolverStatus(st.value), bmatvecs.value)
    return (w, X.T, info) if return_eigenvectors else (w, info)


def lobpcg_dev(a, k, which, d_w, d_X, ldx, M=None, d_X0=None, ldx0=0, tol=0.0, max_iterations=1000, seed=0, stream=None):
    """device-pointer lobpcg: d_w receives the k eigenvalues, d_X (may be None) eigenvector j at d_X + j * ldx; d_X0: None or k start
    columns on the device, column j at d_X0 + j * ldx0.  Returns a LobpcgInfo (residuals: a host array).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    nconv, its, matvecs, applies, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_fn("smm_hip_lobpcg_dev", suf)(a._h, k, _eigsh_which(which), int(max_iterations), a.dtype.type(tol), _mh(M), _dptr(d_X0), int(ldx0), int(seed), _dptr(d_w),
                                         _dptr(d_X), int(ldx), _dptr(stream), res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv), ctypes.byref(its),
                                         ctypes.byref(matvecs), ctypes.byref(applies), ctypes.byref(st)))
    return LobpcgInfo(res, nconv.value, its.value, matvecs.value, applies.value, SolverStatus(st.value))


def lobpcg_gen_dev(a, B, k, which, d_w, d_X, ldx, M=None, d_X0=None, ldx0=0, tol=0.0, max_iterations=1000, seed=0, stream=None):
    """device-pointer lobpcg for A x = lambda B x: lobpcg_dev's arguments with the CSRMatrix B after `a` (None: the standard problem, the
    bits of lobpcg_dev, bmatvecs 0).  Returns a LobpcgGenInfo (residuals: a host array).  Synchronises `stream`."""
    suf = a._suf
    k = int(k)
    res = np.zeros(max(k, 0), dtype=a.dtype)
    nconv, its, matvecs, bmatvecs, applies, st = (ctypes.c_int() for _ in range(6))
    check(_fn("smm_hip_lobpcg_gen_dev", suf)(a._h, _mh(B), k, _eigsh_which(which), int(max_iterations), a.dtype.type(tol), _mh(M), _dptr(d_X0), int(ldx0), int(seed),
                                             _dptr(d_w), _dptr(d_X), int(ldx), _dptr(stream), res.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nconv),
                                             ctypes.byref(its), ctypes.byref(matvecs), ctypes.byref(bmatvecs), ctypes.byref(applies), ctypes.byref(st)))
    return LobpcgGenInfo(res, nconv.value, its.value, matvecs.value, applies.value, SolverStatus(st.value), bmatvecs.value)


def _dptr_array(items):
    """a host array of device pointers (None entries are null pointers)"""
    return (ctypes.c_void_p * len(items))(*[_dptr(t) for t in items])


def multi_block_axpy_bases_dev(n, m, l, d_V, ldV, d_H, ldH, d_W, ldW, dtype, stream=None):
    """multi_block_axpy_dev on the pairs (d_V[i], d_W[i]) of two equally long sequences of 1 .. LOBPCG_MAX_BASES device pointers with one
    d_H, in ONE launch; every pair gets the bits of multi_block_axpy_dev alone.  No V may overlap any W.  Asynchronous."""
    if len(d_V) != len(d_W):
        raise ValueError("d_V and d_W must hold as many bases")
    check(_fn("smm_hip_multi_block_axpy_bases_dev", _suffix(dtype))(int(n), int(m), int(l), len(d_V), _dptr_array(d_V), int(ldV), _dptr(d_H), int(ldH), _dptr_array(d_W),
                                                                    int(ldW), _dptr(stream)))


def multi_rotate_bases_dev(n, m, l, d_V, ld, Y, dtype, stream=None):
    """multi_rotate_dev on every basis of the sequence d_V (1 .. LOBPCG_MAX_BASES device pointers) with one (m, l) HOST array Y, staged
    once, in ONE launch; every basis gets the bits of multi_rotate_dev alone.  Synchronises `stream`."""
    Y = np.asarray(Y)
    if Y.dtype != np.dtype(dtype) or Y.shape != (int(m), int(l)):
        raise TypeError(f"Y must be an ({m}, {l}) array of {np.dtype(dtype)}")
    Yf = np.asfortranarray(Y)  # element (i, c) at i + c * m
    check(_fn("smm_hip_multi_rotate_bases_dev", _suffix(dtype))(int(n), int(m), int(l), len(d_V), _dptr_array(d_V), int(ld), Yf.ctypes.data_as(ctypes.c_void_p), int(m),
                                                                _dptr(stream)))


def multi_gram_dev(n, m, l, d_V, ldV, d_W, ldW, d_G, ldG, dtype, stream=None):
    """d_G (m x l, column-major, leading dimension ldG, on the device) = V^T W for m columns of V and l of W (column i at d_V + i * ldV);
    d_W may be d_V (the symmetric case).  Fixed-order sums: two calls give the same bits.  Asynchronous."""
    check(_fn("smm_hip_multi_gram_dev", _suffix(dtype))(int(n), int(m), int(l), _dptr(d_V), int(ldV), _dptr(d_W), int(ldW), _dptr(d_G), int(ldG), _dptr(stream)))


def multi_block_axpy_dev(n, m, l, d_V, ldV, d_H, ldH, d_W, ldW, dtype, stream=None):
    """W[:, c] -= sum_j H[j][c] V[:, j], j ascending through _smm_fma, for the l columns of W; d_H: m x l, column-major, on the device.
    V and W must not overlap.  Asynchronous."""
    check(_fn("smm_hip_multi_block_axpy_dev", _suffix(dtype))(int(n), int(m), int(l), _dptr(d_V), int(ldV), _dptr(d_H), int(ldH), _dptr(d_W), int(ldW), _dptr(stream)))


def BiCG(a, b, x, maxIterations, eps, at=None, info=None):
    """BiCG for general matrices: BiCGSymmetric's text (ref:2021-2102) with the shadow sequence on `at`, the transpose (a.transpose()).
    at=None builds one for the duration of the solve; at=a asserts symmetry and gives BiCGSymmetric's bits.  That `at` is the transpose
    is trusted.  x is the initial guess and receives the result; `info`, when a dict, receives iterations and resnorm2 (the last r.r)."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_bicg", suf)(a._h, _mh(at), _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.rows, True), int(maxIterations),
                                   a.dtype.type(eps), ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    if info is not None:
        info.update(iterations=it.value, resnorm2=res.value)
    return SolverStatus(st.value)


def bicg_dev(a, d_b, d_x, maxIterations, eps, at=None, stream=None):
    """device-pointer BiCG; returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_bicg_dev", suf)(a._h, _mh(at), _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _dptr(stream), ctypes.byref(st),
                                       ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


def LSQR(a, b, x, maxIterations, eps, damp=0.0, at=None, info=None):
    """LSQR for min ||a x - b|| with a matrix of any shape -- an addition (include/smm_hip.h states the loop).  b has a.rows elements, x
    has a.cols, is the initial guess and receives the result; maxIterations < 0 means cols, with no other clamp.  The stop tests are
    absolute: eps against the estimates of ||b - a x|| (reason 1) and of ||at (b - a x)|| (reason 2, how an inconsistent system ends).
    damp > 0 damps the correction x - x0.  at=None builds a transpose for the duration of the solve, at=a.transpose() keeps one, at=a
    asserts symmetry (square matrices only); that `at` is the transpose is trusted.  `info`, when a dict, receives iterations, reason,
    resnorm2 and arnorm2 (the two squared estimates)."""
    suf = a._suf
    st, it, why, res, arn = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), _CT[suf](), _CT[suf]()
    check(_fn("smm_hip_lsqr", suf)(a._h, _mh(at), _host(b, a.dtype, "b", a.rows), _host(x, a.dtype, "x", a.cols, True), int(maxIterations),
                                   a.dtype.type(eps), a.dtype.type(damp), ctypes.byref(st), ctypes.byref(it), ctypes.byref(why), ctypes.byref(res),
                                   ctypes.byref(arn)))
    if info is not None:
        info.update(iterations=it.value, reason=why.value, resnorm2=res.value, arnorm2=arn.value)
    return SolverStatus(st.value)


def lsqr_dev(a, d_b, d_x, maxIterations, eps, damp=0.0, at=None, stream=None):
    """device-pointer LSQR (d_b: a.rows elements, d_x: a.cols); returns (SolverStatus, iterations, reason, resnorm2, arnorm2).
    Synchronises `stream`."""
    suf = a._suf
    st, it, why, res, arn = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), _CT[suf](), _CT[suf]()
    check(_fn("smm_hip_lsqr_dev", suf)(a._h, _mh(at), _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), a.dtype.type(damp), _dptr(stream),
                                       ctypes.byref(st), ctypes.byref(it), ctypes.byref(why), ctypes.byref(res), ctypes.byref(arn)))
    return SolverStatus(st.value), it.value, why.value, res.value, arn.value


def cg_dev(a, d_b, d_x0, d_x, maxIterations, eps, M=None, stream=None):
    """device-pointer CG; returns (SolverStatus, iterations, resnorm2).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_cg_dev", suf)(a._h, _dptr(d_b), _dptr(d_x0), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _mh(M), _dptr(stream),
                                     ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


CG_RESIDENT_OFF, CG_RESIDENT_AUTO, CG_RESIDENT_REQUIRE = 0, 1, 2


def cg_resident(mode=-1):
    """sets (0 off, 1 auto, 2 require) or only queries (-1) the register-resident CG path; returns the previous mode"""
    return int(_lib.load().smm_hip_cg_resident(int(mode)))


def set_cg_lazy_x_min_bytes(nbytes):
    """test / measurement knob: bytes per vector from which CG defers its x update (negative: the default, 64 MB)"""
    check(_lib.load().smm_hip_set_cg_lazy_x_min_bytes(int(nbytes)))


def set_cg_fuse_p(on):
    """test / measurement knob: False keeps CG from forming its next direction inside the 2.5-D SpMV kernel"""
    check(_lib.load().smm_hip_set_cg_fuse_p(1 if on else 0))


def bicgstab_resident(mode=-1):
    """sets (0 off, 1 auto, 2 require) or only queries (-1) the single-launch BiCGStab path; returns the previous mode"""
    return int(_lib.load().smm_hip_bicgstab_resident(int(mode)))


def bicgstab_dev(a, d_b, d_x, maxIterations, eps, M=None, stream=None):
    """device-pointer BiCGStab; returns (SolverStatus, iterations, resnorm).  Synchronises `stream`."""
    suf = a._suf
    st, it, res = ctypes.c_int(), ctypes.c_int(), _CT[suf]()
    check(_fn("smm_hip_bicgstab_dev", suf)(a._h, _dptr(d_b), _dptr(d_x), int(maxIterations), a.dtype.type(eps), _mh(M), _dptr(stream),
                                           ctypes.byref(st), ctypes.byref(it), ctypes.byref(res)))
    return SolverStatus(st.value), it.value, res.value


# ---- device-side generators (csrc/smm_gen.hip) ------------------------------------------------------------
def gen_banded_nnz(n, k=25, seed=0x5EED, max_offset=1 << 20):
    return int(_lib.load().smm_hip_gen_banded_nnz(int(n), int(k), int(seed), int(max_offset)))


def gen_poisson2d_nnz(nx, ny):
    return int(_lib.load().smm_hip_gen_poisson2d_nnz(int(nx), int(ny)))


def gen_stencil3d_nnz(nx, ny, nz):
    return int(_lib.load().smm_hip_gen_stencil3d_nnz(int(nx), int(ny), int(nz)))


def gen_banded_dev(n, k, seed, max_offset, d_start, d_positions, d_values, dtype, stream=None, diag_shift=1.0):
    check(_fn("smm_hip_gen_banded_dev", _suffix(dtype))(int(n), int(k), int(seed), int(max_offset), np.dtype(dtype).type(diag_shift), _dptr(d_start), _dptr(d_positions), _dptr(d_values), _dptr(stream)))


def gen_banded_row_start(n, k, seed, max_offset, row):
    """start[row] of the full banded matrix in closed form (no device needed)"""
    return int(_lib.load().smm_hip_gen_banded_row_start(int(n), int(k), int(seed), int(max_offset), int(row)))


def gen_banded_rows_dev(n, k, seed, max_offset, diag_shift, row_begin, row_end, d_start, d_positions, d_values, dtype, stream=None):
    """rows [row_begin, row_end) of the banded matrix: local start[], GLOBAL columns (what one rank owns)"""
    check(_fn("smm_hip_gen_banded_rows_dev", _suffix(dtype))(int(n), int(k), int(seed), int(max_offset), np.dtype(dtype).type(diag_shift),
                                                               int(row_begin), int(row_end), _dptr(d_start), _dptr(d_positions), _dptr(d_values),
                                                               _dptr(stream)))


def gen_poisson2d_dev(nx, ny, d_start, d_positions, d_values, dtype, stream=None):
    check(_fn("smm_hip_gen_poisson2d_dev", _suffix(dtype))(int(nx), int(ny), _dptr(d_start), _dptr(d_positions), _dptr(d_values), _dptr(stream)))


def gen_stencil3d_dev(nx, ny, nz, diag, lo, hi, d_start, d_positions, d_values, dtype, stream=None):
    t = np.dtype(dtype).type
    check(_fn("smm_hip_gen_stencil3d_dev", _suffix(dtype))(int(nx), int(ny), int(nz), t(diag), t(lo), t(hi), _dptr(d_start), _dptr(d_positions),
                                                            _dptr(d_values), _dptr(stream)))
