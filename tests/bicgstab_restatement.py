"""BiCGStab restated on the CPU, line for line after the reference's text (ref:2191-2283): the unpreconditioned overload and the template
with a Jacobi preconditioner (x = rhs / diag) plugged in.

A helper, not a test: this is the definition the long-run audit of the GPU drivers (tests/test_gpu_bicgstab_long.py) is compared with,
and oracle/gen_golden_v5.py runs it to record tests/golden/bicgstab_long_v5.npz.  With `dot = sequential` and the oracle's SpMV it is
oracle.bicgstab bit for bit (tests/test_bicgstab_restatement_cpu.py), and the oracle is pinned to the reference.

What can be chosen is what a parallel machine is free to choose: the working dtype and HOW A GLOBAL SUM IS FORMED (`dot`).  Everything
else is fixed: the row sums are `spmv` (the oracle's: the reference's row arithmetic), the element-wise lines are NumPy in the working
dtype written so that every operation rounds once -- _smm_fma's default a * x + b (ref:28-36) is two roundings, as the oracle has them
under -ffp-contract=off.  (With the SMM_WITH_STD_FMA flavour those lines cannot be reproduced bit for bit in NumPy.)

The `dot` variants -- together the ENSEMBLE:
  sequential   oracle.dot: one accumulator, left to right (ref:322-326)
  pairwise     numpy's pairwise fp sum of the rounded products
  fp64acc      products and sum in fp64, rounded once to the working dtype
  chunked      fixed chunks of 512 rows summed left to right, then the chunk sums summed left to right: a partition in the style of
               the GPU's (one partial per workgroup, the partials added in order)"""
import numpy as np

OP_ASSIGN, OP_SUB = 0, 2
SUCCESS, MAX_ITERATIONS_REACHED = 0, 2
CHUNK = 512
HISTORY_FIELDS = ("rho", "alpha", "omega", "beta", "resnorm", "xnorm")


def _fma(a, x, b):
    """_smm_fma's default form (ref:28-36): a * x + b, two roundings"""
    t = a * x
    return t + b


def dot_sequential(oracle):
    def dot(a, b):
        return oracle.dot(a, b)

    return dot


def dot_pairwise(a, b):
    return np.sum(a * b, dtype=a.dtype)


def dot_fp64acc(a, b):
    """(np.sum, not np.dot: NumPy's own pairwise sum adds in the same order on every machine, a BLAS need not)"""
    return a.dtype.type(np.sum(a.astype(np.float64) * b.astype(np.float64)))


def dot_chunked(a, b, chunk=CHUNK):
    """the products rounded to the working dtype (as the sequential sum has them), `chunk` rows per partial, every sum left to right
    (np.cumsum adds one element after the other; the zeros that fill the last chunk change no sum)"""
    prod = a * b
    n = len(prod)
    nchunks = -(-n // chunk)
    padded = np.zeros(nchunks * chunk, dtype=a.dtype)
    padded[:n] = prod
    partials = np.cumsum(padded.reshape(nchunks, chunk), axis=1, dtype=a.dtype)[:, -1]
    return a.dtype.type(np.cumsum(partials, dtype=a.dtype)[-1]) if nchunks else a.dtype.type(0)


def norm2(v):
    """||v||_2 accumulated in fp64 (NumPy's pairwise sum: the same bits on every machine)"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.sqrt(np.sum(v * v)))


def scipy_matrix(csr):
    """A in fp64 (scipy.sparse.csr_matrix) for the true residuals"""
    import scipy.sparse as sp

    start, pos, val = csr
    rows = len(start) - 1
    nnz = int(start[-1])
    return sp.csr_matrix((val[:nnz].astype(np.float64), pos[:nnz], start), shape=(rows, rows))


def true_residual(A64, b, x, diag=None):
    """t = ||b - A x||_2 in fp64 -- of the system the recurrence residual belongs to: with the Jacobi template r is the preconditioned
    residual from ref:2217-2224 on, so t = ||D^-1 (b - A x)||_2 there"""
    d = np.asarray(b, dtype=np.float64) - A64 @ np.asarray(x, dtype=np.float64)
    if diag is not None:
        d = d / np.asarray(diag, dtype=np.float64)
    return norm2(d)


def residual_gap_bounds(dtype, A64, resnorm, xnorm):
    """bound_k = u k (longest row + 4) (||A||_inf max_{j<=k} ||x_j||_2 + max_{j<=k} resnorm_j), k = 1 ... len(resnorm): the standard
    bound of the gap between the recurrence residual and b - A x_k (every iteration adds two roundings of an update of x and the
    rounding errors of two row sums of at most `longest row` terms; Greenbaum 1997, Theorem 1).  Non-finite entries propagate."""
    u = float(np.finfo(dtype).eps)
    longest = int(np.diff(A64.indptr).max())
    norm_a = float(abs(A64).sum(axis=1).max())
    k = np.arange(1, len(resnorm) + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        return u * k * (longest + 4) * (norm_a * np.maximum.accumulate(np.asarray(xnorm, dtype=np.float64))
                                        + np.maximum.accumulate(np.asarray(resnorm, dtype=np.float64)))


def dot_variants(oracle):
    """name -> dot(a, b): the ensemble, in a fixed order"""
    return {"sequential": dot_sequential(oracle), "pairwise": dot_pairwise, "fp64acc": dot_fp64acc, "chunked": dot_chunked}


def bicgstab(oracle, csr, b, x0, max_iterations, eps, diag=None, dtype=None, dot=None, spmv=None, keep_x=False, on_x=None):
    """returns (status, x, iterations, resnorm, history); x0 is not modified.
    diag     None: the unpreconditioned overload (ref:2294-2303); else the Jacobi template: every preconditioner application is rhs / diag
    dtype    the working dtype of the vectors and the scalars (default: the matrix's; the matrix is converted to it)
    dot      dot(a, b) -> scalar: how a global sum is formed (default: the oracle's sequential one)
    spmv     spmv(csr, op, lhs, x) -> out (default: oracle.spmv)
    history  dict of arrays, one entry per pass through the body: rho (r.r0 the pass starts with), alpha, omega, beta, resnorm (the
             recurrence residual the loop condition reads) and xnorm (||x_k||_2, accumulated in fp64); with keep_x also "x", the list
             of the x_k.  on_x(k, x_k) is called after pass k (x_k must not be kept: copy it)"""
    start, pos, val = csr
    dt = np.dtype(val.dtype if dtype is None else dtype)
    T = dt.type
    if val.dtype != dt:
        csr = (start, pos, val.astype(dt))
    dot = dot_sequential(oracle) if dot is None else dot
    spmv = oracle.spmv if spmv is None else spmv
    rows = len(start) - 1
    eps = T(eps)
    x = np.array(x0, dtype=dt, copy=True)
    b = np.ascontiguousarray(b, dtype=dt)
    max_iterations = min(int(max_iterations), rows)  # ref:2200
    if max_iterations == -1:  # ref:2201-2203
        max_iterations = rows
    if diag is not None:
        diag = np.ascontiguousarray(diag, dtype=dt)

    def apply_a(v):
        """ref:2233-2241 / 2249-2257: A v, then the preconditioner"""
        av = spmv(csr, OP_ASSIGN, None, v)
        return av if diag is None else av / diag

    history = {f: [] for f in HISTORY_FIELDS}
    xs = []
    with np.errstate(all="ignore"):  # no breakdown test (ref:2260, 2270): 0 / 0 and x / 0 go into x as in the reference
        r = spmv(csr, OP_SUB, b, x)  # ref:2215
        if diag is not None:  # ref:2217-2227
            r = r / diag
        r0, p = r.copy(), r.copy()
        res = T(0)
        iterations = 0
        rr0 = T(dot(r, r0))  # ref:2231
        while True:  # do {
            ap = apply_a(p)
            denom = T(dot(ap, r0))  # ref:2243
            alpha = T(rr0 / denom)
            s = _fma(-alpha, ap, r)  # ref:2245-2247
            as_ = apply_a(s)
            denom = T(dot(as_, as_))  # ref:2259
            omega = T(T(dot(as_, s)) / denom)  # ref:2261
            x = _fma(alpha, p, _fma(omega, s, x))  # ref:2264
            r = _fma(-omega, as_, s)  # ref:2265
            res = T(np.sqrt(T(dot(r, r))))  # ref:2266, 2268
            new_rr0 = T(dot(r, r0))  # ref:2269
            beta = T(T(new_rr0 * alpha) / T(rr0 * omega))  # ref:2271
            p = _fma(beta, _fma(-omega, ap, p), r)  # ref:2272-2274
            for f, v in zip(HISTORY_FIELDS, (rr0, alpha, omega, beta, res, norm2(x))):
                history[f].append(v)
            rr0 = new_rr0
            iterations += 1
            if keep_x:
                xs.append(x.copy())
            if on_x is not None:
                on_x(iterations, x)
            if not (res > eps and iterations < max_iterations):  # } while (...), ref:2277
                break
    history = {f: np.array(history[f], dtype=np.float64 if f == "xnorm" else dt) for f in HISTORY_FIELDS}
    if keep_x:
        history["x"] = xs
    status = MAX_ITERATIONS_REACHED if iterations > max_iterations else SUCCESS  # ref:2279-2282
    return status, x, iterations, res, history
