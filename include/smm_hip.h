/*
 * smm_hip.h -- C ABI of libsmm_hip.so: the MI355X (gfx950) implementation of the CSR SpMV + Krylov inner
 * loop behind SMM::ConjugateGradient / SMM::BiCGStab over SMM::CSRMatrix
 * (vasil-pashov/sparse_matrix_math v0.2.0, include/sparse_matrix_math.h -- cited below as "ref").
 *
 * The reference is a header-only C++ template library with no FFI seam, so this header
 * IS the drop-in boundary: plain pointers and sizes, no C++ / torch types.  Each entry point names the
 * reference interface it replaces.  include/smm_hip/sparse_matrix_math.h layers the reference's own C++
 * signatures (SMM::CSRMatrix<T>::rMult, SMM::ConjugateGradient, SMM::BiCGStab, ...) on top of these calls;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns an int shim status: SMM_HIP_OK (0) or a negative SMM_HIP_ERR_* code.  Nothing
 *     throws.  The reference's own SolverStatus (ref:2010-2014) is returned through *solver_status.
 *   - `_f32` / `_f64` select T = float / double (the reference's template parameter).  Index arrays are
 *     int32 exactly as in the reference (ref:1243-1259).
 *   - functions without `_dev` take HOST pointers, like the reference's API: they copy in, run on the GPU,
 *     copy out and synchronise before returning.
 *   - `_dev` functions take DEVICE pointers and a hipStream_t (as void*, NULL = the null stream); they only enqueue
 *     work unless they must return a value to the host (solvers synchronise the stream before returning their
 *     status).  Temporaries are recycled in stream order: drive one matrix from one stream at a time.
 *     Host-pointer functions run on a private non-blocking stream of the library.
 *   - pointers: an array needs the alignment of its ELEMENT type only (4 bytes for int / float, 8 for double) -- host or device, the
 *     arrays smm_hip_csr_create_dev_* borrows included.  A view into the middle of a larger allocation (several matrices packed into
 *     one buffer, a slice of a vector) is a valid argument and gives the bits of the same call on an allocation of its own.  No call
 *     reads or writes outside [p, p + n) of an array of n elements.  tests/test_gpu_device_views.py holds both.
 *   - there is NO CPU fallback: without a HIP device every call fails with SMM_HIP_ERR_NO_DEVICE.
 *   - rounding: multiply-adds are a*x+b (two roundings) like the reference's default _smm_fma (ref:28-36);
 *     a library built with -DSMM_WITH_STD_FMA uses fma(a,x,b) instead.  smm_hip_uses_std_fma() tells which.
 */
#ifndef SMM_HIP_H
#define SMM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMM_HIP_VERSION_MAJOR 0
#define SMM_HIP_VERSION_MINOR 1

/* shim status */
#define SMM_HIP_OK 0
#define SMM_HIP_ERR_INVALID (-1)   /* bad argument (null pointer, dtype mismatch, negative size, aliasing x==out) */
#define SMM_HIP_ERR_HIP (-2)       /* HIP runtime failure; text in smm_hip_last_error() */
#define SMM_HIP_ERR_NO_DEVICE (-3) /* no HIP device / smm_hip_init not possible */
#define SMM_HIP_ERR_PRECOND (-4)   /* structural failure in a preconditioner (missing / tiny diagonal, empty row): the
                                      reference's non-zero return of apply()/init() (ref:1668-1693) */
#define SMM_HIP_ERR_NOMEM (-5)
#define SMM_HIP_ERR_COMM (-6)      /* multi-GPU communicator failure (RCCL error, missing librccl, failed host callback) */

/* SolverStatus, ref:2010-2014 */
#define SMM_SOLVER_SUCCESS 0
#define SMM_SOLVER_DIVERGED 1
#define SMM_SOLVER_MAX_ITERATIONS_REACHED 2

/* SpMV op: rMult / rMultAdd / rMultSub, ref:1501-1515 */
#define SMM_OP_ASSIGN 0 /* out = A*x          */
#define SMM_OP_ADD 1    /* out = lhs + A*x    */
#define SMM_OP_SUB 2    /* out = lhs - A*x    */

/* Preconditioner kinds.  NONE = IDPreconditioner (ref:1166-1170), SGS = SGSPreconditioner (ref:1173-1186,
 * SolverPreconditioner::SYMMETRIC_GAUS_SEIDEL ref:1002-1006).  JACOBI is absent from the reference and ILU0 is
 * declared but unusable there (ref:1189-1212, 1715-1790); both are additions (BASELINE.json north_star).
 * IC0 = IC0Preconditioner (ref:1216-1235), used by the preconditioned ConjugateGradient overload. */
#define SMM_PRECOND_NONE 0
#define SMM_PRECOND_JACOBI 1
#define SMM_PRECOND_ILU0 2
#define SMM_PRECOND_SGS 3
#define SMM_PRECOND_IC0 4
/* Block-diagonal forms (additions, no counterpart in the reference).  The rows are cut into contiguous blocks; M is the ILU0 /
 * SGS preconditioner of the block-diagonal part of A: an entry that couples two blocks is dropped from M only (the solver keeps
 * multiplying with all of A).  Inside a block the arithmetic is the global preconditioner's, entry for entry -- BLOCK_SGS is
 * SGSPreconditioner::apply (ref:1658-1713) of the block-diagonal matrix, and with one block covering all rows both kinds give the
 * global preconditioner's bits.  What it buys on MI355X: a block is factorised and swept by ONE wavefront out of LDS, all blocks at
 * once, one launch per apply -- no dependency chain across the chip (csrc/smm_precond_block.hip). */
#define SMM_PRECOND_BLOCK_ILU0 5
#define SMM_PRECOND_BLOCK_SGS 6
/* Chebyshev polynomial in D^-1 A, D the stored diagonal taken with its sign (an addition; csrc/smm_precond_cheb.hip, the definition line
 * by line is tests/chebyshev_restatement.py).  With bounds 0 < lambda_min < lambda_max on the spectrum of D^-1 A and a degree d >= 0:
 *   theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma
 *   rho_k = 1 / (2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = 2 rho_k / delta      (double, on the host, each cast to T once)
 *   z = M^-1 r:  d = (r / diag) * T(1 / theta);  z = d                                              (degree 0: a scaled Jacobi)
 *                k = 1 .. d:  q = r - A z;  t = q / diag;  u = c2_k * t;  d = _smm_fma(c1_k, d, u);  z = z + d
 * q = r - A z is the library's SpMV in whatever kernel family the matrix runs; every element-wise operation rounds once in T.  I - M^-1 A
 * has the eigenvalues T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma): the spectrum inside [lmin, lmax] is damped uniformly.  d SpMVs
 * and d + 1 element-wise passes per apply, no dependency chain between rows, no inner product.  M^-1 is symmetric positive definite
 * when A is (and lambda_min > 0): ConjugateGradient accepts it, as do BiCGStab and GMRES.  smm_hip_precond_create(a, 7, &M) means
 * degree 3, GERSHGORIN, eig_ratio 30; smm_hip_precond_create_chebyshev below takes every parameter. */
#define SMM_PRECOND_CHEBYSHEV 7
/* Smoothed-aggregation multigrid with a symmetric V-cycle (an addition; csrc/smm_precond_amg.hip, the definition line by line is
 * tests/amg_restatement.py).  Integer results are exact; values are bit for bit wherever the parts they come from are.
 * Per level l, from A_l with n rows (A_0 = a); every row needs a stored diagonal with |d| >= 1e-5 (else SMM_HIP_ERR_PRECOND):
 *   strength   a stored entry (i, j), j != i, is strong iff a_ij^2 >= ((theta_l^2 |a_ii|) |a_jj|) in double, theta_l = theta 0.5^l.
 *              N(i) = the columns of row i's strong entries, as stored, not symmetrised.
 *   roots      a distance-2 maximal independent set in synchronous rounds.  Every row starts undecided (state 1; 2 = root, 0 = not a root).
 *              The key of row i is (state, h(i), i), compared lexicographically, h = the 32-bit murmur3 finaliser of i + 1
 *              (h ^= h>>16; h *= 0x85ebca6b; h ^= h>>13; h *= 0xc2b2ae35; h ^= h>>16).  In a round K1_i = max(K_i, max_{j in N(i)} K_j), then
 *              K2_i = max(K1_i, max_{j in N(i)} K1_j), each from the previous array as a whole.  An undecided row whose K2 carries its own
 *              index becomes a root; otherwise an undecided row whose K2 has state 2 becomes a non-root.  Rounds repeat until no row is
 *              undecided.  Roots are numbered in ascending row order.
 *   aggregates phase 1: a non-root with a root in N(i) joins the root with the smallest number.  Phase 2: a row still unassigned joins the
 *              smallest aggregate number among the assigned members of N(i); each pass works from the previous assignment as a whole and
 *              passes repeat until one assigns nothing.  Rows still unassigned become aggregates of their own, numbered after the roots
 *              in ascending row order.  n_c = the number of aggregates.
 *   operators  T is n x n_c with one entry 1 per row.  S = I - omega D^-1 A_l on A_l's pattern, omega = 4 / (3 lambda), lambda the
 *              Gershgorin bound of D^-1 A_l as the Chebyshev kind computes it: s = T(omega) / d_i, an off-diagonal entry is -(s a_ij), the
 *              diagonal entry 1 - s a_ii, every operation rounding once.  P_l = S T, R_l = P_l^T, A_{l+1} = R_l (A_l P_l) by
 *              smm_hip_csr_multiply_create and smm_hip_csr_transpose_create; each is an ordinary smm_hip_csr.
 *   smoother   M_l = the Chebyshev preconditioner of A_l: degree smooth_degree, GERSHGORIN, eig_ratio.
 * Level l is the coarsest when n <= coarse_rows, or l + 1 == max_levels, or the level would not shrink (10 n_c >= 9 n).  A coarsest level
 * of more than 1024 rows: SMM_HIP_ERR_PRECOND, the message names the level sizes.  With max_levels 1 or rows <= coarse_rows the
 * preconditioner is the dense solve alone.  Coarsest level: A_L is copied to the host once, inverted in double by Gauss-Jordan with
 * partial pivoting (a pivot that is zero or not finite: SMM_HIP_ERR_PRECOND), rounded to T once and kept dense on the device; an apply is
 * one launch, one wavefront per row: lane k sums columns k, k + 64, ... in ascending order from +0.0 with _smm_fma, the 64 partial sums
 * are combined by the xor butterfly (32, 16, ... 1) of the dot kernels.
 * The cycle V_l(b), every step a device operation:
 *   x = M_l b;  r = b - A_l x;  r_c = R_l r;  e_c = V_{l+1}(r_c);  x = x + P_l e_c;  r = b - A_l x;  d = M_l r;  x = x + d
 * (the SpMVs with OP_SUB, OP_ASSIGN, OP_ADD in whatever kernel family the level's matrix runs).  z = M^-1 r is V_0(r): a fixed linear
 * operator, symmetric positive definite when A is (the Gershgorin bound keeps the Chebyshev residual polynomial below 1 on (0, lambda]).
 * Launches only: no host round trip, no allocation; every launch honours the solver's done flag.  ConjugateGradient (symmetric positive
 * definite matrices only), BiCGStab and GMRES accept it; the batched, row-partitioned and single-launch paths refuse it or are not
 * taken.  smm_hip_precond_create(a, 8, &M) means theta 0.08, max_levels 10, coarse_rows 256, smooth_degree 2, eig_ratio 30. */
#define SMM_PRECOND_AMG 8
/* MULTICOLOR_SGS / _ILU0 / _IC0 -- additions: the exact kind on a MULTICOLOUR REORDERING of the matrix (csrc/smm_precond_mc.hip; the
 * definition, line by line, is tests/multicolor_restatement.py).
 *   colours = smm_hip_csr_color(a) (or the caller's, smm_hip_precond_create_multicolor); perm = the rows sorted by colour, stably (the
 *   original index ascends inside a colour); B = P A Pᵀ (smm_hip_csr_permute_create); for ILU0 / IC0 the factor of B;
 *   M^-1 r = Pᵀ sweeps_B(P r), sweeps_B being the two sweeps of SGS / ILU0 / IC0 on B -- bit for bit the sequential sweeps on B.
 * Rows of one colour do not reference each other, so either sweep has exactly `ncolors` dependent levels (smm_hip_precond_info reports
 * them) -- a handful on a grid, where the natural order has hundreds.  The price is convergence: a solver typically needs somewhat more
 * iterations than with the exact kind in the natural order (INTEGRATION.md "Multicolour ordering").
 * Accepted wherever the exact kind is (smm_hip_bicgstab_*, smm_hip_gmres_*, the refinement driver's inner solves: MULTICOLOR_SGS and
 * MULTICOLOR_ILU0); smm_hip_cg_* takes MULTICOLOR_IC0 and MULTICOLOR_SGS, both symmetric positive definite when A is.  Batched and
 * row-partitioned solvers and smm_hip_precond_apply_spmv_* refuse the kinds (SMM_HIP_ERR_INVALID).
 * Errors of create: those of the exact kind (SMM_HIP_ERR_PRECOND for a missing / tiny diagonal, an empty row, a failed pivot;
 * SMM_HIP_ERR_INVALID for a matrix that is not square).  The handle owns B and the vector the sweeps work on, so ONE HANDLE MUST NOT BE
 * APPLIED FROM TWO STREAMS AT ONCE.  It is a SNAPSHOT, MULTICOLOR_SGS included: it does not follow a value edit of `a` -- call
 * smm_hip_precond_multicolor_refresh.  smm_hip_precond_values_* returns the ILU0 / IC0 factor on B's pattern (nnz values). */
#define SMM_PRECOND_MULTICOLOR_SGS 9
#define SMM_PRECOND_MULTICOLOR_ILU0 10
#define SMM_PRECOND_MULTICOLOR_IC0 11
/* FSAI and SPAI -- additions: preconditioners that ARE sparse matrices, so an apply is the library's SpMV (csrc/smm_precond_ainv.hip; the
 * definition, line by line, is tests/ainv_restatement.py).  FSAI is for symmetric positive definite matrices: M^-1 = G^T G with G lower
 * triangular and diag(G A G^T) = 1.  SPAI is for general matrices: M ~ A^-1, row i minimising ||e_i^T - m_i A||_2 over a fixed pattern.
 *   pattern   Pat = a for power 1; for power p > 1 the structural product of p copies of a (smm_hip_csr_multiply_create; only the pattern
 *             is used).  J_i = the distinct columns of row i of Pat, ascending; FSAI keeps the columns <= i only.  n = |J_i|.  i not in J_i
 *             (a missing diagonal) and n > SMM_AINV_MAX_ROW are SMM_HIP_ERR_PRECOND; the message names the row (for n > 64 also n and the
 *             power; a row of Pat whose columns do not ascend and that holds more than 64 distinct ones is reported by its stored entries).
 *   source    look(X, r, c) = the value of the FIRST stored entry of row r of X with column c, +0.0 when there is none.
 *             FSAI: Src = a, b = e_{n-1} (the 1 stands at i, the last of J_i).
 *             SPAI: At = smm_hip_csr_transpose_create(a), Src = N = a At (smm_hip_csr_multiply_create), b[p] = look(At, i, J[p]).
 *             S[p][q] = look(Src, J[p], J[q]) for q <= p; the upper triangle is never read.
 *   solve     in the matrix dtype T, every operation rounding once, s - l m written _smm_fma(-l, m, s):
 *               j = 0 .. n-1:  d = S[j][j]; not (d > 0) or not finite: the row FAILS; S[j][j] = sqrt(d)
 *                              i > j:              S[i][j] = S[i][j] / S[j][j]
 *                              i > j, j < k <= i:  S[i][k] = S[i][k] - S[i][j] S[k][j]
 *               j = 0 .. n-1:  y[j] = b[j] / S[j][j];  i > j:  b[i] = b[i] - S[i][j] y[j]
 *               j = n-1 .. 0:  y[j] = y[j] / S[j][j];  i < j:  y[i] = y[i] - S[j][i] y[j]
 *             FSAI: row i of G on the columns J_i = y / sqrt(y[n-1]).  SPAI: row i of M on the columns J_i = y.
 *             Every entry is updated in ascending j and nothing is summed across lanes: the bits are those of the sequential loops.
 *             A failed row makes create and refresh return SMM_HIP_ERR_PRECOND naming the smallest such row: the matrix is not symmetric
 *             positive definite (FSAI), or has dependent rows or is too ill-conditioned for T (SPAI solves NORMAL EQUATIONS: the condition
 *             number of the row systems is that of a squared; fine for diagonally dominant matrices, fragile in fp32 otherwise).
 *   result    G (or M) is an ordinary smm_hip_csr on the pattern J; Gt = smm_hip_csr_transpose_create(G).  The handle owns both.
 *   apply     FSAI: w = G r, z = Gt w.  SPAI: z = M r.  The library's SpMV with SMM_OP_ASSIGN in whatever kernel family those matrices run.
 *             Launches only, every launch honours the solver's done flag, and the kind itself allocates nothing in an apply; w belongs to
 *             the handle, so ONE HANDLE MUST NOT BE APPLIED FROM TWO STREAMS AT ONCE.  What an SpMV of any matrix builds lazily on its
 *             first launch in a kernel family (the tile table, the PATTERN analysis and its copies) is built by the first apply after
 *             create, after smm_hip_csr_set_kernel on a borrowed handle, and re-verified after ainv_refresh, as for any other matrix.
 * smm_hip_cg_* accepts FSAI (G^T G is symmetric positive definite whenever the create succeeded) and refuses SPAI (SMM_HIP_ERR_INVALID);
 * smm_hip_bicgstab_*, smm_hip_gmres_* and the refinement driver's inner solves (the handle made on the fp32 matrix) accept both;
 * smm_hip_precond_apply_spmv_* runs the SpMV and then the apply.  The batched, row-partitioned and single-launch paths refuse both kinds or
 * are not taken, as for AMG.  smm_hip_precond_info reports 0 levels; smm_hip_precond_values_* returns the nnz values of G (FSAI) or M (SPAI).
 * Memory: G and Gt (FSAI), or M, a^T and a a^T (SPAI; both kept for the refresh: about 7 + 25 entries per row for a 7-point stencil beside
 * M's own 7 / 25 / 63 at power 1 / 2 / 3), each entry sizeof(T) + 4 bytes, Gt and a^T 4 more for the transpose's permutation.
 * It is a SNAPSHOT: it does not follow a value edit of `a` -- call smm_hip_precond_ainv_refresh.
 * smm_hip_precond_create(a, 12 | 13, &M) means power 1. */
#define SMM_PRECOND_FSAI 12
#define SMM_PRECOND_SPAI 13
/* JSWEEP_SGS / _ILU0 / _IC0 -- additions: the exact kind's factor in the NATURAL numbering, each of its two triangular solves replaced by
 * a fixed number of JACOBI STEPS, i.e. a truncated Neumann series of the triangular factor (csrc/smm_precond_jsweep.hip; the definition,
 * line by line, is tests/jsweep_restatement.py).  The factor, the create-time checks and the errors are the exact kind's.
 *   row walk   the exact sweep's arithmetic of one row: acc = start(own); for the entries of the row's triangular part in the stored order
 *              (lower: from the row's start while col < row; upper: from the row's end backwards while col > row)
 *              acc = term(acc, value, y[col]); result = finish(acc, own, d), d the diagonal entry of the swept values:
 *                SGS lower  start = own      term = _smm_fma(-value, y, acc)   finish = acc / d        (values: a)
 *                SGS upper  start = 0        term = _smm_fma(value, y, acc)    finish = own - acc / d
 *                ILU lower  start = own      term = _smm_fma(-value, y, acc)   finish = acc            (values: the ILU0 factor)
 *                ILU upper  start = own      term = _smm_fma(-value, y, acc)   finish = acc / d
 *                IC  both   start = own      term = acc - value * y            finish = acc / d        (values: the IC0 factor)
 *   step       the row walk for ALL rows at once, every y[col] read from the PREVIOUS iterate.  Iterate 0 is the walk with no terms,
 *              finish(start(own), own, d): own itself for ILU lower, own / d for SGS / IC lower and ILU / IC upper, own for SGS upper.
 *   apply      lower phase: own = rhs, sweeps_lower steps.  Upper phase: own = the lower phase's last iterate, sweeps_upper steps.
 * A fixed, linear, deterministic operator.  Two properties:
 *   EXACTNESS  after k steps every row of dependency level <= k (levels counted from 0) holds the exact sweep's bits and keeps them, so
 *              with sweeps_lower >= levels_lower - 1 and sweeps_upper >= levels_upper - 1 the apply equals the exact kind's bit for bit
 *              (the levels are what smm_hip_precond_info reports for the exact kind, and for these kinds).
 *   SYMMETRY   with sweeps_lower == sweeps_upper the IC0 form is P^T P and the SGS form is symmetric for symmetric a: smm_hip_cg_* takes
 *              JSWEEP_IC0 and JSWEEP_SGS then, and refuses them (SMM_HIP_ERR_INVALID) with unequal counts.  Positive definiteness is
 *              P^T P's for IC0; for SGS with few steps it is the caller's to judge (a truncated series of a definite operator).
 * No in-kernel wait of any sort: an apply is sweeps_lower + sweeps_upper launches shaped like an SpMV over one triangle (one more for
 * SGS / IC0, an element-wise pass), every launch honours the solver's done flag, every step writes every row exactly once.  A step reads
 * its triangle only: nnz_tri (4 + sizeof T) bytes + 4 rows of row pointers + the vectors.
 * smm_hip_bicgstab_*, smm_hip_gmres_*, smm_hip_idrs_*, smm_hip_cgs_*, smm_hip_bicg_* and the refinement driver's inner solves take
 * JSWEEP_SGS and JSWEEP_ILU0 with any counts, and so does smm_hip_bicgstab_batch_* (every column goes through the apply on its own, the
 * dot products the SpMM would have fused are formed afterwards).  The row-partitioned solvers, smm_hip_precond_apply_spmv_* and
 * smm_hip_precond_set_sweep refuse the kinds (SMM_HIP_ERR_INVALID).  smm_hip_precond_values_* returns the ILU0 / IC0 factor on a's
 * pattern (nnz values; JSWEEP_SGS holds none, like SGS).  The iterates live in two vectors per stream the handle is applied on (the exact
 * kinds' rule: at most 8 streams are kept), so applies on several streams and from several host threads are allowed.
 * Memory: the exact factor (nnz values, kept for the refresh), the split triangles (nnz - rows entries of 4 + sizeof T bytes, 2 rows + 2
 * row pointers, rows diagonal values) and, for ILU0 / IC0, the lower sweep's level schedule (rows + levels integers: the refresh factorises over it).  It is a SNAPSHOT, JSWEEP_SGS included: it does not follow a
 * value edit of `a` -- call smm_hip_precond_jsweep_refresh.  smm_hip_precond_create(a, 14 | 15 | 16, &M) means 3 / 3 steps. */
#define SMM_PRECOND_JSWEEP_SGS 14
#define SMM_PRECOND_JSWEEP_ILU0 15
#define SMM_PRECOND_JSWEEP_IC0 16

#define SMM_DTYPE_F32 0
#define SMM_DTYPE_F64 1
#define SMM_DTYPE_I64 2 /* only as the element type handed to smm_hip_host_allreduce_fn */

/* SpMV kernel families (smm_hip_csr_set_kernel).  AUTO picks from nnz/row, and for large matrices tries PATTERN (below). */
#define SMM_SPMV_AUTO 0
#define SMM_SPMV_VECTOR 1 /* L lanes of a wavefront per row, wave shuffle reduction */
#define SMM_SPMV_STREAM 2 /* row blocks staged through LDS with 16-byte coalesced loads, row-sequential sums */
/* For matrices whose entries take their columns from a limited set of offsets relative to the row (stencil, banded and band-numbered
 * mesh matrices).  positions[] (4 bytes per entry) is replaced, in one of two encodings (smm_hip_csr_pattern_info tells which):
 *   MASKS  <= 64 distinct offsets and rows of <= 64 entries: one 64-bit mask per ROW, verified against EVERY entry on the device before
 *          the family is used; an SpMV streams only values[] (half the bytes for fp32);
 *          When in addition every entry of a diagonal holds the same value (constant-coefficient stencils: the Laplacians) -- CONST --
 *          values[] is not read either: 24 bytes per fp64 row instead of 104 -- 20 for grid-shaped matrices of >= 2^21 rows, which run the
 *          2.5-D kernel (csrc/smm_spmv_march.hip: a plane's window of x in LDS, the planes above and below in registers, 32-bit masks);
 *   CODES  <= 65536 distinct offsets: one 16-bit index into the matrix's sorted offset dictionary per ENTRY (6 instead of 8 bytes per
 *          fp32 entry), built on the device from all entries.
 * Same result bit for bit as the other families at the same lanes_per_row.  Selected explicitly (smm_hip_csr_set_kernel returns
 * SMM_HIP_ERR_INVALID when the matrix fits neither encoding) or by AUTO: the first SpMV of a matrix with >= 2^25 stored entries and
 * <= 64 entries per row on average runs the analysis once, on the caller's stream, and switches the matrix over when it passes
 * (smm_hip_csr_get_kernel then reports SMM_SPMV_PATTERN); a matrix that does not fit stays with STREAM.
 * Environment: SMM_HIP_AUTO_PATTERN=0 keeps AUTO on STREAM, SMM_HIP_AUTO_PATTERN_MIN_NNZ moves the threshold, SMM_HIP_AUTO_DICT=0 keeps
 * AUTO from using the CODES encoding, SMM_HIP_PATTERN_CONST=0 turns the constant-diagonal form off. */
#define SMM_SPMV_PATTERN 3
#define SMM_PATTERN_NONE 0  /* smm_hip_csr_pattern_info: not analysed, or the matrix fits neither encoding */
#define SMM_PATTERN_MASKS 1
#define SMM_PATTERN_CODES 2
#define SMM_PATTERN_CONST 3 /* MASKS, and every diagonal holds one value (verified bit for bit against every entry): with one lane per
                             * row an SpMV reads the row's mask, x and <= 32 numbers -- no positions[], no values[] (the Laplacians) */

/* For matrices that are a sparse matrix of dense b x b blocks, b = 2, 3 or 4 (vector-valued problems on unstructured meshes: elasticity,
 * Stokes, shells, multi-species transport).  A matrix fits block size b when rows and cols are multiples of b, the b rows of every block
 * row R (rows R b .. R b + b - 1) hold the same number of entries, a multiple of b (0 is allowed), the k-th group of b entries of each of
 * those rows has the columns c, c + 1, .. c + b - 1 with c a multiple of b, the same c in all b rows, and a row holds at most
 * max_row_entries entries (smm_hip_csr_blocks_info; 2048 / 1365 / 1024 for b = 2 / 3 / 4: the b rows of a block row fit one tile of 4096
 * entries).  Explicitly stored zeros count as entries.  Every entry is checked on the device (smm_hip_csr_find_blocks).  positions[] is
 * then replaced by ONE column index per block -- 4 / b^2 bytes per entry instead of 4 -- and the b entries of x a block needs are read once
 * for its b rows.  values[] is read in place: every value edit is seen at once.  One lane per block row; same result bit for bit as
 * STREAM at one lane per row (the reference's order).  Opt-in only: AUTO and smm_hip_csr_autotune never choose it;
 * smm_hip_csr_set_kernel(m, SMM_SPMV_BLOCKS, 0 or 1) runs the analysis if none is kept and returns SMM_HIP_ERR_INVALID -- the handle
 * keeps its kernel -- when no size fits. */
#define SMM_SPMV_BLOCKS 4

/* For matrices with a few very long rows among ordinary ones (a dense constraint row of a KKT system, the dense row the transpose of a
 * global regressor column is, the hub rows of a graph Laplacian).  The other families give such a row to one wavefront; this one cuts it
 * into segments that all compute units sum at once, and a second launch adds the segment sums up.  One lane per short row.
 * THE ARITHMETIC IS A FIXED FUNCTION OF THE ROW'S ENTRIES, split_len AND segment_len (smm_hip_csr_longrows_info) and of nothing else --
 * not of where the row sits in values[], the grid, the device, op, dot_mode or which workgroup ends first; no floating-point atomics:
 *   a row of at most split_len entries   d = 0; d = fma(v[k], x[p[k]], d) for k in stored order -- the reference's sum (ref:1484-1489), the
 *                                        bits of STREAM at one lane per row;
 *   a longer row                         is cut into segments of segment_len entries counted from the row's own first entry (the last one
 *                                        may be shorter).  Segment: 64 chains c[l] = 0; c[l] = fma(v[j], x[p[j]], c[l]) over the segment's
 *                                        entries j = l, l + 64, l + 128, ... in ascending order (a chain without entries stays 0); then
 *                                        six butterfly steps o = 32, 16, 8, 4, 2, 1: c[l] = c[l] + c[l xor o] for all l at once; the
 *                                        segment's sum is c[0].  Row: d = 0; d = d + (sum of segment i) for i ascending.
 * fma(a, x, b) is a * x + b with two roundings in libsmm_hip.so and one in libsmm_hip_fma.so, as everywhere.  The three ops, the fused dot
 * products with their partial-sum slots and the device-pointer contract are STREAM's.  values[] is read in place and the analysis
 * depends on start[] only: value edits need no refresh.  Opt-in only: AUTO and smm_hip_csr_autotune never choose it.
 * smm_hip_csr_set_kernel(m, SMM_SPMV_LONGROWS, 0 or 1) runs the analysis if none is kept and succeeds for every valid matrix (one
 * without long rows is served too: it costs one launch, like STREAM); another lane count is SMM_HIP_ERR_INVALID and the handle keeps
 * its kernel. */
#define SMM_SPMV_LONGROWS 5
#define SMM_LONGROWS_SPLIT_MIN 1
#define SMM_LONGROWS_SPLIT_MAX 2045 /* what the row kernel's tile of one lane per row holds in both precisions */
#define SMM_LONGROWS_SPLIT_DEFAULT 1024
#define SMM_LONGROWS_SEGMENT_MIN 64 /* segment_len is a multiple of 64 */
#define SMM_LONGROWS_SEGMENT_MAX 2048
#define SMM_LONGROWS_SEGMENT_DEFAULT 1024

typedef struct smm_hip_csr smm_hip_csr;         /* device-resident CSRMatrix<T> (ref:1243-1259) */
typedef struct smm_hip_precond smm_hip_precond; /* device-resident preconditioner */
typedef void* smm_hip_stream;                   /* hipStream_t with HIP's own meaning: NULL = the null (default) stream */

/* ---- runtime ------------------------------------------------------------------------------------------- */
/* Select the HIP device this process uses (one process per GPU) and create the library stream.  Idempotent. */
int smm_hip_init(int device);
int smm_hip_shutdown(void);
/* Text of the last failure on the calling thread ("" if none). */
const char* smm_hip_last_error(void);
int smm_hip_uses_std_fma(void);
/* name: device name (may be NULL), cus: compute units, hbm_bytes: total device memory */
int smm_hip_device_info(char* name, size_t name_cap, int* cus, size_t* hbm_bytes);
/* Blocks until everything enqueued on `stream` has finished. */
int smm_hip_stream_synchronize(smm_hip_stream stream);

/* TEST HOOK: the next device allocation of the library of at least min_bytes bytes fails ONCE with SMM_HIP_ERR_NOMEM, as if the device
 * were full (0 disarms it).  What the tests use to check that an optional step which cannot get its memory -- the automatic PATTERN
 * analysis -- leaves the caller's SpMV / solve untouched. */
int smm_hip_debug_fail_next_alloc(size_t min_bytes);
/* ---- live kernel timing (bench.py roofline) ------------------------------------------------------------------
 * When enabled every SpMV launch -- standalone or inside a solver loop -- is bracketed by a pair of HIP events on the
 * stream it is launched on.  smm_hip_profile_read waits for the recorded events, returns the summed SpMV kernel time
 * in milliseconds and the number of launches since the last reset, and optionally resets the tally. */
int smm_hip_profile_enable(int on);
int smm_hip_profile_read(double* spmv_ms, long long* spmv_launches, int reset);
/* The row-partitioned SpMV (smm_hip_dist_*): while profiling is on, every halo exchange leaves a pair of events -- the end of the local
 * block A_loc on the caller's stream, the end of the exchange on the communicator's stream.  exposed_ms = the sum over the pairs of
 * max(0, exchange end - A_loc end): the part of the exchanges the local block did NOT cover; pairs = the number of exchanges. */
int smm_hip_profile_read_waits(double* exposed_ms, long long* pairs, int reset);

/* ---- CSRMatrix<T> (ref:1243-1259; replaces CSRMatrix::init(TripletMatrix) ref:1326-1349 as the way in) ---- */
/* Copies the three host arrays of a CSRMatrix (values[nnz], positions[nnz] ascending per row, start[rows+1])
 * to the device.  The host arrays stay owned by the caller. */
int smm_hip_csr_create_f32(int rows, int cols, const int* start, const int* positions, const float* values, smm_hip_csr** out);
int smm_hip_csr_create_f64(int rows, int cols, const int* start, const int* positions, const double* values, smm_hip_csr** out);
/* Wraps arrays that already live in device memory (no copy; the caller keeps them alive, and start[] / positions[] unchanged).  The
 * values may change: through the edit calls below, or written by the caller followed by smm_hip_csr_values_changed_*. */
int smm_hip_csr_create_dev_f32(int rows, int cols, const int* d_start, const int* d_positions, const float* d_values, smm_hip_csr** out);
int smm_hip_csr_create_dev_f64(int rows, int cols, const int* d_start, const int* d_positions, const double* d_values, smm_hip_csr** out);
int smm_hip_csr_destroy(smm_hip_csr* m);
/* getDenseRowCount / getDenseColCount / getNonZeroCount (ref:1351-1364) + dtype + firstActiveStart (ref:1619-1628) */
int smm_hip_csr_info(const smm_hip_csr* m, int* rows, int* cols, int* nnz, int* dtype, int* first_active_start);
/* Force a SpMV kernel family / lanes-per-row (0 = heuristic).  Tuning knob, not needed for correctness. */
int smm_hip_csr_set_kernel(smm_hip_csr* m, int family, int lanes_per_row);
int smm_hip_csr_get_kernel(const smm_hip_csr* m, int* family, int* lanes_per_row);
/* The STREAM family's tile table as the last SpMV built it (0 tiles before the first SpMV or for the other families): number of
 * tiles, the nonzeros / rows a tile was cut for, and whether the launches go to spmvTileKernel (1: the pieces of a row in different
 * waves -- 2 or 4 lanes per row, the benchmark matrix) or to the pipelined spmvStreamKernel (0).  Diagnostics for tests and benches. */
int smm_hip_csr_tile_info(const smm_hip_csr* m, int* tiles, int* tile_nnz_cap, int* tile_max_rows, int* tile_kernel);
/* The PATTERN family's encoding of this matrix (SMM_PATTERN_*) and the number of distinct offsets it found; NONE / 0 before the
 * analysis has run (the first SpMV of a large matrix, or smm_hip_csr_set_kernel(m, SMM_SPMV_PATTERN, ...)). */
int smm_hip_csr_pattern_info(const smm_hip_csr* m, int* encoding, int* offsets);
/* Which kernel the next SpMV of this matrix launches and what one launch of it has to move: `name` receives the kernel's template name
 * as a profiler prints it, without the template arguments ("spmvTileKernel", "spmvPatternTileKernel", "spmvPatternConstKernel" ...;
 * name_cap bytes, always terminated); *bytes_per_launch the bytes of the layout THAT kernel reads and writes once -- for the CSR
 * kernels SURVEY section 8d's B_spmv = nnz (s + 4) + (rows + 1) 4 + cols s + rows s, for the PATTERN encodings what they store instead of
 * positions[] (8 bytes per row of mask; 2 bytes per entry of code; no values[] for CONST) + start[] where the kernel reads it + x +
 * out.  Benchmarks price a kernel's launch time with THIS number, never with another layout's.  Diagnostics, like tile_info. */
int smm_hip_csr_kernel_desc(const smm_hip_csr* m, char* name, int name_cap, long long* bytes_per_launch);
/* The BLOCKS family's analysis (SMM_SPMV_BLOCKS above).  A synchronous set-up call, like smm_hip_csr_set_kernel(m, SMM_SPMV_PATTERN, ..).
 * block_size 2, 3 or 4 tests that size; 0 tries 4, then 3, then 2 and keeps the first that fits (a 6 x 6-blocked matrix is served as 3);
 * other sizes are SMM_HIP_ERR_INVALID.  *found (may be NULL) receives the size kept by this call, or 0: a matrix that does not fit is
 * SMM_HIP_OK with *found = 0, not an error.  A later call with another size that fits replaces the kept analysis; one that does not
 * fit leaves it in place.  The kernel choice of the handle is not changed. */
int smm_hip_csr_find_blocks(smm_hip_csr* m, int block_size, int* found);
/* The kept analysis: block size, number of blocks (nnz / b^2) and the most entries a row may hold at that size; 0 / 0 / 0 before an
 * analysis or when the matrix did not fit.  kernel_desc prices a BLOCKS launch as nnz s + (nnz / b^2) 4 + (rows / b + 1) 4 + cols s + rows s. */
int smm_hip_csr_blocks_info(const smm_hip_csr* m, int* block_size, long long* blocks, int* max_row_entries);
/* The LONGROWS family's two lengths (SMM_SPMV_LONGROWS above).  A tuning and test knob, in the spirit of smm_hip_set_march_min_rows:
 * split_len in SMM_LONGROWS_SPLIT_MIN .. SMM_LONGROWS_SPLIT_MAX, segment_len a multiple of 64 in SMM_LONGROWS_SEGMENT_MIN ..
 * SMM_LONGROWS_SEGMENT_MAX, 0 = the default of either; anything else is SMM_HIP_ERR_INVALID and changes nothing.  A kept analysis is
 * replaced at once (a synchronous set-up call; launches already enqueued finish with the old one); without one the lengths are kept
 * for the analysis smm_hip_csr_set_kernel(m, SMM_SPMV_LONGROWS, ..) runs.  The kernel choice of the handle is not changed.  The lengths
 * change the bits of the long rows (the order above), never those of the short ones. */
int smm_hip_csr_longrows_configure(smm_hip_csr* m, int split_len, int segment_len);
/* The kept analysis: the two lengths in force, the rows longer than split_len and the segments they are cut into (the sum of
 * ceil(len / segment_len) over them); 0 / 0 / 0 / 0 before an analysis.  Any pointer may be NULL.  kernel_desc prices a LONGROWS SpMV as
 * B_spmv + 2 segments s + (long_rows + 1) 8: the segment sums written once and read once, and the long-row list. */
int smm_hip_csr_longrows_info(const smm_hip_csr* m, int* split_len, int* segment_len, int* long_rows, long long* segments);
/* From how many rows grid-shaped matrices are served by the 2.5-D kernels (csrc/smm_spmv_march.hip): constant diagonals (default
 * 2^21) and values read (default 6 x 2^20 fp64 / 2^24 fp32) -- below, the gather / wave kernels are as fast or faster
 * (profiles/r04/march_threshold.txt).
 * -1 restores a default.  Applies to matrices analysed afterwards.  Tuning knob; the tests use it to run the kernels on small grids. */
int smm_hip_set_march_min_rows(long long const_diagonals_rows, long long values_read_rows);
/* Test / measurement knob: from how many BYTES PER VECTOR the unpreconditioned ConjugateGradient defers its x update (csrc/smm_solvers.hip,
 * cgLazyXP: the last eight directions are kept and x is brought up to date every eighth iteration -- the reference's roundings in the
 * reference's order, bit for bit, 0.875 vector pass less per iteration, eight more vectors of device memory).  Default 64 MB (where five
 * vectors no longer fit the Infinity Cache); a negative value restores the default; SMM_HIP_CG_LAZY_X=0 in the environment turns it off. */
int smm_hip_set_cg_lazy_x_min_bytes(long long bytes);
/* Test / measurement knob: 0 keeps ConjugateGradient from forming its next direction inside the 2.5-D SpMV kernel (MarchFuse,
 * csrc/smm_spmv_march.hip; on by default wherever the deferred x update is on and that kernel serves the matrix): same bits either way. */
int smm_hip_set_cg_fuse_p(int on);
/* allow = 0: a matrix with constant diagonals keeps reading values[] (the MASKS kernels); 1 (default): CONST where it applies.  For
 * measurements of one against the other; the results are the same bits either way. */
int smm_hip_csr_pattern_allow_const(smm_hip_csr* m, int allow);
/* The PATTERN family's slots kernel (row masks with values read, 2 or 4 lanes per row: the values of every 64-row wave whose rows hold the
 * same offsets copied once, wave by wave, at about nnz * sizeof(value) bytes of device memory).  mode -1 (default): AUTO -- where the
 * library adopted the family by itself, >= 99 % of the waves qualify and the copy fits (SMM_HIP_PATTERN_SLOTS=0|1 turns it off / forces it);
 * 0: off; 1: wherever it applies; 2: AUTO's rules also on a kernel set with smm_hip_csr_set_kernel; 3: wherever it applies, and the copy
 * walked by the sweep kernel (offset-major, up to 32 x 64 rows per wave held in registers, so that x stays in the L2 between two offsets;
 * SMM_HIP_PATTERN_SLOTS=3 is the same per process).  AUTO and mode 2 take the sweep kernel by themselves where it was measured to win:
 * fp32, from about 9.4 M rows, offsets spanning more than a row-by-row walk keeps cached.  Same bits as the tile kernel in every mode. */
int smm_hip_csr_pattern_slots(smm_hip_csr* m, int mode);
/* Test / measurement knob: how many 64-row waves a hardware wave of the sweep kernel holds open (8, 16 or 32; 0 restores the default,
 * SMM_HIP_PATTERN_SWEEP_ROWS in the environment).  Same bits at every setting.  SMM_HIP_PATTERN_SWEEP_WGS=1..8 in the environment (read
 * once per process) is the other lab knob: workgroups of that kernel per CU, default 3 or as many as the variant's registers allow. */
int smm_hip_set_pattern_sweep_rows(int rows_open);
/* Times the candidate SpMV configurations on this matrix and keeps the fastest. */
int smm_hip_csr_autotune(smm_hip_csr* m);

/* ---- editing the VALUES of a matrix on the device (CSRMatrix<T>::operator*=, inplaceAdd / inplaceSubtract, zeroValues, updateEntry /
 * addEntry: ref:1525-1604) -------------------------------------------------------------------------------------------------------
 * The pattern (rows, cols, start[], positions[]) never changes; only values[nnz] does.  What the library derived from the pattern alone
 * (tile tables, row masks, dictionary codes, the 2.5-D plan, the kernel choice) is kept: the first SpMV after an edit runs no analysis.
 * What it derived from the values is kept coherent by the edit itself: a matrix in the constant-diagonal encoding (SMM_PATTERN_CONST)
 * stays in it after scale, zero, and axpy of two such matrices (the k diagonal values are updated exactly, in stream order); any other edit re-verifies
 * every entry with one device pass (the call then synchronises `stream`) and drops the matrix to SMM_PATTERN_MASKS when a diagonal no
 * longer holds one value.  A matrix is never promoted back to CONST by an edit (same results either way; only speed differs).
 *
 * Cost: scale / zero move nnz * sizeof(T) once (read + write), axpy three times that; update_entries is one pass over the batch plus a
 * sort of it; set_values is one copy of values[] (host link or HBM) -- positions[] / start[] are never uploaded again.
 *
 * Ordering: asynchronous on `stream` (NULL = the null stream) like the `_dev` calls, except where noted.  An edit is a device write
 * like any other: do not edit a matrix while another thread runs a solve or SpMV on it, and order the streams yourself.  The host-pointer
 * forms (update_entries, set_values, get_values) run on the library's stream and synchronise before returning.
 * For a matrix created with smm_hip_csr_create_dev_* these calls WRITE THE CALLER'S d_values array.
 *
 * Preconditioners made from the matrix before an edit:
 *   SGS     reads A's values at every apply: after an edit it applies the EDITED A (bit for bit an SGS created after the edit), as the
 *           reference's SGSPreconditioner, which holds a reference to A (ref:1185).  Nothing of A's values is kept at create (the
 *           diagonal is only checked there).
 *   ILU0, IC0, JACOBI, BLOCK_ILU0, BLOCK_SGS, CHEBYSHEV, AMG  are snapshots taken at create (the reference's ilu0Val / ic0Val members): their factors
 *           do not follow the edit -- create a new one to follow it.  The A v half of smm_hip_precond_apply_spmv always uses the
 *           current A, in the encoding A is in at apply time.
 * Distributed handles (smm_hip_dist_csr) cannot be edited. */
#define SMM_UPDATE_SET 0 /* updateEntry (ref:1572-1580): values[k] = v */
#define SMM_UPDATE_ADD 1 /* addEntry    (ref:1596-1604): values[k] = values[k] + v */
/* operator*= (ref:1525-1531): values[k] = values[k] * alpha */
int smm_hip_csr_scale_f32(smm_hip_csr* m, float alpha, smm_hip_stream stream);
int smm_hip_csr_scale_f64(smm_hip_csr* m, double alpha, smm_hip_stream stream);
/* values[k] = values[k] + alpha * other.values[k] (two roundings); alpha = 1 / -1 give the bits of inplaceAdd / inplaceSubtract
 * (ref:1533-1549).  `other` must have the same dtype and pattern (rows, cols, nnz, start[], positions[]), else SMM_HIP_ERR_INVALID and
 * nothing changes.  The first call for a pair of matrices compares the two patterns on the device (and synchronises `stream`); the verdict
 * is kept in both handles, so later calls for the same pair compare nothing.  other may be m. */
int smm_hip_csr_axpy_f32(smm_hip_csr* m, float alpha, const smm_hip_csr* other, smm_hip_stream stream);
int smm_hip_csr_axpy_f64(smm_hip_csr* m, double alpha, const smm_hip_csr* other, smm_hip_stream stream);
/* zeroValues (ref:1591-1594): every value +0 */
int smm_hip_csr_zero_f32(smm_hip_csr* m, smm_hip_stream stream);
int smm_hip_csr_zero_f64(smm_hip_csr* m, smm_hip_stream stream);
/* A batch of n entries (rows[i], cols[i], values[i]) applied in ONE device pass, each found by a binary search of its row like
 * getValueIndex (ref:1551-1570); mode SMM_UPDATE_SET or SMM_UPDATE_ADD.  The result is that of applying the entries one after another in
 * the order given, bit for bit: duplicates of one entry are summed in order (ADD) or the last one wins (SET).  An entry that is not
 * stored -- or whose row or column is out of range -- changes nothing and reports 0 in found[i] (found may be NULL; 1 = applied).
 * Host form: host arrays, synchronous.  _dev form: device arrays (d_found device memory or NULL), asynchronous on `stream`. */
int smm_hip_csr_update_entries_f32(smm_hip_csr* m, int n, const int* rows, const int* cols, const float* values, int mode, unsigned char* found);
int smm_hip_csr_update_entries_f64(smm_hip_csr* m, int n, const int* rows, const int* cols, const double* values, int mode, unsigned char* found);
int smm_hip_csr_update_entries_dev_f32(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const float* d_values, int mode, unsigned char* d_found,
                                       smm_hip_stream stream);
int smm_hip_csr_update_entries_dev_f64(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const double* d_values, int mode, unsigned char* d_found,
                                       smm_hip_stream stream);
/* Replace all nnz values: from host memory (synchronous) or device memory (asynchronous on `stream`).  Only values[] is copied. */
int smm_hip_csr_set_values_f32(smm_hip_csr* m, const float* values);
int smm_hip_csr_set_values_f64(smm_hip_csr* m, const double* values);
int smm_hip_csr_set_values_dev_f32(smm_hip_csr* m, const float* d_values, smm_hip_stream stream);
int smm_hip_csr_set_values_dev_f64(smm_hip_csr* m, const double* d_values, smm_hip_stream stream);
/* Copy the nnz values to host memory (synchronous). */
int smm_hip_csr_get_values_f32(const smm_hip_csr* m, float* values);
int smm_hip_csr_get_values_f64(const smm_hip_csr* m, double* values);
/* For matrices over caller-owned device arrays (smm_hip_csr_create_dev_*): the caller has written d_values itself (ordered before this
 * call on `stream`) and announces it; the matrix re-derives its value-dependent state as after any other edit. */
int smm_hip_csr_values_changed_f32(smm_hip_csr* m, smm_hip_stream stream);
int smm_hip_csr_values_changed_f64(smm_hip_csr* m, smm_hip_stream stream);
/* hasSameNonZeroPattern (ref:1366-1385): *same = 1 when rows, cols, nnz, start[] and positions[] are equal.  Synchronous; cached per pair
 * like smm_hip_csr_axpy_*. */
int smm_hip_csr_same_pattern(const smm_hip_csr* a, const smm_hip_csr* b, int* same);

/* ---- assembling a matrix from TRIPLETS on the device (TripletMatrix::addEntry ref:606-618 + CSRMatrix::fillArrays ref:1606-1641) -----
 * A plan (smm_hip_assembly) is the symbolic result of ONE list of n (row, col) pairs, independent of dtype and of values: the pairs
 * sorted once (stable, on the device), the runs of equal pairs found, the pattern written.  With the plan, turning a list of n values --
 * values[i] belongs to pair i -- into the values of the matrix is one gather-and-sum pass (csrc/smm_assembly.hip): what a time or Newton
 * loop repeats for every new set of element contributions, instead of a sort and a search per call (smm_hip_csr_update_entries_*).
 *
 * Pattern: the stored entries are the distinct (row, col) pairs, rows ascending, columns ascending inside a row (ref:1634-1635);
 *   start[rows + 1], positions[nnz] and first_active_start (smm_hip_csr_info) exactly as fillArrays leaves them (ref:1619-1628).  n == 0,
 *   empty rows and rows == 0 are legal.
 * Values: the value of a stored entry is that of the reference's addEntry calls IN LIST ORDER: the first contribution of a pair is taken
 *   as it is (not 0 + v: a lone -0.0 stays -0.0), every later one is added to it in list order, one rounding each.  Bit for bit: no
 *   floating-point atomics, no tree sums -- the result does not depend on the launch geometry.
 * Out of range: a pair with row outside [0, rows) or col outside [0, cols) (the reference asserts) makes create return
 *   SMM_HIP_ERR_INVALID, with the FIRST offending list index named in smm_hip_last_error(); nothing is created.  Found by a flag on the
 *   device, never by a fault.
 * Limits: n > 2^31 - 1 returns SMM_HIP_ERR_INVALID (the library's 32-bit limit; nnz <= n).
 * create_dev may synchronise `stream` (nnz is needed on the host to allocate); the index arrays are only read and are not needed once
 *   the call has returned.  Host forms take host arrays and synchronise.
 * csr_create_*: a matrix that owns its three device arrays and does not depend on the plan's lifetime -- an smm_hip_csr like any other
 *   (AUTO kernel choice, PATTERN analysis on first use, edits, preconditioners, smm_hip_csr_same_pattern) --, stamped by the plan.
 * refill_*: new values for a matrix THIS plan created (same dtype), else SMM_HIP_ERR_INVALID and nothing changes.  mode SMM_UPDATE_SET:
 *   the values of the assembly of the new list, the bits of a fresh csr_create from it; SMM_UPDATE_ADD: values[k] = values[k] +
 *   assembled[k], one rounding.  A refill is a value edit like smm_hip_csr_set_values_dev_*: what was derived from the pattern is kept
 *   (the first SpMV after it runs no analysis), what was derived from the values follows (constant diagonals re-verified -- that call
 *   then synchronises `stream` --, the slots / sweep copy, the single-launch BiCGStab's copy), and the rules for preconditioners made
 *   before an edit apply unchanged.
 * Cost of csr_create / refill: n (s + 4) + (nnz + 1) 4 bytes read, nnz s written (+ nnz s read for ADD), s = sizeof(T); without repeated
 *   pairs n (s + 4) read and n s written.  The gather of values[] is as local as the caller's list order.
 * Distributed handles are not covered. */
typedef struct smm_hip_assembly smm_hip_assembly;
int smm_hip_assembly_create(int rows, int cols, long long n, const int* row_idx, const int* col_idx, smm_hip_assembly** out);
int smm_hip_assembly_create_dev(int rows, int cols, long long n, const int* d_row_idx, const int* d_col_idx, smm_hip_stream stream, smm_hip_assembly** out);
/* n = pairs in the list, nnz = distinct pairs, longest_run = the most contributions any one entry receives (any pointer may be NULL) */
int smm_hip_assembly_info(const smm_hip_assembly* plan, int* rows, int* cols, long long* n, int* nnz, int* longest_run);
/* copies start[rows + 1] / positions[nnz] to host memory (synchronous; either may be NULL) */
int smm_hip_assembly_pattern(const smm_hip_assembly* plan, int* start, int* positions);
int smm_hip_assembly_destroy(smm_hip_assembly* plan);
int smm_hip_assembly_csr_create_f32(const smm_hip_assembly* plan, const float* values, smm_hip_csr** out);
int smm_hip_assembly_csr_create_f64(const smm_hip_assembly* plan, const double* values, smm_hip_csr** out);
int smm_hip_assembly_csr_create_dev_f32(const smm_hip_assembly* plan, const float* d_values, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_assembly_csr_create_dev_f64(const smm_hip_assembly* plan, const double* d_values, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_assembly_refill_f32(const smm_hip_assembly* plan, smm_hip_csr* m, const float* values, int mode);
int smm_hip_assembly_refill_f64(const smm_hip_assembly* plan, smm_hip_csr* m, const double* values, int mode);
int smm_hip_assembly_refill_dev_f32(const smm_hip_assembly* plan, smm_hip_csr* m, const float* d_values, int mode, smm_hip_stream stream);
int smm_hip_assembly_refill_dev_f64(const smm_hip_assembly* plan, smm_hip_csr* m, const double* d_values, int mode, smm_hip_stream stream);

/* ---- the TRANSPOSE of a matrix, built on the device (csrc/smm_transpose.hip); additions with no counterpart in the reference --------------
 * transpose_create: *out is the cols x rows matrix Aᵀ of `a`'s dtype.  It owns its three device arrays and does not depend on `a`'s
 *   lifetime -- an smm_hip_csr like any other (AUTO kernel choice, PATTERN analysis on first use, edits, preconditioners,
 *   smm_hip_csr_same_pattern).  May synchronise `stream`.
 * Pattern: row j of Aᵀ holds the entries of column j of A with columns (A's rows) ascending -- a stable sort of the entries by column.
 *   start[cols + 1], positions[nnz] and what smm_hip_csr_info reports are those of smm_hip_csr_create_* for the same arrays built on the
 *   host.  Rectangular matrices, empty rows and columns, nnz == 0, rows == 0 or cols == 0 are legal.
 * Values: copied bit for bit (-0.0 stays -0.0, NaN payloads are kept).  No arithmetic and no floating-point atomics: the result does not
 *   depend on the launch geometry.
 * A column outside [0, cols), or a start[] that does not ascend from 0, is found by a flag on the device before it is used as an address:
 *   SMM_HIP_ERR_INVALID, never a fault; nothing is created.
 * transpose_refresh_*: `at` must have been made by transpose_create from a matrix with `a`'s pattern; the library keeps the permutation
 *   perm[nnz] (4 bytes per entry) in `at`.  values_T[k] = a.values[perm[k]]: one gather pass, asynchronous on `stream`, and a value edit of
 *   `at` with exactly the rules of smm_hip_csr_set_values_dev_* (what was derived from the pattern stays, no analysis on the next SpMV,
 *   constant diagonals re-verified, the slots / sweep / single-launch copies follow).  Cost: nnz (2 s + 4) bytes (s = sizeof(T)) plus the
 *   locality of the gather -- local for banded matrices, whose perm[k] stays within the band's width of k.
 *   SMM_HIP_ERR_INVALID, nothing changed: `at` was not made by transpose_create; a dtype differs; `a`'s rows / cols / nnz do not match; `a`
 *   has another pattern than the matrix `at` was built from.  The verdict on the pattern is cached in `a` like that of
 *   smm_hip_csr_same_pattern (the source handle itself costs nothing; another handle one device pass and a synchronisation, once).
 *   Distributed handles are not covered.
 * is_symmetric (synchronous): a matrix that is not square gives 0 / 0.  *pattern_symmetric = 1 when start[] / positions[] of Aᵀ equal those
 *   of A; *values_symmetric = 1 when in addition every values_T[k] == values[k] by IEEE == (-0.0 equals +0.0, a NaN is never equal).
 *   Builds a temporary transpose and frees it; either output may be NULL.
 * get_pattern (synchronous): start[rows + 1] and positions[nnz] copied to host memory (either may be NULL), the companion of
 *   smm_hip_csr_get_values_*: how a caller reads a matrix the device built. */
int smm_hip_csr_transpose_create(const smm_hip_csr* a, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_transpose_refresh_f32(smm_hip_csr* at, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_transpose_refresh_f64(smm_hip_csr* at, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_is_symmetric(const smm_hip_csr* a, int* pattern_symmetric, int* values_symmetric);

/* ---- a COLOURING of the rows and the SYMMETRIC PERMUTATION B = P A Pᵀ of a matrix, on the device -- additions (csrc/smm_color.hip) ----
 * smm_hip_csr_color*: colours (0-based) of the rows of a square matrix such that no stored entry (i, j), i != j, joins two rows of one
 *   colour; explicit zeros count.  Rows i != j are adjacent when (i, j) or (j, i) is stored (the in-neighbours come from the library's
 *   transpose when the pattern is not symmetric).  THE RULE, fixed so that the result does not depend on scheduling:
 *     key(i) = splitmix64(i + 1), splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)   (64-bit wrapping arithmetic; a bijection, so no two keys tie);
 *     the rows are taken in DESCENDING key order and each gets the smallest colour none of its already coloured neighbours holds.
 *   On the device this runs in rounds (every uncoloured row whose key beats all its uncoloured neighbours' is coloured); the host reads
 *   one count per round.  The number of colours is bounded by `rows` alone (a dense block needs as many colours as it has rows).
 *   count must be `rows`; *ncolors = the largest colour + 1 (0 for a matrix without rows).  SMM_HIP_ERR_INVALID: a matrix that is not
 *   square, a wrong count, a null output, a column outside the matrix.  The host form is a set-up call (it drains the device once);
 *   the _dev form writes d_colors on `stream` and synchronises it.
 * smm_hip_csr_permute_create*: b = P A Pᵀ as an ordinary handle that owns its arrays: perm[i] is the row of `a` that becomes row i,
 *   b(i, j) = a(perm[i], perm[j]); columns ascend inside each row; values are carried bit for bit.  perm (host) / d_perm (device) holds
 *   `count` == rows entries.  The check that perm is a permutation of 0 .. rows - 1 runs on the device; a value out of range or named
 *   twice, a wrong count or a matrix that is not square give SMM_HIP_ERR_INVALID with nothing created (*out = NULL).  Synchronises
 *   `stream`.  Set-up: one radix sort of the entries over the bits 2 x rows need; the entry map (4 bytes per entry) and the permutation
 *   stay with b.
 * smm_hip_csr_permute_refresh_*: b's values from the present values of `a` in one gather pass, asynchronous on `stream` -- a value edit
 *   of b, in the manner of smm_hip_csr_transpose_refresh_*.  `a` may be the source or any matrix with its pattern (checked on the device
 *   the first time, remembered afterwards).  SMM_HIP_ERR_INVALID, nothing changed: b was not made by smm_hip_csr_permute_create, another
 *   shape, entry count, pattern or dtype. */
int smm_hip_csr_color(const smm_hip_csr* a, int* colors, size_t count, int* ncolors);
int smm_hip_csr_color_dev(const smm_hip_csr* a, int* d_colors, size_t count, smm_hip_stream stream, int* ncolors);
int smm_hip_csr_permute_create(const smm_hip_csr* a, const int* perm, size_t count, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_permute_create_dev(const smm_hip_csr* a, const int* d_perm, size_t count, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_permute_refresh_f32(smm_hip_csr* b, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_permute_refresh_f64(smm_hip_csr* b, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_get_pattern(const smm_hip_csr* m, int* start, int* positions);

/* ---- a BANDWIDTH-REDUCING ORDERING: reverse Cuthill-McKee, computed on the device -- additions (csrc/smm_rcm.hip) ------------------------
 * smm_hip_csr_rcm*: perm[] such that P a Pᵀ has its entries near the diagonal; perm[i] is the row of `a` that becomes row i -- the
 *   convention of smm_hip_csr_permute_create, so the output goes straight into it.  What it is for: SMM_SPMV_PATTERN serves "band-numbered
 *   mesh matrices", and whether a mesh matrix is band-numbered was decided by the program that wrote it out; after this ordering the
 *   entries take their columns from about 2 x bandwidth offsets, which the CODES encoding accepts up to 65536, and x is gathered from a
 *   band.  THE RULE, fixed so that the permutation is a function of the pattern alone (its definition, line by line, is
 *   tests/rcm_restatement.py):
 *     graph: the matrix must be square.  Vertices i != j are adjacent when (i, j) or (j, i) is stored (explicit zeros count; the
 *       diagonal is ignored).  deg(v) = the number of distinct neighbours of v; key(v) = (deg(v), v), compared lexicographically.
 *     Repeat 1 - 3 while unnumbered vertices remain; every breadth-first search visits unnumbered vertices only (one component):
 *     1 start: s = the unnumbered vertex of smallest key.  (So all isolated vertices come first, in index order.)
 *     2 root (George-Liu): r = s; let v be the vertex of smallest key in the LAST level of the search from r; if the search from v has
 *       more levels than the one from r, r = v and repeat; otherwise keep r.
 *     3 numbering (Cuthill-McKee): a queue holding r; pop u, append the still unnumbered neighbours of u in ascending key order; until
 *       the queue is empty.  The component's vertices are appended to the order in queue order.
 *     4 with reverse != 0 (RCM, what callers want) the whole concatenated order is reversed.
 *   On the device step 3 runs level by level: a new vertex takes parent = the smallest rank among its neighbours in the current level
 *   (a 32-bit integer atomicMin), the new level is numbered in ascending (parent, deg, index) -- exactly the queue's order.  Integer
 *   atomics only: two calls give the same permutation.  The graph is `a`'s own pattern when it equals its transpose's (decided on the
 *   device), else the union pattern from the library's transpose and sum; `a` is not changed.
 *   COST: work per level is proportional to the edges of that level's vertices, but the host reads one small record per level of every
 *   search -- a component costs (its levels) x (the root searches of step 2, usually 2 - 4, plus the numbering) round trips of some tens
 *   of microseconds, plus one per component.  The isolated vertices are numbered by one launch.  Fine for meshes (a 40^3 grid has 118
 *   levels); LONG THIN GRAPHS ARE SLOW: a band of half-width 24 with 10^7 rows has about 400 000 levels.  *levels and *components let
 *   the caller see it.  A row of more than 64 entries is walked by a whole wavefront, shorter ones by 8 lanes.
 *   count must be `rows`.  The four information outputs may be NULL: *components = the connected components, isolated vertices
 *   included; *levels = the most levels among the searches from the kept roots (0 for a matrix without rows, 1 when every vertex is
 *   isolated); *bandwidth_before / *bandwidth_after = max |i - j| over the stored entries of `a` / of P a Pᵀ, the latter computed from
 *   the ordering without building the matrix (it does not depend on `reverse`).
 *   SMM_HIP_ERR_INVALID, nothing written: a matrix that is not square, a wrong count, a null perm (rows == 0 is legal and needs none); a
 *   column outside the matrix or a start[] that does not ascend from 0 -- found by a flag on the device, never a fault --; a pattern that
 *   is not symmetric AND has a row whose columns do not ascend strictly (the sum's rule; every matrix the library builds does).
 *   Both forms are set-up calls: the host form drains the device once; the _dev form writes d_perm (device, `count` ints) on `stream`
 *   and synchronises it.  Distributed handles are not covered.
 * smm_hip_csr_bandwidth (synchronous; any handle, rectangular included): *bandwidth = max |i - j| over the stored entries (0 for none),
 *   *distinct_offsets = the exact number of distinct j - i, counted by a pass of its own over a bitmap of rows + cols - 1 bits (what
 *   SMM_SPMV_PATTERN compares with 64 and 65536).  Either output may be NULL.  SMM_HIP_ERR_INVALID for a column outside the matrix or
 *   a start[] that does not ascend from 0. */
int smm_hip_csr_rcm(const smm_hip_csr* a, int* perm, size_t count, int reverse, int* components, int* levels, long long* bandwidth_before,
                    long long* bandwidth_after);
int smm_hip_csr_rcm_dev(const smm_hip_csr* a, int* d_perm, size_t count, int reverse, smm_hip_stream stream, int* components, int* levels,
                        long long* bandwidth_before, long long* bandwidth_after);
int smm_hip_csr_bandwidth(const smm_hip_csr* a, long long* bandwidth, long long* distinct_offsets);

/* ---- the PRODUCT C = A B of two matrices, built on the device (csrc/smm_spgemm.hip); additions with no counterpart in the reference --------
 * `a` is m x k, `b` is k x n, same dtype; C is m x n.
 * Pattern: entry (i, j) is stored in C iff some p has (i, p) stored in `a` and (p, j) stored in `b` -- the structural product.  Terms that
 *   cancel to 0 and explicitly stored zeros keep their entry: nothing is dropped by value.  Rows ascend, columns ascend inside a row;
 *   start[m + 1], positions[nnz] and what smm_hip_csr_info reports are those of smm_hip_csr_create_* for the same arrays built on the host.
 *   Legal: rectangular matrices, empty rows in `a`, rows of `b` that are empty or never referenced, nnz == 0, any of m, k, n equal to 0,
 *   and a == b (A A).
 * Values: c = +0.0; then, for the stored entries (i, p) of `a`'s row i IN STORED ORDER that have (p, j) stored in `b`:
 *   c = _smm_fma(a_ip, b_pj, c) -- the row sum of rMult (ref:1484-1489).  No floating-point atomics and no tree sums: the result does not
 *   depend on the launch geometry, two runs give the same bits.  Consequence: for finite values, column j of C equals A.rMult of the dense
 *   column j of B at one lane per row, bit for bit, in both rounding flavours.
 * Bad input: a column of `a` outside [0, k), a column of `b` outside [0, n) or a start[] that does not ascend from 0 (caller-owned device
 *   arrays) is found by a flag on the device before it is used as an address: SMM_HIP_ERR_INVALID, never a fault; nothing is created.
 * Limits: a product of more than 2^31 - 1 stored entries returns SMM_HIP_ERR_INVALID (the count of scalar products, sum of ub_i, is kept
 *   in 64 bits and may exceed 32).
 * multiply_create: the symbolic phase followed by the numeric phase.  *out owns its three arrays and does not depend on `a` or `b` -- an
 *   smm_hip_csr like any other (AUTO kernel choice, PATTERN analysis on first use, edits, preconditioners, smm_hip_csr_same_pattern,
 *   transpose).  Synchronises `stream` (nnz is needed on the host).  SMM_HIP_ERR_INVALID: a null handle, a dtype mismatch,
 *   a.cols != b.rows.  Distributed handles (smm_hip_dist_csr) are not covered.
 * multiply_into_*: the numeric phase only, into the existing pattern of `c`: every stored entry of `c` gets the value defined above, an
 *   entry no product lands on gets +0.0.  `c` may come from multiply_create of matrices with these patterns, of supersets of them, or
 *   from anywhere: no bookkeeping ties it to `a` or `b`.  A product whose (i, j) is not stored in `c` returns SMM_HIP_ERR_INVALID: `c`
 *   keeps its old bits (values, pattern, kernel choice) and smm_hip_last_error() names the first such row.  The values are computed into
 *   scratch memory (nnz(c) sizeof(T) bytes), the device flag is read -- the call synchronises `stream` --, and only then the scratch
 *   becomes c's values (arrays the handle owns) or is copied into them (caller-owned arrays, smm_hip_csr_create_dev_*).  On success it
 *   is a value edit of `c` with exactly the rules of smm_hip_csr_set_values_dev_*: what was derived from the pattern stays, what was
 *   derived from the values follows.  SMM_HIP_ERR_INVALID, nothing changed: c == a or c == b, a null handle, a shape or dtype mismatch,
 *   bad input as above.
 * Cost beside the set-up passes (bins, scan, one segmented sort of positions[] in create): `a` read once per phase, sum of ub_i (s + 4)
 *   bytes gathered from `b` (s = sizeof(T); 4 in each of the two symbolic passes), nnz(C) (s + 4) written. */
int smm_hip_csr_multiply_create(const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_multiply_into_f32(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream);
int smm_hip_csr_multiply_into_f64(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream);

/* ---- the SUM C = alpha A + beta B of two matrices with ANY two patterns, built on the device (csrc/smm_add.hip); additions with no
 * counterpart in the reference (inplaceAdd / inplaceSubtract, ref:1533-1549, and smm_hip_csr_axpy_* need equal patterns) -----------------
 * Operands: `a` and `b` have the same rows, cols and dtype; the suffix names that dtype.  Anything else is SMM_HIP_ERR_INVALID.
 *   The columns of every row of either operand must ASCEND STRICTLY.  Every matrix the library builds does (assembly, transpose, permute,
 *   product, convert, the generators), and so does the reference's fillArrays (ref:1634-1635).  A flag on the device finds, before any
 *   column is used as an address: a row whose columns do not ascend strictly (caller-made arrays), a column outside [0, cols), a start[]
 *   that does not ascend from 0.  Each returns SMM_HIP_ERR_INVALID, never a fault, and creates nothing; smm_hip_last_error() names the
 *   operand (a / b / c) and the first offending row.  A handle that has passed is not checked again.
 *   Legal: rectangular matrices, empty rows in either operand, nnz == 0, rows == 0 or cols == 0, a == b.
 * Pattern of C: (i, j) is stored iff it is stored in `a` or in `b`.  Rows ascend, columns ascend strictly inside a row.  Nothing is
 *   dropped by value: an entry whose terms cancel, an explicitly stored zero, alpha == 0 or beta == 0 all keep their entries.  start[],
 *   positions[] and what smm_hip_csr_info reports are those of smm_hip_csr_create_* for the same arrays built on the host.  The entry
 *   count is kept in 64 bits while it is formed; more than 2^31 - 1 stored entries returns SMM_HIP_ERR_INVALID.
 * Values: u = alpha * a_ij (one rounding) where `a` stores (i, j), v = beta * b_ij (one rounding) where `b` stores it;
 *   c_ij = u + v (one more rounding) where both store it, u where only `a` does, v where only `b` does -- never u + 0: a lone -0.0 times
 *   1 stays -0.0.  No _smm_fma, no contraction, no special-casing of alpha or beta: both library flavours give the same bits.  No
 *   floating-point atomics: every stored entry of C is written exactly once by one lane, nothing depends on the launch geometry.
 *   Consequences: with equal patterns, alpha = 1 gives the bits of smm_hip_csr_axpy_*(a, beta, b); for any patterns the result has the
 *   bits of smm_hip_assembly_csr_create_* on the list that holds a's triplets with values alpha * a_ij followed by b's with beta * b_ij.
 * add_create_*: *out owns its three arrays and does not depend on `a` or `b` -- an smm_hip_csr like any other (AUTO kernel choice, PATTERN
 *   analysis on first use, edits, preconditioners, smm_hip_csr_same_pattern, transpose, product).  Synchronises `stream` (nnz is needed on
 *   the host).
 * add_into_*: the numeric phase alone, into the existing pattern of `c`: every stored entry of `c` gets the value defined above, an entry
 *   neither operand stores gets +0.0.  No bookkeeping ties `c` to `a` or `b`.  Unlike multiply_into, `c` MAY BE `a`, `b`, OR BOTH: the
 *   values are formed in scratch memory first, so A <- A + sigma D with D's pattern inside A's is one call.  An operand that stores an
 *   entry `c` does not returns SMM_HIP_ERR_INVALID: `c` keeps all its old bits (values, pattern, kernel choice) and smm_hip_last_error()
 *   names the first such row.  Order of work as in multiply_into_*: the values go into scratch (nnz(c) sizeof(T) bytes), the device flag is
 *   read -- the call synchronises `stream` --, and only then the scratch becomes c's values (arrays the handle owns) or is copied into them
 *   (caller-owned arrays).  On success it is a value edit of `c` with exactly the rules of smm_hip_csr_set_values_dev_*: what was derived
 *   from the pattern stays (the next SpMV runs no analysis), what was derived from the values follows (constant diagonals re-verified, the
 *   slots / sweep / single-launch copies; preconditioners by their own rules).  SMM_HIP_ERR_INVALID, nothing changed: a null handle, a
 *   shape or dtype mismatch, bad input as above.
 * How (a merge by ranking; nothing is sorted): a stored entry of `b` is new iff a binary search of a's row does not find its column; one
 *   scan of those flags gives every entry of either operand its place in C.  Entries are dealt flat over lanes, so a 7-entry row and a
 *   5 000-entry row load alike; the searched row segments sit in LDS when a workgroup's are at most 1024 columns.
 * Cost (s = sizeof(T)): the operand check reads (nnz + rows) 4 bytes once per handle; create reads (nnz_a + nnz_b) 4 in the symbolic pass
 *   (plus nnz_b 8 written and scanned) and (nnz_a + nnz_b)(s + 4) plus the search probes in the fill, and writes nnz_c (s + 4); into reads
 *   (nnz_a + nnz_b)(s + 4) + nnz_c 4 plus the probes (the operands' columns once more to prove that c covers them) and writes nnz_c s.
 * Distributed handles are not covered. */
int smm_hip_csr_add_create_f32(const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_add_create_f64(const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_add_into_f32(smm_hip_csr* c, const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta, smm_hip_stream stream);
int smm_hip_csr_add_into_f64(smm_hip_csr* c, const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta, smm_hip_stream stream);

/* ---- COMPOSING and SLICING matrices on the device (csrc/smm_compose.hip); additions with no counterpart in the reference ------------------
 * The block matrix of a table of handles, the submatrix of chosen rows and columns, the diagonal as a vector, rows and columns scaled by
 * vectors.  Every created matrix owns its three arrays, does not depend on its operands' lifetime, holds its columns ascending strictly
 * inside every row and is an smm_hip_csr like any other (AUTO kernel choice, PATTERN analysis on first use, edits, preconditioners,
 * solvers, transpose, product, sum).  No floating-point atomics: the result depends on the operands alone, two calls give the same bits.
 * Operands whose arrays steer addresses (the blocks, a submatrix's source) must hold strictly ascending columns and pass the device check
 * of smm_hip_csr_add_* first (SMM_HIP_ERR_INVALID, never a fault; kept in the handle once passed).  The creates synchronise `stream`.
 *
 * block_create_*: `blocks` is a row-major p x q table of handles, p q <= 64; NULL is a zero block and one handle may fill several slots.
 *   `coef` is NULL (all ones) or p q scalars.  Block row I is as high as its blocks, block column J as wide as its blocks; row_sizes[p] /
 *   col_sizes[q] (either may be NULL; an entry < 0 says nothing) are needed only for a block row / column that holds nothing but NULLs.
 *   Entry (i, j) of block (I, J) lands at (row offset of I + i, column offset of J + j): inside an output row the segments follow in
 *   ascending block column.  Its value is coef * v rounded once; a coef of exactly 1 copies the bits (-0.0, NaN payloads); a coef of 0
 *   keeps the entries as stored zeros -- nothing is dropped by value, as in add.  0 x n, m x 0 and entry-free blocks are legal.
 *   SMM_HIP_ERR_INVALID, *out untouched: p, q out of range, a block of the other dtype, blocks of one block row (column) with different
 *   heights (widths) or against row_sizes (col_sizes), a block row / column whose size cannot be derived, total rows, columns or entries
 *   beyond 2^31 - 1.
 * block_refresh_*: the numeric phase alone into the kept pattern of `c` (made by block_create from a p x q table), for a matrix rebuilt
 *   every time step or Newton step: every slot must again be NULL or not as at create and have the rows, cols and entry count recorded
 *   there, else SMM_HIP_ERR_INVALID and nothing changed.  THAT EVERY BLOCK HAS THE PATTERN OF THE BLOCK AT CREATE BEYOND THAT IS THE CALLER'S
 *   CONTRACT, as for smm_hip_csr_convert_refresh (smm_hip_csr_transpose_refresh_* checks more); a block with other row lengths gives
 *   wrong values in c, never a write outside it.  `coef` may differ from create's.  Asynchronous on `stream` once every handle is ready.
 *   Afterwards `c` is in the state smm_hip_csr_values_changed_* leaves it in: what was derived from the pattern stays, what was derived
 *   from the values follows (constant diagonals re-verified, the slots / sweep / single-launch copies).  Nothing of size nnz is kept
 *   for it: the place of a segment is recomputed from the blocks' row pointers.
 *   How: a count launch (one lane per output row), the scan, ONE fill launch for the whole table: a slot gets L lanes per row, L the
 *   power of two next to a quarter of its mean row length, up to 65536 -- a lone row of 100 000 entries is copied by 32768 lanes --, and
 *   inside a slot with short rows what a long row holds beyond 8 L entries is copied by whole wavefronts.
 *   Cost (s = sizeof(T)): create nnz (2 s + 8) bytes plus the row pointers ((q + 2) rows 4), refresh nnz 2 s plus the row pointers.
 *
 * submatrix_create / _create_dev: row i of *out is row rows_idx[i] of `a` (any in-range indices in any order, repeats allowed: a gather
 *   of rows), restricted to the columns cols_idx[0] < cols_idx[1] < ... (strictly ascending, so the output's columns ascend), renumbered
 *   0 .. nc - 1.  Either list may be NULL: all rows / all columns (its count is then ignored).  _create takes host arrays, _create_dev
 *   int32 device arrays.  submatrix_range_create: rows [r0, r1) and columns [c0, c1), no lists.  Values are a's, bit for bit.
 *   SMM_HIP_ERR_INVALID, *out untouched: an index outside the matrix, a column list that does not ascend strictly (found on the device;
 *   smm_hip_last_error() names the first offending position as rows_idx[k] / cols_idx[k]), ranges outside the matrix, more than 2^31 - 1
 *   entries.  Cost: a.cols 4 bytes for the column map (index form), two passes over the selected rows' columns, nnz_out (2 s + 8) written
 *   and gathered.
 * submatrix_refresh_*: a value edit of `a` carried over by one gather pass through the kept map of one source index per output entry
 *   (4 bytes per entry of the submatrix): nnz_out (2 s + 4) bytes, asynchronous.  `a` must have the rows, cols and entry count of the
 *   source; that it has its pattern is the caller's contract.  Then as every value edit (see block_refresh).
 *
 * diagonal_dev_*: d_out[i] = a_ii for i < min(rows, cols), 0 where no diagonal entry is stored; *d_missing (int32 on the device, may be
 *   NULL) = the number of such i.  Asynchronous.  diagonal_*: the same into host memory, synchronous; *missing may be NULL.
 * scale_rows_cols_dev_*: v_ij <- (r_i * v_ij) * c_j in place, two roundings in this order; d_r has rows elements, d_c cols.  A NULL
 *   vector skips its factor (one rounding; both NULL: nothing is touched).  A value edit with the rules of smm_hip_csr_set_values_dev_*.
 *   scale_rows_cols_*: the same with the vectors in host memory, synchronous.
 * Distributed handles are not covered. */
int smm_hip_csr_block_create_f32(int p, int q, const smm_hip_csr* const* blocks, const float* coef, const int* row_sizes, const int* col_sizes, smm_hip_stream stream,
                                 smm_hip_csr** out);
int smm_hip_csr_block_create_f64(int p, int q, const smm_hip_csr* const* blocks, const double* coef, const int* row_sizes, const int* col_sizes, smm_hip_stream stream,
                                 smm_hip_csr** out);
int smm_hip_csr_block_refresh_f32(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const float* coef, smm_hip_stream stream);
int smm_hip_csr_block_refresh_f64(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const double* coef, smm_hip_stream stream);
int smm_hip_csr_submatrix_create(const smm_hip_csr* a, const int* rows_idx, size_t nr, const int* cols_idx, size_t nc, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_submatrix_create_dev(const smm_hip_csr* a, const int* d_rows_idx, size_t nr, const int* d_cols_idx, size_t nc, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_submatrix_range_create(const smm_hip_csr* a, int r0, int r1, int c0, int c1, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_submatrix_refresh_f32(smm_hip_csr* sub, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_submatrix_refresh_f64(smm_hip_csr* sub, const smm_hip_csr* a, smm_hip_stream stream);
int smm_hip_csr_diagonal_f32(const smm_hip_csr* a, float* out, int* missing);
int smm_hip_csr_diagonal_f64(const smm_hip_csr* a, double* out, int* missing);
int smm_hip_csr_diagonal_dev_f32(const smm_hip_csr* a, float* d_out, int* d_missing, smm_hip_stream stream);
int smm_hip_csr_diagonal_dev_f64(const smm_hip_csr* a, double* d_out, int* d_missing, smm_hip_stream stream);
int smm_hip_csr_scale_rows_cols_dev_f32(smm_hip_csr* m, const float* d_r, const float* d_c, smm_hip_stream stream);
int smm_hip_csr_scale_rows_cols_dev_f64(smm_hip_csr* m, const double* d_r, const double* d_c, smm_hip_stream stream);
int smm_hip_csr_scale_rows_cols_f32(smm_hip_csr* m, const float* r, const float* c);
int smm_hip_csr_scale_rows_cols_f64(smm_hip_csr* m, const double* r, const double* c);

/* ---- a matrix in the OTHER PRECISION, converted on the device (csrc/smm_convert.hip); additions with no counterpart in the reference -------
 * convert_create: *out is `a`'s matrix with values of `dtype` (SMM_DTYPE_F32 or SMM_DTYPE_F64).  It owns its three device arrays -- start[]
 *   and positions[] are copies -- and does not depend on `a`'s lifetime: an smm_hip_csr like any other (AUTO kernel choice, PATTERN analysis
 *   on first use, edits, preconditioners, smm_hip_csr_same_pattern, transpose, product).  Nothing travels through the host.  Rectangular
 *   matrices, empty rows, nnz == 0 and rows == 0 are legal.  Synchronises `stream` (the range flag and nnz are read before the handle is
 *   handed out).
 * Values: f64 -> f32 rounds to nearest, ties to even: every element carries the bits of static_cast<float>(v).  f32 -> f64 is exact.
 *   `dtype` equal to a's own: a copy, bit for bit.  NaN converts to NaN, +-Inf to +-Inf, -0.0 keeps its sign.  UNDERFLOW IS ALLOWED: a
 *   value too small for fp32 becomes a subnormal or a signed zero without notice.
 * Range: a FINITE fp64 value whose fp32 rounding is not finite (|v| >= 2^128 - 2^103) returns SMM_HIP_ERR_INVALID; smm_hip_last_error()
 *   names the first such entry (its index in values[]) and nothing is created.  Found by a word raised on the device.
 * convert_refresh: `src`'s present values converted into `dst` (either precision on either side): the counterpart of
 *   smm_hip_csr_transpose_refresh_* for a value edit of `src`.  dst must have src's rows, cols and nnz, else SMM_HIP_ERR_INVALID; that the
 *   two PATTERNS agree is the caller's contract, as for multiply_into (smm_hip_csr_same_pattern tells).  On success it is a value edit of
 *   `dst` with exactly the rules of smm_hip_csr_set_values_dev_*: what was derived from the pattern stays (no analysis on the next SpMV),
 *   what was derived from the values follows (constant diagonals re-verified, the slots / sweep / single-launch copies, the finiteness
 *   record; preconditioners by their own rules).  A narrowing refresh converts into scratch memory (nnz * 4 bytes), reads the range word --
 *   it synchronises `stream` -- and only then installs the values: on a range failure `dst` keeps all its old bits (values, kernel
 *   choice).  A widening or same-type refresh cannot fail that way and is asynchronous on `stream`.
 *   SMM_HIP_ERR_INVALID, nothing changed: a null handle, dst == src, a shape or entry-count mismatch, a value out of fp32's range.
 * Cost: one pass over values[], nnz (sizeof(src T) + sizeof(dst T)) bytes, 16-byte loads and stores when both arrays allow it after a
 *   common element-wise head (arrays the library owns always do; caller-owned arrays of smm_hip_csr_create_dev_* may be element-aligned and
 *   then take one element per lane); create adds the copy of the pattern, (rows + 1 + nnz) 8 bytes.
 * Distributed handles are not covered. */
int smm_hip_csr_convert_create(const smm_hip_csr* a, int dtype, smm_hip_stream stream, smm_hip_csr** out);
int smm_hip_csr_convert_refresh(smm_hip_csr* dst, const smm_hip_csr* src, smm_hip_stream stream);

/* ---- SpMV: CSRMatrix<T>::rMult / rMultAdd / rMultSub (ref:1458-1515) -------------------------------------- */
/* out[i] = op(lhs[i], sum_k values[k]*x[positions[k]]); empty rows give op(lhs[i],0) (ref:1479-1483);
 * out may alias lhs, x must not alias out (ref:1503).  lhs is ignored for SMM_OP_ASSIGN. */
int smm_hip_spmv_f32(const smm_hip_csr* m, int op, const float* lhs, const float* x, float* out);
int smm_hip_spmv_f64(const smm_hip_csr* m, int op, const double* lhs, const double* x, double* out);
int smm_hip_spmv_dev_f32(const smm_hip_csr* m, int op, const float* d_lhs, const float* d_x, float* d_out, smm_hip_stream stream);
int smm_hip_spmv_dev_f64(const smm_hip_csr* m, int op, const double* d_lhs, const double* d_x, double* d_out, smm_hip_stream stream);

/* ---- several right-hand sides at once: CSR SpMM (csrc/smm_spmm.hip) ------------------------------------------
 * An addition: the reference multiplies by one vector (ref:1501-1515).  A block of k vectors is ONE dense array of n x k elements,
 * row-major ("interleaved"): element (i, j) is at i * k + j; 1 <= k <= SMM_HIP_MAX_RHS.  x has cols x k elements, lhs and out rows x k.
 *   out(i, j) = op(lhs(i, j), sum_e values[e] * x(positions[e], j))
 * The matrix is streamed once for all k columns.  Column j of out carries the bits smm_hip_spmv_* gives for column j alone with one
 * lane per row (a row's entries in stored order through _smm_fma, ref:1484-1490), whatever smm_hip_csr_set_kernel chose for the
 * SpMV; only a row longer than one tile of the STREAM family's tile table (smm_hip_csr_tile_info: tile_nnz_cap) is split over the
 * lanes of a wavefront and agrees to the rounding of a re-ordered sum.  It reads the handle's CSR arrays, so it follows every edit of
 * the values (smm_hip_csr_scale / _update_entries / smm_hip_assembly_refill ...).  out may alias lhs, x must not alias out (ref:1503);
 * lhs is ignored for SMM_OP_ASSIGN.  k outside 1 .. SMM_HIP_MAX_RHS, a null array or a dtype mismatch: SMM_HIP_ERR_INVALID. */
#define SMM_HIP_MAX_RHS 8
int smm_hip_spmm_f32(const smm_hip_csr* m, int op, int k, const float* lhs, const float* x, float* out);
int smm_hip_spmm_f64(const smm_hip_csr* m, int op, int k, const double* lhs, const double* x, double* out);
int smm_hip_spmm_dev_f32(const smm_hip_csr* m, int op, int k, const float* d_lhs, const float* d_x, float* d_out, smm_hip_stream stream);
int smm_hip_spmm_dev_f64(const smm_hip_csr* m, int op, int k, const double* d_lhs, const double* d_x, double* d_out, smm_hip_stream stream);

/* ---- reductions: Vector<T>::operator* (ref:305-328), secondNormSquared (ref:296-303) ---------------------- */
int smm_hip_dot_f32(int n, const float* a, const float* b, float* result);
int smm_hip_dot_f64(int n, const double* a, const double* b, double* result);
/* d_result: one T in device memory */
int smm_hip_dot_dev_f32(int n, const float* d_a, const float* d_b, float* d_result, smm_hip_stream stream);
int smm_hip_dot_dev_f64(int n, const double* d_a, const double* d_b, double* d_result, smm_hip_stream stream);

/* ---- AXPY-style updates of the solver loops (device pointers; scalars by value) ---------------------------
 * y = a*x + y_in form used by every update loop of ref:2245-2247, 2263-2267, 2272-2274, 2362-2394:
 *   smm_hip_axpby_dev: out[i] = _smm_fma(a, x[i], y[i])      (out may alias x or y) */
int smm_hip_axpy_dev_f32(int n, float a, const float* d_x, const float* d_y, float* d_out, smm_hip_stream stream);
int smm_hip_axpy_dev_f64(int n, double a, const double* d_x, const double* d_y, double* d_out, smm_hip_stream stream);

/* ---- solvers ------------------------------------------------------------------------------------------------
 * smm_hip_cg_*  replaces  SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* b, const T* x0, T* x,
 *                                                      int maxIterations, T eps)            (ref:2316-2398)
 *   maxIterations == -1 means rows (not clamped otherwise); convergence test eps*eps > ||r||^2; when the
 *   initial residual already passes, x is NOT written (ref:2342-2344).  x may alias x0.
 *   With M != NULL (kind SMM_PRECOND_IC0) it replaces the IC0 overload (ref:2414-2505); kinds SMM_PRECOND_CHEBYSHEV and SMM_PRECOND_AMG run the same loop
 *   (every other kind: SMM_HIP_ERR_INVALID).
 * smm_hip_bicgstab_*  replaces  SolverStatus BiCGStab(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps
 *                                                   [, const Preconditioner& M])          (ref:2191-2303)
 *   x is in/out; maxIterations is clamped to rows, -1 means rows; the loop body always runs once; status is
 *   SUCCESS unless iterations > maxIterations (ref:2277-2282); M == NULL is the IDPreconditioner overload.
 * Additive outputs (may be NULL; the reference API has no equivalent): iterations = loop passes executed,
 * resnorm = last ||r||^2 (cg) or ||r|| (bicgstab) the loop computed.
 * The zero start: smm_hip_cg_*, smm_hip_bicgstab_* and smm_hip_cgs_* read x0 once before their set-up; from an x0 of zeros (-0.0
 * counts, a NaN does not) on a matrix whose values are all finite, r = b - A x0 is b bit for bit and no SpMV is launched for it.  The
 * values are looked through once per version (every edit call above and smm_hip_csr_values_changed_* start a new one).  Same results;
 * SMM_HIP_ZERO_START=0 in the environment (read at every call) launches the SpMV regardless.
 */
int smm_hip_cg_f32(const smm_hip_csr* a, const float* b, const float* x0, float* x, int maxIterations, float eps,
                   const smm_hip_precond* M, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_cg_f64(const smm_hip_csr* a, const double* b, const double* x0, double* x, int maxIterations, double eps,
                   const smm_hip_precond* M, int* solver_status, int* iterations, double* resnorm2);
int smm_hip_cg_dev_f32(const smm_hip_csr* a, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps,
                       const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_cg_dev_f64(const smm_hip_csr* a, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                       const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2);

/* Register-resident ConjugateGradient (csrc/smm_resident.hip).  An unpreconditioned CG whose matrix fits the register file of the chip
 * (rows <= 512 * CUs * {8, 4, 2, 1} for rows of at most {5, 9, 16, 27} entries: BASELINE config 2 does) runs as ONE launch with the
 * matrix held in registers and two grid-wide barriers per iteration, instead of three launches per iteration that re-read the matrix.
 * Same algorithm, same per-row arithmetic; the global sums add the rows in a different (fixed) partition, so alpha / beta differ from the
 * three-launch loop in the last bits.  mode: SMM_CG_RESIDENT_OFF never, _AUTO when it fits (default; falls back silently otherwise),
 * _REQUIRE fail with SMM_HIP_ERR_INVALID when it does not apply (tests, measurements); any other value only queries.  Returns the
 * previous mode.  Initial value from the environment variable SMM_HIP_CG_RESIDENT (0 / 1 / 2). */
#define SMM_CG_RESIDENT_OFF 0
#define SMM_CG_RESIDENT_AUTO 1
#define SMM_CG_RESIDENT_REQUIRE 2
int smm_hip_cg_resident(int mode);

/* Single-launch BiCGStab (csrc/smm_resident_bicg.hip).  A BiCGStab without a preconditioner, or with the library's Jacobi, whose matrix is in
 * the PATTERN family's row-mask encoding (banded / stencil matrices: what the solvers adopt from 2^20 stored entries) with at most 16
 * column offsets and whose vectors fit the register file (rows <= 512 * CUs * 12 in fp64, * 24 in fp32: BASELINE config 5 does) runs as
 * ONE launch: r, p, s, A p, A s in registers, x and r0 in LDS, five grid-wide barriers per iteration instead of seven dependent launches.
 * Same per-row arithmetic and update expressions as the loop; the global sums add the rows in another (fixed) partition, so alpha / omega /
 * beta differ from the loop's in the last bits.  mode as for smm_hip_cg_resident (OFF / AUTO / REQUIRE; any other value only queries);
 * returns the previous mode.  Initial value from the environment variable SMM_HIP_BICGSTAB_RESIDENT (0 / 1 / 2). */
int smm_hip_bicgstab_resident(int mode);

int smm_hip_bicgstab_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps,
                         const smm_hip_precond* M, int* solver_status, int* iterations, float* resnorm);
int smm_hip_bicgstab_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps,
                         const smm_hip_precond* M, int* solver_status, int* iterations, double* resnorm);
int smm_hip_bicgstab_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps,
                             const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm);
int smm_hip_bicgstab_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps,
                             const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm);

/* The generic form of the reference's template `BiCGStab<Preconditioner, T>` (ref:2191-2199): ANY preconditioner, given as a host
 * function with the reference's contract `int apply(const T* rhs, T* x)` on HOST vectors of length rows (non-zero = failure; rhs
 * and x never alias).  SpMV, reductions and updates run on the device as in smm_hip_bicgstab_*; every apply costs two PCIe copies of
 * one vector and two stream drains, so this is the slow path for preconditioners the library does not have.  A failing apply ends
 * the solve with SMM_HIP_ERR_PRECOND. */
typedef int (*smm_hip_apply_fn_f32)(void* user, const float* rhs, float* x);
typedef int (*smm_hip_apply_fn_f64)(void* user, const double* rhs, double* x);
int smm_hip_bicgstab_functor_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, smm_hip_apply_fn_f32 apply, void* user,
                                 int* solver_status, int* iterations, float* resnorm);
int smm_hip_bicgstab_functor_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, smm_hip_apply_fn_f64 apply, void* user,
                                 int* solver_status, int* iterations, double* resnorm);

/* ---- several right-hand sides at once: batched BiCGStab / ConjugateGradient (csrc/smm_solvers_batch.hip) --------------------
 * Additions: the reference's solvers take one b (ref:2191, 2316).  b, x (and x0) are interleaved rows x k blocks as for smm_hip_spmm_*,
 * 1 <= k <= SMM_HIP_MAX_RHS; solver_status, iterations and resnorm are HOST arrays of k elements (each may be NULL).  Every SpMM of the
 * loop streams the matrix once for all k columns.  Column j is solved exactly as smm_hip_bicgstab_* / smm_hip_cg_* solve it alone:
 * its own alpha / omega / beta and dot products, the reference's loop do { } while (res_j > eps && it_j < maxIterations) with the same
 * clamp of maxIterations, status rule and NaN behaviour (ref:2200-2283, 2330-2398).  A column that has left its loop is frozen -- its
 * x, iterations, status and resnorm are not written again while the others go on -- and nothing of it (a NaN, a zero) reaches another
 * column.  The dot products add the rows in another (fixed) partition than the single loops, so x agrees with the single solve to the
 * rounding of re-ordered sums, not bit for bit.  The plain loops only: no resident, lazy-x or PATTERN form is entered from here.
 *   bicgstab_batch: M may be NULL or of kind SMM_PRECOND_NONE / SMM_PRECOND_JACOBI (created for `a`; its division is folded into the
 *   rows of the SpMM as in the single loop) or SMM_PRECOND_JSWEEP_SGS / _JSWEEP_ILU0 (applied column by column after the SpMM); every
 *   other kind returns SMM_HIP_ERR_INVALID.  cg_batch takes no preconditioner; a column
 *   whose first residual already passes reports 0 iterations and its x(:, j) is not written (ref:2342-2344).
 * SMM_HIP_ERR_INVALID: k outside 1 .. SMM_HIP_MAX_RHS, null arrays, dtype mismatch, a matrix that is not square. */
int smm_hip_bicgstab_batch_f32(const smm_hip_csr* a, int k, float* b, float* x, int maxIterations, float eps, const smm_hip_precond* M,
                               int* solver_status, int* iterations, float* resnorm);
int smm_hip_bicgstab_batch_f64(const smm_hip_csr* a, int k, double* b, double* x, int maxIterations, double eps, const smm_hip_precond* M,
                               int* solver_status, int* iterations, double* resnorm);
int smm_hip_bicgstab_batch_dev_f32(const smm_hip_csr* a, int k, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M,
                                   smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm);
int smm_hip_bicgstab_batch_dev_f64(const smm_hip_csr* a, int k, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M,
                                   smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm);
int smm_hip_cg_batch_f32(const smm_hip_csr* a, int k, const float* b, const float* x0, float* x, int maxIterations, float eps, int* solver_status,
                         int* iterations, float* resnorm2);
int smm_hip_cg_batch_f64(const smm_hip_csr* a, int k, const double* b, const double* x0, double* x, int maxIterations, double eps, int* solver_status,
                         int* iterations, double* resnorm2);
int smm_hip_cg_batch_dev_f32(const smm_hip_csr* a, int k, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps,
                             smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_cg_batch_dev_f64(const smm_hip_csr* a, int k, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                             smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2);

/* BiCGSymmetric (ref:2021-2102): same kernels as CG plus the DIVERGED heuristics (ref:2056-2058, 2079-2081) */
int smm_hip_bicgsymmetric_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations);
int smm_hip_bicgsymmetric_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations);

/* smm_hip_bicg_*: BiCG for GENERAL matrices -- an addition: BiCGSymmetric (ref:2021-2102) is this method with Aᵀ = A assumed; here the
 * shadow sequence is written out and runs on `at` (csrc/smm_solvers_bicg.hip).
 * `at` is Aᵀ, e.g. from smm_hip_csr_transpose_create.  NULL: the library builds a transpose for the duration of the solve (a device sort
 *   of the entries and 2 nnz (s + 4) bytes of memory per call: keep a transpose when solving more than once).  `a` itself: the caller
 *   asserts symmetry.  Checked, SMM_HIP_ERR_INVALID: the dtypes, at.rows == a.cols, at.cols == a.rows, equal nnz, `a` square.  THAT `at`
 *   REALLY IS THE TRANSPOSE IS THE CALLER'S CONTRACT: another matrix of that shape gives another (meaningless) iteration, not an error.
 * Semantics (x in/out):
 *   maxIterations = min(maxIterations, rows); -1 -> rows                                                   (ref:2030-2033)
 *   r = b - A x;  rt = r;  p = r;  pt = rt;  rho = rt.r;  rr = r.r;  iterations = 0
 *   do {
 *     ap = A p;  atp = At pt;  denom = sum ap[i] * pt[i]
 *     if (eps > |denom| && rr > 1) return DIVERGED                                                         (ref:2056)
 *     alpha = rho / denom
 *     x[i] += alpha * p[i];  r[i] -= alpha * ap[i];  rt[i] -= alpha * atp[i]       (plain forms, ref:2069-2070, not _smm_fma)
 *     newRho = rt.r;  newRR = r.r
 *     if (newRR > 1 && rr < eps) return DIVERGED                                                           (ref:2079)
 *     beta = newRho / rho
 *     p[i] = r[i] + beta * p[i];  pt[i] = rt[i] + beta * pt[i]                                             (ref:2091)
 *     rho = newRho;  rr = newRR;  iterations++
 *   } while (rr > eps * eps && iterations < maxIterations)
 *   status: MAX_ITERATIONS_REACHED iff iterations > maxIterations, else SUCCESS                            (ref:2098-2100)
 * No further breakdown test: rho == 0 puts Inf / NaN into x, as in smm_hip_cgs_*; a NaN rr leaves the loop.  rows == 0 behaves as
 * smm_hip_cgs_* does (one pass over empty vectors, MAX_ITERATIONS_REACHED).  Additive outputs (may be NULL): iterations, resnorm2 = the
 * last rr.
 * THE BIT RULE: when `at` gives the bits of `a` -- the same handle, or a built transpose of a symmetric matrix -- rt == r, pt == p and
 * rho == rr hold bit for bit and the solve returns the status, iteration count and x of smm_hip_bicgsymmetric_* bit for bit: the sums
 * are partitioned and the updates written exactly as there. */
int smm_hip_bicg_f32(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations,
                     float* resnorm2);
int smm_hip_bicg_f64(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations,
                     double* resnorm2);
int smm_hip_bicg_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, const float* d_b, float* d_x, int maxIterations, float eps, smm_hip_stream stream,
                         int* solver_status, int* iterations, float* resnorm2);
int smm_hip_bicg_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, const double* d_b, double* d_x, int maxIterations, double eps, smm_hip_stream stream,
                         int* solver_status, int* iterations, double* resnorm2);

/* smm_hip_cgs_*  replaces  SolverStatus ConjugateGradientSquared(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps)
 *                                                                                                        (ref:2104-2178)
 * The transpose-free method for general matrices: two SpMVs per pass, like BiCGStab (csrc/smm_solvers_cgs.hip).
 * THE ONE REPAIR: the semantics are exactly ref:2110-2178 with `residualSquared` declared before the `do`, so that the loop
 * condition reads the value the body has just computed.  As published it is declared inside the body and read in the `while`
 * (ref:2171-2172), so the reference's template compiles only as long as nobody instantiates it.
 * Everything else is the reference's text:
 *   - x is in/out; maxIterations is clamped to rows, -1 means rows (ref:2111-2114);
 *   - r = b - A x, p = u = r0 = r, rr0 = r.r0 (ref:2118-2128); the body is do { } while (r.r > eps*eps && iterations < maxIterations):
 *     it always runs once, even for maxIterations == 0, and a NaN residual leaves the loop;
 *   - per element q = _smm_fma(-alpha, ap, u); alphaUQ = alpha * (u + q) (an add, then a multiply); x = x + alphaUQ;
 *     r = r - A alphaUQ; u = _smm_fma(beta, q, r); p = _smm_fma(beta, _smm_fma(beta, p, q), u) (ref:2145-2166);
 *   - status is SUCCESS unless iterations > maxIterations (ref:2174-2177): only maxIterations == 0 gives MAX_ITERATIONS_REACHED, with
 *     1 iteration; never DIVERGED;
 *   - there is no breakdown test (ref:2134, 2153 leave it open): a zero ap.r0 or rr0 puts Inf / NaN into x, as in the reference.
 * rows == 0 takes the same path as smm_hip_bicgstab_* does: the body runs once on empty vectors -- 1 iteration, and since
 * maxIterations is clamped to 0 rows, MAX_ITERATIONS_REACHED; nothing is read or written through b / x (they may be NULL).
 * SMM_HIP_ERR_INVALID: a null or dtype-mismatched matrix, a matrix that is not square, null vectors with rows > 0.
 * Additive outputs (may be NULL): iterations = loop passes executed, resnorm2 = the last r.r the loop computed.
 * In fp32 the method is fragile (the residual polynomial of BiCG is squared, rounding errors with it): see INTEGRATION.md. */
int smm_hip_cgs_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_cgs_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations, double* resnorm2);
int smm_hip_cgs_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, smm_hip_stream stream, int* solver_status,
                        int* iterations, float* resnorm2);
int smm_hip_cgs_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, smm_hip_stream stream, int* solver_status,
                        int* iterations, double* resnorm2);

/* smm_hip_gmres_*: restarted GMRES(restart) with right preconditioning -- an addition, the reference has no GMRES
 * (csrc/smm_solvers_gmres.hip; the definition, line by line, is tests/gmres_restatement.py).
 * For general matrices.  Its residual never grows, it needs no transpose and divides by no inner product that can vanish.
 * Semantics (x in/out; `iterations` counts Arnoldi steps):
 *   maxIterations < 0 means rows; there is no other clamp (a restarted run may need more than `rows` steps)
 *   r = b - A x;  rr = r.r
 *   while (rr > eps*eps && iterations < maxIterations && not DIVERGED) {              -- a cycle
 *     beta = sqrt(rr);  v_0 = r / beta;  g = (beta, 0, ...)
 *     for j = 0 .. restart-1:
 *       w = A M^-1 v_j                                              (right preconditioning: the residual tested is the true one)
 *       twice (classical Gram-Schmidt): h_i = v_i.w for all i <= j from the same w; w = _smm_fma(-h_i, v_i, w), i ascending
 *       H[i][j] = the sum of the two passes' h_i;  H[j+1][j] = sqrt(w.w);  the earlier rotations are applied to the column
 *       d = sqrt(H[j][j]^2 + H[j+1][j]^2);  iterations++;  d == 0 or not finite: the column is dropped, DIVERGED, the cycle ends
 *       the new rotation (cs = H[j][j] / d, sn = H[j+1][j] / d) is applied to the column and to g
 *       H[j+1][j] != 0: v_{j+1} = w / H[j+1][j]
 *       the cycle ends when !(g[j+1]^2 > eps*eps), iterations >= maxIterations or H[j+1][j] == 0
 *     y by back-substitution;  x = x + M^-1 (sum_i y_i v_i);  r = b - A x;  rr = r.r
 *   }
 *   status: DIVERGED if a column was dropped or rr is not finite; else SUCCESS if rr <= eps*eps; else MAX_ITERATIONS_REACHED
 * A solve that starts with rr <= eps*eps (an exact x included) returns x untouched, 0 iterations, SUCCESS.  rows == 0: SUCCESS, 0
 * iterations, nothing is read or written through b / x.  A matrix whose stored values are all zero: DIVERGED after 1 step, x untouched.
 * M: NULL, or any kind smm_hip_bicgstab_* accepts (JACOBI / ILU0 / SGS / BLOCK_ILU0 / BLOCK_SGS / CHEBYSHEV / AMG / MULTICOLOR_SGS /
 *   MULTICOLOR_ILU0 created for `a`).
 * Memory: (restart + 1) * rows elements for the basis (leading dimension rounded up to 64) plus two vectors.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one solve give the same bits.
 * SMM_HIP_ERR_INVALID: restart outside 1 .. SMM_GMRES_MAX_RESTART, a null or dtype-mismatched matrix, a matrix that is not square,
 * null vectors with rows > 0, a preconditioner of another matrix or kind.
 * Additive outputs (may be NULL, like solver_status): iterations, resnorm2 = the last rr. */
#define SMM_GMRES_MAX_RESTART 64
int smm_hip_gmres_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int restart, const smm_hip_precond* M, int* solver_status,
                      int* iterations, float* resnorm2);
int smm_hip_gmres_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int restart, const smm_hip_precond* M, int* solver_status,
                      int* iterations, double* resnorm2);
int smm_hip_gmres_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, int restart, const smm_hip_precond* M,
                          smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_gmres_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, int restart, const smm_hip_precond* M,
                          smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2);

/* smm_hip_minres_*: MINRES (Paige and Saunders 1975) with a symmetric positive definite preconditioner -- an addition, the reference
 * has no MINRES (csrc/smm_solvers_minres.hip; the definition, line by line, is tests/minres_restatement.py).
 * For SYMMETRIC matrices, indefinite ones included (shifted operators, saddle-point / KKT systems), where smm_hip_cg_* divides by a
 * p.Ap that can be zero or negative.  One SpMV and two inner products per step, seven vectors (eight with M), no transpose, and a
 * residual norm that never grows.  Symmetry of `a` is the caller's business, as with smm_hip_cg_*: smm_hip_csr_is_symmetric tells.
 * Semantics (x in/out: the start is read from it; `iterations` counts steps):
 *   maxIterations == -1 means rows; otherwise it is clamped to 0 .. rows
 *   r1 = b - A x;  y = M^-1 r1;  beta1 = sqrt(r1.y);  r2 = r1
 *   oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0
 *   while (phibar^2 > eps*eps && iterations < maxIterations) {
 *     v = y / beta;  Av = A v;  alfa = v.Av
 *     t = Av;  from the second step on: t = _smm_fma(-(beta / oldb), r1, t);  t = _smm_fma(-(alfa / beta), r2, t);  r1 = r2;  r2 = t
 *     y = M^-1 r2;  oldb = beta;  beta = sqrt(r2.y)
 *     r2.y < 0 (M is not positive definite), or beta not finite: DIVERGED, the step is not taken, x keeps its last value
 *     oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
 *     gamma = max(sqrt(gbar^2 + beta^2), machine epsilon of T); cs = gbar / gamma; sn = beta / gamma; phi = cs phibar; phibar = sn phibar
 *     phibar not finite: DIVERGED, likewise
 *     w1 = w2; w2 = w;  w = _smm_fma(-delta, w2, _smm_fma(-oldeps, w1, v)) / gamma;  x = _smm_fma(phi, w, x);  iterations++
 *     beta == 0: the Krylov space is exhausted (phibar is 0 now): the loop ends
 *   }
 *   status: DIVERGED on the tests above; else SUCCESS if phibar^2 <= eps*eps; else MAX_ITERATIONS_REACHED
 * (alfa is formed from A v before r1 is subtracted: v.r1 = 0 in exact arithmetic, so it is the textbook alfa up to rounding.)
 * The stop test is smm_hip_cg_*'s: absolute, on the squared norm.  WHICH NORM: with M == NULL y and r2 are one vector and phibar is
 * ||b - A x||_2 (up to rounding).  With M, phibar is the M^-1-norm of the residual, sqrt(r.M^-1 r): a caller who needs the 2-norm
 * recomputes it.  resnorm2 returns the last phibar^2.
 * A solve that starts with phibar^2 <= eps*eps (an exact x included) returns x untouched, 0 iterations, SUCCESS; maxIterations == 0
 * takes no step either.  rows == 0: SUCCESS, 0 iterations, nothing is read or written through b / x.  The zero start of the other
 * drivers applies (an x of zeros and finite values: r1 = b with no SpMV).
 * M: NULL, or a handle of T's dtype on a matrix with as many rows as `a`, of a kind smm_hip_cg_* takes (IC0 / CHEBYSHEV / AMG /
 *   MULTICOLOR_SGS / MULTICOLOR_IC0 / FSAI / JSWEEP_SGS / JSWEEP_IC0; the JSWEEP kinds with as many lower steps as upper ones).  It
 *   need NOT be created for `a`: a preconditioner of an indefinite `a` is refused at create or is not positive definite, so M is built on
 *   a positive definite relative of `a` -- the unshifted operator, the (1,1) block plus a mass matrix.  A handle of kind NONE is refused.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one solve give the same bits.
 * SMM_HIP_ERR_INVALID (the message starts with "minres:"): a null or dtype-mismatched matrix, a matrix that is not square, null vectors
 * with rows > 0, an M that fails the check above.
 * Additive outputs (may be NULL, like solver_status): iterations, resnorm2. */
int smm_hip_minres_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, const smm_hip_precond* M, int* solver_status, int* iterations,
                       float* resnorm2);
int smm_hip_minres_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, const smm_hip_precond* M, int* solver_status, int* iterations,
                       double* resnorm2);
int smm_hip_minres_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M, smm_hip_stream stream,
                           int* solver_status, int* iterations, float* resnorm2);
int smm_hip_minres_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M, smm_hip_stream stream,
                           int* solver_status, int* iterations, double* resnorm2);

/* smm_hip_lsqr_*: LSQR (Paige and Saunders 1982) for min ||A x - b||_2 with a matrix of ANY shape, with Tikhonov damping -- an addition,
 * the reference has no LSQR (csrc/smm_solvers_lsqr.hip; the definition, line by line, is tests/lsqr_restatement.py).
 * For overdetermined systems (data fitting: the least-squares answer), underdetermined ones (from x = 0: the minimum-norm answer),
 * rank-deficient ones (from x = 0: the minimum-norm least-squares answer) and square ones that are not symmetric.  It works on A, never
 * on AtA, whose condition number is the square.  Two SpMVs per step -- one on `a`, one on `at` -- and two inner products; five work
 * vectors (two of rows, three of cols elements).
 * Operands: `a` is rows x cols; b has rows elements, x has cols (in/out: the start is read from it).  `at` is the transpose of `a`:
 *   NULL     the library builds one for the duration of the solve (a device sort per call: keep one when solving more than once)
 *   a handle from smm_hip_csr_transpose_create_* or the caller's own.  Checked: its dtype, at.rows == a.cols, at.cols == a.rows, equal
 *            entry counts.  That it IS the transpose is the caller's contract.
 *   `a`      the caller asserts symmetry; legal only for a square `a`.
 * Semantics (`iterations` counts steps; the sums are those of smm_hip_minres_*):
 *   maxIterations < 0 means cols; there is no other clamp (LSQR in floating point may need more than cols steps)
 *   ub = b - A x  (the zero start of the other drivers applies: an x of zeros and finite values, ub = b with no SpMV)
 *   bb = ub.ub;  beta = sqrt(bb)                                   -- ub stays UNNORMALISED in memory: u = ub / beta
 *   t = At ub;  vb = t / beta  (beta == 0: vb = 0);  aa = vb.vb;  alpha = sqrt(aa)
 *   beta or alpha not finite: DIVERGED, 0 iterations, x untouched
 *   bb == 0: SUCCESS, 0 iterations, reason 1, x untouched
 *   aa == 0: SUCCESS, 0 iterations, reason 2, x untouched (b - A x is orthogonal to the range of A)
 *   v = vb / alpha;  w = v;  phibar = beta; rhobar = alpha; psi2 = 0; res = bb; arn = (alpha beta)^2
 *   while (res > eps*eps && arn > eps*eps && iterations < maxIterations) {
 *     q = A v;  ub = _smm_fma(-(alpha / beta), ub, q);  bb = ub.ub;  beta = sqrt(bb)
 *     t = At ub;  vb = _smm_fma(-beta, v, t / beta)  (beta == 0: vb = 0, nothing is divided);  aa = vb.vb;  alpha = sqrt(aa)
 *     damp == 0: rb1 = rhobar; psi = 0  (the first rotation is the identity, bit for bit)
 *     otherwise: rb1 = sqrt(rhobar^2 + damp^2); c1 = rhobar / rb1; s1 = damp / rb1; psi = s1 phibar; phibar = c1 phibar
 *     rho = sqrt(rb1^2 + bb); c = rb1 / rho; s = beta / rho; theta = s alpha; rhobar = -c alpha; phi = c phibar; phibar = s phibar
 *     beta, alpha, rho or phibar not finite, or rho == 0: DIVERGED, the step is not taken, x keeps its last value
 *     x = _smm_fma(phi / rho, w, x);  v = vb / alpha  (alpha == 0: v = 0);  w = _smm_fma(-(theta / rho), w, v)
 *     psi2 += psi^2;  res = phibar^2 + psi2;  arn = (alpha |c| phibar)^2;  iterations++
 *     beta == 0 or alpha == 0: the bidiagonalisation has ended (res or arn is 0 now): the loop ends
 *   }
 *   status: DIVERGED on the tests above; else SUCCESS if res <= eps*eps (reason 1) or arn <= eps*eps (reason 2; reason 1 wins when both
 *   hold); else MAX_ITERATIONS_REACHED (reason 0).  maxIterations == 0 takes no step: the status is that of the start values.
 * x IS UPDATED IN PLACE.  The solve is for the correction dx = x - x0 of A dx = b - A x0, and each step adds its term to x itself; no
 *   separate dx is kept, so from x0 = 0 x holds dx's bits.  With damp > 0 the problem solved is min ||A dx - (b - A x0)||^2 + damp^2 ||dx||^2:
 *   it is the CORRECTION that is damped, not x.  Start from x = 0 to damp x.
 * THE STOP TESTS ARE ABSOLUTE and on squared norms, as in smm_hip_cg_* and smm_hip_minres_*: res estimates ||b - A x||^2 + damp^2 ||dx||^2
 *   and arn estimates ||At (b - A x) - damp^2 dx||^2; both come from the recurrence, not from a residual that is formed.  There are no
 *   relative atol / btol tests and no condition estimate.
 * AN INCONSISTENT SYSTEM ENDS BY REASON 2 WITH A RESIDUAL THAT IS NOT SMALL: that is what least squares means.  resnorm2 then tells how
 *   far b is from the range of A.
 * Edges, none of them a fault or a NaN: rows == 0 (SUCCESS, reason 1) or cols == 0 (SUCCESS, reason 2): 0 iterations, resnorm2 =
 *   arnorm2 = 0, nothing is read or written through b / x.  A matrix without entries: reason 2 at once (reason 1 for b == 0), no SpMV and
 *   no transpose.  Empty rows and empty columns are legal; an x element of an empty column keeps its start value.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one solve give the same bits.
 * SMM_HIP_ERR_INVALID (the message starts with "lsqr:"): a null or dtype-mismatched matrix, an `at` of the other dtype, of another shape
 * or entry count, `a` as `at` when `a` is not square, null vectors when rows > 0 and cols > 0, an eps or damp that is negative or not
 * finite.  Nothing is written then.
 * Additive outputs (may be NULL, like solver_status): iterations, reason, resnorm2 = the last res, arnorm2 = the last arn. */
int smm_hip_lsqr_f32(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int maxIterations, float eps, float damp, int* solver_status, int* iterations,
                     int* reason, float* resnorm2, float* arnorm2);
int smm_hip_lsqr_f64(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int maxIterations, double eps, double damp, int* solver_status,
                     int* iterations, int* reason, double* resnorm2, double* arnorm2);
int smm_hip_lsqr_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, const float* d_b, float* d_x, int maxIterations, float eps, float damp, smm_hip_stream stream,
                         int* solver_status, int* iterations, int* reason, float* resnorm2, float* arnorm2);
int smm_hip_lsqr_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, const double* d_b, double* d_x, int maxIterations, double eps, double damp,
                         smm_hip_stream stream, int* solver_status, int* iterations, int* reason, double* resnorm2, double* arnorm2);

/* smm_hip_eigsh_*: the k algebraically LARGEST or SMALLEST eigenvalues of a symmetric matrix, with their eigenvectors, by thick-restart
 * Lanczos (Wu and Simon 2000) with full reorthogonalisation -- an addition, the reference has no eigensolver
 * (csrc/smm_solvers_eigsh.hip; the definition, line by line, is tests/eigsh_restatement.py).  Symmetry of `a` is the caller's business,
 * as with smm_hip_cg_* and smm_hip_minres_*: smm_hip_csr_is_symmetric tells.
 * Parameters: k >= 1 wanted pairs; which = SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST; ncv basis columns with
 *   k + 2 <= ncv <= min(rows, SMM_EIGSH_MAX_NCV), ncv == 0 meaning min(rows, max(2k + 1, 20)); maxRestarts >= 0; tol, with tol <= 0
 *   meaning the machine epsilon of T; a start vector v0, or NULL for the hash vector of `seed`.
 * The basis V has ncv + 1 columns (leading dimension rounded up to 64); its first l columns are kept Ritz vectors, l = 0 at first.
 *   v_0 = v0 / ||v0||.  The hash vector of (seed, col) has the elements of smm_hip_idrs_shadow_dev_*: ((h >> 40) + 0.5) 2^-23 - 1 with
 *     h = sm(sm(sm(seed) ^ col) ^ row); the start is col = 0, and every later fresh vector takes the next col.
 *   a cycle, for j = l .. ncv-1:
 *     w = A v_j
 *     twice (classical Gram-Schmidt): h_i = v_i.w for all i <= j from the same w; w = _smm_fma(-h_i, v_i, w), i ascending
 *     alpha_j = the sum of the two passes' h_j;  beta_j = sqrt(w.w);  scale = max(scale, |alpha_j|, beta_j)
 *     beta_j <= eps(T) * scale: a BREAKDOWN at j -- v_{j+1} is not formed, nothing divides by beta_j, the cycle ends with m = j + 1
 *     v_{j+1} = w / beta_j
 *   (scale: the largest |alpha|, beta or kept |theta| seen so far in the solve.  All of this runs on the device without a host read.)
 *   the Ritz step, once per cycle, on the host in fp64 for both dtypes (cyclic Jacobi): with m = ncv, or j + 1 after a breakdown,
 *     T (m x m) = diag(theta_kept), the arrow s in row and column l, alpha on the rest of the diagonal, beta beside it;  T = Y diag(theta) Y^T
 *     rho_i = |beta_{m-1} Y[m-1][i]|, 0 after a breakdown
 *   the k wanted pairs have converged when rho_i <= tol * max_i |theta_i| for each of them (the maximum over all m Ritz values: an
 *     estimate of ||A||_2 from below, so that an eigenvalue at 0 can be tested)
 *   the solve ends on convergence, on a breakdown with m >= k (an exact invariant subspace) or when maxRestarts restarts were made:
 *     X = V[:, 0..m-1] Y[:, wanted];  eigenvalues in the order of `which`: descending for LARGEST, ascending for SMALLEST
 *   otherwise a restart: l = k + (ncv - k) / 2;  V[:, 0..l-1] = V[:, 0..m-1] Y[:, best l] in place (smm_hip_multi_rotate_dev_*);
 *     v_l = v_m;  theta_kept = those Ritz values;  s_i = beta_{m-1} Y[m-1][i]
 *   a breakdown with m < k: all m Ritz vectors are kept (l = m), s = 0, and v_m = the next hash vector, orthogonalised twice against
 *     the kept columns and normalised; this counts as a restart.  Copies of a multiple eigenvalue are found this way.
 * Outputs: eigenvalues[k]; eigenvectors (may be NULL: none are formed) column-major, vector i at eigenvectors + i * ldx, ldx >= rows.
 *   smm_hip_eigsh_* takes host arrays; smm_hip_eigsh_dev_* takes d_v0, d_eigenvalues and d_eigenvectors in device memory (element
 *   alignment suffices) and synchronises `stream`.  The additive outputs are host words and may each be NULL: residuals[k] (rho_i),
 *   nconv (wanted pairs that passed the test), restarts, matvecs (SpMVs: ncv + restarts * (ncv - l) when nothing broke down),
 *   solver_status: SUCCESS if all k converged, MAX_ITERATIONS_REACHED if not -- the pairs returned are then the best available, with
 *   their rho_i (only min(k, m) of them when a breakdown left fewer) --, DIVERGED if an alpha, a beta, a theta or a start vector's norm
 *   is not finite (or that norm is 0): the eigenpairs are not written then.
 * rows == 0 or k == 0: SUCCESS, nothing is touched.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one call give the same bits.
 * Memory: (ncv + 1) * rows elements for the basis, nothing else of that size.
 * WHAT THIS IS NOT: no shift-invert, no interior eigenvalues, and no preconditioning -- smm_hip_lobpcg_* (below) is the preconditioned
 *   method, and a block one.  The smallest eigenvalues of a large Laplacian converge slowly here, as with any plain Lanczos: they are
 *   what smm_hip_lobpcg_* with an AMG or incomplete-factorisation preconditioner is for.  From a start vector that lies in an invariant
 *   subspace the pairs returned are that subspace's: the method cannot leave it.
 * SMM_HIP_ERR_INVALID (the message starts with "eigsh:"; checked before the device is touched, the outputs are not written): a null or
 * dtype-mismatched matrix, a matrix that is not square, k < 0, another `which`, maxRestarts < 0, an ncv (after the default) outside
 * k + 2 .. min(rows, SMM_EIGSH_MAX_NCV) -- so k > rows - 2 always --, null eigenvalues, ldx < rows with eigenvectors. */
#define SMM_EIGSH_LARGEST 0
#define SMM_EIGSH_SMALLEST 1
#define SMM_EIGSH_MAX_NCV 64
int smm_hip_eigsh_f32(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, float tol, const float* v0, unsigned long long seed, float* eigenvalues,
                      float* eigenvectors, long long ldx, float* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status);
int smm_hip_eigsh_f64(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, double tol, const double* v0, unsigned long long seed, double* eigenvalues,
                      double* eigenvectors, long long ldx, double* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status);
int smm_hip_eigsh_dev_f32(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, float tol, const float* d_v0, unsigned long long seed, float* d_eigenvalues,
                          float* d_eigenvectors, long long ldx, smm_hip_stream stream, float* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status);
int smm_hip_eigsh_dev_f64(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, double tol, const double* d_v0, unsigned long long seed,
                          double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream, double* residuals, int* nconv, int* restarts,
                          int* matvecs, int* solver_status);

/* smm_hip_svds_*: the k LARGEST singular values of a matrix of ANY shape, with their left and right singular vectors, by thick-restart
 * Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005, restarted with Ritz vectors) with full reorthogonalisation of both
 * bases -- an addition, the reference has no SVD (csrc/smm_solvers_svds.hip; the definition, line by line, is
 * tests/svds_restatement.py).  It works on A and A^T, never on A^T A: the condition number is not squared and no product is formed.
 * `a` is rows x cols.  `at` is its transpose as a handle of its own, as in smm_hip_lsqr_*: the caller's (smm_hip_csr_transpose_create_*;
 *   kept across calls), or NULL -- the library then builds one for the call and destroys it afterwards.  `a` itself as `at` asserts
 *   symmetry and needs a square matrix.
 * Parameters: k >= 1 wanted triplets; ncv with k + 2 <= ncv <= min(rows, cols, SMM_SVDS_MAX_NCV), ncv == 0 meaning
 *   min(rows, cols, max(2k + 1, 20)); maxRestarts >= 0; tol, with tol <= 0 meaning the machine epsilon of T; a start vector v0 of cols
 *   elements, or NULL for the hash vector of (seed, col = 0) -- smm_hip_eigsh_*'s generator; every later fresh vector takes the next col.
 * The bases: V is cols x (ncv + 1), U is rows x ncv (leading dimensions rounded up to 64); the first l columns of each are kept Ritz
 *   vectors, l = 0 at first.  v_0 = v0 / ||v0||.
 *   a cycle, for j = l .. ncv-1:
 *     w = A v_j
 *     twice (classical Gram-Schmidt): h_i = u_i.w for all i < j from the same w; w = _smm_fma(-h_i, u_i, w), i ascending
 *     alpha_j = sqrt(w.w);  scale = max(scale, alpha_j)
 *     alpha_j <= eps(T) * scale: an ALPHA-BREAKDOWN at j -- u_j is not formed, nothing divides by alpha_j, the cycle ends
 *     u_j = w / alpha_j
 *     w = A^T u_j
 *     twice: g_i = v_i.w for all i <= j; w = _smm_fma(-g_i, v_i, w), i ascending
 *     beta_j = sqrt(w.w);  scale = max(scale, beta_j)
 *     beta_j <= eps(T) * scale: a BETA-BREAKDOWN at j -- v_{j+1} is not formed, the cycle ends
 *     v_{j+1} = w / beta_j
 *   (scale: the largest alpha, beta or kept sigma seen so far in the solve.  All of this runs on the device without a host read.)
 *   the projected matrix B, upper triangular: diag(sigma_kept) in the leading l x l block, the arrow s in column l (rows 0 .. l-1),
 *     alpha_j on the rest of the diagonal, beta_j at (j, j+1).  Its entries are the recurrence's norms and the arrow; the Gram-Schmidt
 *     products h and g serve orthogonality only.  A V_m = U_m B and A^T U_m = V_m B^T + beta_{m-1} v_m e_{m-1}^T.
 *   the Ritz step, once per cycle, on the host in fp64 for both dtypes (one-sided Jacobi):
 *     no breakdown: m = ncv, B = X diag(sigma) Y^T, sigma descending, rho_i = |beta_{m-1} X[m-1][i]|
 *     beta-breakdown at j: m = j + 1, B is m x m, every rho_i = 0
 *     alpha-breakdown at j: m = j, B^ = B[0..j-1][0..j] (j x (j + 1): column j is the coupling of v_j) = X diag(sigma) Y^^T gives j
 *       exact triplets with right vectors in V_{j+1}; every rho_i = 0; j == 0 gives none
 *   the k wanted triplets have converged when rho_i <= tol * sigma_0 for each (sigma_0: the largest Ritz value of the step, an estimate
 *     of ||A||_2 from below)
 *   the solve ends on convergence, on a breakdown that leaves at least k triplets, or when maxRestarts restarts were made:
 *     U_k = U[:, 0..m-1] X[:, 0..k-1], V_k = V[:, 0..m-1 (m after an alpha-breakdown)] Y[:, 0..k-1] (smm_hip_multi_rotate_dev_*)
 *   otherwise a restart: l = k + (ncv - k) / 2; both bases compressed in place; v_l = v_m; sigma_kept = those Ritz values;
 *     s_i = beta_{m-1} X[m-1][i]
 *   a breakdown that leaves fewer than k triplets: all of them are kept (l = their count), s = 0, and v_l = the next hash vector,
 *     orthogonalised twice against the kept V columns and normalised; this counts as a restart.  Copies of a multiple singular value
 *     are found this way.  A matrix of rank below k therefore ends by maxRestarts with nconv < k, or returns a singular value at
 *     rounding level as converged; it never returns a number that is not finite.
 * Outputs: singular_values[k], descending; U (rows x k, vector i at U + i * ldu, ldu >= rows) and V (cols x k, ldv >= cols), each may
 *   be NULL: that factor is not formed, and with both NULL no basis is rotated at the end.  smm_hip_svds_* takes host arrays;
 *   smm_hip_svds_dev_* takes d_v0, d_singular_values, d_U and d_V in device memory (element alignment suffices) and synchronises
 *   `stream`.  The additive outputs are host words and may each be NULL: residuals[k] (rho_i), nconv, restarts, matvecs (SpMVs on `a`
 *   and on `at` together: 2 (ncv + restarts * (ncv - l)) when nothing broke down), solver_status: SUCCESS if all k converged,
 *   MAX_ITERATIONS_REACHED if not -- the triplets returned are then the best available, with their rho_i (only as many as a breakdown
 *   left when those are fewer than k) --, DIVERGED if an alpha, a beta, a sigma or the start vector's norm is not finite (or that norm
 *   is 0): the triplets are not written then.
 * k == 0, rows == 0 or cols == 0: SUCCESS, nothing is touched.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one call give the same bits.
 * Memory: (ncv + 1) * cols + ncv * rows elements for the bases, plus the transpose if the library built it.
 * WHAT THIS IS NOT: not the SMALLEST singular values -- Ritz restarts converge poorly there, harmonic restarts are not implemented --,
 *   no shift, no block method, no implicit A^T A.  From a start vector that lies in an invariant subspace of A^T A the triplets returned
 *   are that subspace's, as with smm_hip_eigsh_*.
 * SMM_HIP_ERR_INVALID (the message starts with "svds:"; checked before the device is touched, the outputs are not written): a null or
 * dtype-mismatched `a`, an `at` of the other dtype, of another shape or entry count, `a` as `at` when `a` is not square, k < 0,
 * maxRestarts < 0, an ncv (after the default) outside k + 2 .. min(rows, cols, SMM_SVDS_MAX_NCV) -- so k > min(rows, cols) - 2 always --,
 * null singular_values, ldu < rows with U, ldv < cols with V. */
#define SMM_SVDS_MAX_NCV 64
int smm_hip_svds_f32(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, float tol, const float* v0, unsigned long long seed,
                     float* singular_values, float* U, long long ldu, float* V, long long ldv, float* residuals, int* nconv, int* restarts, int* matvecs,
                     int* solver_status);
int smm_hip_svds_f64(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, double tol, const double* v0, unsigned long long seed,
                     double* singular_values, double* U, long long ldu, double* V, long long ldv, double* residuals, int* nconv, int* restarts, int* matvecs,
                     int* solver_status);
int smm_hip_svds_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, float tol, const float* d_v0, unsigned long long seed,
                         float* d_singular_values, float* d_U, long long ldu, float* d_V, long long ldv, smm_hip_stream stream, float* residuals, int* nconv,
                         int* restarts, int* matvecs, int* solver_status);
int smm_hip_svds_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, double tol, const double* d_v0, unsigned long long seed,
                         double* d_singular_values, double* d_U, long long ldu, double* d_V, long long ldv, smm_hip_stream stream, double* residuals, int* nconv,
                         int* restarts, int* matvecs, int* solver_status);

/* smm_hip_lobpcg_*: the k algebraically LARGEST or SMALLEST eigenvalues of a symmetric matrix, with their eigenvectors, by LOBPCG
 * (Knyazev 2001), the locally optimal block preconditioned conjugate gradient method, with the SVQB orthonormalisation of the search
 * block (Stathopoulos and Wu 2002) -- an addition, the reference has no eigensolver (csrc/smm_solvers_lobpcg.hip; the definition,
 * line by line, is tests/lobpcg_restatement.py).  Where smm_hip_eigsh_* is plain Lanczos, this takes a PRECONDITIONER -- the smallest
 * eigenpairs of a stiffness or Laplacian matrix with the AMG V-cycle or an incomplete factorisation are what it is for -- and it is a
 * block method: a cluster or a multiple eigenvalue inside the block is an ordinary input.  Symmetry of `a` is the caller's business.
 * Parameters: 1 <= k <= SMM_LOBPCG_MAX_K wanted pairs, the block size, with 3k <= rows; which = SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST;
 *   maxIterations >= 0; tol, with tol <= 0 meaning the machine epsilon of T; M, NULL or a symmetric positive definite preconditioner
 *   (below); a start block X0 of k columns, column j at X0 + j * ldx0 (ldx0 >= rows), or NULL for the hash columns (seed, col = 0..k-1)
 *   of smm_hip_idrs_shadow_dev_* as they are before that routine's orthonormalisation.
 * The loop.  S = [X P W] and AS = [AX AP AW] are two bases of 3k columns (leading dimension rounded up to 64); Z = [P W]:
 *   X = the start block, made orthonormal column by column: classical Gram-Schmidt twice against the columns before, then a division by
 *       the norm d.  A d, or the column's norm d0 before the two passes, that is not finite, or d <= sqrt(eps(T)) d0 (the block has
 *       rank below k to working precision): DIVERGED.
 *   AX = A X (k SpMVs);  T = X^T AX;  on the host in fp64 for both dtypes: 1/2 (T + T^T) = C diag(theta) C^T by cyclic Jacobi, ordered
 *       by `which`;  X = X C, AX = AX C (smm_hip_multi_rotate_dev_*);  P, AP empty;  scale = 0
 *   for it = 0, 1, ...:
 *     R_j = AX_j - theta_j X_j,  rn_j = ||R_j||_2 for all j < k                            (rn comes to the host)
 *     scale = max(scale, |theta_i|) over EVERY Ritz value of the last Rayleigh-Ritz step (an estimate of ||A||_2 from below, as in eigsh)
 *     active = the j with !(rn_j <= tol * scale);  none: SUCCESS;  it == maxIterations: MAX_ITERATIONS_REACHED
 *     W = M^-1 R[:, active], column by column (smm_hip_precond_apply_dev_*), or R[:, active] without M;  AW = A W, column by column
 *     twice:
 *       H = X^T Z (smm_hip_multi_gram_dev_*);  Z = Z - X H;  AZ = AZ - AX H (smm_hip_multi_block_axpy_dev_*; H stays on the device)
 *       G = Z^T Z -> host, 1/2 (G + G^T), fp64;  d = sqrt(diag G), the columns with d == 0 dropped;  G / (d d^T) = Q diag(w) Q^T
 *       kept: the w_i > (columns left) * eps(T) * max w, the largest first
 *       Y = diag(1 / d) Q[:, kept] diag(w_kept^-1/2);  Z = Z Y, AZ = AZ Y              (SVQB: a rank-deficient direction is dropped,
 *                                                                                       nothing divides by a vanishing norm)
 *     T = S^T AS over S = [X Z] -> host, 1/2 (T + T^T) = C diag(theta) C^T;  C = the k eigenvectors wanted by `which`
 *     P = Z C_Z[:, the first min(|active|, columns of Z) active columns], AP likewise (C_Z: the rows of C below the first k)
 *     X = S C,  AX = AS C                                (one in-place multi_rotate per basis forms [X P]; AX and AP are never recomputed)
 *   The host reads four things per iteration: rn, the two G and T.
 * Outputs: eigenvalues[k] in the order of `which` (descending for LARGEST, ascending for SMALLEST); eigenvectors (may be NULL)
 *   column-major, vector j at eigenvectors + j * ldx, ldx >= rows.  smm_hip_lobpcg_* takes host arrays; smm_hip_lobpcg_dev_* takes d_X0,
 *   d_eigenvalues and d_eigenvectors in device memory (element alignment suffices) and synchronises `stream`.  The additive outputs are
 *   host words and may each be NULL: residuals[k] (the last rn_j), nconv (columns that passed the test), iterations, matvecs
 *   (k + the sum of |active|), applies (the sum of |active| with M, 0 without), solver_status: SUCCESS, MAX_ITERATIONS_REACHED -- the
 *   pairs returned are then the best available -- or DIVERGED: a theta, an rn, a Gram entry or a start column's norm that is not finite, or
 *   a start block of rank below k; the eigenpairs are not written then.
 * rows == 0 or k == 0: SUCCESS, nothing is touched.
 * M: NULL, or any kind smm_hip_cg_* accepts (an iterated sweep needs equal step counts), or JACOBI or SGS -- symmetric positive definite
 *   for a positive definite matrix too; smm_hip_cg_*'s fused loop has no path for them, here every kind runs through its apply.  As with
 *   smm_hip_minres_* it must FIT `a` (same dtype, same rows), it need not be created for it: a shifted L - sigma I takes the
 *   preconditioner of L.  With SMM_EIGSH_LARGEST an M is legal but seldom useful: a preconditioner that approximates A^-1 damps the
 *   very directions wanted.
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one call give the same bits.
 * Memory: 6k vectors plus the preconditioner's own.
 * WHAT THIS IS NOT: the generalised problem A x = lambda B x is smm_hip_lobpcg_gen_*'s (below); no interior eigenvalues, no hard locking (a converged column stays in the
 *   Rayleigh-Ritz basis and only stops producing a residual direction), no column-major SpMM: A W is |active| SpMVs.
 * SMM_HIP_ERR_INVALID (the message starts with "lobpcg:"; checked before the device is touched, the outputs are not written): a null or
 * dtype-mismatched matrix, a matrix that is not square, k < 0 or k > SMM_LOBPCG_MAX_K, 3k > rows (a matrix that small is dense work, or
 * smm_hip_eigsh_*'s), another `which`, maxIterations < 0, null eigenvalues, ldx < rows with eigenvectors, ldx0 < rows with X0, a
 * preconditioner of a kind smm_hip_cg_* refuses other than JACOBI and SGS, of the other dtype or of another size. */
#define SMM_LOBPCG_MAX_K 8
#define SMM_LOBPCG_MAX_BASIS 24
#define SMM_LOBPCG_MAX_BASES 3
int smm_hip_lobpcg_f32(const smm_hip_csr* a, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* X0, long long ldx0,
                       unsigned long long seed, float* eigenvalues, float* eigenvectors, long long ldx, float* residuals, int* nconv, int* iterations, int* matvecs,
                       int* applies, int* solver_status);
int smm_hip_lobpcg_f64(const smm_hip_csr* a, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* X0, long long ldx0,
                       unsigned long long seed, double* eigenvalues, double* eigenvectors, long long ldx, double* residuals, int* nconv, int* iterations, int* matvecs,
                       int* applies, int* solver_status);
int smm_hip_lobpcg_dev_f32(const smm_hip_csr* a, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* d_X0, long long ldx0,
                           unsigned long long seed, float* d_eigenvalues, float* d_eigenvectors, long long ldx, smm_hip_stream stream, float* residuals, int* nconv,
                           int* iterations, int* matvecs, int* applies, int* solver_status);
int smm_hip_lobpcg_dev_f64(const smm_hip_csr* a, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* d_X0, long long ldx0,
                           unsigned long long seed, double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream, double* residuals, int* nconv,
                           int* iterations, int* matvecs, int* applies, int* solver_status);

/* smm_hip_lobpcg_gen_*: the GENERALISED symmetric eigenproblem A x = lambda B x by the loop of smm_hip_lobpcg_* -- the vibration modes
 * K x = lambda M x of a finite-element model with its consistent mass matrix are what it is for (csrc/smm_solvers_lobpcg.hip; the
 * definition, line by line, is tests/lobpcg_gen_restatement.py).  LOBPCG needs neither a factorisation of B nor B^-1: only products with B.
 * `b` is a symmetric positive definite matrix of a's dtype and size; its symmetry and definiteness are the caller's business, like the
 * symmetry of `a`.  b == NULL forwards to smm_hip_lobpcg_*: the same bits, bmatvecs = 0.  b == a is legal (every eigenvalue is 1).
 * Every other parameter and output is smm_hip_lobpcg_*'s; bmatvecs (may be NULL) follows matvecs.
 * The loop.  BS = [BX BP BW] is a third basis beside S and AS, laid out the same way; BX and BP are carried through every rotation and
 * never recomputed, like AX and AP.  eps = eps(T):
 *   start: for j = 0 .. k-1:  w = X0_j (or the hash column);  q = B w;  d0 = sqrt(w . q)
 *            j > 0, twice:  h = BX[:, 0..j-1]^T w;  w = _smm_fma(-h_i, X_i, w), i ascending
 *            j > 0:  q = B w
 *            d = sqrt(w . q);  d0 or d not finite, or !(d > sqrt(eps) d0): DIVERGED
 *            X_j = w / d;  BX_j = q / d                                                        (2k - 1 products with B)
 *          AX = A X;  T = X^T AX -> host, the Ritz step of smm_hip_lobpcg_*;  X, AX and BX rotated by C
 *   for it = 0, 1, ...:
 *     R_j = AX_j - theta_j BX_j;  rn_j = ||R_j||_2;  bn_j = ||BX_j||_2       (one pass over the two blocks; rn and bn come to the host together)
 *     scale = max(scale, |theta_i|) over every Ritz value of the last Rayleigh-Ritz step
 *     active = the j with !(rn_j <= tol * scale * bn_j);  none: SUCCESS;  it == maxIterations: MAX_ITERATIONS_REACHED
 *     W = M^-1 R[:, active] (or R[:, active]);  AW = A W;  BW = B W, column by column
 *     twice:
 *       H = BX^T Z;  Z = Z - X H;  AZ = AZ - AX H;  BZ = BZ - BX H           (smm_hip_multi_block_axpy_bases_dev_*: one launch)
 *       G = Z^T BZ -> host, 1/2 (G + G^T);  d, the live columns, w, kept and Y exactly as in smm_hip_lobpcg_*
 *       Z = Z Y, AZ = AZ Y, BZ = BZ Y                                          (smm_hip_multi_rotate_bases_dev_*: one launch)
 *     T = S^T AS -> host -> C;  [X P], [AX AP] and [BX BP] = S, AS, BS times [C | C_P] exactly as in smm_hip_lobpcg_*
 *   S is B-orthonormal after the two SVQB passes, so the small problem stays the standard one on T: S^T B S is not formed.
 *   The host reads four things per iteration: rn with bn, the two G and T.
 * The eigenvectors returned are B-orthonormal: X^T B X = I.  residuals[j] is the last rn_j.  matvecs counts products with `a` only
 * (k + the sum of |active|); bmatvecs = 2k - 1 + the sum of |active|.
 * DIVERGED is smm_hip_lobpcg_*'s, and also a bn_j, or a start w . q, that is not finite or not positive: B = -I ends DIVERGED at the start
 *   with nothing written.  An indefinite B that slips past the start is NOT promised to be detected: the answer is then meaningless.
 * M approximates A^-1 and must fit `a`: the rule of smm_hip_lobpcg_*, unchanged.
 * Memory: 9k vectors plus the preconditioner's own.  Fixed-order sums, no floating-point atomics: two runs give the same bits.
 * WHAT THIS IS NOT: no column-major SpMM (A W and B W are |active| SpMVs each), no indefinite B (buckling problems), no interior
 *   eigenvalues, no generalised smm_hip_eigsh_*, no hard locking.
 * SMM_HIP_ERR_INVALID (the message starts with "lobpcg:"; checked before the device is touched, the outputs are not written): everything
 * smm_hip_lobpcg_* refuses, a `b` of the other dtype, a `b` that is not square, a `b` with other rows than `a`. */
int smm_hip_lobpcg_gen_f32(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* X0,
                           long long ldx0, unsigned long long seed, float* eigenvalues, float* eigenvectors, long long ldx, float* residuals, int* nconv, int* iterations,
                           int* matvecs, int* bmatvecs, int* applies, int* solver_status);
int smm_hip_lobpcg_gen_f64(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* X0,
                           long long ldx0, unsigned long long seed, double* eigenvalues, double* eigenvectors, long long ldx, double* residuals, int* nconv, int* iterations,
                           int* matvecs, int* bmatvecs, int* applies, int* solver_status);
int smm_hip_lobpcg_gen_dev_f32(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* d_X0,
                               long long ldx0, unsigned long long seed, float* d_eigenvalues, float* d_eigenvectors, long long ldx, smm_hip_stream stream,
                               float* residuals, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* solver_status);
int smm_hip_lobpcg_gen_dev_f64(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* d_X0,
                               long long ldx0, unsigned long long seed, double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream,
                               double* residuals, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* solver_status);

/* smm_hip_idrs_*: IDR(s) in the biorthogonal form (Sonneveld and van Gijzen 2008; van Gijzen and Sonneveld 2011) with right
 * preconditioning -- an addition, the reference has no IDR(s) (csrc/smm_solvers_idrs.hip; the definition, line by line, is
 * tests/idrs_restatement.py).  For general matrices: transpose-free, one SpMV per step, recurrences of the fixed length s with no
 * restart, and s shadow vectors where BiCGStab has one (s = 1 is mathematically BiCGStab).
 * Semantics (x in/out; `iterations` counts SpMVs: every inner step and every dimension-reduction step is one):
 *   maxIterations < 0 means rows; there is no other clamp
 *   r = b - A x;  rr = r.r;  G = U = 0 (rows x s);  M = I (s x s);  om = 1
 *   while (rr > eps*eps && iterations < maxIterations) {                               -- a cycle
 *     f = P^T r                                                      (s dot products)
 *     for k = 0 .. s-1:
 *       c[k:] = solve(lower(M[k:, k:]), f[k:])                       forward substitution
 *       v = r;  v = _smm_fma(-c_i, G_i, v), i = k .. s-1 ascending
 *       z = M^-1 v                                                   (right preconditioning: the residual tested is the recurrence
 *                                                                     residual of the original system)
 *       u = om * z;  u = _smm_fma(c_i, U_i, u), i = k .. s-1 ascending
 *       g = A u;  h = P^T g                                          (s dot products, all from the same g)
 *       a_i = (h_i - sum_{j<i} M[i][j] a_j) / M[i][i], i < k         (one pass of classical Gram-Schmidt against the biorthogonal set)
 *       g = _smm_fma(-a_i, G_i, g);  u = _smm_fma(-a_i, U_i, u), i < k ascending;  G_k = g;  U_k = u
 *       M[i][k] = h_i - sum_{j<k} M[i][j] a_j for i >= k, 0 for i < k (algebraic: no second product pass)
 *       M[k][k] == 0 or not finite: DIVERGED, x and r as they are, the solve ends
 *       beta = f_k / M[k][k];  r = _smm_fma(-beta, g, r);  x = _smm_fma(beta, u, x);  rr = r.r;  iterations++
 *       !(rr > eps*eps && iterations < maxIterations): the solve ends
 *       f_i = f_i - beta M[i][k], i > k
 *     z = M^-1 r;  t = A z;  tt = t.t;  tr = t.r
 *     tt == 0 or not finite: DIVERGED, the solve ends
 *     rho = |tr| / sqrt(tt * rr);  om = tr / tt;  if (rho < 0.7) om = om * (0.7 / rho)       ("maintaining the convergence")
 *     x = _smm_fma(om, z, x);  r = _smm_fma(-om, t, r);  rr = r.r;  iterations++
 *   }
 *   status: SUCCESS iff the last rr <= eps*eps; else DIVERGED on the two tests above; else MAX_ITERATIONS_REACHED (a NaN rr leaves
 *   the loop and reports MAX_ITERATIONS_REACHED unless one of the two tests fired)
 * maxIterations == 0, rows == 0 and an x that already passes the test take no step: x untouched; SUCCESS in the last two cases.
 * The shadow space P: 1 <= s <= SMM_IDRS_MAX_S columns of `rows` elements.  smm_hip_idrs_dev_*: d_P != NULL is a device array, column i
 *   at d_P + i * ldP (ldP >= rows; element alignment suffices), read only and used as given; d_P == NULL: the library generates P from
 *   `seed` for the duration of the call, as smm_hip_idrs_* (host vectors) always does.
 * smm_hip_idrs_shadow_dev_*: fills d_P (column i at d_P + i * ld) the way the library generates it, so that a caller who solves many
 *   systems keeps one P: element (row, col) = ((h >> 40) + 0.5) 2^-23 - 1 with h = sm(sm(sm(seed) ^ col) ^ row), sm(z) the splitmix64
 *   step (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31) -- exact
 *   in fp32 and fp64 -- then the columns are made orthonormal by classical Gram-Schmidt applied twice, column by column, and a division
 *   by the norm.  Synchronises `stream`.  A solve with this P passed in (16-byte aligned, ld a multiple of 64) gives the bits of the
 *   solve that generates it from the same seed.  s > rows gives dependent columns: no error, the solve reports what the loop makes of it.
 * M: NULL, or any kind smm_hip_gmres_* accepts, created for `a`.
 * Memory: 3 s vectors (G, U and P, leading dimension rounded up to 64; 2 s with a caller's P) plus two (four with a preconditioner).
 * The sums run in a fixed order and nothing uses floating-point atomics: two runs of one solve give the same bits.
 * SMM_HIP_ERR_INVALID: s outside 1 .. SMM_IDRS_MAX_S, ldP < rows with a d_P, a null or dtype-mismatched matrix, a matrix that is not
 * square, null vectors with rows > 0, a preconditioner of another matrix or kind; x is not touched.
 * Additive outputs (may be NULL, like solver_status): iterations, resnorm2 = the last rr. */
#define SMM_IDRS_MAX_S 8
int smm_hip_idrs_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int s, const smm_hip_precond* M, unsigned long long seed,
                     int* solver_status, int* iterations, float* resnorm2);
int smm_hip_idrs_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int s, const smm_hip_precond* M, unsigned long long seed,
                     int* solver_status, int* iterations, double* resnorm2);
int smm_hip_idrs_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, int s, const smm_hip_precond* M, const float* d_P,
                         long long ldP, unsigned long long seed, smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_idrs_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, int s, const smm_hip_precond* M, const double* d_P,
                         long long ldP, unsigned long long seed, smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2);
int smm_hip_idrs_shadow_dev_f32(int n, int s, unsigned long long seed, float* d_P, long long ld, smm_hip_stream stream);
int smm_hip_idrs_shadow_dev_f64(int n, int s, unsigned long long seed, double* d_P, long long ld, smm_hip_stream stream);

/* smm_hip_refine_*: MIXED-PRECISION ITERATIVE REFINEMENT -- an fp64 answer from fp32 solves; an addition, the reference has none
 * (csrc/smm_solvers_refine.hip; the definition, line by line, is tests/refine_restatement.py).
 * `a` is the fp64 matrix, `a32` an fp32 matrix of the same rows, cols and nnz: a's values rounded (smm_hip_csr_convert_create(a,
 * SMM_DTYPE_F32, ...)) -- that it holds them is the caller's contract: another matrix of that shape is no error, it gives steps that the
 * acceptance rule below rejects.  a32 == NULL: the library converts `a` for the duration of the call (M32 must be NULL then); callers
 * solving more than once should keep an a32 -- and with it the PATTERN analysis, the preconditioner and the conversion pass itself.
 * Semantics (x in/out):
 *   r = b - A x (fp64);  rr = r.r;  outer = 0;  inner_total = 0
 *   while (rr > eps*eps && outer < maxOuter) {
 *     (m, e) = frexp(sqrt(rr))                     -- sqrt(rr) = m 2^e, m in [0.5, 1)
 *     r32[i] = (float)(r[i] * 2^-e)                -- exact scaling, one rounding: ||r32|| is in about [0.5, 1) whatever ||b|| is
 *     d32 = 0;  the inner solve of A32 d32 = r32 by smm_hip_cg_dev_f32 / smm_hip_bicgstab_dev_f32 / smm_hip_gmres_dev_f32 with
 *               (maxInner, innerEps[, restart], M32) unchanged: its own -1 rule and convergence test, AUTO kernel choice, the resident
 *               forms and the zero start apply as they do for any fp32 solve
 *     inner_total += the inner driver's iterations
 *     xc[i] = fma(2^e, (double)d32[i], x[i])       -- a candidate, in a vector of its own (the product is exact: one rounding)
 *     rc = b - A xc;  rrc = rc.rc
 *     if (!(rrc < rr)) { rejected; break }         -- a NaN included: x keeps its bits
 *     x = xc;  r = rc;  rr = rrc;  outer++
 *   }
 *   status: DIVERGED if a step was rejected or rr is not finite; else SUCCESS if !(rr > eps*eps); else MAX_ITERATIONS_REACHED
 * Guarantees: the true fp64 residual of the returned x is never larger than that of the given x.  A rejected step or a failed call leaves
 * x bit for bit.  resnorm2 is the true ||b - A x||^2 of the returned x, computed in fp64 by the handle's SpMV and a dot product -- not a
 * recurrence.  A start with rr <= eps*eps returns x untouched, 0 outer and 0 inner iterations, SUCCESS.  rows == 0: SUCCESS with zeros,
 * nothing is read or written through b / x.  Whatever status the inner solve reports, the candidate is judged by its true residual alone.
 * A negative return of the inner driver (a preconditioner of another matrix or of a kind that solver does not take, a restart out of
 * range) is handed on and x keeps its bits.
 * Refinement contracts only while cond(A) 2^-24 is well below 1; beyond that the first step is rejected: DIVERGED, x intact.
 * M32: NULL, or a preconditioner created for a32 of a kind the chosen inner solver accepts.  restart is read for GMRES only.
 * Host: rr comes to the host once per outer step (it decides the loop and e); the call synchronises `stream`.  Workspace: two fp64 and two
 * fp32 vectors.  Per outer step beside the inner solve: two element-wise passes (12 bytes per row each) and one fp64 SpMV with its sum.
 * SMM_HIP_ERR_INVALID: maxOuter < 0, an unknown `inner`, a null `a`, a handle of the wrong dtype, an a32 of another shape or entry count,
 * a matrix that is not square, null vectors with rows > 0, a32 == NULL with M32 != NULL.
 * Outputs (each may be NULL): solver_status, outer_iterations, inner_iterations (summed over the outer steps), resnorm2. */
#define SMM_REFINE_INNER_CG 0
#define SMM_REFINE_INNER_BICGSTAB 1
#define SMM_REFINE_INNER_GMRES 2
int smm_hip_refine_f64(const smm_hip_csr* a, const smm_hip_csr* a32, double* b, double* x, int inner, int maxOuter, int maxInner, double eps, float innerEps,
                       int restart, const smm_hip_precond* M32, int* solver_status, int* outer_iterations, int* inner_iterations, double* resnorm2);
int smm_hip_refine_dev_f64(const smm_hip_csr* a, const smm_hip_csr* a32, const double* d_b, double* d_x, int inner, int maxOuter, int maxInner, double eps,
                           float innerEps, int restart, const smm_hip_precond* M32, smm_hip_stream stream, int* solver_status, int* outer_iterations,
                           int* inner_iterations, double* resnorm2);

/* The two dense kernels of GMRES's Gram-Schmidt on device pointers: d_V holds k columns of n elements, column i at d_V + i * ld (ld >= n;
 * what lies between n and ld is never read), 1 <= k <= SMM_GMRES_MAX_RESTART + 1.  Asynchronous on `stream`.
 *   multi_dot:  d_out[i] = v_i . d_w for all i < k, d_w read once per 8 columns; accumulation in T, fixed order
 *   multi_axpy: d_out = d_w + sum_i d_coef[i] v_i, i ascending, each term through _smm_fma; d_out may alias d_w (not d_V)
 * Every pointer may be element-aligned; 16-byte loads are used when d_V, d_w (and d_out) are 16-byte aligned and ld keeps the columns so.
 * SMM_HIP_ERR_INVALID: n < 0, k out of range, ld < n, a null array with n > 0 (multi_dot: a null d_out always). */
int smm_hip_multi_dot_dev_f32(int n, int k, const float* d_V, long long ld, const float* d_w, float* d_out, smm_hip_stream stream);
int smm_hip_multi_dot_dev_f64(int n, int k, const double* d_V, long long ld, const double* d_w, double* d_out, smm_hip_stream stream);
int smm_hip_multi_axpy_dev_f32(int n, int k, const float* d_V, long long ld, const float* d_coef, const float* d_w, float* d_out, smm_hip_stream stream);
int smm_hip_multi_axpy_dev_f64(int n, int k, const double* d_V, long long ld, const double* d_coef, const double* d_w, double* d_out, smm_hip_stream stream);

/* multi_rotate: the in-place basis compression of smm_hip_eigsh_*: V[:, 0..l-1] = V[:, 0..m-1] Y, with d_V as above (m columns of n
 * elements, column i at d_V + i * ld) and h_Y an m x l matrix in HOST memory, column-major, element (i, c) at h_Y[i + c * ldY]
 * (ldY >= m); 1 <= l <= m <= SMM_EIGSH_MAX_NCV.  Rows are independent: a lane loads the m values of its rows, forms the l outputs one
 * after the other -- out_c = V_0 Y[0][c], then _smm_fma(Y[j][c], V_j, out_c) for j = 1 .. m-1 ascending -- and stores each as it is formed;
 * it holds its whole row by then, so column c may be overwritten.  n m elements are read and n l written, none twice; the columns
 * l .. m-1 keep their bits, and what lies between n and ld is neither read nor written.  m is padded to 16 / 32 / 64 by zero rows of
 * Y (the padding columns of V are not loaded).  16-byte loads and stores (four fp32 or two fp64 rows per lane) are used when d_V is
 * 16-byte aligned, ld keeps the columns so and the padded m is at most 32; otherwise -- and always for the padding 64, where a pack of
 * rows would need 256 registers a lane -- a lane owns one row, and a wavefront's load of a column is still one contiguous run.
 * Synchronises `stream` (the staged copy of Y is released on return).
 * SMM_HIP_ERR_INVALID: n < 0, l < 1, m < l, m > SMM_EIGSH_MAX_NCV, ld < n, ldY < m, a null h_Y, a null d_V with n > 0; checked before
 * the device is touched. */
int smm_hip_multi_rotate_dev_f32(int n, int m, int l, float* d_V, long long ld, const float* h_Y, long long ldY, smm_hip_stream stream);
int smm_hip_multi_rotate_dev_f64(int n, int m, int l, double* d_V, long long ld, const double* h_Y, long long ldY, smm_hip_stream stream);

/* The two block x block kernels of smm_hip_lobpcg_* on device pointers (csrc/smm_multiblock.h).  d_V holds m columns and d_W l columns of
 * n elements, column i at d_V + i * ldV (ldV, ldW >= n; what lies between n and ld is neither read nor written); 1 <= m, l <=
 * SMM_LOBPCG_MAX_BASIS.  Every pointer may be element-aligned; 16-byte accesses are used when both blocks are 16-byte aligned and both
 * leading dimensions keep the columns so.  Asynchronous on `stream`.
 *   multi_gram:  d_G (m x l, column-major, element (i, j) at d_G[i + j * ldG], ldG >= m, DEVICE memory) = V^T W.  d_V == d_W with m == l
 *     and ldV == ldW is legal: the symmetric case, every element is then loaded once.  On the matrix cores (v_mfma_f64_16x16x4_f64 /
 *     v_mfma_f32_16x16x4_f32, fp32 in and out, no reduced precision): a lane loads the one element it feeds as operand, so every element
 *     of V and of W is read from memory ONCE per call; accumulation in T, per-workgroup partial sums and a finishing pass in a fixed
 *     order, no floating-point atomics: two calls give the same bits.  n == 0 gives zeros.
 *   multi_block_axpy:  W[:, c] = W[:, c] - sum_j d_H[j + c * ldH] V[:, j] for all c < l, j ascending, each term
 *     _smm_fma(-H[j][c], V_j, W_c).  d_H is m x l, column-major, ldH >= m, in DEVICE memory: a multi_gram result feeds it with no host
 *     read in between.  V and W must not overlap.  A lane holds its rows of V: each element of V is read once, each of W read and
 *     written once.
 * SMM_HIP_ERR_INVALID (checked before the device is touched): n < 0, m or l outside 1 .. SMM_LOBPCG_MAX_BASIS, ldV < n, ldW < n,
 * ldG / ldH < m, a null d_G / d_H, a null d_V or d_W with n > 0. */
int smm_hip_multi_gram_dev_f32(int n, int m, int l, const float* d_V, long long ldV, const float* d_W, long long ldW, float* d_G, long long ldG, smm_hip_stream stream);
int smm_hip_multi_gram_dev_f64(int n, int m, int l, const double* d_V, long long ldV, const double* d_W, long long ldW, double* d_G, long long ldG,
                               smm_hip_stream stream);
int smm_hip_multi_block_axpy_dev_f32(int n, int m, int l, const float* d_V, long long ldV, const float* d_H, long long ldH, float* d_W, long long ldW,
                                     smm_hip_stream stream);
int smm_hip_multi_block_axpy_dev_f64(int n, int m, int l, const double* d_V, long long ldV, const double* d_H, long long ldH, double* d_W, long long ldW,
                                     smm_hip_stream stream);

/* multi_block_axpy and multi_rotate on 1 <= nb <= SMM_LOBPCG_MAX_BASES bases with ONE coefficient matrix in ONE launch (smm_hip_lobpcg_gen_*
 * updates S, AS and BS by the same small matrix).  d_V and d_W are HOST arrays of nb device pointers, copied into the kernel's arguments:
 * a grid dimension runs over the bases.  All bases share one ldV and one ldW (one ld for multi_rotate_bases); d_H, h_Y and every other
 * parameter are the single-basis entry's, and for every i < nb the result on d_V[i] / d_W[i] is bit for bit that of
 * smm_hip_multi_block_axpy_dev_*(n, m, l, d_V[i], ldV, d_H, ldH, d_W[i], ldW) / smm_hip_multi_rotate_dev_*(n, m, l, d_V[i], ld, h_Y, ldY)
 * alone: each basis takes the 16-byte path or the element path by its own alignment, and what lies between n and ld is neither read
 * nor written.  multi_block_axpy_bases is asynchronous on `stream`; multi_rotate_bases stages Y once for all bases and synchronises `stream`.
 * SMM_HIP_ERR_INVALID (the message starts with "multi_block_axpy_bases:" / "multi_rotate_bases:"; checked before the device is touched):
 * what the single-basis entry refuses, nb outside 1 .. SMM_LOBPCG_MAX_BASES, a null d_V / d_W, a null entry in either with n > 0, and for
 * multi_block_axpy_bases any V[i] (m columns) that overlaps any W[j] (l columns). */
int smm_hip_multi_block_axpy_bases_dev_f32(int n, int m, int l, int nb, const float* const* d_V, long long ldV, const float* d_H, long long ldH, float* const* d_W,
                                           long long ldW, smm_hip_stream stream);
int smm_hip_multi_block_axpy_bases_dev_f64(int n, int m, int l, int nb, const double* const* d_V, long long ldV, const double* d_H, long long ldH, double* const* d_W,
                                           long long ldW, smm_hip_stream stream);
int smm_hip_multi_rotate_bases_dev_f32(int n, int m, int l, int nb, float* const* d_V, long long ld, const float* h_Y, long long ldY, smm_hip_stream stream);
int smm_hip_multi_rotate_bases_dev_f64(int n, int m, int l, int nb, double* const* d_V, long long ld, const double* h_Y, long long ldY, smm_hip_stream stream);

/* ---- preconditioners: `int apply(const T* rhs, T* x) const noexcept` (ref:1173-1235) --------------------------
 * create: replaces CSRMatrix<T>::getPreconditioner<kind>() (ref:1643-1651) / IC0Preconditioner::init (ref:1798).
 * The matrix must outlive the preconditioner (the reference holds a const CSRMatrix&).  Structural failures
 * (missing or |d|<1e-5 diagonal, empty row, non-SPD IC0 pivot) return SMM_HIP_ERR_PRECOND. */
int smm_hip_precond_create(const smm_hip_csr* a, int kind, smm_hip_precond** out);
/* The block kinds with a chosen block size: blocks of at most block_rows rows (64 .. 2048; 0 = the default, 1024) and at most 8192
 * stored entries; smm_hip_precond_create uses the default.  The partition is a property of the handle:
 * smm_hip_precond_block_bounds returns nblocks + 1 numbers (bounds[0] = 0, bounds[nblocks] = rows) -- row numbers when the blocks are
 * runs of consecutive rows, positions in the row order of smm_hip_precond_block_rows when they are bricks of a grid (see
 * smm_hip_precond_create_block_ex: grid stencils get bricks by default). */
int smm_hip_precond_create_block(const smm_hip_csr* a, int kind, int block_rows, smm_hip_precond** out);
/* ... and a chosen LEVEL CUT.  Inside a block the forward sweep gives every row a level (0 when it keeps no entry left of the
 * diagonal, else 1 + the deepest level of the rows its kept entries point to), the backward sweep likewise; entries that point to
 * a row of level level_cap - 1 are dropped from M (like the entries that couple two blocks), so no sweep of any block runs deeper
 * than level_cap dependent levels.  level_cap: -1 = the default (16), 0 = no cut (M = the block-diagonal part of A exactly), else
 * 2 .. 4095.  The rule is a recurrence in the sweep's own row order; the tests' CPU checker states it sequentially
 * (block_level_cut) and the device result is compared with it bit for bit.  smm_hip_precond_create / _create_block use the default. */
int smm_hip_precond_create_block_capped(const smm_hip_csr* a, int kind, int block_rows, int level_cap, smm_hip_precond** out);
/* ... and a chosen PARTITION.  CONTIGUOUS: blocks are runs of consecutive rows (cut greedily from row 0).  BRICKS: for a matrix that is
 * a 2-D / 3-D grid stencil in natural order -- its entries use the offsets {0, +-1, +-nx[, +-nx ny]}, found and verified by the PATTERN
 * analysis -- the blocks are bricks of the grid (16 x 8 x 8 points for 1024 rows; squares in 2-D), so that M keeps the couplings of all
 * grid directions inside a block; the rows of a block keep their natural order.  Any other matrix: SMM_HIP_ERR_INVALID.  AUTO (what
 * every other create call uses): bricks where they apply, contiguous otherwise (SMM_HIP_BLOCK_BRICKS=0: always contiguous).
 * smm_hip_precond_block_rows returns the rows block by block (order[bounds[b] .. bounds[b+1]) are block b's rows; the identity for
 * contiguous blocks) and the brick's extent along the grid axes ({0, 0, 0} for contiguous blocks); either pointer may be NULL. */
#define SMM_BLOCKS_AUTO 0
#define SMM_BLOCKS_CONTIGUOUS 1
#define SMM_BLOCKS_BRICKS 2
int smm_hip_precond_create_block_ex(const smm_hip_csr* a, int kind, int block_rows, int level_cap, int partition, smm_hip_precond** out);
int smm_hip_precond_block_rows(const smm_hip_precond* M, int* order, size_t count, int* brick);
/* Bytes one apply reads per row besides rhs / x (/ w1): the fixed-size record of the lower and of the upper sweep, and the row-order
 * entries of a brick partition.  (Rows with more in-block entries than a record holds continue in overflow lists, not counted.) */
int smm_hip_precond_block_record_bytes(const smm_hip_precond* M, int* lower, int* upper, int* order);
int smm_hip_precond_block_level_cap(const smm_hip_precond* M, int* level_cap);
int smm_hip_precond_block_count(const smm_hip_precond* M, int* nblocks);
int smm_hip_precond_block_bounds(const smm_hip_precond* M, int* bounds, size_t count);
/* The Chebyshev preconditioner (SMM_PRECOND_CHEBYSHEV) with every parameter.  degree 0 .. SMM_CHEB_MAX_DEGREE.  The bounds on the spectrum
 * of D^-1 A are fixed at create time, on the device, and kept in the handle:
 *   GERSHGORIN  lambda_max = max_i (sum_j |a_ij|) / |a_ii|: each row summed in DOUBLE, sequentially, in stored order, divided in double,
 *               the maximum taken over the rows -- independent of the launch geometry, the same bits in both dtypes as that sentence
 *               evaluated on the host.  A true upper bound.  One kernel and one 8-byte read-back.
 *   POWER       power_steps (1 .. 1000; 10 is the usual choice) steps of the power method on D^-1 A from the fixed start
 *               v[i] = 1 + (i mod 7) / 8: w = (A v) / diag, rq = (v.w) / (v.v), v = w / sqrt(w.w) (dot products in T, quotient and root in
 *               double); lambda_max = min(GERSHGORIN, 1.1 * the last rq).  A HEURISTIC, NOT A BOUND: the Rayleigh quotient approaches the
 *               largest eigenvalue from below, and 1.1 is a customary safety factor, not a proof.  An eigenvalue above lambda_max is
 *               amplified by the polynomial instead of damped; a solver then stalls or diverges.
 *   USER        lambda_min and lambda_max are the caller's, returned unchanged by smm_hip_precond_chebyshev_info.
 * Outside USER lambda_min = lambda_max / eig_ratio (lambda_min, lambda_max arguments ignored).  30 is the customary smoother setting
 * and what smm_hip_precond_create uses; it has NOT been tuned or measured on this hardware.
 * SMM_HIP_ERR_PRECOND: a missing diagonal or one with |d| < 1e-5 (the Jacobi rule), an empty row, a bound that is not finite or not
 * positive, lambda_min >= lambda_max, eig_ratio <= 1.  SMM_HIP_ERR_INVALID: degree outside 0 .. 64, an unknown bound_mode, power_steps
 * outside 1 .. 1000 with POWER, a matrix that is not square.  A matrix with no rows gives a handle whose apply does nothing (bounds
 * reported: 1 / eig_ratio and 1, or the caller's).
 * The handle owns the two scratch vectors of an apply (allocated here; an apply allocates nothing), so ONE HANDLE MUST NOT BE APPLIED
 * FROM TWO STREAMS AT ONCE -- create one handle per stream.  Like every snapshot kind it does not follow a value edit of `a` (the
 * diagonal copy and the bounds are taken here; the SpMVs inside an apply would use the edited A): create a new one after an edit.
 * smm_hip_precond_values_* returns the diagonal copy (rows values).  Batched and row-partitioned solvers refuse the kind. */
#define SMM_CHEB_BOUND_GERSHGORIN 0
#define SMM_CHEB_BOUND_POWER 1
#define SMM_CHEB_BOUND_USER 2
#define SMM_CHEB_MAX_DEGREE 64
int smm_hip_precond_create_chebyshev(const smm_hip_csr* a, int degree, int bound_mode, double eig_ratio, int power_steps, double lambda_min,
                                     double lambda_max, smm_hip_precond** out);
/* degree, bound mode and the two bounds (as doubles) of a Chebyshev handle; any pointer may be NULL.  SMM_HIP_ERR_INVALID for other kinds. */
int smm_hip_precond_chebyshev_info(const smm_hip_precond* M, int* degree, int* bound_mode, double* lambda_min, double* lambda_max);
/* The multigrid preconditioner (SMM_PRECOND_AMG, defined above) with every parameter.
 * SMM_HIP_ERR_INVALID: a matrix that is not square; theta outside [0, 1) or not finite; max_levels outside 1 .. 16; coarse_rows outside
 * 1 .. 1024; smooth_degree outside 0 .. 64.  SMM_HIP_ERR_PRECOND: eig_ratio not finite or <= 1; on any level an empty row, a missing
 * diagonal or |d| < 1e-5; a coarsest level of more than 1024 rows; a singular coarsest matrix.  A matrix with no rows gives a handle
 * whose apply does nothing.
 * Set-up cost: per level three sparse products (S T, A P, R (A P)) and one transpose, a handful of one-lane-per-row passes per round of
 * the root selection with ONE 4-byte read-back per round, two scans, and the host inversion of the coarsest matrix (n_L^3 operations).
 * The handle owns every level's matrices, smoothers and vectors (allocated here; an apply allocates nothing), so ONE HANDLE MUST NOT BE
 * APPLIED FROM TWO STREAMS AT ONCE.  It is a SNAPSHOT: it does not follow a value edit of `a` -- call smm_hip_precond_amg_refresh, or
 * create a new one.
 * amg_refresh: keeps every aggregate and every pattern and redoes the values from the present values of `a`: S is refilled, P, A P and
 *   A_{l+1} are recomputed by smm_hip_csr_multiply_into_*, R by smm_hip_csr_transpose_refresh_*, the smoothers are re-made and the coarse
 *   inverse recomputed.  Afterwards the values equal those of a fresh create on a matrix whose aggregates come out the same.
 *   Synchronous.  On an error the handle must not be applied any more (destroy it).
 * amg_info: the number of levels, rows[l] and nnz[l] of A_l for l < count (either array may be NULL), and the operator complexity
 *   sum_l nnz(A_l) / nnz(A_0).
 * amg_level: BORROWED handles owned by M (do not destroy them; they die with M): A_l, P_l, R_l; P_l and R_l are NULL on the coarsest
 *   level.  They may be read (smm_hip_csr_get_pattern / _get_values_*) and their kernel choice set (smm_hip_csr_set_kernel).
 * amg_aggregates: the aggregate number of the first `count` rows of level l (count <= rows of that level); the coarsest level has none
 *   (SMM_HIP_ERR_INVALID).
 * amg_coarse_inverse_*: the first `count` values of the dense inverse of the coarsest matrix, row-major, n_L x n_L. */
#define SMM_AMG_MAX_LEVELS 16
#define SMM_AMG_MAX_COARSE_ROWS 1024
int smm_hip_precond_create_amg(const smm_hip_csr* a, double theta, int max_levels, int coarse_rows, int smooth_degree, double eig_ratio,
                               smm_hip_precond** out);
int smm_hip_precond_amg_refresh(smm_hip_precond* M);
int smm_hip_precond_amg_info(const smm_hip_precond* M, int* levels, int* rows, int* nnz, size_t count, double* operator_complexity);
int smm_hip_precond_amg_level(const smm_hip_precond* M, int level, smm_hip_csr** a_l, smm_hip_csr** p_l, smm_hip_csr** r_l);
int smm_hip_precond_amg_aggregates(const smm_hip_precond* M, int level, int* agg, size_t count);
int smm_hip_precond_amg_coarse_inverse_f32(const smm_hip_precond* M, float* out, size_t count);
int smm_hip_precond_amg_coarse_inverse_f64(const smm_hip_precond* M, double* out, size_t count);
/* The multigrid preconditioner created with NEAR-NULL-SPACE CANDIDATES: smoothed aggregation after Vanek, Mandel and Brezina (1996), for
 * vector-valued problems.  For linear elasticity the candidates are the rigid body modes (3 in the plane, 6 in space); with one dof per
 * node and the constant vector it is the hierarchy above up to the scaling of T.  smm_hip_precond_create_amg is untouched by all this.
 * The definition, line by line: tests/amg_candidates_restatement.py.
 * B: n x k, COLUMN-MAJOR with leading dimension n, 1 <= k <= 6, in the matrix dtype (the suffix names it); read during the call only.
 *   The _dev_ forms take it in device memory, in use on `stream` (which they synchronise).
 * dofs_per_node: b, 1 .. 4, a divisor of n: rows b I .. b I + b - 1 are node I.  Deeper levels have k dofs per node.
 * Per level l (block size b_l = b on level 0, k below), where it differs from SMM_PRECOND_AMG above:
 *   node graph  b_l > 1: N = Tb^T ((A_l o A_l) Tb) by smm_hip_csr_multiply_create and smm_hip_csr_transpose_create, Tb the n x n / b_l
 *               matrix with one 1 per row at column i / b_l, A o A the values squared (one rounding), then the square root of every
 *               value of N: N_IJ is the Frobenius norm of block (I, J).  Strength, roots and aggregates are those above, on N with N's
 *               diagonal; a dof takes its node's aggregate.  b_l = 1: A_l itself, as above.
 *   T           n x n_agg k.  The member dofs of aggregate a in ascending order are the rows 0 .. m - 1 of its block V of B_l (m x k).
 *               Thin QR by modified Gram-Schmidt.  EVERY inner product x . y: lane t of 64 sums the rows t, t + 64, ... in ascending
 *               order from +0.0 with _smm_fma, then the xor butterfly (32, 16, ... 1) of the dot kernels: a function of m alone, the
 *               same bits in every run.  Column by column, c ascending: norm0 = sqrt(v_c . v_c) as given; for j < c ascending
 *               r_jc = q_j . v_c and, where column j was kept, v_c = _smm_fma(-r_jc, q_j, v_c); nrm = sqrt(v_c . v_c); the column is
 *               KEPT iff nrm > SMM_AMG_DROP_TOL * norm0 (one product in T): r_cc = nrm, q_c = v_c / nrm.  Otherwise it is DROPPED:
 *               q_c = 0, r_cc = 0 and row c of R is zero.  An aggregate of fewer than k rows, candidates that are dependent on it and
 *               a column that is zero there all end this way: rank deficiency is an ordinary input.  Row i of T holds q_c of its
 *               aggregate at column a k + c for the kept c only; B_{l+1} (n_agg k x k) holds R at rows a k .. a k + k - 1, so that
 *               T B_{l+1} = B_l up to rounding and what was dropped.
 *   A_{l+1}     R_l (A_l P_l) + E, E the matrix with a stored 1 on the diagonal of every coarse dof whose column of T is empty (its row
 *               and column of R_l (A_l P_l) are empty): a decoupled identity row, by smm_hip_csr_add_create_*; a level with no dropped
 *               column takes R_l (A_l P_l) itself.  No level has a zero diagonal.
 *   the level is the coarsest when it would not shrink: 10 n_agg k >= 9 n.
 * SMM_AMG_DROP_TOL = 2^-13: far above the rounding left by an exact dependency in either dtype (a few k eps of norm0), far below the
 * part of a rigid rotation that is independent of the translations on an aggregate unless the body lies some thousand aggregate
 * diameters from the point the rotations turn about -- so fp32, fp64 and the restatement decide alike.
 * SMM_HIP_ERR_INVALID: what smm_hip_precond_create_amg refuses so; k outside 1 .. 6; dofs_per_node outside 1 .. 4 or not a divisor of
 * the rows; rows * k >= 2^31; the other dtype; a value of B that is not finite.  A column of B that is zero everywhere is dropped on
 * every aggregate, not refused.  SMM_HIP_ERR_PRECOND: as smm_hip_precond_create_amg.
 * Set-up cost beyond the above, per level: two products and a transpose for N, one stable radix sort of n keys, the QR kernel (one
 * wavefront per aggregate, 16 or 32 lanes where no aggregate of the level is larger; the block sits in LDS up to
 * SMM_AMG_QR_LDS_ROWS rows and in global memory beyond: reads and writes n k values once each), three 4 n_agg-byte read-backs.
 * amg_refresh keeps the aggregates, T and every B_l (the QR does not depend on the values of `a`) and redoes S, the products and the sum
 * with E.  amg_info, amg_level, amg_aggregates (the aggregate of every DOF) and amg_coarse_inverse_* serve such a handle as any other.
 * amg_candidates_*: the first `count` values of B_l of level `level` (n_l x k column-major; b_l may be NULL with count 0), *k, the
 *   number of columns dropped on that level (0 on the coarsest) and T_l, BORROWED like amg_level's handles (NULL on the coarsest level);
 *   any of the three pointers may be NULL.  SMM_HIP_ERR_INVALID for a handle created without candidates. */
#define SMM_AMG_MAX_CANDIDATES 6
#define SMM_AMG_MAX_DOFS_PER_NODE 4
#define SMM_AMG_DROP_TOL 0.0001220703125 /* 2^-13 */
#define SMM_AMG_QR_LDS_ROWS 256
int smm_hip_precond_create_amg_candidates_f32(const smm_hip_csr* a, const float* B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                              int smooth_degree, double eig_ratio, smm_hip_precond** out);
int smm_hip_precond_create_amg_candidates_f64(const smm_hip_csr* a, const double* B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                              int smooth_degree, double eig_ratio, smm_hip_precond** out);
int smm_hip_precond_create_amg_candidates_dev_f32(const smm_hip_csr* a, const float* d_B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                                  int smooth_degree, double eig_ratio, smm_hip_stream stream, smm_hip_precond** out);
int smm_hip_precond_create_amg_candidates_dev_f64(const smm_hip_csr* a, const double* d_B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                                  int smooth_degree, double eig_ratio, smm_hip_stream stream, smm_hip_precond** out);
int smm_hip_precond_amg_candidates_f32(const smm_hip_precond* M, int level, float* b_l, size_t count, int* k, int* dropped, smm_hip_csr** t_l);
int smm_hip_precond_amg_candidates_f64(const smm_hip_precond* M, int level, double* b_l, size_t count, int* k, int* dropped, smm_hip_csr** t_l);
/* The multicolour kinds (SMM_PRECOND_MULTICOLOR_*, defined above) with a colouring of the caller's.  base_kind: SMM_PRECOND_SGS, _ILU0 or
 * _IC0.  colors: NULL (count ignored) for smm_hip_csr_color's, or `count` == rows colours on the HOST, each in [0, rows); it is checked
 * on the device -- a stored entry (i, j), i != j, with colors[i] == colors[j] gives SMM_HIP_ERR_INVALID.  Colours nobody holds are
 * allowed (they are empty levels); ncolors = the largest colour + 1.  smm_hip_precond_create(a, SMM_PRECOND_MULTICOLOR_*, ...) passes NULL.
 * multicolor_refresh: keeps the colouring, the permutation and B's pattern; B's values are gathered from the present values of `a`
 *   and the factor is recomputed: afterwards the handle equals a newly created one bit for bit.  Synchronous.  Errors as create's; on
 *   an error the handle must not be applied any more (destroy it).
 * multicolor_info: ncolors, and the first `count` (<= ncolors + 1) of the row bounds of the colours in B (bounds[0] = 0,
 *   bounds[ncolors] = rows); either pointer may be NULL.
 * multicolor_perm: the first `count` (<= rows) entries of perm[] (new row i is row perm[i] of `a`).
 * multicolor_matrix: B as a BORROWED handle owned by M (do not destroy it; it dies with M); it may be read (smm_hip_csr_get_pattern /
 *   _get_values_*). */
int smm_hip_precond_create_multicolor(const smm_hip_csr* a, int base_kind, const int* colors, size_t count, smm_hip_precond** out);
int smm_hip_precond_multicolor_refresh(smm_hip_precond* M);
int smm_hip_precond_multicolor_info(const smm_hip_precond* M, int* ncolors, int* bounds, size_t count);
int smm_hip_precond_multicolor_perm(const smm_hip_precond* M, int* perm, size_t count);
int smm_hip_precond_multicolor_matrix(const smm_hip_precond* M, smm_hip_csr** b);
/* The approximate-inverse kinds (SMM_PRECOND_FSAI / SMM_PRECOND_SPAI, defined above) on the pattern of the power-th structural power of a.
 * SMM_HIP_ERR_INVALID: a matrix that is not square, a kind other than 12 or 13, power outside 1 .. SMM_AINV_MAX_POWER, a column outside
 * the matrix.  SMM_HIP_ERR_PRECOND: a missing diagonal, a row of the pattern longer than SMM_AINV_MAX_ROW, a failed row (above).  A matrix
 * with no rows gives a handle whose apply does nothing.  Set-up: power - 1 symbolic products, (SPAI) one transpose and one product, one
 * launch that gathers and solves all row systems out of LDS, (FSAI) one transpose.
 * ainv_refresh: keeps every pattern and redoes the values from the present values of `a`: a^T by smm_hip_csr_transpose_refresh_*, a a^T by
 *   smm_hip_csr_multiply_into_*, the solve, Gt by transpose_refresh; afterwards the handle equals a newly created one bit for bit.
 *   Synchronous.  Errors as create's; on an error the handle must not be applied any more (destroy it).
 * ainv_info: the power, the longest row of the pattern and the entries of G / M; any pointer may be NULL.
 * ainv_matrix: G (FSAI) or M (SPAI) and Gt (NULL for SPAI) as BORROWED handles owned by M (do not destroy them; they die with M); they may
 *   be read (smm_hip_csr_get_pattern / _get_values_*) and their kernel choice set (smm_hip_csr_set_kernel).  Either pointer may be NULL.
 * The three queries return SMM_HIP_ERR_INVALID for a handle of another kind. */
#define SMM_AINV_MAX_ROW 64
#define SMM_AINV_MAX_POWER 4
int smm_hip_precond_create_ainv(const smm_hip_csr* a, int kind, int power, smm_hip_precond** out);
int smm_hip_precond_ainv_refresh(smm_hip_precond* M);
int smm_hip_precond_ainv_info(const smm_hip_precond* M, int* power, int* max_row, size_t* nnz);
int smm_hip_precond_ainv_matrix(const smm_hip_precond* M, smm_hip_csr** g, smm_hip_csr** gt);
/* The iterated-sweep kinds (SMM_PRECOND_JSWEEP_*, defined above) with chosen step counts.  base_kind: SMM_PRECOND_SGS, _ILU0 or _IC0.
 * sweeps_lower / sweeps_upper: 0 for the default (SMM_JSWEEP_DEFAULT_SWEEPS), else 1 .. SMM_JSWEEP_MAX_SWEEPS; anything else, or another
 * base_kind, is SMM_HIP_ERR_INVALID.  Other errors: the exact kind's.  A matrix with no rows gives a handle whose apply does nothing.
 * jsweep_info: the base kind, the two step counts, and the dependency levels of the two exact sweeps (one level analysis at create time;
 *   counts of levels - 1 make the apply exact); any pointer may be NULL.
 * jsweep_set_sweeps: changes the counts (0: the default), no rebuild; applies enqueued earlier keep the counts they were enqueued with.
 * jsweep_refresh: keeps the pattern, the split and the level counts; the ILU0 / IC0 factor is recomputed from the present values of `a`
 *   and the triangles' values are rewritten: afterwards the handle equals a newly created one bit for bit.  Synchronous.  Errors as
 *   create's; on an error the handle must not be applied any more (destroy it).  Like create it drains the device first, so value edits
 *   enqueued on any stream before the call are seen.
 * The three return SMM_HIP_ERR_INVALID for a handle of another kind. */
#define SMM_JSWEEP_DEFAULT_SWEEPS 3
#define SMM_JSWEEP_MAX_SWEEPS 1024
int smm_hip_precond_create_jsweep(const smm_hip_csr* a, int base_kind, int sweeps_lower, int sweeps_upper, smm_hip_precond** out);
int smm_hip_precond_jsweep_info(const smm_hip_precond* M, int* base_kind, int* sweeps_lower, int* sweeps_upper, int* levels_lower, int* levels_upper);
int smm_hip_precond_jsweep_set_sweeps(smm_hip_precond* M, int sweeps_lower, int sweeps_upper);
int smm_hip_precond_jsweep_refresh(smm_hip_precond* M);
int smm_hip_precond_destroy(smm_hip_precond* M);
int smm_hip_precond_info(const smm_hip_precond* M, int* kind, int* levels_lower, int* levels_upper);
/* How the two triangular sweeps of SGS / ILU0 / IC0 run (same numbers bit for bit either way):
 * LEVELS: one launch per dependency level (runs of small levels share a launch); SYNCFREE: one launch per sweep, rows wait on
 * per-entry ready values.  AUTO = SYNCFREE.  A sweep that fails to finish (cannot happen; bounded for safety) makes the solve
 * or apply that used it return SMM_HIP_ERR_HIP. */
#define SMM_SWEEP_AUTO 0
#define SMM_SWEEP_LEVELS 1
#define SMM_SWEEP_SYNCFREE 2
#define SMM_SWEEP_SYNCFREE_XCD 3 /* SYNCFREE with every wavefront of a sweep on ONE XCD: rows meet in that XCD's L2 */
int smm_hip_precond_set_sweep(smm_hip_precond* M, int mode);
/* x = M^-1 rhs; rhs must not alias x (ref:1667) */
int smm_hip_precond_apply_f32(const smm_hip_precond* M, const float* rhs, float* x);
int smm_hip_precond_apply_f64(const smm_hip_precond* M, const double* rhs, double* x);
int smm_hip_precond_apply_dev_f32(const smm_hip_precond* M, const float* d_rhs, float* d_x, smm_hip_stream stream);
int smm_hip_precond_apply_dev_f64(const smm_hip_precond* M, const double* d_rhs, double* d_x, smm_hip_stream stream);
/* x = M^-1 (A v), A being the matrix M was created for: the operator a preconditioned loop applies twice per pass (ref:2234-2235,
 * 2250-2251).  BLOCK_ILU0 / BLOCK_SGS form A v inside the apply's launch, each row summed in the order of its stored entries (the
 * reference's rMult, ref:1484-1489) -- no SpMV launch, A v never travels through memory; every other kind runs the SpMV and then the
 * apply.  For the BLOCK_ kinds the result is bit for bit that of smm_hip_spmv_* followed by smm_hip_precond_apply_* ONLY WHILE THE
 * MATRIX RUNS ONE LANE PER ROW (smm_hip_csr_get_kernel): with L > 1 lanes the SpMV kernels sum a row in L pieces, this call still sums
 * it as one chain, and the two agree to rounding only.  smm_hip_bicgstab_* with a BLOCK_ kind uses this call or the two launches,
 * decided per solve from the block count against the device's compute units, from whether the PATTERN analysis has run on the matrix
 * and from SMM_HIP_BLOCK_FUSE_SPMV; so with L > 1 the iterates of the same solve may differ in the last bits, and a converged run in its
 * pass count, between devices, between the first and a later solve on one handle, and with that switch
 * (tests/test_gpu_precond_block_lanes.py bounds both).  v must not alias x. */
int smm_hip_precond_apply_spmv_f32(const smm_hip_precond* M, const float* v, float* x);
int smm_hip_precond_apply_spmv_f64(const smm_hip_precond* M, const double* v, double* x);
int smm_hip_precond_apply_spmv_dev_f32(const smm_hip_precond* M, const float* d_v, float* d_x, smm_hip_stream stream);
int smm_hip_precond_apply_spmv_dev_f64(const smm_hip_precond* M, const double* d_v, double* d_x, smm_hip_stream stream);
/* The asynchronous apply cannot report a triangular sweep that failed to finish (the escape bound of the synchronisation-free sweeps:
 * it then publishes NaN and raises a sticky flag).  This call synchronises `stream`, returns SMM_HIP_ERR_HIP when a sweep applied on it
 * since the last call tripped the bound, and clears the flag.  The solver entry points call it themselves before they return. */
int smm_hip_precond_take_error(const smm_hip_precond* M, smm_hip_stream stream);
/* copies the factor values (ILU0 / IC0 / BLOCK_ILU0: nnz values on A's pattern -- for BLOCK_ILU0 the entries that couple two blocks
 * keep A's value; JACOBI, CHEBYSHEV, AMG: rows diagonal entries of (level 0 of) the matrix; FSAI / SPAI: the values of G / M on their own
 * pattern, smm_hip_precond_ainv_info tells how many) to the host */
int smm_hip_precond_values_f32(const smm_hip_precond* M, float* out, size_t count);
int smm_hip_precond_values_f64(const smm_hip_precond* M, double* out, size_t count);

/* ---- stage-wise BiCGStab for row-partitioned multi-GPU solves (one process per GPU) -------------------------------
 * The loop of ref:2191-2283 cut at its global reductions.  Each rank owns rows [row_begin, row_end) of A and the matching
 * slices of every vector.  Between a *_LOCAL stage and the following *_APPLY stage the caller all-reduces (sum) the first
 * 1 or 2 scalars of the workspace's `sums` buffer across ranks (RCCL); before each SpMV it exchanges the x-vector halo.
 * Every stage only enqueues kernels; all scalars of the recurrence stay on the device.
 *
 *   r = b - A x  (caller, SpMV)                       INIT_LOCAL  -> all-reduce sums[0]   -> INIT_APPLY
 *   ap = A p  with dot_mode 1, w1 = r0 (caller)       ALPHA_LOCAL -> all-reduce sums[0]   -> ALPHA_APPLY  (alpha, s)
 *   as = A s  with dot_mode 2, w1 = s  (caller)       OMEGA_LOCAL -> all-reduce sums[0:2] -> OMEGA_APPLY  (omega, x, r)
 *                                                                 -> all-reduce sums[0:2] -> BETA_APPLY   (res, beta, p)
 */
#define SMM_STAGE_INIT_LOCAL 1
#define SMM_STAGE_INIT_APPLY 2
#define SMM_STAGE_ALPHA_LOCAL 3
#define SMM_STAGE_ALPHA_APPLY 4
#define SMM_STAGE_OMEGA_LOCAL 5
#define SMM_STAGE_OMEGA_APPLY 6
#define SMM_STAGE_BETA_APPLY 7
typedef struct smm_hip_bicgstab_ws smm_hip_bicgstab_ws;
/* number of partial sums per reduced quantity a fused SpMV writes (d_partials holds 2x this many T) */
int smm_hip_partials_count(void);
/* SpMV with the dot products of the fresh out[] fused into the epilogue: dot_mode 0 none; 1: out.w1 -> partials[0..P);
 * 2: out.out -> partials[0..P) and out.w1 -> partials[P..2P), P = smm_hip_partials_count() */
int smm_hip_spmv_fused_dev_f32(const smm_hip_csr* m, int op, const float* d_lhs, const float* d_x, float* d_out, int dot_mode,
                               const float* d_w1, float* d_partials, smm_hip_stream stream);
int smm_hip_spmv_fused_dev_f64(const smm_hip_csr* m, int op, const double* d_lhs, const double* d_x, double* d_out, int dot_mode,
                               const double* d_w1, double* d_partials, smm_hip_stream stream);
/* The same with the reduction FINISHED in the launch: the workgroup that ends last adds the partial sums (same fixed order, same bits as
 * a separate summing kernel) and leaves the totals at d_finish[smm_hip_finish_totals_offset() + {0, 1}] (dot_mode 1: out.w1; dot_mode 2:
 * out.out, out.w1).  d_finish: smm_hip_finish_len() elements, zeroed ONCE by the caller before the first use (it carries the arrival
 * counter between launches); one buffer per stream.  What the row-partitioned solvers all-reduce right behind their SpMV. */
int smm_hip_finish_len(void);
int smm_hip_finish_totals_offset(void);
int smm_hip_spmv_fused_finish_dev_f32(const smm_hip_csr* m, int op, const float* d_lhs, const float* d_x, float* d_out, int dot_mode,
                                      const float* d_w1, float* d_finish, smm_hip_stream stream);
int smm_hip_spmv_fused_finish_dev_f64(const smm_hip_csr* m, int op, const double* d_lhs, const double* d_x, double* d_out, int dot_mode,
                                      const double* d_w1, double* d_finish, smm_hip_stream stream);
/* workspace for n local rows: owns r, r0, ap, as, the partial-sum buffer, `sums` (4 scalars) and the recurrence state */
int smm_hip_bicgstab_ws_create_f32(int n, smm_hip_bicgstab_ws** out);
int smm_hip_bicgstab_ws_create_f64(int n, smm_hip_bicgstab_ws** out);
int smm_hip_bicgstab_ws_destroy(smm_hip_bicgstab_ws* ws);
/* p and s live in the caller's halo-extended buffers (they are SpMV inputs): bind the owned slices.  d_sums (optional,
 * >= 4 scalars) replaces the workspace's own `sums` buffer, e.g. with memory the caller's collective library can see. */
int smm_hip_bicgstab_ws_bind(smm_hip_bicgstab_ws* ws, void* d_p, void* d_s, void* d_sums);
int smm_hip_bicgstab_ws_pointers(const smm_hip_bicgstab_ws* ws, void** d_r, void** d_r0, void** d_ap, void** d_as, void** d_partials,
                                 void** d_sums);
int smm_hip_bicgstab_ws_stage_f32(smm_hip_bicgstab_ws* ws, int stage, float* d_x, float eps, smm_hip_stream stream);
int smm_hip_bicgstab_ws_stage_f64(smm_hip_bicgstab_ws* ws, int stage, double* d_x, double eps, smm_hip_stream stream);
/* synchronises `stream` and returns the loop state: done flag, iterations executed, last ||r|| */
int smm_hip_bicgstab_ws_result_f32(const smm_hip_bicgstab_ws* ws, smm_hip_stream stream, int* done, int* iterations, float* resnorm);
int smm_hip_bicgstab_ws_result_f64(const smm_hip_bicgstab_ws* ws, smm_hip_stream stream, int* done, int* iterations, double* resnorm);

/* ConjugateGradient (ref:2316-2398) in the same stage-wise form, on the same workspace type (r, ap and the bound p are used):
 *   r = b - A x0 (caller)                          CG_INIT_LOCAL  -> all-reduce sums[0] -> CG_INIT_APPLY  (early exit test)
 *   Ap = A p with dot_mode 1, w1 = p (caller)      CG_ALPHA_LOCAL -> all-reduce sums[0] -> CG_ALPHA_APPLY (alpha, x, r, local ||r||^2)
 *                                                                 -> all-reduce sums[0] -> CG_BETA_APPLY  (test, beta, p)
 * d_xcur is x0 on the first iteration and x afterwards (ref:2351, 2395); x is only written once the loop runs. */
#define SMM_CG_STAGE_INIT_LOCAL 1
#define SMM_CG_STAGE_INIT_APPLY 2
#define SMM_CG_STAGE_ALPHA_LOCAL 3
#define SMM_CG_STAGE_ALPHA_APPLY 4
#define SMM_CG_STAGE_BETA_APPLY 5
int smm_hip_cg_ws_stage_f32(smm_hip_bicgstab_ws* ws, int stage, const float* d_xcur, float* d_x, float eps, smm_hip_stream stream);
int smm_hip_cg_ws_stage_f64(smm_hip_bicgstab_ws* ws, int stage, const double* d_xcur, double* d_x, double eps, smm_hip_stream stream);
/* synchronises `stream`; SolverStatus of the stage-wise CG (iterations / ||r||^2 / done come from smm_hip_bicgstab_ws_result_*) */
int smm_hip_cg_ws_status(const smm_hip_bicgstab_ws* ws, smm_hip_stream stream, int* solver_status);

/* ---- multi-GPU: rows range-partitioned over the GPUs of one node, ONE PROCESS PER GPU ------------------------------------------
 * The reference is a single-process CPU library (no counterpart).  Rank g owns rows
 * [bounds[g], bounds[g+1]) of the n_global x n_global matrix -- its slice of values / positions / start (ref:1243-1259) with
 * GLOBAL column numbers and a local start[] (start[0] == 0) -- and the matching slices of b and x.  Each SpMV first fetches the
 * x-vector halo from the owning ranks (point to point), each dot product is completed by an all-reduce of 1-2 scalars; both run
 * on a side stream of the communicator while the caller's stream computes what does not depend on them.
 *
 * Communicators:
 *   smm_hip_comm_create_rccl   RCCL over xGMI.  Rank 0 calls smm_hip_comm_unique_id and hands the 128 bytes to every rank (any
 *                              out-of-band channel: torch.distributed, MPI, a file); then every rank calls create_rccl.  librccl is
 *                              resolved with dlopen at this point, so single-GPU users of the library never need it.
 *   smm_hip_comm_create_host   the caller moves the bytes: two callbacks (sum all-reduce of a small host array; a batch of sends and
 *                              receives of host buffers).  For tests / rehearsals with several ranks on one GPU, where RCCL cannot run.
 *   smm_hip_comm_create_self   a single rank (no communication).
 * The library's device (smm_hip_init) is the one the communicator uses.  Calls on a communicator and on the distributed matrices
 * built on it are collective: every rank makes the same calls in the same order. */
typedef struct smm_hip_comm smm_hip_comm;
typedef struct smm_hip_dist_csr smm_hip_dist_csr;
#define SMM_HIP_COMM_ID_BYTES 128
#define SMM_COMM_SELF 0
#define SMM_COMM_RCCL 1
#define SMM_COMM_HOST 2
/* in-place sum over all ranks of buf[0..count); dtype is SMM_DTYPE_F32 / F64 / I64.  Return 0 on success. */
typedef int (*smm_hip_host_allreduce_fn)(void* user, void* buf, int count, int dtype);
/* post n_recv receives and n_send sends of host buffers (peer rank, pointer, byte count each) and wait for all of them */
typedef int (*smm_hip_host_sendrecv_fn)(void* user, int n_send, const int* send_peer, void* const* send_buf, const size_t* send_bytes,
                                        int n_recv, const int* recv_peer, void* const* recv_buf, const size_t* recv_bytes);
int smm_hip_comm_unique_id(void* id /* SMM_HIP_COMM_ID_BYTES */);
int smm_hip_comm_create_rccl(int rank, int world, const void* id, smm_hip_comm** out);
int smm_hip_comm_create_host(int rank, int world, smm_hip_host_allreduce_fn allreduce, smm_hip_host_sendrecv_fn sendrecv, void* user,
                             smm_hip_comm** out);
int smm_hip_comm_create_self(smm_hip_comm** out);
int smm_hip_comm_destroy(smm_hip_comm* comm);
int smm_hip_comm_info(const smm_hip_comm* comm, int* rank, int* world, int* kind);
/* the communicator's size as RCCL itself reports it (ncclCommCount); 0 for the other kinds */
int smm_hip_comm_rccl_ranks(const smm_hip_comm* comm, int* count);
/* Failure containment: ncclCommInitRank and every wait on a stream that carries RCCL work are bounded by SMM_HIP_COMM_TIMEOUT_S
 * seconds (environment, default 180); on a time-out -- or on any failure inside a distributed call -- the communicator is aborted
 * (ncclCommAbort), the call returns SMM_HIP_ERR_COMM and every later call on it fails at once: the peers then run into their own
 * bounded wait instead of hanging in the next collective.  The process should exit. */
/* runs every collective the solvers use once and checks the results (collective) */
int smm_hip_comm_selftest(smm_hip_comm* comm);
/* bounds[0..world]: contiguous row ranges with ~equal nonzeros, from a host start[rows+1] */
int smm_hip_partition_rows_by_nnz(const int* start, int rows, int world, int* bounds);
/* This rank's rows as DEVICE arrays (d_start local, d_positions global columns).  Collective: exchanges the column ranges,
 * plans the halo, splits the rows on the device into A_loc (owned columns) and A_rem (halo columns).  The arrays are copied. */
int smm_hip_dist_csr_create_dev_f32(smm_hip_comm* comm, int n_global, const int* bounds, const int* d_start, const int* d_positions,
                                    const float* d_values, smm_hip_dist_csr** out);
int smm_hip_dist_csr_create_dev_f64(smm_hip_comm* comm, int n_global, const int* bounds, const int* d_start, const int* d_positions,
                                    const double* d_values, smm_hip_dist_csr** out);
int smm_hip_dist_csr_destroy(smm_hip_dist_csr* A);
int smm_hip_dist_csr_info(const smm_hip_dist_csr* A, int* n_local, int* ext_len, int* own_offset, int* halo_elements, long long* nnz_loc,
                          long long* nnz_rem);
/* Pieces the halo of this matrix is exchanged in (1 unless SMM_HIP_HALO_CHUNKS asked for 2 .. 4 on EVERY rank when the matrix was created):
 * with k pieces every SpMV issues k exchanges back to back, and the remote block is cut by columns into k parts, part j starting as soon as
 * piece j has landed (row sums are then formed as ((loc + rem_0) + rem_1) + ...: deterministic, rounding differs from the one-piece form). */
int smm_hip_dist_csr_halo_chunks(const smm_hip_dist_csr* D, int* chunks);
/* How this matrix's halo and scalars travel (decided collectively when it was created):
 *   p2p          1: peer to peer (csrc/smm_p2p.h) -- every rank maps every rank's block of fine-grained device memory (hipIpcMemHandle; over
 *                xGMI between GPUs), pushes the boundary slices of a vector straight into the neighbours' landing areas and completes the
 *                dot products by one single-workgroup kernel that writes into / reads from per-rank slots: no collective is launched inside
 *                the loop.  r06: the DEFAULT between processes -- taken whenever every rank could map every peer and passed the self-test
 *                through every path at create time; SMM_HIP_P2P=0 on any rank keeps every rank with the communicator's collectives (0).
 *                2: the hybrid -- the scalars through the slots, the halo through the communicator's grouped send / receive (the halo part of
 *                the self-test failed on some rank, or SMM_HIP_P2P_HALO=0).  Ranks that are threads of ONE process always get 0.
 *                Results: the halo is pure data movement (same bits); the scalars are added in rank order on every rank (deterministic,
 *                identical on all ranks).
 *   relays       relay ranks per halo segment (SMM_HIP_P2P_RELAYS; default world - 4, i.e. 4 at 8 ranks): the segment's direct_share goes
 *                over the link src -> dst, the rest in equal shares src -> relay -> dst over links a nearest-neighbour exchange leaves idle.
 *   halo_first   1: the rows of an updated vector that a peer receives are produced by a small launch of their own and the exchange is
 *                posted right behind it, before the bulk of the update runs (SMM_HIP_HALO_FIRST=0 turns it off); same bits either way. */
int smm_hip_dist_csr_options(const smm_hip_dist_csr* D, int* p2p, int* relays, int* halo_first, double* direct_share);
/* How many SpMVs with a halo this matrix has run so far as ONE launch (csrc/smm_spmv_split.hip: the local half of a workgroup's rows, a
 * bounded wait for the word the exchange raises, the remote half; out[] written once) and how many as TWO (A_loc, then A_rem behind the
 * exchange's event).  One launch is taken whenever both local blocks are in the row-mask encoding with values read at 1 / 2 / 4 lanes per
 * row (what the solvers adopt from 2^20 entries); SMM_HIP_SPLIT_SPMV=0 keeps the two launches.  Same bits either way. */
int smm_hip_dist_csr_matvec_forms(const smm_hip_dist_csr* D, long long* one_launch, long long* two_launches);
/* A THIN remote block: when at most an eighth of this rank's rows hold an entry in another rank's columns (the slabs of a 3-D grid: the two
 * boundary planes) those rows are listed at creation (*rows; 0: the block is not thin) and the second half of an SpMV is a launch over the
 * listed rows only -- out[row] (+|-)= A_rem[row] . halo, the row's entries in order -- instead of a pass over all of out[]; the dot products
 * ride in the local launch and the thin one adds what its rows change (o . w = a . w + d . w,  o . o = a . a + d (a + o)).  *matvecs: SpMVs
 * run in this form so far (they are not counted by smm_hip_dist_csr_matvec_forms).  Taken when the remote block's kernel reads one lane per
 * row and no Jacobi division rides in the epilogue; out[] has the bits of the general form, the dot products differ in the order of their
 * additions.  SMM_HIP_THIN_REMOTE=0 at creation keeps the general second launch. */
int smm_hip_dist_csr_thin_remote(const smm_hip_dist_csr* D, int* rows, long long* matvecs);
/* SpMVs of smm_hip_dist_cg_* on this matrix that formed the next direction themselves (p = beta p_old + r in the load phase of the 2.5-D
 * constant-diagonal kernel, csrc/smm_spmv_march.hip): taken when x is deferred (vectors beyond the caches), the local block is served by that
 * kernel with non-temporal outputs and the remote block is empty or thin; the halo of r then travels instead of the direction's and every rank
 * forms the halo of the new direction itself -- the owner's expression on the owner's operands.  Same bits as the loop that forms p in a
 * launch of its own (smm_hip_set_cg_fuse_p(0)). */
int smm_hip_dist_csr_cg_fused(const smm_hip_dist_csr* D, long long* matvecs);
/* Milliseconds that workgroup 0 of this matrix's one-launch SpMVs has spent, in total, waiting for the word its halo exchange raises after
 * finishing the local half of its rows (100 MHz device clock): what the exchanges cost beyond the compute that ran beside them -- the one-launch
 * form's counterpart of smm_hip_profile_read_waits (`exposed_comm_ms` of `bench.py --gpus N`).  Synchronises the device; reset != 0 clears it. */
int smm_hip_dist_csr_split_wait(smm_hip_dist_csr* D, double* waited_ms, int reset);
/* The peer-to-peer plan of one rank as plain numbers: host arithmetic only (no device, no communicator), the same function the set-up uses.
 * needs[2 q], needs[2 q + 1] = the column range [cmin, cmax) rank q's rows touch; bounds[0 .. world] = the row partition.  Writes records of
 * 8 values into out (capacity in values; *out_count = records): push {0, dst, relay or -1, first global column, position at dst / relay,
 * count, path, relay job}, forward {1, src, dst, staging position, landing position at dst, count, path, job}, land {2, src, offset in the
 * halo-extended vector, landing position, count, paths, 0, 0}.  For tests (tests/test_p2p_plan_cpu.py replays a world of 8 on the CPU). */
int smm_hip_dist_p2p_plan(int world, int rank, const long long* needs, const int* bounds, int relays, double direct_share, long long* out, int out_capacity,
                          int* out_count);
/* the two local blocks (owned by A): a_loc is the square diagonal block a block-Jacobi preconditioner is built on
 * (smm_hip_precond_create(a_loc, kind, &M)); both accept smm_hip_csr_set_kernel */
int smm_hip_dist_csr_local_block(const smm_hip_dist_csr* A, smm_hip_csr** a_loc, smm_hip_csr** a_rem);
/* out = op(lhs, A x) on the owned rows; d_x, d_lhs, d_out are this rank's slices (n_local).  rMult / rMultAdd / rMultSub, ref:1458-1515 */
int smm_hip_dist_spmv_dev_f32(smm_hip_dist_csr* A, int op, const float* d_lhs, const float* d_x, float* d_out, smm_hip_stream stream);
int smm_hip_dist_spmv_dev_f64(smm_hip_dist_csr* A, int op, const double* d_lhs, const double* d_x, double* d_out, smm_hip_stream stream);
/* BiCGStab (ref:2191-2303) / ConjugateGradient (ref:2316-2398) with the semantics of smm_hip_bicgstab_dev_* / smm_hip_cg_dev_*; every
 * rank gets the same status / iterations / resnorm.  M_loc (may be NULL): JACOBI / ILU0 / SGS of this rank's diagonal block, applied
 * block-Jacobi by rank -- the same preconditioner as on one GPU only for JACOBI or world == 1. */
int smm_hip_dist_bicgstab_dev_f32(smm_hip_dist_csr* A, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M_loc,
                                  smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm);
int smm_hip_dist_bicgstab_dev_f64(smm_hip_dist_csr* A, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M_loc,
                                  smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm);
int smm_hip_dist_cg_dev_f32(smm_hip_dist_csr* A, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps,
                            smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2);
int smm_hip_dist_cg_dev_f64(smm_hip_dist_csr* A, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                            smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2);

/* ---- synthetic workload generators (BASELINE.json configs; device-side so 5e8-entry matrices need no host
 *      std::map as in ref:606-618).  d_start[rows+1], d_positions[nnz], d_values[nnz] are DEVICE arrays sized by
 *      the *_nnz query.  Same laws as sparse_matrix_math_amd.generators (numpy), bit for bit. --------------- */
long long smm_hip_gen_poisson2d_nnz(int nx, int ny);
long long smm_hip_gen_stencil3d_nnz(int nx, int ny, int nz);
long long smm_hip_gen_banded_nnz(int n, int k, unsigned long long seed, int max_offset);
int smm_hip_gen_poisson2d_dev_f32(int nx, int ny, int* d_start, int* d_positions, float* d_values, smm_hip_stream stream);
int smm_hip_gen_poisson2d_dev_f64(int nx, int ny, int* d_start, int* d_positions, double* d_values, smm_hip_stream stream);
/* 7-point stencil: diagonal `diag`, lower neighbours `lo`, upper neighbours `hi` (Laplacian: 6,-1,-1;
 * convection-diffusion stand-in for atmosmodd: 6,-1-c,-1+c) */
int smm_hip_gen_stencil3d_dev_f32(int nx, int ny, int nz, float diag, float lo, float hi, int* d_start, int* d_positions, float* d_values, smm_hip_stream stream);
int smm_hip_gen_stencil3d_dev_f64(int nx, int ny, int nz, double diag, double lo, double hi, int* d_start, int* d_positions, double* d_values, smm_hip_stream stream);
/* banded-random symmetric strictly diagonally dominant matrix: A[i][i] = diag_shift +
 * sum|offdiag| (SURVEY's law is diag_shift = 1; A*1 = diag_shift*1, so 1/diag_shift sets the condition number) */
int smm_hip_gen_banded_dev_f32(int n, int k, unsigned long long seed, int max_offset, float diag_shift, int* d_start, int* d_positions, float* d_values, smm_hip_stream stream);
int smm_hip_gen_banded_dev_f64(int n, int k, unsigned long long seed, int max_offset, double diag_shift, int* d_start, int* d_positions, double* d_values, smm_hip_stream stream);
/* rows [row_begin, row_end) only -- what one rank of a row-partitioned run owns: d_start[row_end - row_begin + 1] is local
 * (d_start[0] == 0), d_positions hold GLOBAL columns.  smm_hip_gen_banded_row_start(row) is start[row] of the full matrix
 * in closed form, so the local nnz is row_start(row_end) - row_start(row_begin). */
long long smm_hip_gen_banded_row_start(int n, int k, unsigned long long seed, int max_offset, int row);
int smm_hip_gen_banded_rows_dev_f32(int n, int k, unsigned long long seed, int max_offset, float diag_shift, int row_begin, int row_end,
                                    int* d_start, int* d_positions, float* d_values, smm_hip_stream stream);
int smm_hip_gen_banded_rows_dev_f64(int n, int k, unsigned long long seed, int max_offset, double diag_shift, int row_begin, int row_end,
                                    int* d_start, int* d_positions, double* d_values, smm_hip_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SMM_HIP_H */
