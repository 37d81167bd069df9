// smm_solvers_svds.hip -- thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and Reichel 2005, restarted with Ritz vectors) with
// full reorthogonalisation of both bases: the k largest singular triplets of a matrix of any shape.  An addition: the reference has no
// SVD.  The definition, line by line, is tests/svds_restatement.py; the contract is in include/smm_hip.h.  It is eigsh's rectangular
// sibling (smm_solvers_eigsh.hip) and works as LSQR does (smm_solvers_lsqr.hip) on A and on a transpose handle, never on A^T A.
//
// Two bases, each ONE allocation, column-major, leading dimension rounded up to 64 elements: V (cols x (ncv + 1)) and U (rows x ncv).
// Their first l columns are the Ritz vectors kept by the last restart.  A v_j is written straight into column j of U, A^T u_j into
// column j + 1 of V, and each is orthogonalised and normalised there.  A half step is, besides its SpMV, eigsh's step:
//   multiDot + finish   h_i = q_i . w for all columns q_i before it from the same w
//   multiAxpy           w = w + sum_i (-h_i) q_i, i ascending, smmFma nesting
//   multiDot + finish   the same again
//   multiAxpy           ... with the partial sums of w . w in its epilogue
//   svdsStep            one workgroup: alpha_j (or beta_j) = sqrt(w . w), the running scale, the breakdown test
//   scaleKernel         u_j = w / alpha_j (or v_{j+1} = w / beta_j)
// Eight launches per SpMV, as in eigsh (three for u_0, which has no column before it); nothing is read by the host inside a cycle.
// `done` (raised by svdsStep on a breakdown or on a value that is not finite) turns the launches still queued for the cycle into no-ops.
// The entries of the projected matrix B are these norms and the restart's arrow; the Gram-Schmidt products serve orthogonality only.
// At the end of a cycle the host reads the state once, takes the small SVD (one-sided Jacobi, smm_jacobi.h; fp64 results) and either
// ends the solve or compresses both bases (multiRotate, smm_multivec.h).  No floating-point atomics, every sum in a fixed order: two
// runs of one call give the same bits.
// NOT here: the smallest singular values (harmonic restarts), a shift, a block method, an implicit A^T A.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_jacobi.h"
#include "smm_multivec.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;
constexpr int MAXC = SMM_SVDS_MAX_NCV;
static_assert(MAXC == MR_MAX, "the compression kernel holds a row of a whole basis");

template <typename T>
struct SvdsState {
	T alpha[MAXC], beta[MAXC];        // of the running cycle, at the step's index
	T h[MAXC + 1], coef[MAXC + 1];   // the running Gram-Schmidt pass: its products and the coefficients (-h)
	T scale;                          // the largest alpha, beta or kept sigma seen so far in the solve
	T nrm;                            // the divisor of the next scaleKernel
	int done, brk, brkBeta, bad, steps;  // brk: the step that broke down (-1: none), brkBeta: at its beta ; steps: SpMVs of the running cycle
};

// the start of a cycle: the flags, and the kept Ritz values' share of the scale
template <typename T>
__global__ void svdsBegin(SvdsState<T>* st, T sigmaMax) {
	st->done = 0;
	st->brk = -1;
	st->brkBeta = 0;
	st->steps = 0;
	if (sigmaMax > st->scale) st->scale = sigmaMax;
}

// One workgroup per half step: the norm (alpha_j, or beta_j with BETA), the scale and the breakdown test.
template <typename T, bool BETA>
__global__ __launch_bounds__(TPB) void svdsStep(SvdsState<T>* st, const T* __restrict__ wwParts, int nb, int j) {
	__shared__ T red[4];
	if (st->done) return;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) acc += wwParts[i];
	const T ww = blockSum256(acc, red);
	if (threadIdx.x != 0) return;
	const T nrm = sqrt(ww);
	if (BETA) st->beta[j] = nrm;
	else st->alpha[j] = nrm;
	st->steps = st->steps + 1;
	if (!isfinite(nrm)) {
		st->bad = 1;
		st->done = 1;
		return;
	}
	T scale = st->scale;
	if (nrm > scale) scale = nrm;
	st->scale = scale;
	if (nrm <= std::numeric_limits<T>::epsilon() * scale) {  // the next vector is not formed: nothing divides by this norm
		st->brk = j;
		st->brkBeta = BETA ? 1 : 0;
		st->done = 1;
		return;
	}
	st->nrm = nrm;
}

static int svdsResolveNcv(int rows, int cols, int k, int ncv) { return ncv == 0 ? std::min(std::min(rows, cols), std::max(2 * k + 1, 20)) : ncv; }

// what can be refused before the device is touched
template <typename T>
static int svdsCheck(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, const T* values, const T* U, long long ldu, const T* V, long long ldv) {
	if (!a || a->dtype != dtypeOf<T>()) {
		setError("svds: null matrix or dtype mismatch");
		return SMM_HIP_ERR_INVALID;
	}
	if (at && at->dtype != dtypeOf<T>()) {
		setError("svds: `at` holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (at == a && a->rows != a->cols) {
		setError("svds: `a` itself as `at` asserts symmetry, and a %d x %d matrix is not square", a->rows, a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	if (at && (at->rows != a->cols || at->cols != a->rows || at->nnz != a->nnz)) {
		setError("svds: `at` has not the shape or the entry count of the transpose");
		return SMM_HIP_ERR_INVALID;
	}
	if (k < 0 || maxRestarts < 0 || ncv < 0) {
		setError("svds: bad arguments (k >= 0, ncv >= 0, maxRestarts >= 0)");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows == 0 || a->cols == 0 || k == 0) return SMM_HIP_OK;
	const int least = std::min(a->rows, a->cols);
	const int use = svdsResolveNcv(a->rows, a->cols, k, ncv);
	if (use < k + 2 || use > std::min(least, MAXC)) {
		setError("svds: ncv = %d is outside k + 2 = %d .. min(rows, cols, %d) = %d", use, k + 2, MAXC, std::min(least, MAXC));
		return SMM_HIP_ERR_INVALID;
	}
	if (!values) {
		setError("svds: null singular_values");
		return SMM_HIP_ERR_INVALID;
	}
	if (U && ldu < a->rows) {
		setError("svds: ldu = %lld is less than the %d rows", ldu, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	if (V && ldv < a->cols) {
		setError("svds: ldv = %lld is less than the %d columns", ldv, a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

struct SvdsCsrOwner {  // the transpose a solve built for itself
	smm_hip_csr* m = nullptr;
	~SvdsCsrOwner() { smm_hip_csr_destroy(m); }
};

template <typename T>
static int svdsDev(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, T tol, const T* v0, unsigned long long seed, T* d_vals, T* d_U,
                   long long ldu, T* d_V, long long ldv, hipStream_t s, T* residuals, RitzOut* out) {
	SMM_TRY(svdsCheck<T>(a, at, k, ncv, maxRestarts, d_vals, d_U, ldu, d_V, ldv));
	const int rows = a->rows, cols = a->cols;
	if (rows == 0 || cols == 0 || k == 0) return SMM_HIP_OK;
	ncv = svdsResolveNcv(rows, cols, k, ncv);
	const double bound = tol > T(0) ? static_cast<double>(tol) : static_cast<double>(std::numeric_limits<T>::epsilon());
	// (in this order: an error return synchronises, then releases the vectors, then destroys the transpose -- never under queued kernels)
	SvdsCsrOwner built;
	DevBuf<T> V, U, parts, parts1, dX, dY;
	DevBuf<SvdsState<T>> st;
	SyncOnExit drain{s};
	const bool empty = a->nnz == 0;  // A v = 0 and At u = 0: no SpMV is launched and no transpose is built
	SMM_TRY(ensureCsrReady(a, s, true));
	if (!empty) {
		if (!at) {
			SMM_TRY(csrTransposeCreate(a, s, &built.m));
			at = built.m;
		}
		SMM_TRY(ensureCsrReady(at, s, true));
		SMM_TRY(adoptPatternForSolver(a, ncv, s));
		if (at != a) SMM_TRY(adoptPatternForSolver(at, ncv, s));
	}
	const long long ldV = std::max<long long>(64, (static_cast<long long>(cols) + 63) / 64 * 64);
	const long long ldU = std::max<long long>(64, (static_cast<long long>(rows) + 63) / 64 * 64);
	SMM_TRY(V.alloc(static_cast<size_t>(ldV) * (ncv + 1)));
	SMM_TRY(U.alloc(static_cast<size_t>(ldU) * ncv));
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXC + 1) * NPART));
	SMM_TRY(parts1.alloc(NPART));
	SMM_TRY(dX.alloc(static_cast<size_t>(MAXC) * MAXC));
	SMM_TRY(dY.alloc(static_cast<size_t>(MAXC) * MAXC));
	SMM_TRY(st.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(SvdsState<T>), s));
	SvdsState<T>* sp = st.p;
	const int* done = &sp->done;
	const int gmvV = gridMV(cols, sizeof(T)), gmvU = gridMV(rows, sizeof(T));
	const int gV = solverGrid(cols), gU = solverGrid(rows);
	auto vcol = [&](int j) { return V.p + static_cast<long long>(j) * ldV; };
	auto ucol = [&](int j) { return U.p + static_cast<long long>(j) * ldU; };
	auto orthogonalise = [&](const T* Q, long long ld, int n, int gmv, int c, T* w, const int* flag) {
		orthogonaliseTwice<T>(Q, ld, n, gmv, c, w, parts, parts1, sp->h, sp->h, sp->coef, flag, s);
	};

	int l = 0;              // kept Ritz vectors
	int fresh = 0;          // hash vectors used so far
	bool needStart = true;  // column l of V has no vector yet
	std::vector<double> kept, arrow;  // sigma and s of the kept columns
	std::vector<double> bt, sigma, x, y;
	std::vector<T> hX, hY, vals, rho;  // staged to the device: alive until the stream is synchronised
	SvdsState<T> h;
	for (;;) {
		double keptMax = 0;
		for (double v : kept) keptMax = std::max(keptMax, v);
		svdsBegin<T><<<1, 1, 0, s>>>(sp, static_cast<T>(keptMax));
		if (needStart) {
			T* c = vcol(l);
			if (l == 0 && v0) {
				multiAxpyKernel<T, true><<<gmvV, TPB, 0, s>>>(cols, 0, nullptr, V.p, ldV, sp->coef, v0, c, parts1.p, nullptr);  // (no column: a copy and v0 . v0)
			} else {
				hashFillKernel<T><<<gV, TPB, 0, s>>>(cols, seed, fresh, c, ldV);
				++fresh;
				orthogonalise(V.p, ldV, cols, gmvV, l, c, nullptr);
			}
			normaliseKernel<T><<<gV, TPB, 0, s>>>(cols, c, parts1, gmvV, &sp->bad, &sp->done);
			needStart = false;
		}
		for (int j = l; j < ncv; ++j) {
			if (empty) SMM_HIP_TRY(hipMemsetAsync(ucol(j), 0, sizeof(T) * rows, s));
			else SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, vcol(j), ucol(j), 0, nullptr, nullptr, done, s));
			orthogonalise(U.p, ldU, rows, gmvU, j, ucol(j), done);
			svdsStep<T, false><<<1, TPB, 0, s>>>(sp, parts1.p, gmvU, j);
			scaleKernel<T><<<gU, TPB, 0, s>>>(rows, &sp->nrm, ucol(j), ucol(j), &sp->done);
			if (empty) SMM_HIP_TRY(hipMemsetAsync(vcol(j + 1), 0, sizeof(T) * cols, s));
			else SMM_TRY(launchSpmv<T>(at, SMM_OP_ASSIGN, nullptr, ucol(j), vcol(j + 1), 0, nullptr, nullptr, done, s));
			orthogonalise(V.p, ldV, cols, gmvV, j + 1, vcol(j + 1), done);
			svdsStep<T, true><<<1, TPB, 0, s>>>(sp, parts1.p, gmvV, j);
			scaleKernel<T><<<gV, TPB, 0, s>>>(cols, &sp->nrm, vcol(j + 1), vcol(j + 1), &sp->done);
		}
		LoopWatch none;
		SMM_TRY(loopFinish(none, &h, sp, sizeof(h), s));  // the one host read of the cycle
		out->matvecs += h.steps;
		if (h.bad) {
			out->status = SMM_SOLVER_DIVERGED;
			break;
		}
		// m triplets from U[:, 0..m-1] and V[:, 0..mv-1]
		const bool broke = h.brk >= 0;
		const bool alphaBroke = broke && !h.brkBeta;
		const int m = !broke ? ncv : alphaBroke ? h.brk : h.brk + 1;
		const int mv = alphaBroke ? m + 1 : m;
		// B^T (mv x m): diag(kept sigma), the arrow s in B's column l, alpha on the rest of the diagonal, beta above it
		bt.assign(static_cast<size_t>(mv) * m, 0.0);
		for (int i = 0; i < std::min(l, m); ++i) {
			bt[i * m + i] = kept[i];
			bt[l * m + i] = arrow[i];
		}
		for (int j = l; j < m; ++j) {
			bt[j * m + j] = static_cast<double>(h.alpha[j]);
			if (j + 1 < mv) bt[(j + 1) * m + j] = static_cast<double>(h.beta[j]);
		}
		if (!jacobiSvd(mv, m, bt, sigma, x, y)) {
			out->status = SMM_SOLVER_DIVERGED;
			break;
		}
		const double last = broke ? 0.0 : static_cast<double>(h.beta[m - 1]);
		const double sigma0 = m > 0 ? sigma[0] : 0.0;
		const int have = std::min(k, m);
		int nconv = 0;
		for (int i = 0; i < have; ++i) nconv += std::fabs(last * x[(m - 1) * m + i]) <= bound * sigma0 ? 1 : 0;
		const bool converged = nconv == k;
		if (converged || (broke && m >= k) || out->restarts >= maxRestarts) {
			vals.resize(have);
			rho.resize(have);
			for (int i = 0; i < have; ++i) {
				vals[i] = static_cast<T>(sigma[i]);
				rho[i] = static_cast<T>(std::fabs(last * x[(m - 1) * m + i]));
			}
			if (d_U && have > 0) {  // U_k = U[:, 0..m-1] X[:, 0..k-1]
				SMM_TRY(stageRotation<T>(m, m, have, x, nullptr, hX, dX, s));
				multiRotateLaunch<T>(rows, m, have, U.p, ldU, dX.p, s);
				for (int i = 0; i < have; ++i) SMM_TRY(launchCopy2<T>(rows, ucol(i), d_U + static_cast<long long>(i) * ldu, nullptr, s));
			}
			if (d_V && have > 0) {  // V_k = V[:, 0..mv-1] Y[:, 0..k-1]
				SMM_TRY(stageRotation<T>(mv, m, have, y, nullptr, hY, dY, s));
				multiRotateLaunch<T>(cols, mv, have, V.p, ldV, dY.p, s);
				for (int i = 0; i < have; ++i) SMM_TRY(launchCopy2<T>(cols, vcol(i), d_V + static_cast<long long>(i) * ldv, nullptr, s));
			}
			if (have > 0) SMM_TRY(hostToDev(d_vals, vals.data(), sizeof(T) * have, s));
			if (residuals) std::copy(rho.begin(), rho.end(), residuals);
			out->nconv = nconv;
			out->wrote = have;
			out->status = converged ? SMM_SOLVER_SUCCESS : SMM_SOLVER_MAX_ITERATIONS_REACHED;
			break;
		}
		// the restart: the best lNew Ritz vectors into the first columns of both bases; after a breakdown short of k all m of them, and a
		// fresh vector
		const int lNew = broke ? m : k + (ncv - k) / 2;
		if (lNew > 0) {
			SMM_TRY(stageRotation<T>(m, m, lNew, x, nullptr, hX, dX, s));
			multiRotateLaunch<T>(rows, m, lNew, U.p, ldU, dX.p, s);
			SMM_TRY(stageRotation<T>(mv, m, lNew, y, nullptr, hY, dY, s));
			multiRotateLaunch<T>(cols, mv, lNew, V.p, ldV, dY.p, s);
		}
		if (!broke) SMM_TRY(launchCopy2<T>(cols, vcol(m), vcol(lNew), nullptr, s));
		kept.resize(lNew);
		arrow.resize(lNew);
		for (int i = 0; i < lNew; ++i) {
			kept[i] = sigma[i];
			arrow[i] = broke ? 0.0 : last * x[(m - 1) * m + i];
		}
		needStart = broke;
		l = lNew;
		++out->restarts;
	}
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	return SMM_HIP_OK;
}

template <typename T>
static int svdsDevEntry(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, T tol, const T* d_v0, unsigned long long seed, T* d_vals, T* d_U,
                        long long ldu, T* d_V, long long ldv, smm_hip_stream stream, T* residuals, int* nconv, int* restarts, int* matvecs, int* status) {
	SMM_TRY(svdsCheck<T>(a, at, k, ncv, maxRestarts, d_vals, d_U, ldu, d_V, ldv));
	RitzOut o;
	if (a->rows > 0 && a->cols > 0 && k > 0) {
		SMM_TRY(ensureInit());
		SMM_TRY(svdsDev<T>(a, at, k, ncv, maxRestarts, tol, d_v0, seed, d_vals, d_U, ldu, d_V, ldv, pickStream(stream), residuals, &o));
	}
	ritzReport(o, nconv, restarts, matvecs, status);
	return SMM_HIP_OK;
}

// host arrays: v0 (may be null), singular_values[k], U and V (each may be null) column-major with ldu, ldv
template <typename T>
static int svdsHost(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, T tol, const T* v0, unsigned long long seed, T* values, T* hU,
                    long long ldu, T* hV, long long ldv, T* residuals, int* nconv, int* restarts, int* matvecs, int* status) {
	SMM_TRY(svdsCheck<T>(a, at, k, ncv, maxRestarts, values, hU, ldu, hV, ldv));
	RitzOut o;
	if (a->rows == 0 || a->cols == 0 || k == 0) {
		ritzReport(o, nconv, restarts, matvecs, status);
		return SMM_HIP_OK;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	const size_t rows = static_cast<size_t>(a->rows), cols = static_cast<size_t>(a->cols);
	DevBuf<T> dv0, dvals, dU, dV;
	SyncOnExit drain{s};
	if (v0) {
		SMM_TRY(dv0.alloc(cols));
		SMM_TRY(hostToDev(dv0, v0, sizeof(T) * cols, s));
	}
	SMM_TRY(dvals.alloc(k));
	if (hU) SMM_TRY(dU.alloc(rows * k));
	if (hV) SMM_TRY(dV.alloc(cols * k));
	SMM_TRY(svdsDev<T>(a, at, k, ncv, maxRestarts, tol, v0 ? dv0.p : nullptr, seed, dvals.p, hU ? dU.p : nullptr, static_cast<long long>(rows), hV ? dV.p : nullptr,
	                   static_cast<long long>(cols), s, residuals, &o));
	if (o.wrote > 0) {
		SMM_TRY(devToHost(values, dvals, sizeof(T) * o.wrote, s));
		for (int i = 0; hU && i < o.wrote; ++i) SMM_TRY(devToHost(hU + static_cast<long long>(i) * ldu, dU.p + i * rows, sizeof(T) * rows, s));
		for (int i = 0; hV && i < o.wrote; ++i) SMM_TRY(devToHost(hV + static_cast<long long>(i) * ldv, dV.p + i * cols, sizeof(T) * cols, s));
	}
	drain.armed = false;
	ritzReport(o, nconv, restarts, matvecs, status);
	return SMM_HIP_OK;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_svds_f32(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, float tol, const float* v0, unsigned long long seed,
                     float* singular_values, float* U, long long ldu, float* V, long long ldv, float* residuals, int* nconv, int* restarts, int* matvecs,
                     int* solver_status) {
	return svdsHost<float>(a, at, k, ncv, maxRestarts, tol, v0, seed, singular_values, U, ldu, V, ldv, residuals, nconv, restarts, matvecs, solver_status);
}
int smm_hip_svds_f64(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, double tol, const double* v0, unsigned long long seed,
                     double* singular_values, double* U, long long ldu, double* V, long long ldv, double* residuals, int* nconv, int* restarts, int* matvecs,
                     int* solver_status) {
	return svdsHost<double>(a, at, k, ncv, maxRestarts, tol, v0, seed, singular_values, U, ldu, V, ldv, residuals, nconv, restarts, matvecs, solver_status);
}
int smm_hip_svds_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, float tol, const float* d_v0, unsigned long long seed,
                         float* d_singular_values, float* d_U, long long ldu, float* d_V, long long ldv, smm_hip_stream stream, float* residuals, int* nconv,
                         int* restarts, int* matvecs, int* solver_status) {
	return svdsDevEntry<float>(a, at, k, ncv, maxRestarts, tol, d_v0, seed, d_singular_values, d_U, ldu, d_V, ldv, stream, residuals, nconv, restarts, matvecs,
	                           solver_status);
}
int smm_hip_svds_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int maxRestarts, double tol, const double* d_v0, unsigned long long seed,
                         double* d_singular_values, double* d_U, long long ldu, double* d_V, long long ldv, smm_hip_stream stream, double* residuals, int* nconv,
                         int* restarts, int* matvecs, int* solver_status) {
	return svdsDevEntry<double>(a, at, k, ncv, maxRestarts, tol, d_v0, seed, d_singular_values, d_U, ldu, d_V, ldv, stream, residuals, nconv, restarts, matvecs,
	                            solver_status);
}

}  // extern "C"
