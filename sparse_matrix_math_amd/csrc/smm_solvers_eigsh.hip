// smm_solvers_eigsh.hip -- thick-restart Lanczos (Wu and Simon 2000) with full reorthogonalisation: the k algebraically largest or
// smallest eigenpairs of a symmetric matrix.  An addition: the reference has no eigensolver.  The definition, line by line, is
// tests/eigsh_restatement.py; the contract is in include/smm_hip.h.
//
// The basis V is ONE allocation, column-major, ncv + 1 columns, leading dimension rounded up to 64 elements (every column starts 16-byte
// aligned).  Its first l columns are the Ritz vectors kept by the last restart.  w = A v_j is written straight into column j + 1,
// orthogonalised and normalised there.  A step j is, besides the SpMV, GMRES's Arnoldi step with a shorter tail:
//   multiDot + finish   h1_i = v_i . w for all i <= j from the same w
//   multiAxpy           w = w + sum_i (-h1_i) v_i, i ascending, smmFma nesting
//   multiDot + finish   h2 the same again
//   multiAxpy           ... with the partial sums of w . w in its epilogue
//   eigshStep           one workgroup: alpha_j = h1_j + h2_j, beta_j = sqrt(w . w), the running scale, the breakdown test
//   scaleKernel         v_{j+1} = w / beta_j
// Eight launches and the SpMV; nothing is read by the host inside a cycle.  `done` (raised by eigshStep on a breakdown or on a value that
// is not finite) turns the launches still queued for the cycle into no-ops.  At the end of a cycle the host reads the state once, solves
// the small eigenproblem (cyclic Jacobi, smm_jacobi.h; fp64 results) and either ends the solve or compresses the basis (multiRotate, smm_multivec.h).
// No floating-point atomics, every sum in a fixed order: two runs of one call give the same bits.
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_jacobi.h"
#include "smm_multivec.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;
constexpr int MAXC = SMM_EIGSH_MAX_NCV;
static_assert(MAXC == MR_MAX, "the compression kernel holds a row of the whole basis");

template <typename T>
struct EigshState {
	T alpha[MAXC], beta[MAXC];                      // of the running cycle, at the step's index
	T h1[MAXC + 1], h2[MAXC + 1], coef[MAXC + 1];  // the two Gram-Schmidt passes' products and the coefficients (-h) of the running pass
	T scale;                                        // the largest |alpha|, beta or kept |theta| seen so far in the solve
	T nrm;                                          // the divisor of the next scaleKernel
	int done, brk, bad, steps;                      // brk: the step that broke down (-1: none) ; steps: SpMVs of the running cycle
};

// the start of a cycle: the flags, and the kept Ritz values' share of the scale
template <typename T>
__global__ void eigshBegin(EigshState<T>* st, T thetaMax) {
	st->done = 0;
	st->brk = -1;
	st->steps = 0;
	if (thetaMax > st->scale) st->scale = thetaMax;
}

// One workgroup per Lanczos step: alpha, beta, the scale and the breakdown test.
template <typename T>
__global__ __launch_bounds__(TPB) void eigshStep(EigshState<T>* st, const T* __restrict__ wwParts, int nb, int j) {
	__shared__ T red[4];
	if (st->done) return;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) acc += wwParts[i];
	const T ww = blockSum256(acc, red);
	if (threadIdx.x != 0) return;
	const T alpha = st->h1[j] + st->h2[j];
	const T beta = sqrt(ww);
	st->alpha[j] = alpha;
	st->beta[j] = beta;
	st->steps = st->steps + 1;
	if (!isfinite(alpha) || !isfinite(beta)) {
		st->bad = 1;
		st->done = 1;
		return;
	}
	T scale = st->scale;
	if (fabs(alpha) > scale) scale = fabs(alpha);
	if (beta > scale) scale = beta;
	st->scale = scale;
	if (beta <= std::numeric_limits<T>::epsilon() * scale) {  // v_{j+1} is not formed: nothing divides by this beta
		st->brk = j;
		st->done = 1;
		return;
	}
	st->nrm = beta;
}

static int eigshResolveNcv(int rows, int k, int ncv) { return ncv == 0 ? std::min(rows, std::max(2 * k + 1, 20)) : ncv; }

template <typename T>
static int eigshCheck(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, const T* eigenvalues, const T* eigenvectors, long long ldx) {
	SMM_TRY(solverCheck<T>("eigsh", a));
	if (k < 0 || (which != SMM_EIGSH_LARGEST && which != SMM_EIGSH_SMALLEST) || maxRestarts < 0 || ncv < 0) {
		setError("eigsh: bad arguments (k >= 0, which SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST, ncv >= 0, maxRestarts >= 0)");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows == 0 || k == 0) return SMM_HIP_OK;
	const int use = eigshResolveNcv(a->rows, k, ncv);
	if (use < k + 2 || use > std::min(a->rows, MAXC)) {
		setError("eigsh: ncv = %d is outside k + 2 = %d .. min(rows, %d) = %d", use, k + 2, MAXC, std::min(a->rows, MAXC));
		return SMM_HIP_ERR_INVALID;
	}
	if (!eigenvalues) {
		setError("eigsh: null eigenvalues");
		return SMM_HIP_ERR_INVALID;
	}
	if (eigenvectors && ldx < a->rows) {
		setError("eigsh: ldx = %lld is less than the %d rows", ldx, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int eigshDev(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, T tol, const T* v0, unsigned long long seed, T* d_vals, T* d_X, long long ldx,
                    hipStream_t s, T* residuals, RitzOut* out) {
	SMM_TRY(eigshCheck<T>(a, k, which, ncv, maxRestarts, d_vals, d_X, ldx));
	const int n = a->rows;
	if (n == 0 || k == 0) return SMM_HIP_OK;
	ncv = eigshResolveNcv(n, k, ncv);
	const double bound = tol > T(0) ? static_cast<double>(tol) : static_cast<double>(std::numeric_limits<T>::epsilon());
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, ncv, s));
	const long long ld = std::max<long long>(64, (static_cast<long long>(n) + 63) / 64 * 64);
	DevBuf<T> V, parts, parts1, dY;
	DevBuf<EigshState<T>> st;
	SyncOnExit drain{s};
	SMM_TRY(V.alloc(static_cast<size_t>(ld) * (ncv + 1)));
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXC + 1) * NPART));
	SMM_TRY(parts1.alloc(NPART));
	SMM_TRY(dY.alloc(static_cast<size_t>(MAXC) * MAXC));
	SMM_TRY(st.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(EigshState<T>), s));
	EigshState<T>* sp = st.p;
	const int* done = &sp->done;
	const int gmv = gridMV(n, sizeof(T));
	const int g = solverGrid(n);
	auto col = [&](int j) { return V.p + static_cast<long long>(j) * ld; };
	// column j against the j columns before it, with the partial sums of its square at the end
	auto orthogonalise = [&](int j, const int* flag) { orthogonaliseTwice<T>(V.p, ld, n, gmv, j, col(j), parts, parts1, sp->h1, sp->h2, sp->coef, flag, s); };

	int l = 0;                  // kept Ritz vectors
	int fresh = 0;              // hash vectors used so far
	bool needStart = true;      // column l has no vector yet
	std::vector<double> kept, arrow;  // theta and s of the kept columns
	std::vector<double> t, theta, y;
	std::vector<int> order;
	std::vector<T> hY, vals, rho;  // staged to the device: alive until the stream is synchronised
	EigshState<T> h;
	for (;;) {
		double keptMax = 0;
		for (double v : kept) keptMax = std::max(keptMax, std::fabs(v));
		eigshBegin<T><<<1, 1, 0, s>>>(sp, static_cast<T>(keptMax));
		if (needStart) {
			T* c = col(l);
			if (l == 0 && v0) {
				multiAxpyKernel<T, true><<<gmv, TPB, 0, s>>>(n, 0, nullptr, V.p, ld, sp->coef, v0, c, parts1, nullptr);  // (no column: a copy and v0 . v0)
			} else {
				hashFillKernel<T><<<g, TPB, 0, s>>>(n, seed, fresh, c, ld);
				++fresh;
				orthogonalise(l, nullptr);
			}
			normaliseKernel<T><<<g, TPB, 0, s>>>(n, c, parts1, gmv, &sp->bad, &sp->done);
			needStart = false;
		}
		for (int j = l; j < ncv; ++j) {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, col(j), col(j + 1), 0, nullptr, nullptr, done, s));
			orthogonalise(j + 1, done);
			eigshStep<T><<<1, TPB, 0, s>>>(sp, parts1, gmv, j);
			scaleKernel<T><<<g, TPB, 0, s>>>(n, &sp->nrm, col(j + 1), col(j + 1), &sp->done);
		}
		LoopWatch none;
		SMM_TRY(loopFinish(none, &h, sp, sizeof(h), s));  // the one host read of the cycle
		out->matvecs += h.steps;
		if (h.bad) {
			out->status = SMM_SOLVER_DIVERGED;
			break;
		}
		const bool broke = h.brk >= 0;
		const int m = broke ? h.brk + 1 : ncv;
		// T = diag(kept theta), the arrow s in row and column l, the new tridiagonal part
		t.assign(static_cast<size_t>(m) * m, 0.0);
		for (int i = 0; i < l; ++i) {
			t[i * m + i] = kept[i];
			t[i * m + l] = t[l * m + i] = arrow[i];
		}
		for (int j = l; j < m; ++j) {
			t[j * m + j] = static_cast<double>(h.alpha[j]);
			if (j + 1 < m) t[j * m + j + 1] = t[(j + 1) * m + j] = static_cast<double>(h.beta[j]);
		}
		if (!jacobiEigen(m, t, theta, y)) {
			out->status = SMM_SOLVER_DIVERGED;
			break;
		}
		order.resize(m);  // positions of the Ritz values in the order of `which`
		for (int i = 0; i < m; ++i) order[i] = which == SMM_EIGSH_LARGEST ? m - 1 - i : i;
		const double last = broke ? 0.0 : static_cast<double>(h.beta[m - 1]);
		double normA = 0;
		for (double v : theta) normA = std::max(normA, std::fabs(v));
		const int have = std::min(k, m);
		int nconv = 0;
		for (int i = 0; i < have; ++i) nconv += std::fabs(last * y[(m - 1) * m + order[i]]) <= bound * normA ? 1 : 0;
		const bool converged = nconv == k;
		if (converged || (broke && m >= k) || out->restarts >= maxRestarts) {
			vals.resize(have);
			rho.resize(have);
			for (int i = 0; i < have; ++i) {
				vals[i] = static_cast<T>(theta[order[i]]);
				rho[i] = static_cast<T>(std::fabs(last * y[(m - 1) * m + order[i]]));
			}
			if (d_X) {  // X = V[:, 0..m-1] Y[:, wanted]
				SMM_TRY(stageRotation<T>(m, m, have, y, order.data(), hY, dY, s));
				multiRotateLaunch<T>(n, m, have, V.p, ld, dY.p, s);
				for (int i = 0; i < have; ++i) SMM_TRY(launchCopy2<T>(n, col(i), d_X + static_cast<long long>(i) * ldx, nullptr, s));
			}
			SMM_TRY(hostToDev(d_vals, vals.data(), sizeof(T) * have, s));
			if (residuals) std::copy(rho.begin(), rho.end(), residuals);
			out->nconv = nconv;
			out->wrote = have;
			out->status = converged ? SMM_SOLVER_SUCCESS : SMM_SOLVER_MAX_ITERATIONS_REACHED;
			break;
		}
		// the restart: the best lNew Ritz vectors into the first columns; after a breakdown short of k all m of them, and a fresh vector
		const int lNew = broke ? m : k + (ncv - k) / 2;
		SMM_TRY(stageRotation<T>(m, m, lNew, y, order.data(), hY, dY, s));
		multiRotateLaunch<T>(n, m, lNew, V.p, ld, dY.p, s);
		if (!broke) SMM_TRY(launchCopy2<T>(n, col(m), col(lNew), nullptr, s));
		kept.resize(lNew);
		arrow.resize(lNew);
		for (int i = 0; i < lNew; ++i) {
			kept[i] = theta[order[i]];
			arrow[i] = broke ? 0.0 : last * y[(m - 1) * m + order[i]];
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
static int eigshDevEntry(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, T tol, const T* d_v0, unsigned long long seed, T* d_vals, T* d_X,
                         long long ldx, hipStream_t s, T* residuals, int* nconv, int* restarts, int* matvecs, int* status) {
	RitzOut o;
	SMM_TRY(eigshDev<T>(a, k, which, ncv, maxRestarts, tol, d_v0, seed, d_vals, d_X, ldx, s, residuals, &o));
	ritzReport(o, nconv, restarts, matvecs, status);
	return SMM_HIP_OK;
}

// host arrays: v0 (may be null), eigenvalues[k], eigenvectors (may be null) column-major with ldx
template <typename T>
static int eigshHost(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, T tol, const T* v0, unsigned long long seed, T* eigenvalues, T* eigenvectors,
                     long long ldx, T* residuals, int* nconv, int* restarts, int* matvecs, int* status) {
	SMM_TRY(eigshCheck<T>(a, k, which, ncv, maxRestarts, eigenvalues, eigenvectors, ldx));
	RitzOut o;
	if (a->rows == 0 || k == 0) {
		ritzReport(o, nconv, restarts, matvecs, status);
		return SMM_HIP_OK;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	const size_t n = static_cast<size_t>(a->rows);
	DevBuf<T> dv0, dvals, dX;
	SyncOnExit drain{s};
	if (v0) {
		SMM_TRY(dv0.alloc(n));
		SMM_TRY(hostToDev(dv0, v0, sizeof(T) * n, s));
	}
	SMM_TRY(dvals.alloc(k));
	if (eigenvectors) SMM_TRY(dX.alloc(n * k));
	SMM_TRY(eigshDev<T>(a, k, which, ncv, maxRestarts, tol, v0 ? dv0.p : nullptr, seed, dvals.p, eigenvectors ? dX.p : nullptr, static_cast<long long>(n), s, residuals,
	                    &o));
	if (o.wrote > 0) {
		SMM_TRY(devToHost(eigenvalues, dvals, sizeof(T) * o.wrote, s));
		for (int i = 0; eigenvectors && i < o.wrote; ++i) SMM_TRY(devToHost(eigenvectors + static_cast<long long>(i) * ldx, dX.p + i * n, sizeof(T) * n, s));
	}
	drain.armed = false;
	ritzReport(o, nconv, restarts, matvecs, status);
	return SMM_HIP_OK;
}

template <typename T>
static int multiRotateDev(int n, int m, int l, T* V, long long ld, const T* hY, long long ldY, smm_hip_stream stream) {
	if (n < 0 || l < 1 || m < l || m > MR_MAX || ld < n || ldY < m || !hY || (n > 0 && !V)) {
		setError("multi_rotate: bad arguments (n >= 0, 1 <= l <= m <= %d, ld >= n, ldY >= m, no null array)", MR_MAX);
		return SMM_HIP_ERR_INVALID;
	}
	if (n == 0) return SMM_HIP_OK;
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	const int MP = multiRotatePad(m);
	std::vector<T> h(static_cast<size_t>(MP) * l, T(0));
	for (int c = 0; c < l; ++c) std::copy(hY + c * ldY, hY + c * ldY + m, h.begin() + static_cast<size_t>(c) * MP);
	DevBuf<T> dY;
	SyncOnExit drain{s};  // (the staged Y is released when this returns)
	SMM_TRY(dY.alloc(h.size()));
	SMM_TRY(hostToDev(dY, h.data(), sizeof(T) * h.size(), s));
	multiRotateLaunch<T>(n, m, l, V, ld, dY.p, s);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_eigsh_f32(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, float tol, const float* v0, unsigned long long seed, float* eigenvalues,
                      float* eigenvectors, long long ldx, float* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status) {
	return eigshHost<float>(a, k, which, ncv, maxRestarts, tol, v0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, restarts, matvecs, solver_status);
}
int smm_hip_eigsh_f64(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, double tol, const double* v0, unsigned long long seed, double* eigenvalues,
                      double* eigenvectors, long long ldx, double* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status) {
	return eigshHost<double>(a, k, which, ncv, maxRestarts, tol, v0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, restarts, matvecs, solver_status);
}
int smm_hip_eigsh_dev_f32(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, float tol, const float* d_v0, unsigned long long seed, float* d_eigenvalues,
                          float* d_eigenvectors, long long ldx, smm_hip_stream stream, float* residuals, int* nconv, int* restarts, int* matvecs, int* solver_status) {
	SMM_TRY(eigshCheck<float>(a, k, which, ncv, maxRestarts, d_eigenvalues, d_eigenvectors, ldx));
	SMM_TRY(ensureInit());
	return eigshDevEntry<float>(a, k, which, ncv, maxRestarts, tol, d_v0, seed, d_eigenvalues, d_eigenvectors, ldx, pickStream(stream), residuals, nconv, restarts,
	                            matvecs, solver_status);
}
int smm_hip_eigsh_dev_f64(const smm_hip_csr* a, int k, int which, int ncv, int maxRestarts, double tol, const double* d_v0, unsigned long long seed,
                          double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream, double* residuals, int* nconv, int* restarts,
                          int* matvecs, int* solver_status) {
	SMM_TRY(eigshCheck<double>(a, k, which, ncv, maxRestarts, d_eigenvalues, d_eigenvectors, ldx));
	SMM_TRY(ensureInit());
	return eigshDevEntry<double>(a, k, which, ncv, maxRestarts, tol, d_v0, seed, d_eigenvalues, d_eigenvectors, ldx, pickStream(stream), residuals, nconv, restarts,
	                             matvecs, solver_status);
}

int smm_hip_multi_rotate_dev_f32(int n, int m, int l, float* d_V, long long ld, const float* h_Y, long long ldY, smm_hip_stream stream) {
	return multiRotateDev<float>(n, m, l, d_V, ld, h_Y, ldY, stream);
}
int smm_hip_multi_rotate_dev_f64(int n, int m, int l, double* d_V, long long ld, const double* h_Y, long long ldY, smm_hip_stream stream) {
	return multiRotateDev<double>(n, m, l, d_V, ld, h_Y, ldY, stream);
}

}  // extern "C"
