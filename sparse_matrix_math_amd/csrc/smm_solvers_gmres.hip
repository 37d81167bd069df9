// smm_solvers_gmres.hip -- restarted GMRES(m) with classical Gram-Schmidt applied twice and right preconditioning, device-resident.
// An addition: the reference has no GMRES.  The definition is tests/gmres_restatement.py; the contract is in include/smm_hip.h.
//
// The basis V is ONE allocation, column-major, restart + 1 columns, leading dimension rounded up to 64 elements (every column starts
// 16-byte aligned).  w = A M^-1 v_j is written straight into column j + 1, orthogonalised and normalised there.
// An Arnoldi step j is, besides the preconditioner apply and the SpMV:
//   multiDot + finish   h1_i = v_i . w for all i <= j from the same w; the finish launch (j + 1 workgroups) adds each column's partials
//   multiAxpy           w = w + sum_i (-h1_i) v_i, i ascending, smmFma nesting
//   multiDot + finish   h2 the same again
//   multiAxpy           ... with the partial sums of w . w in its epilogue
//   gmresStep           one workgroup: H[.][j] = h1 + h2, H[j+1][j] = sqrt(w . w), the rotations, the tests, the counters
//   scaleKernel         v_{j+1} = w / H[j+1][j]
// The host never sees H.  Two device flags: cycleOver (raised by gmresStep) stops the launches that are still queued for the cycle;
// solveOver (raised by gmresOuter after the residual was recomputed) stops everything.  The cycle-end kernels read the k that was reached
// from device memory.  No floating-point atomics, every sum in a fixed order: two runs of one solve give the same bits.
#include <algorithm>
#include <cmath>
#include <map>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_multivec.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;
constexpr int MAXR = SMM_GMRES_MAX_RESTART;

template <typename T>
struct GmresState {
	T R[MAXR * MAXR];  // H after the rotations, column-major with leading dimension MAXR: upper triangular
	T cs[MAXR], sn[MAXR], g[MAXR + 1], y[MAXR];
	T h1[MAXR + 1], h2[MAXR + 1], coef[MAXR + 1];  // the two Gram-Schmidt passes' products and the coefficients (-h) of the running pass
	T rr, beta, hn;                                 // r.r ; its root ; H[j+1][j] of the step just taken
	int cycleOver, solveOver, k, iters, status, pad[3];
};

// x = x + z at the end of a cycle that reached k > 0 columns
template <typename T>
__global__ __launch_bounds__(TPB) void gmresAddX(int n, const GmresState<T>* __restrict__ st, const T* z, T* x) {
	if (st->solveOver || st->k == 0) return;
	const T* const in[2] = {x, z};
	T* const o1[1] = {x};
	streamMap<T, false, 2, 1>(n, in, o1, [&](const T(&v)[2], T(&o)[1]) { o[0] = v[0] + v[1]; });
}

// One workgroup per Arnoldi step: the column of H, the earlier rotations, the new one, the tests and the counters.
template <typename T>
__global__ __launch_bounds__(TPB) void gmresStep(GmresState<T>* st, const T* __restrict__ wwParts, int nb, int j, int restart, int maxIterations, T eps) {
	__shared__ T red[4];
	__shared__ T col[MAXR + 1];
	if (st->cycleOver) return;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) acc += wwParts[i];
	const T ww = blockSum256(acc, red);
	if (static_cast<int>(threadIdx.x) <= j) col[threadIdx.x] = st->h1[threadIdx.x] + st->h2[threadIdx.x];
	__syncthreads();
	if (threadIdx.x != 0) return;
	const T hn = sqrt(ww);
	for (int i = 0; i < j; ++i) {
		const T c = st->cs[i], s = st->sn[i];
		const T t = c * col[i] + s * col[i + 1];
		col[i + 1] = -s * col[i] + c * col[i + 1];
		col[i] = t;
	}
	const T a = col[j];
	const T d = sqrt(a * a + hn * hn);
	const int iters = st->iters + 1;  // the step has been taken, whatever becomes of its column
	st->iters = iters;
	st->hn = hn;
	if (d == T(0) || !isfinite(d)) {  // the column is dropped: k stays j
		st->status = SMM_SOLVER_DIVERGED;
		st->cycleOver = 1;
		return;
	}
	const T c = a / d, s = hn / d;
	st->cs[j] = c;
	st->sn[j] = s;
	col[j] = c * a + s * hn;
	for (int i = 0; i <= j; ++i) st->R[i + j * MAXR] = col[i];
	const T gj = st->g[j];
	const T gn = -s * gj;
	st->g[j + 1] = gn;
	st->g[j] = c * gj;
	st->k = j + 1;
	if (!(gn * gn > eps * eps) || iters >= maxIterations || hn == T(0) || j + 1 >= restart) st->cycleOver = 1;
}

// y of the k x k upper triangular system, the known terms subtracted from the last one down (one column per round, rows in parallel)
template <typename T>
__global__ __launch_bounds__(TPB) void gmresBackSub(GmresState<T>* st) {
	__shared__ T sg[MAXR];
	__shared__ T sy;
	if (st->solveOver) return;
	const int k = st->k;
	if (k == 0) return;
	const int t = threadIdx.x;
	if (t < k) sg[t] = st->g[t];
	__syncthreads();
	for (int i = k - 1; i >= 0; --i) {
		if (t == i) {
			const T y = sg[i] / st->R[i + i * MAXR];
			st->y[i] = y;
			sy = y;
		}
		__syncthreads();
		if (t < i) sg[t] = sg[t] - st->R[t + i * MAXR] * sy;
		__syncthreads();
	}
}

// r.r of the recomputed residual, the outer loop's test, and the start of the next cycle: beta, g = (beta, 0, ...)
template <typename T>
__global__ __launch_bounds__(TPB) void gmresOuter(GmresState<T>* st, const T* __restrict__ rrParts, int first, int maxIterations, T eps) {
	__shared__ T red[4];
	if (!first && st->solveOver) return;
	const T rr = sumParts(rrParts, red);
	if (threadIdx.x != 0) return;
	if (first) {
		st->iters = 0;
		st->status = SMM_SOLVER_SUCCESS;
		st->solveOver = 0;
	}
	st->rr = rr;
	st->k = 0;
	if (!(rr > eps * eps) || st->iters >= maxIterations || st->status == SMM_SOLVER_DIVERGED) {  // (a NaN residual leaves too)
		st->solveOver = 1;
		st->cycleOver = 1;
		return;
	}
	const T beta = sqrt(rr);
	st->beta = beta;
	st->g[0] = beta;
	st->cycleOver = 0;
}

template <typename T>
static int gmresCheck(const smm_hip_csr* a, const T* b, const T* x, int restart) {
	SMM_TRY(solverCheck<T>("gmres", a, b, x));
	if (restart < 1 || restart > MAXR) {
		setError("gmres: restart must be 1 .. %d", MAXR);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int gmresDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, int restart, const smm_hip_precond* M, hipStream_t s, int* status,
                    int* iterations, T* resnorm2) {
	SMM_TRY(gmresCheck<T>(a, b, x, restart));
	const bool precondition = M != nullptr && M->kind != SMM_PRECOND_NONE;
	SMM_TRY(precondAdmissible("gmres", M, a, SOLVER_GENERAL));
	if (precondition && M->dtype != dtypeOf<T>()) {
		setError("gmres: the preconditioner holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	const int n = a->rows;
	if (maxIterations < 0) maxIterations = n;  // no other clamp: a restarted run may need more than `rows` steps
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	const long long ld = std::max<long long>(64, (static_cast<long long>(n) + 63) / 64 * 64);
	DevBuf<T> V, tv, zv, parts, parts1;
	DevBuf<GmresState<T>> st;
	SMM_TRY(V.alloc(static_cast<size_t>(ld) * (restart + 1)));
	SMM_TRY(tv.alloc(n));
	if (precondition) SMM_TRY(zv.alloc(n));
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXR + 1) * NPART));
	SMM_TRY(parts1.alloc(NPART));  // w.w of a step, r.r between the cycles
	SMM_TRY(st.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(GmresState<T>), s));
	SMM_HIP_TRY(hipMemsetAsync(tv.p, 0, sizeof(T) * std::max(n, 1), s));  // (a cycle that reached no column leaves t alone; the apply behind it reads it)
	GmresState<T>* sp = st.p;
	const int* cycleOver = &sp->cycleOver;
	const int* solveOver = &sp->solveOver;
	const int gmv = gridMV(n, sizeof(T));
	auto col = [&](int j) { return V.p + static_cast<long long>(j) * ld; };

	auto residual = [&](int first) -> int {  // r = b - A x into column 0, r.r, the outer test, v_0 = r / beta
		SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, col(0), 0, nullptr, nullptr, first ? nullptr : solveOver, s));
		SMM_TRY(launchDotPartials<T>(n, col(0), col(0), parts1, first ? nullptr : solveOver, s));
		gmresOuter<T><<<1, TPB, 0, s>>>(sp, parts1, first, maxIterations, eps);
		if (n > 0) scaleKernel<T><<<solverGrid(n), TPB, 0, s>>>(n, &sp->beta, col(0), col(0), cycleOver);
		return SMM_HIP_OK;
	};
	SMM_TRY(residual(1));

	LoopWatch watch;
	SMM_TRY(watch.begin(s, solveOver, 1, 1));  // asked before every cycle but the first
	// every cycle that does not end the solve takes at least one step, so cycle c starts with at most maxIterations - c steps left
	for (int c = 0; c < maxIterations && !watch.leave(c); ++c) {
		const int steps = std::min(restart, maxIterations - c);
		for (int j = 0; j < steps; ++j) {
			const T* z = col(j);
			if (precondition) {
				SMM_TRY(precondApplyDev<T>(M, col(j), zv, cycleOver, s));
				z = zv;
			}
			T* w = col(j + 1);
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, z, w, 0, nullptr, nullptr, cycleOver, s));
			orthogonaliseTwice<T>(V.p, ld, n, gmv, j + 1, w, parts, parts1, sp->h1, sp->h2, sp->coef, cycleOver, s);
			gmresStep<T><<<1, TPB, 0, s>>>(sp, parts1, gmv, j, restart, maxIterations, eps);
			if (n > 0) scaleKernel<T><<<solverGrid(n), TPB, 0, s>>>(n, &sp->hn, w, w, cycleOver);
		}
		// the end of the cycle: y, t = sum y_i v_i, x = x + M^-1 t, the residual again
		gmresBackSub<T><<<1, TPB, 0, s>>>(sp);
		multiAxpyKernel<T, false><<<gmv, TPB, 0, s>>>(n, 0, &sp->k, V.p, ld, sp->y, nullptr, tv.p, nullptr, solveOver);
		const T* z = tv;
		if (precondition) {
			SMM_TRY(precondApplyDev<T>(M, tv, zv, solveOver, s));
			z = zv;
		}
		if (n > 0) gmresAddX<T><<<solverGrid(n), TPB, 0, s>>>(n, sp, z, x);
		SMM_TRY(residual(0));
	}
	struct {  // GmresState<T> from `rr` on
		T rr, beta, hn;
		int cycleOver, solveOver, k, iters, status, pad[3];
	} tail;
	static_assert(sizeof(tail) == sizeof(GmresState<T>) - offsetof(GmresState<T>, rr), "the tail of GmresState");
	SMM_TRY(loopFinish(watch, &tail, &sp->rr, sizeof(tail), s));
	const T rr = tail.rr;
	int st_out = SMM_SOLVER_MAX_ITERATIONS_REACHED;
	if (tail.status == SMM_SOLVER_DIVERGED || !std::isfinite(rr)) st_out = SMM_SOLVER_DIVERGED;
	else if (rr <= eps * eps) st_out = SMM_SOLVER_SUCCESS;
	if (status) *status = st_out;
	if (iterations) *iterations = tail.iters;
	if (resnorm2) *resnorm2 = rr;
	return precondition ? precondTakeError(M, s) : SMM_HIP_OK;
}

// host vectors (x in / out)
template <typename T>
static int gmresHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, int restart, const smm_hip_precond* M, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(gmresCheck<T>(a, b, x, restart));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return gmresDev<T>(a, db, dx, maxIterations, eps, restart, M, s, status, iterations, resnorm2);
	});
}

static int multiCheck(const char* what, int n, int k, long long ld, bool nullArray) {
	if (n < 0 || k < 1 || k > MAXR + 1 || ld < n || nullArray) {
		setError("%s: bad arguments (n >= 0, 1 <= k <= %d, ld >= n, no null array)", what, MAXR + 1);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int multiDotDev(int n, int k, const T* V, long long ld, const T* w, T* d_out, hipStream_t s) {
	SMM_TRY(multiCheck("multi_dot", n, k, ld, !d_out || (n > 0 && (!V || !w))));
	// one persistent partial-sum buffer per stream and scalar type, the two launches enqueued under one lock (see dotDev, smm_blas1.hip)
	static std::map<hipStream_t, T*> buffers;
	static std::mutex mu;
	std::lock_guard<std::mutex> lock(mu);
	auto it = buffers.find(s);
	if (it == buffers.end()) {
		T* p = nullptr;
		SMM_TRY(devAlloc(reinterpret_cast<void**>(&p), static_cast<size_t>(MAXR + 1) * NPART * sizeof(T)));
		it = buffers.emplace(s, p).first;
	}
	const int g = gridMV(n, sizeof(T));
	multiDotKernel<T><<<g, TPB, 0, s>>>(n, k, V, ld, w, it->second, nullptr);
	multiDotFinish<T><<<k, TPB, 0, s>>>(it->second, g, d_out, nullptr, nullptr);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template <typename T>
static int multiAxpyDev(int n, int k, const T* V, long long ld, const T* coef, const T* w, T* d_out, hipStream_t s) {
	SMM_TRY(multiCheck("multi_axpy", n, k, ld, n > 0 && (!V || !coef || !w || !d_out)));
	if (n == 0) return SMM_HIP_OK;
	multiAxpyKernel<T, false><<<gridMV(n, sizeof(T)), TPB, 0, s>>>(n, k, nullptr, V, ld, coef, w, d_out, nullptr, nullptr);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// (see preloadSolversUnit, smm_solvers.hip)
void preloadGmresUnit() {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(gmresBackSub<float>));
	(void)hipGetLastError();
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_gmres_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int restart, const smm_hip_precond* M, int* solver_status,
                      int* iterations, float* resnorm2) {
	return gmresHost<float>(a, b, x, maxIterations, eps, restart, M, solver_status, iterations, resnorm2);
}
int smm_hip_gmres_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int restart, const smm_hip_precond* M, int* solver_status,
                      int* iterations, double* resnorm2) {
	return gmresHost<double>(a, b, x, maxIterations, eps, restart, M, solver_status, iterations, resnorm2);
}
int smm_hip_gmres_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, int restart, const smm_hip_precond* M,
                          smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return gmresDev<float>(a, d_b, d_x, maxIterations, eps, restart, M, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_gmres_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, int restart, const smm_hip_precond* M,
                          smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return gmresDev<double>(a, d_b, d_x, maxIterations, eps, restart, M, pickStream(stream), solver_status, iterations, resnorm2);
}

int smm_hip_multi_dot_dev_f32(int n, int k, const float* d_V, long long ld, const float* d_w, float* d_out, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return multiDotDev<float>(n, k, d_V, ld, d_w, d_out, pickStream(stream));
}
int smm_hip_multi_dot_dev_f64(int n, int k, const double* d_V, long long ld, const double* d_w, double* d_out, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return multiDotDev<double>(n, k, d_V, ld, d_w, d_out, pickStream(stream));
}
int smm_hip_multi_axpy_dev_f32(int n, int k, const float* d_V, long long ld, const float* d_coef, const float* d_w, float* d_out, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return multiAxpyDev<float>(n, k, d_V, ld, d_coef, d_w, d_out, pickStream(stream));
}
int smm_hip_multi_axpy_dev_f64(int n, int k, const double* d_V, long long ld, const double* d_coef, const double* d_w, double* d_out, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return multiAxpyDev<double>(n, k, d_V, ld, d_coef, d_w, d_out, pickStream(stream));
}

}  // extern "C"
