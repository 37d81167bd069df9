// smm_solvers_cgs.hip -- device-resident ConjugateGradientSquared (ref:2104-2178): the transpose-free method for general matrices, two
// SpMVs per pass like BiCGStab.
//
// The definition is the reference's text with ONE repair (stated in include/smm_hip.h): `residualSquared` is declared before the `do`, so
// that the loop condition reads the value the body has just computed.  As published the template cannot be instantiated (ref:2171-2172).
//
// A pass is four launches -- no scalar-only launch, no host round trip besides the DonePoller checks of bicgstabLoop (smm_solvers.hip):
//   1. ap = A p with the partial sums of ap.r0 in the epilogue                                      (ref:2132-2133)
//   2. cgsFusedQX: alpha = rr0 / (ap.r0); q, alphaUQ, x            reads ap, u, x   writes q, alphaUQ, x   (ref:2135, 2145-2149)
//   3. r = r - A alphaUQ in place with the partial sums of r.r and r.r0 in the epilogue             (ref:2151-2152, 2171)
//   4. cgsFusedUP: the loop test, beta, u, p                       reads q, r, p    writes u, p            (ref:2154, 2164-2172)
// 11 n vector elements per pass besides the two SpMVs (BiCGStab's three update kernels move 14 n).  The update expressions keep the
// reference's shapes (_smm_fma nesting; alpha * (u + q) is an add and then a multiply), so given the same scalars they are the CPU loop's bits.
#include <algorithm>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;

// p = u = r0 = r   (ref:2124-2126)
template <typename T>
__global__ __launch_bounds__(TPB) void cgsCopy3(int n, const T* r, T* p, T* u, T* r0) {
	const T* const in[1] = {r};
	T* const out[3] = {p, u, r0};
	streamMap<T, false, 1, 3>(n, in, out, [&](const T(&v)[1], T(&o)[3]) { o[0] = o[1] = o[2] = v[0]; });
}

// alpha = rr0 / (ap.r0) ; q = -alpha ap + u ; alphaUQ = alpha (u + q) ; x = x + alphaUQ   (ref:2133-2149; no breakdown test, ref:2134)
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgsFusedQX(int n, Scal<T>* sc, int par, const T* __restrict__ partsA, const T* ap, const T* u, T* x, T* q, T* alphaUQ) {
	__shared__ T red[5];
	if (sc->done) return;
	const T alpha = sc->rrPing[par] / sumPartsAll(partsA, red);
	if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;
	const T* const in[3] = {ap, u, x};
	T* const out[3] = {q, alphaUQ, x};
	streamMap<T, NT, 3, 3>(n, in, out, [&](const T(&v)[3], T(&o)[3]) {
		const T qi = smmFma(-alpha, v[0], v[1]);
		const T uq = v[1] + qi;
		const T auq = alpha * uq;
		o[0] = qi;
		o[1] = auq;
		o[2] = v[2] + auq;
	});
}

// r.r and r.r0 ; iterations++ ; while (r.r > eps^2 && iterations < maxIterations): a NaN residual leaves the loop too ; beta = newRR0 / rr0 ;
// u = beta q + r ; p = beta (beta p + q) + u   (ref:2152-2172; no breakdown test, ref:2153).  partsC = [r.r | r.r0]; `pass` counts from 0.
// The pass that leaves the loop returns before u and p (neither is read again); x and r are complete by then.
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgsFusedUP(int n, Scal<T>* sc, int par, int pass, int maxIterations, const T* __restrict__ partsC, T eps, const T* q, const T* r,
                                                  T* u, T* p) {
	__shared__ T red[5];
	if (sc->done) return;
	const T rr = sumPartsAll(partsC, red);
	const T newRR0 = sumPartsAll(partsC + NPART, red);
	const T rr0 = sc->rrPing[par];
	const T beta = newRR0 / rr0;
	const bool leave = !(rr > eps * eps && pass + 1 < maxIterations);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		sc->res = rr;
		sc->beta = beta;
		sc->rrPing[par ^ 1] = newRR0;
		sc->iters = pass + 1;
		if (leave) sc->done = 1;
	}
	if (leave) return;
	const T* const in[3] = {q, r, p};
	T* const out[2] = {u, p};
	streamMap<T, NT, 3, 2>(n, in, out, [&](const T(&v)[3], T(&o)[2]) {
		const T ui = smmFma(beta, v[0], v[1]);
		o[0] = ui;
		o[1] = smmFma(beta, smmFma(beta, v[2], v[0]), ui);
	});
}

template <typename T>
static int cgsDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, hipStream_t s, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(solverCheck<T>("cgs", a, b, x));
	const int n = a->rows;
	maxIterations = std::min(maxIterations, n);  // ref:2111
	if (maxIterations == -1) maxIterations = n;  // ref:2112-2114
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	DevBuf<T> r, r0, p, u, q, alphaUQ, ap, parts, parts2;
	DevBuf<Scal<T>> sc;
	SMM_TRY(r.alloc(n));
	SMM_TRY(r0.alloc(n));
	SMM_TRY(p.alloc(n));
	SMM_TRY(u.alloc(n));
	SMM_TRY(q.alloc(n));
	SMM_TRY(alphaUQ.alloc(n));
	SMM_TRY(ap.alloc(n));
	SMM_TRY(parts.alloc(2 * NPART));   // [ap.r0]
	SMM_TRY(parts2.alloc(2 * NPART));  // [r.r | r.r0]
	SMM_TRY(sc.alloc(1));

	const int* doneFlag = &sc.p->done;
	const int planned = std::max(1, maxIterations);  // do { } while: the body always runs once (ref:2131, 2172)
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, planned));
	bool fromZero = false;  // x = 0 and finite values: r = b without an SpMV (zeroStart, smm_solver_host.h)
	SMM_TRY(zeroStart<T>(a, x, watch, s, &fromZero));
	if (fromZero) {
		SMM_TRY(launchCopyMany<T>(n, b, r, p, u, r0, s));  // r = p = u = r0 = b in one pass over b
	} else {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, nullptr, s));  // ref:2118
		if (n > 0) cgsCopy3<T><<<solverGrid(n), TPB, 0, s>>>(n, r, p, u, r0);               // ref:2124-2126
	}
	SMM_TRY(launchDotPartials<T>(n, r, r0, parts, nullptr, s));                       // ref:2128
	rr0InitScal<T><<<1, TPB, 0, s>>>(parts, sc);                                       // ref:2128 (smm_solver_scal.h)

	for (int i = 0; i < planned && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, ap, 1, r0, parts, doneFlag, s));  // ref:2132-2133
		SMM_LAUNCH_UPDATE(cgsFusedQX, updateNT(n, sizeof(T), 6), solverGrid(n), s, n, sc, i & 1, parts, ap, u, x, q, alphaUQ);
		SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, r, alphaUQ, r, 2, r0, parts2, doneFlag, s));  // ref:2151-2152 + 2171
		SMM_LAUNCH_UPDATE(cgsFusedUP, updateNT(n, sizeof(T), 5), solverGrid(n), s, n, sc, i & 1, i, maxIterations, parts2, eps, q, r, u, p);
	}
	Scal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	if (status) *status = h.iters > maxIterations ? SMM_SOLVER_MAX_ITERATIONS_REACHED : SMM_SOLVER_SUCCESS;  // ref:2174-2177
	if (iterations) *iterations = h.iters;
	if (resnorm2) *resnorm2 = h.res;
	return SMM_HIP_OK;
}

// host vectors: the reference's calling convention (x in / out)
template <typename T>
static int cgsHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(solverCheck<T>("cgs", a, b, x));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return cgsDev<T>(a, db, dx, maxIterations, eps, s, status, iterations, resnorm2);
	});
}

// (see preloadSolversUnit, smm_solvers.hip)
void preloadCgsUnit() {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(cgsCopy3<float>));
	(void)hipGetLastError();
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_cgs_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations, float* resnorm2) {
	return cgsHost<float>(a, b, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_cgs_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations, double* resnorm2) {
	return cgsHost<double>(a, b, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_cgs_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, smm_hip_stream stream, int* solver_status,
                        int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return cgsDev<float>(a, d_b, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_cgs_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, smm_hip_stream stream, int* solver_status,
                        int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return cgsDev<double>(a, d_b, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}

}  // extern "C"
