// smm_solvers_lsqr.hip -- device-resident LSQR (Paige and Saunders 1982): min ||A x - b||_2 for a matrix of ANY shape, with Tikhonov
// damping.  An addition: the reference has no LSQR, and every other solver of the library wants a square matrix.  The definition, line by
// line, is tests/lsqr_restatement.py; the contract is in include/smm_hip.h.
//
//   ub = b - A x;  bb = ub.ub;  beta = sqrt(bb)                                        (ub stays unnormalised: u = ub / beta)
//   t = At ub;  vb = t / beta;  aa = vb.vb;  alpha = sqrt(aa);  v = vb / alpha;  w = v
//   phibar = beta; rhobar = alpha; psi2 = 0
//   each step:
//       q = A v                                                                         (launch 1: the SpMV on `a`)
//       ub = _smm_fma(-(alpha / beta), ub, q);  bb = ub.ub                              (launch 2: lsqrLeft)
//       t = At ub                                                                       (launch 3: the SpMV on `at`)
//       beta = sqrt(bb);  vb = _smm_fma(-beta, v, t / beta);  aa = vb.vb                (launch 4: lsqrRight)
//       alpha = sqrt(aa);  the damping rotation and the plane rotation;  x = _smm_fma(phi / rho, w, x);
//       v = vb / alpha;  w = _smm_fma(-(theta / rho), w, v)                             (launch 5: lsqrRotate)
// The solve is for the correction dx = x - x0 of the system A dx = b - A x0, and x is updated IN PLACE: x = x0 + dx is never formed from
// a separate dx, so from x0 = 0 x holds dx's bits.  With damp > 0 it is therefore dx that is damped.
//
// A step is the two SpMVs and three update launches, no scalar-only launch, no host round trip besides the LoopWatch looks:
//   1. launchSpmv(a)    q = A v                                                         (any SpMV family)                    writes m
//   2. lsqrLeft         alpha / beta from the published scalars; ub in place; partial sums of ub.ub     reads q, ub   writes ub      3 m
//   3. launchSpmv(at)   t = At ub                                                       (the transpose handle's own family)  writes n
//   4. lsqrRight        beta from the partials; vb written over t; partial sums of vb.vb                reads t, v    writes vb      3 n
//   5. lsqrRotate       alpha, both rotations, the tests (every workgroup redoes them; workgroup 0 publishes them, the two estimates, the
//                       count and `done`), then x, v and w in one pass                  reads vb, w, x   writes v, w, x              6 n
// 3 m + 9 n vector elements per step besides the two SpMVs.
//
// The recurrence scalars are double-buffered by step parity (LsqrScal::rot), as MinresScal's are: a launch reads the set its predecessor
// published and workgroup 0 writes the other one, so no workgroup reads a word that a workgroup of the same launch writes.  lsqrRotate looks
// at rot[par].stop, not at `done` -- the launch that ends the loop still applies its x update in every workgroup -- and a set carries the
// step it was published for, so the launches queued behind the end of the loop find either a raised stop or a set that is not theirs (the
// block starts as all-ones bytes: no step's).  `done` is what the SpMV kernels, lsqrLeft, lsqrRight and the host look at.
// Sums: NPART partials added in index order by every workgroup (sumPartsAll); no floating-point atomics.
#include <algorithm>
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;

template <typename T>
struct LsqrRot {
	T alpha, beta, rhobar, phibar, psi2;
	int stop;     // the loop has ended: the step this set was published for is not taken
	int forStep;  // the step this set was published for (a set left over from two steps back is not this step's)
};

template <typename T>
struct LsqrScal {
	LsqrRot<T> rot[2];  // by step parity: step i reads rot[i & 1] and publishes rot[(i & 1) ^ 1]
	T res;              // the last phibar^2 + psi2
	T arn;              // the last (alpha |c| phibar)^2
	int done, iters, status, pad;
};

// ub = _smm_fma(-(alpha / beta), ub, q), in place ; the partial sums of ub.ub
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void lsqrLeft(int m, const LsqrScal<T>* sc, int par, T* __restrict__ partsU, const T* q, T* ub) {
	__shared__ T red[4];
	if (sc->done) return;
	const T c = sc->rot[par].alpha / sc->rot[par].beta;
	T acc = T(0);
	const T* const in[2] = {q, ub};
	T* const out[1] = {ub};
	streamMap<T, NT, 2, 1>(m, in, out, [&](const T(&e)[2], T(&o)[1]) {
		const T u = smmFma(-c, e[1], e[0]);
		o[0] = u;
		acc += u * u;
	});
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) partsU[blockIdx.x] = s;
}

// beta = sqrt(ub.ub) ; vb = _smm_fma(-beta, v, t / beta) written over t (FIRST: vb = t / beta, there is no v yet) ; beta == 0: vb = 0, nothing
// is divided ; the partial sums of vb.vb
template <typename T, bool NT, bool FIRST>
__global__ __launch_bounds__(TPB) void lsqrRight(int n, const LsqrScal<T>* sc, const T* __restrict__ partsU, T* __restrict__ partsV, const T* v, T* t) {
	__shared__ T red[5];
	if (!FIRST && sc->done) return;
	const T beta = sqrt(sumPartsAll(partsU, red));
	const bool none = beta == T(0);
	T acc = T(0);
	const T* const in[2] = {t, FIRST ? t : v};
	T* const out[1] = {t};
	streamMap<T, NT, 2, 1>(n, in, out, [&](const T(&e)[2], T(&o)[1]) {
		T y = T(0);
		if (!none) {
			y = e[0] / beta;
			if (!FIRST) y = smmFma(-beta, e[1], y);
		}
		o[0] = y;
		acc += y * y;
	});
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) partsV[blockIdx.x] = s;
}

// The start: beta = sqrt(ub.ub), alpha = sqrt(vb.vb), the scalars of step 0, the tests of a solve that takes no step; then v = vb / alpha, w = v.
template <typename T>
__global__ __launch_bounds__(TPB) void lsqrStart(int n, LsqrScal<T>* sc, const T* __restrict__ partsU, const T* __restrict__ partsV, int maxIterations, T eps,
                                                 const T* vb, T* v, T* w) {
	__shared__ T red[5];
	const T bb = sumPartsAll(partsU, red);
	const T aa = sumPartsAll(partsV, red);
	const T beta = sqrt(bb);
	const T alpha = sqrt(aa);
	const T ab = alpha * beta;
	const T arn = ab * ab;
	const bool bad = !isfinite(beta) || !isfinite(alpha);
	const bool stop = bad || bb == T(0) || aa == T(0) || !(bb > eps * eps) || !(arn > eps * eps) || maxIterations <= 0;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		LsqrRot<T> o;
		o.alpha = alpha;
		o.beta = beta;
		o.rhobar = alpha;
		o.phibar = beta;
		o.psi2 = T(0);
		o.stop = stop ? 1 : 0;
		o.forStep = 0;
		sc->rot[0] = o;
		sc->res = bb;
		sc->arn = arn;
		sc->iters = 0;
		sc->status = bad ? SMM_SOLVER_DIVERGED : SMM_SOLVER_SUCCESS;
		sc->done = stop ? 1 : 0;
	}
	if (stop) return;
	const T* const in[1] = {vb};
	T* const out[2] = {v, w};
	streamMap<T, false, 1, 2>(n, in, out, [&](const T(&e)[1], T(&o)[2]) {
		const T y = e[0] / alpha;
		o[0] = y;
		o[1] = y;
	});
}

// beta and alpha from the two sets of partials, the damping rotation, the plane rotation, the tests ; x = x + (phi / rho) w ;
// v = vb / alpha (alpha == 0: v = 0) ; w = v - (theta / rho) w.  `step` counts from 0.  The launch that ends the loop still updates x;
// a beta, alpha, rho or phibar that is not finite, or rho == 0: DIVERGED, the step is not taken and x stays.
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void lsqrRotate(int n, LsqrScal<T>* sc, int par, int step, int maxIterations, T eps, T damp, const T* __restrict__ partsU,
                                                  const T* __restrict__ partsV, const T* vb, T* v, T* w, T* x) {
	__shared__ T red[5];
	const LsqrRot<T> in = sc->rot[par];
	if (in.stop || in.forStep != step) return;
	const T bb = sumPartsAll(partsU, red);
	const T aa = sumPartsAll(partsV, red);
	const T beta = sqrt(bb);
	const T alpha = sqrt(aa);
	T rb1 = in.rhobar, psi = T(0), phibar1 = in.phibar;  // damp == 0: the first rotation is the identity, bit for bit
	if (damp != T(0)) {
		rb1 = sqrt(in.rhobar * in.rhobar + damp * damp);
		const T c1 = in.rhobar / rb1;
		const T s1 = damp / rb1;
		psi = s1 * in.phibar;
		phibar1 = c1 * in.phibar;
	}
	const T rho = sqrt(rb1 * rb1 + bb);
	const T c = rb1 / rho;
	const T sn = beta / rho;
	const T theta = sn * alpha;
	const T rhobar = -c * alpha;
	const T phi = c * phibar1;
	const T phibar = sn * phibar1;
	const bool bad = !isfinite(beta) || !isfinite(alpha) || !isfinite(rho) || !isfinite(phibar) || rho == T(0);
	const T psi2 = in.psi2 + psi * psi;
	const T res = phibar * phibar + psi2;
	const T ar = alpha * (c < T(0) ? -c : c) * phibar;
	const T arn = ar * ar;
	const bool stop = bad || beta == T(0) || alpha == T(0) || !(res > eps * eps) || !(arn > eps * eps) || step + 1 >= maxIterations;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		LsqrRot<T> o;
		o.alpha = alpha;
		o.beta = beta;
		o.rhobar = rhobar;
		o.phibar = phibar;
		o.psi2 = psi2;
		o.stop = stop ? 1 : 0;
		o.forStep = step + 1;
		sc->rot[par ^ 1] = o;
		if (bad) {
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->res = res;
			sc->arn = arn;
			sc->iters = step + 1;
		}
		if (stop) sc->done = 1;
	}
	if (bad) return;
	const T t1 = phi / rho;
	const T t2 = theta / rho;
	const bool none = alpha == T(0);
	const T* const src[3] = {vb, w, x};
	T* const out[3] = {v, w, x};
	streamMap<T, NT, 3, 3>(n, src, out, [&](const T(&e)[3], T(&o)[3]) {
		const T vn = none ? T(0) : e[0] / alpha;
		o[0] = vn;
		o[1] = smmFma(-t2, e[1], vn);
		o[2] = smmFma(t1, e[1], e[2]);
	});
}

struct LsqrCsrOwner {  // the transpose a solve built for itself
	smm_hip_csr* m = nullptr;
	~LsqrCsrOwner() { smm_hip_csr_destroy(m); }
};

// what can be refused before anything is staged or enqueued: the matrices' dtypes, the shape of `at`, the vectors, eps and damp
template <typename T>
static int lsqrCheck(const smm_hip_csr* a, const smm_hip_csr* at, const T* b, const T* x, T eps, T damp) {
	SMM_TRY(solverCheckRect<T>("lsqr", a, b, x));
	if (at && at->dtype != dtypeOf<T>()) {
		setError("lsqr: `at` holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (at == a && a->rows != a->cols) {
		setError("lsqr: `a` itself as `at` asserts symmetry, and a %d x %d matrix is not square", a->rows, a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	if (at && (at->rows != a->cols || at->cols != a->rows || at->nnz != a->nnz)) {
		setError("lsqr: `at` has not the shape or the entry count of the transpose");
		return SMM_HIP_ERR_INVALID;
	}
	if (!std::isfinite(eps) || eps < T(0)) {
		setError("lsqr: eps must be finite and not negative");
		return SMM_HIP_ERR_INVALID;
	}
	if (!std::isfinite(damp) || damp < T(0)) {
		setError("lsqr: damp must be finite and not negative");
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int lsqrDev(const smm_hip_csr* a, const smm_hip_csr* at, const T* b, T* x, int maxIterations, T eps, T damp, hipStream_t s, int* status, int* iterations,
                   int* reason, T* resnorm2, T* arnorm2) {
	SMM_TRY(lsqrCheck<T>(a, at, b, x, eps, damp));
	const int m = a->rows, n = a->cols;
	if (m == 0 || n == 0) {  // nothing to fit (m == 0) or nothing to fit with (n == 0: At r is empty): b and x are not touched
		if (status) *status = SMM_SOLVER_SUCCESS;
		if (iterations) *iterations = 0;
		if (reason) *reason = m == 0 ? 1 : 2;
		if (resnorm2) *resnorm2 = T(0);
		if (arnorm2) *arnorm2 = T(0);
		return SMM_HIP_OK;
	}
	if (maxIterations < 0) maxIterations = n;
	// (in this order: an error return synchronises, then releases the vectors, then destroys the transpose -- never under queued kernels)
	LsqrCsrOwner built;
	DevBuf<T> ub, q, t, v, w, partsU, partsV;
	DevBuf<LsqrScal<T>> sc;
	SyncOnExit drain{s};
	const bool empty = a->nnz == 0;  // A v = 0 and At u = 0: no SpMV is launched and no transpose is built
	SMM_TRY(ensureCsrReady(a, s, true));
	if (!empty) {
		if (!at) {
			SMM_TRY(csrTransposeCreate(a, s, &built.m));
			at = built.m;
		}
		SMM_TRY(ensureCsrReady(at, s, true));
		SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
		if (at != a) SMM_TRY(adoptPatternForSolver(at, maxIterations, s));
	}
	SMM_TRY(ub.alloc(m));
	SMM_TRY(q.alloc(m));
	SMM_TRY(t.alloc(n));  // t = At ub, then vb in the same place
	SMM_TRY(v.alloc(n));
	SMM_TRY(w.alloc(n));
	SMM_TRY(partsU.alloc(NPART));  // [ub.ub]
	SMM_TRY(partsV.alloc(NPART));  // [vb.vb]
	SMM_TRY(sc.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(partsU.p, 0, sizeof(T) * NPART, s));  // lsqrLeft and lsqrRight write one slot per workgroup: the others stay 0
	SMM_HIP_TRY(hipMemsetAsync(partsV.p, 0, sizeof(T) * NPART, s));
	SMM_HIP_TRY(hipMemsetAsync(sc.p, 0xFF, sizeof(LsqrScal<T>), s));  // (no set is any step's until it is published)
	const int gm = solverGrid(m), gn = solverGrid(n);
	const int* doneFlag = &sc.p->done;

	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, maxIterations));
	bool fromZero = false;  // x = 0 and finite values: ub = b without an SpMV (zeroStart, smm_solver_host.h); x has n elements
	if (!empty) SMM_TRY(zeroStart<T>(a, x, n, watch, s, &fromZero));
	if (empty || fromZero) SMM_TRY(launchCopy2<T>(m, b, ub, nullptr, s));
	else SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, ub, 0, nullptr, nullptr, nullptr, s));
	SMM_TRY(launchDotPartials<T>(m, ub, ub, partsU, nullptr, s));
	if (empty) SMM_HIP_TRY(hipMemsetAsync(t.p, 0, sizeof(T) * n, s));
	else SMM_TRY(launchSpmv<T>(at, SMM_OP_ASSIGN, nullptr, ub, t, 0, nullptr, nullptr, nullptr, s));
	lsqrRight<T, false, true><<<gn, TPB, 0, s>>>(n, sc, partsU, partsV, v, t);
	lsqrStart<T><<<gn, TPB, 0, s>>>(n, sc, partsU, partsV, maxIterations, eps, t, v, w);

	// (an empty matrix has ended at the start: aa == 0)
	for (int i = 0; !empty && i < maxIterations && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, v, q, 0, nullptr, nullptr, doneFlag, s));
		SMM_LAUNCH_UPDATE(lsqrLeft, updateNT(m, sizeof(T), 3), gm, s, m, sc, i & 1, partsU, q, ub);
		SMM_TRY(launchSpmv<T>(at, SMM_OP_ASSIGN, nullptr, ub, t, 0, nullptr, nullptr, doneFlag, s));
		if (updateNT(n, sizeof(T), 3)) lsqrRight<T, true, false><<<gn, TPB, 0, s>>>(n, sc, partsU, partsV, v, t);
		else lsqrRight<T, false, false><<<gn, TPB, 0, s>>>(n, sc, partsU, partsV, v, t);
		SMM_LAUNCH_UPDATE(lsqrRotate, updateNT(n, sizeof(T), 6), gn, s, n, sc, i & 1, i, maxIterations, eps, damp, partsU, partsV, t, v, w, x);
	}
	LsqrScal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	drain.armed = false;
	int st = SMM_SOLVER_MAX_ITERATIONS_REACHED, why = 0;
	if (h.status == SMM_SOLVER_DIVERGED) {
		st = SMM_SOLVER_DIVERGED;
	} else if (h.res <= eps * eps) {
		st = SMM_SOLVER_SUCCESS;
		why = 1;
	} else if (h.arn <= eps * eps) {
		st = SMM_SOLVER_SUCCESS;
		why = 2;
	}
	if (status) *status = st;
	if (iterations) *iterations = h.iters;
	if (reason) *reason = why;
	if (resnorm2) *resnorm2 = h.res;
	if (arnorm2) *arnorm2 = h.arn;
	return SMM_HIP_OK;
}

// host vectors (x in / out): b has rows elements, x has cols
template <typename T>
static int lsqrHost(const smm_hip_csr* a, const smm_hip_csr* at, T* b, T* x, int maxIterations, T eps, T damp, int* status, int* iterations, int* reason,
                    T* resnorm2, T* arnorm2) {
	SMM_TRY(lsqrCheck<T>(a, at, b, x, eps, damp));
	const bool nothing = a->rows == 0 || a->cols == 0;  // (neither vector is read or written then)
	return solveFromHost2<T>(nothing ? 0 : a->rows, nothing ? 0 : a->cols, b, x, [&](const T* db, T* dx, hipStream_t s) {
		return lsqrDev<T>(a, at, db, dx, maxIterations, eps, damp, s, status, iterations, reason, resnorm2, arnorm2);
	});
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_lsqr_f32(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int maxIterations, float eps, float damp, int* solver_status, int* iterations,
                     int* reason, float* resnorm2, float* arnorm2) {
	return lsqrHost<float>(a, at, b, x, maxIterations, eps, damp, solver_status, iterations, reason, resnorm2, arnorm2);
}
int smm_hip_lsqr_f64(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int maxIterations, double eps, double damp, int* solver_status,
                     int* iterations, int* reason, double* resnorm2, double* arnorm2) {
	return lsqrHost<double>(a, at, b, x, maxIterations, eps, damp, solver_status, iterations, reason, resnorm2, arnorm2);
}
int smm_hip_lsqr_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, const float* d_b, float* d_x, int maxIterations, float eps, float damp, smm_hip_stream stream,
                         int* solver_status, int* iterations, int* reason, float* resnorm2, float* arnorm2) {
	SMM_TRY(ensureInit());
	return lsqrDev<float>(a, at, d_b, d_x, maxIterations, eps, damp, pickStream(stream), solver_status, iterations, reason, resnorm2, arnorm2);
}
int smm_hip_lsqr_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, const double* d_b, double* d_x, int maxIterations, double eps, double damp,
                         smm_hip_stream stream, int* solver_status, int* iterations, int* reason, double* resnorm2, double* arnorm2) {
	SMM_TRY(ensureInit());
	return lsqrDev<double>(a, at, d_b, d_x, maxIterations, eps, damp, pickStream(stream), solver_status, iterations, reason, resnorm2, arnorm2);
}

}  // extern "C"
