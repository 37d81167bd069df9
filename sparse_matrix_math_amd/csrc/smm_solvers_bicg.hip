// smm_solvers_bicg.hip -- device-resident BiCG for general matrices: BiCGSymmetric's text (ref:2021-2102) with the shadow sequence
// written out.  rt and pt follow Aᵀ (a handle of its own, smm_transpose.hip) where the reference, assuming Aᵀ = A, lets r and p stand
// in for them:
//   denom = (A p).pt   alpha = rho / denom   x += alpha p   r -= alpha A p   rt -= alpha Aᵀ pt
//   rho' = rt.r   rr' = r.r   beta = rho' / rho   p = r + beta p   pt = rt + beta pt
// with the reference's two DIVERGED tests on rr (ref:2056, 2079) and its loop test on rr (ref:2096).
//
// A pass is six launches, the stages of bicgsymmetricDev (smm_solvers.hip) at the same launch geometry:
//   1. ap = A p with the partial sums of ap.pt in the epilogue          2. atp = Aᵀ pt
//   3. bicgAlphaScal (one workgroup)                                    4. bicgUpdateXRR: reads p, ap, atp, x, r, rt once, writes x, r, rt,
//   5. bicgBetaScal (one workgroup)                                        leaves the partial sums of rt.r and r.r
//   6. bicgUpdateP: p and pt together
// 10 n elements read and 5 n written per pass besides the two SpMVs.
//
// THE BIT RULE.  When Aᵀ has A's bits, rt == r, pt == p and rho == rr hold bit for bit, and every sum here is partitioned as the bsym*
// stages partition theirs (NPART workgroups of 256 lanes over streamMap, sumParts), every update has the reference's plain shape
// (ref:2069-2070, 2091: a product and then a sum, not _smm_fma): the solve returns BiCGSymmetric's status, pass count and x bit for bit.
#include <algorithm>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;

// Scal<T>: rr = r.r, rrPing[0] = rho = rt.r (equal at the start: rt = r, ref:2043)
template <typename T>
__global__ __launch_bounds__(TPB) void bicgInitRho(const T* __restrict__ partials, Scal<T>* sc) {
	__shared__ T red[4];
	const T rr = sumParts(partials, red);
	if (threadIdx.x == 0) {
		sc->rr = rr;
		sc->rrPing[0] = rr;
		sc->res = rr;
		sc->iters = 0;
		sc->done = 0;
		sc->status = SMM_SOLVER_SUCCESS;
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void bicgAlphaScal(const T* __restrict__ partials, Scal<T>* sc, T eps) {
	__shared__ T red[4];
	if (sc->done) return;
	const T denom = sumParts(partials, red);
	if (threadIdx.x == 0) {
		if (eps > (denom < T(0) ? -denom : denom) && sc->rr > T(1)) {  // ref:2056-2058
			sc->done = 1;
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->alpha = sc->rrPing[0] / denom;
		}
	}
}

// x += alpha p ; r -= alpha ap ; rt -= alpha atp  (ref:2068-2071: plain += / -= forms); partials = [rt.r | r.r]
template <typename T>
__global__ __launch_bounds__(TPB) void bicgUpdateXRR(int n, const Scal<T>* __restrict__ sc, const T* p, const T* ap, const T* atp, T* x, T* r, T* rt,
                                                     T* __restrict__ partials) {
	__shared__ T red[4];
	if (sc->done) return;
	const T alpha = sc->alpha;
	T accRho = T(0), accRR = T(0);
	const T* const in[6] = {p, x, ap, r, atp, rt};
	T* const out[3] = {x, r, rt};
	streamMap<T, false, 6, 3>(n, in, out, [&](const T(&v)[6], T(&o)[3]) {
		const T pa = alpha * v[0];
		o[0] = v[1] + pa;
		const T qa = alpha * v[2];
		const T ri = v[3] - qa;
		o[1] = ri;
		const T qta = alpha * v[4];
		const T rti = v[5] - qta;
		o[2] = rti;
		accRho += rti * ri;
		accRR += ri * ri;
	});
	const T sRho = blockSum256(accRho, red);
	const T sRR = blockSum256(accRR, red);
	if (threadIdx.x == 0) {
		partials[blockIdx.x] = sRho;
		partials[NPART + blockIdx.x] = sRR;
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void bicgBetaScal(const T* __restrict__ partials, Scal<T>* sc, T eps) {
	__shared__ T red[4];
	if (sc->done) return;
	const T newRho = sumParts(partials, red);
	const T newRR = sumParts(partials + NPART, red);  // ref:2075
	if (threadIdx.x == 0) {
		if (newRR > T(1) && sc->rr < eps) {  // ref:2079-2081
			sc->done = 1;
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->beta = newRho / sc->rrPing[0];
			sc->rrPing[0] = newRho;
			sc->rr = newRR;
			sc->res = newRR;
			sc->iters += 1;
			if (!(newRR > eps * eps)) sc->done = 1;  // ref:2096: a NaN residual leaves the loop too
		}
	}
}

// p = r + beta p ; pt = rt + beta pt  (ref:2090-2092)
template <typename T>
__global__ __launch_bounds__(TPB) void bicgUpdateP(int n, const Scal<T>* __restrict__ sc, const T* r, const T* rt, T* p, T* pt) {
	if (sc->done) return;
	const T beta = sc->beta;
	const T* const in[4] = {p, r, pt, rt};
	T* const out[2] = {p, pt};
	streamMap<T, false, 4, 2>(n, in, out, [&](const T(&v)[4], T(&o)[2]) {
		const T bp = beta * v[0];
		o[0] = v[1] + bp;
		const T bpt = beta * v[2];
		o[1] = v[3] + bpt;
	});
}

struct CsrOwner {  // the transpose a solve built for itself
	smm_hip_csr* m = nullptr;
	~CsrOwner() { smm_hip_csr_destroy(m); }
};

template <typename T>
static int bicgDev(const smm_hip_csr* a, const smm_hip_csr* at, const T* b, T* x, int maxIterations, T eps, hipStream_t s, int* status, int* iterations,
                   T* resnorm2) {
	SMM_TRY(solverCheck<T>("bicg", a, b, x));
	if (at && at->dtype != dtypeOf<T>()) {
		setError("bicg: null matrix or dtype mismatch");
		return SMM_HIP_ERR_INVALID;
	}
	const int n = a->rows;
	// (in this order: an error return synchronises, then releases the vectors, then destroys the transpose -- never under queued kernels)
	CsrOwner built;
	DevBuf<T> r, rt, p, pt, ap, atp, partsD, partsU;
	DevBuf<Scal<T>> sc;
	SyncOnExit drain{s};
	SMM_TRY(ensureCsrReady(a, s, true));
	if (!at) {
		SMM_TRY(csrTransposeCreate(a, s, &built.m));
		at = built.m;
	}
	SMM_TRY(ensureCsrReady(at, s, true));
	if (at->rows != a->cols || at->cols != a->rows || at->nnz != a->nnz) {
		setError("bicg: `at` has not the shape or the entry count of the transpose");
		return SMM_HIP_ERR_INVALID;
	}
	maxIterations = std::min(maxIterations, n);  // ref:2030-2033
	if (maxIterations == -1) maxIterations = n;
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	if (at != a) SMM_TRY(adoptPatternForSolver(at, maxIterations, s));
	SMM_TRY(r.alloc(n));
	SMM_TRY(rt.alloc(n));
	SMM_TRY(p.alloc(n));
	SMM_TRY(pt.alloc(n));
	SMM_TRY(ap.alloc(n));
	SMM_TRY(atp.alloc(n));
	SMM_TRY(partsD.alloc(2 * NPART));  // [ap.pt]
	SMM_TRY(partsU.alloc(2 * NPART));  // [rt.r | r.r]
	SMM_TRY(sc.alloc(1));
	SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, nullptr, s));  // ref:2036
	SMM_TRY(launchCopy2<T>(n, r, p, rt, s));
	SMM_TRY(launchCopy2<T>(n, r, pt, nullptr, s));
	SMM_TRY(launchDotPartials<T>(n, r, r, partsD, nullptr, s));
	bicgInitRho<T><<<1, TPB, 0, s>>>(partsD, sc);
	const int* doneFlag = &sc.p->done;
	const int planned = std::max(1, maxIterations);
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, planned));
	for (int i = 0; i < planned && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, ap, 1, pt, partsD, doneFlag, s));  // ref:2048-2049
		SMM_TRY(launchSpmv<T>(at, SMM_OP_ASSIGN, nullptr, pt, atp, 0, nullptr, nullptr, doneFlag, s));
		bicgAlphaScal<T><<<1, TPB, 0, s>>>(partsD, sc, eps);
		bicgUpdateXRR<T><<<NPART, TPB, 0, s>>>(n, sc, p, ap, atp, x, r, rt, partsU);
		bicgBetaScal<T><<<1, TPB, 0, s>>>(partsU, sc, eps);
		bicgUpdateP<T><<<solverGrid(n), TPB, 0, s>>>(n, sc, r, rt, p, pt);
	}
	Scal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	drain.armed = false;
	int st = h.status;
	if (st == SMM_SOLVER_SUCCESS && h.iters > maxIterations) st = SMM_SOLVER_MAX_ITERATIONS_REACHED;  // ref:2098-2100
	if (status) *status = st;
	if (iterations) *iterations = h.iters;
	if (resnorm2) *resnorm2 = h.res;
	return SMM_HIP_OK;
}

// host vectors: the reference's calling convention (x in / out)
template <typename T>
static int bicgHost(const smm_hip_csr* a, const smm_hip_csr* at, T* b, T* x, int maxIterations, T eps, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(solverCheck<T>("bicg", a, b, x));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return bicgDev<T>(a, at, db, dx, maxIterations, eps, s, status, iterations, resnorm2);
	});
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_bicg_f32(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations,
                     float* resnorm2) {
	return bicgHost<float>(a, at, b, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_bicg_f64(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations,
                     double* resnorm2) {
	return bicgHost<double>(a, at, b, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_bicg_dev_f32(const smm_hip_csr* a, const smm_hip_csr* at, const float* d_b, float* d_x, int maxIterations, float eps, smm_hip_stream stream,
                         int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return bicgDev<float>(a, at, d_b, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_bicg_dev_f64(const smm_hip_csr* a, const smm_hip_csr* at, const double* d_b, double* d_x, int maxIterations, double eps, smm_hip_stream stream,
                         int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return bicgDev<double>(a, at, d_b, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}

}  // extern "C"
