// smm_solvers_minres.hip -- device-resident MINRES (Paige and Saunders 1975) with a symmetric positive definite preconditioner: the
// short-recurrence method for symmetric INDEFINITE matrices.  An addition: the reference has no MINRES.  The definition, line by line, is
// tests/minres_restatement.py; the contract is in include/smm_hip.h.
//
//   r1 = b - A x;  y = M^-1 r1;  beta1 = sqrt(r1.y);  r2 = r1
//   oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0;  v = y / beta
//   each step:
//       Av = A v;  alfa = v.Av                                                          (launch 1: the SpMV with the fused dot)
//       t = Av;  step >= 2: t = _smm_fma(-(beta / oldb), r1, t);  t = _smm_fma(-(alfa / beta), r2, t);  r1 = r2;  r2 = t   (launch 2)
//       y = M^-1 r2;  oldb = beta;  beta = sqrt(r2.y)
//       oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
//       gamma = max(sqrt(gbar^2 + beta^2), eps_machine(T)); cs = gbar / gamma; sn = beta / gamma; phi = cs phibar; phibar = sn phibar
//       w1 = w2; w2 = w;  w = _smm_fma(-delta, w2, _smm_fma(-oldeps, w1, v)) / gamma;  x = _smm_fma(phi, w, x);  v = y / beta   (launch 3)
// alfa is taken from A v before r1 is subtracted (the SpMV's epilogue forms it): v.r1 = 0 in exact arithmetic (the Lanczos vectors are
// M^-1-orthogonal), so this is the textbook alfa up to rounding, and it is what the restatement computes.
//
// A step without a preconditioner is three launches, no scalar-only launch, no host round trip besides the LoopWatch looks:
//   1. launchSpmv      Av = A v, partial sums of v.Av in the epilogue                    (any SpMV family)
//   2. minresLanczos   alfa from the partials; the new r2 into the buffer of the old r1 (the host rotates the three pointers);
//                      partial sums of r2.r2                                             reads Av, r1, r2   writes r2'        4 n
//   3. minresRotate    beta, the Givens scalars (every workgroup redoes them; workgroup 0 publishes them, phibar^2, the count and `done`),
//                      then w, x and the next v in one pass                              reads v, y, w1, w2, x   writes w, x, v   8 n
// With a preconditioner y = M^-1 r2 (precondApplyDev) and the dot r2.y (launchDotPartials) sit between 2 and 3, and minresLanczos leaves
// the sum to them.  12 n vector elements per step besides the SpMV and the apply.
//
// The recurrence scalars are double-buffered by step parity (MinresScal::rot): a launch reads the set its predecessor published and
// workgroup 0 writes the other one, so no workgroup reads a word that a workgroup of the same launch writes.  That includes the stop test:
// minresRotate looks at rot[par].stop, not at `done` -- the launch that ends the loop still applies its x update in every workgroup.
// A set carries the step it was published for, so the launches queued behind the end of the loop find either a raised stop or a set that
// is not theirs (the block starts as all-ones bytes: no step's).
// `done` is what the SpMV kernels, the preconditioner applies, minresLanczos and the host look at.
// Sums: NPART partials added in index order by every workgroup (sumPartsAll); no floating-point atomics.
#include <algorithm>
#include <cmath>
#include <limits>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;

template <typename T>
struct MinresRot {
	T beta, oldb, dbar, epsln, phibar, cs, sn;
	int stop;     // the loop has ended: the step this set was published for is not taken
	int forStep;  // the step this set was published for (a set left over from two steps back is not this step's)
};

template <typename T>
struct MinresScal {
	MinresRot<T> rot[2];  // by step parity: step i reads rot[i & 1] and publishes rot[(i & 1) ^ 1]
	T alfa;               // of the running step (minresLanczos -> minresRotate)
	T res;                // the last phibar^2
	int done, iters, status, pad;
};

// The start: beta1 = sqrt(r1.y), the scalars of step 0, the tests of a solve that takes no step; then v = y / beta1, r2 = r1, w = w2 = 0.
// partsB = [r1.y]; y == r1 without a preconditioner.
template <typename T>
__global__ __launch_bounds__(TPB) void minresStart(int n, MinresScal<T>* sc, const T* __restrict__ partsB, int maxIterations, T eps, const T* r1, const T* y, T* r2,
                                                   T* v, T* w, T* w2) {
	__shared__ T red[5];
	const T ry = sumPartsAll(partsB, red);
	const T beta1 = sqrt(ry);
	const bool bad = ry < T(0) || !isfinite(beta1);  // r1.y < 0: the preconditioner is not positive definite
	const bool stop = bad || !(ry > eps * eps) || maxIterations <= 0;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		MinresRot<T> o;
		o.beta = beta1;
		o.oldb = T(0);
		o.dbar = T(0);
		o.epsln = T(0);
		o.phibar = beta1;
		o.cs = T(-1);
		o.sn = T(0);
		o.stop = stop ? 1 : 0;
		o.forStep = 0;
		sc->rot[0] = o;
		sc->alfa = T(0);
		sc->res = ry;
		sc->iters = 0;
		sc->status = bad ? SMM_SOLVER_DIVERGED : SMM_SOLVER_SUCCESS;
		sc->done = stop ? 1 : 0;
	}
	if (stop) return;
	const T* const in[2] = {r1, y};
	T* const out[4] = {r2, v, w, w2};
	streamMap<T, false, 2, 4>(n, in, out, [&](const T(&e)[2], T(&o)[4]) {
		o[0] = e[0];
		o[1] = e[1] / beta1;
		o[2] = T(0);
		o[3] = T(0);
	});
}

// alfa = v.Av ; r2' = Av - (beta / oldb) r1 - (alfa / beta) r2, written over r1 (element-wise in place) ; SUM: the partial sums of r2'.r2'
template <typename T, bool NT, bool SUM>
__global__ __launch_bounds__(TPB) void minresLanczos(int n, MinresScal<T>* sc, int par, int step, const T* __restrict__ partsA, T* __restrict__ partsB, const T* Av,
                                                     const T* r2, T* r1) {
	__shared__ T red[5];
	if (sc->done) return;
	const T alfa = sumPartsAll(partsA, red);
	const T beta = sc->rot[par].beta;
	const T c2 = alfa / beta;
	const T c1 = step > 0 ? beta / sc->rot[par].oldb : T(0);
	if (blockIdx.x == 0 && threadIdx.x == 0) sc->alfa = alfa;
	T acc = T(0);
	const T* const in[3] = {Av, r1, r2};
	T* const out[1] = {r1};
	streamMap<T, NT, 3, 1>(n, in, out, [&](const T(&e)[3], T(&o)[1]) {
		T t = e[0];
		if (step > 0) t = smmFma(-c1, e[1], t);
		t = smmFma(-c2, e[2], t);
		o[0] = t;
		if (SUM) acc += t * t;
	});
	if (SUM) {
		const T s = blockSum256(acc, red);
		if (threadIdx.x == 0) partsB[blockIdx.x] = s;
	}
}

// beta = sqrt(r2.y), the rotation, the tests ; w' = (v - oldeps w1 - delta w2) / gamma over w1 ; x = x + phi w' ; v = y / beta.
// `step` counts from 0.  The launch that ends the loop still updates x (beta == 0: the Krylov space is exhausted, phibar becomes 0);
// r2.y < 0 or a beta / phibar that is not finite: DIVERGED, the step is not taken and x stays.
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void minresRotate(int n, MinresScal<T>* sc, int par, int step, int maxIterations, T eps, const T* __restrict__ partsB, const T* y,
                                                    T* v, T* w1, const T* w2, T* x) {
	__shared__ T red[5];
	const MinresRot<T> in = sc->rot[par];
	if (in.stop || in.forStep != step) return;
	const T ry = sumPartsAll(partsB, red);
	const T alfa = sc->alfa;
	const T beta = sqrt(ry);
	const T oldeps = in.epsln;
	const T delta = in.cs * in.dbar + in.sn * alfa;
	const T gbar = in.sn * in.dbar - in.cs * alfa;
	const T epsln = in.sn * beta;
	const T dbar = -in.cs * beta;
	const T root = sqrt(gbar * gbar + beta * beta);
	const T tiny = std::numeric_limits<T>::epsilon();
	const T gamma = root > tiny ? root : (root == root ? tiny : root);  // max(root, eps_machine); a NaN stays one
	const T cs = gbar / gamma;
	const T sn = beta / gamma;
	const T phi = cs * in.phibar;
	const T phibar = sn * in.phibar;
	const bool bad = ry < T(0) || !isfinite(beta) || !isfinite(phibar);
	const T res = phibar * phibar;
	const bool stop = bad || beta == T(0) || !(res > eps * eps) || step + 1 >= maxIterations;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		MinresRot<T> o;
		o.beta = beta;
		o.oldb = in.beta;
		o.dbar = dbar;
		o.epsln = epsln;
		o.phibar = phibar;
		o.cs = cs;
		o.sn = sn;
		o.stop = stop ? 1 : 0;
		o.forStep = step + 1;
		sc->rot[par ^ 1] = o;
		if (bad) {
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->res = res;
			sc->iters = step + 1;
		}
		if (stop) sc->done = 1;
	}
	if (bad) return;
	const T* const src[5] = {v, y, w1, w2, x};
	T* const out[3] = {w1, x, v};
	streamMap<T, NT, 5, 3>(n, src, out, [&](const T(&e)[5], T(&o)[3]) {
		const T w = smmFma(-delta, e[3], smmFma(-oldeps, e[2], e[0])) / gamma;
		o[0] = w;
		o[1] = smmFma(phi, w, e[4]);
		o[2] = e[1] / beta;
	});
}

// The entry check of the preconditioner, MINRES's own: M must be symmetric positive definite, which a handle created for an indefinite `a`
// cannot be -- so it is NOT asked to be created for `a` (it is built on a positive definite relative of `a`), only to fit it.
template <typename T>
static int minresPrecondCheck(const smm_hip_precond* M, const smm_hip_csr* a) {
	if (!M) return SMM_HIP_OK;
	if (M->dtype != dtypeOf<T>()) {
		setError("minres: the preconditioner holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (!M->a || M->a->rows != a->rows) {
		setError("minres: the preconditioner was created for a matrix of %d rows, this one has %d", M->a ? M->a->rows : 0, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	if (!precondKindTaken(M->kind, SOLVER_CG)) {
		std::string names;
		for (int kind = SMM_PRECOND_NONE + 1; kind < N_PRECOND_KINDS; ++kind) {
			if (precondKindTaken(kind, SOLVER_CG)) names += std::string(names.empty() ? "" : " / ") + PRECOND_KINDS[kind].name;
		}
		const char* name = M->kind >= 0 && M->kind < N_PRECOND_KINDS ? PRECOND_KINDS[M->kind].name : "unknown";
		setError("minres: the preconditioner must be symmetric positive definite (%s, created for a positive definite matrix of the same size), not %s", names.c_str(),
		         name);
		return SMM_HIP_ERR_INVALID;
	}
	if (isJsweepKind(M->kind) && !jsweepSymmetric(M)) {
		setError("minres: a %s preconditioner is symmetric only with as many lower steps as upper ones (smm_hip_precond_jsweep_set_sweeps)", PRECOND_KINDS[M->kind].name);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int minresCheck(const smm_hip_csr* a, const T* b, const T* x, const smm_hip_precond* M) {
	SMM_TRY(solverCheck<T>("minres", a, b, x));
	return minresPrecondCheck<T>(M, a);
}

template <typename T>
static int minresDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, hipStream_t s, int* status, int* iterations,
                     T* resnorm2) {
	SMM_TRY(minresCheck<T>(a, b, x, M));
	const int n = a->rows;
	if (n == 0) {
		if (status) *status = SMM_SOLVER_SUCCESS;
		if (iterations) *iterations = 0;
		if (resnorm2) *resnorm2 = T(0);
		return SMM_HIP_OK;
	}
	maxIterations = maxIterations == -1 ? n : std::max(0, std::min(maxIterations, n));
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	DevBuf<T> ra, rb, yv, v, Av, wa, wb, partsA, partsB;
	DevBuf<MinresScal<T>> sc;
	SMM_TRY(ra.alloc(n));
	SMM_TRY(rb.alloc(n));
	if (M) SMM_TRY(yv.alloc(n));
	SMM_TRY(v.alloc(n));
	SMM_TRY(Av.alloc(n));
	SMM_TRY(wa.alloc(n));
	SMM_TRY(wb.alloc(n));
	SMM_TRY(partsA.alloc(2 * NPART));  // [v.Av]
	SMM_TRY(partsB.alloc(NPART));      // [r2.y]
	SMM_TRY(sc.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(partsB.p, 0, sizeof(T) * NPART, s));  // minresLanczos writes one slot per workgroup: the others stay 0
	SMM_HIP_TRY(hipMemsetAsync(sc.p, 0xFF, sizeof(MinresScal<T>), s));  // (no set is any step's until it is published)
	const int g = solverGrid(n);
	const int* doneFlag = &sc.p->done;

	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, maxIterations));
	bool fromZero = false;  // x = 0 and finite values: r1 = b without an SpMV (zeroStart, smm_solver_host.h)
	SMM_TRY(zeroStart<T>(a, x, watch, s, &fromZero));
	T *r1 = ra, *r2 = rb, *w = wa, *w2 = wb;
	if (fromZero) SMM_TRY(launchCopy2<T>(n, b, r1, nullptr, s));
	else SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r1, 0, nullptr, nullptr, nullptr, s));
	if (M) SMM_TRY(precondApplyDev<T>(M, r1, yv, nullptr, s));
	SMM_TRY(launchDotPartials<T>(n, r1, M ? yv.p : r1, partsB, nullptr, s));
	minresStart<T><<<g, TPB, 0, s>>>(n, sc, partsB, maxIterations, eps, r1, M ? yv.p : r1, r2, v, w, w2);

	for (int i = 0; i < maxIterations && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, v, Av, 1, v, partsA, doneFlag, s));
		const bool nt = updateNT(n, sizeof(T), 4);
		if (M && nt) minresLanczos<T, true, false><<<g, TPB, 0, s>>>(n, sc, i & 1, i, partsA, partsB, Av, r2, r1);
		else if (M) minresLanczos<T, false, false><<<g, TPB, 0, s>>>(n, sc, i & 1, i, partsA, partsB, Av, r2, r1);
		else if (nt) minresLanczos<T, true, true><<<g, TPB, 0, s>>>(n, sc, i & 1, i, partsA, partsB, Av, r2, r1);
		else minresLanczos<T, false, true><<<g, TPB, 0, s>>>(n, sc, i & 1, i, partsA, partsB, Av, r2, r1);
		std::swap(r1, r2);  // r2: the new vector ; r1: the one before
		if (M) {
			SMM_TRY(precondApplyDev<T>(M, r2, yv, doneFlag, s));
			SMM_TRY(launchDotPartials<T>(n, r2, yv, partsB, doneFlag, s));
		}
		// w1 is `w2` (two steps back): the new w is written over it
		SMM_LAUNCH_UPDATE(minresRotate, updateNT(n, sizeof(T), 8), g, s, n, sc, i & 1, i, maxIterations, eps, partsB, M ? yv.p : r2, v, w2, w, x);
		std::swap(w, w2);
	}
	MinresScal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	int st = SMM_SOLVER_MAX_ITERATIONS_REACHED;
	if (h.status == SMM_SOLVER_DIVERGED) st = SMM_SOLVER_DIVERGED;
	else if (h.res <= eps * eps) st = SMM_SOLVER_SUCCESS;
	if (status) *status = st;
	if (iterations) *iterations = h.iters;
	if (resnorm2) *resnorm2 = h.res;
	return M ? precondTakeError(M, s) : SMM_HIP_OK;
}

// host vectors (x in / out)
template <typename T>
static int minresHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(minresCheck<T>(a, b, x, M));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return minresDev<T>(a, db, dx, maxIterations, eps, M, s, status, iterations, resnorm2);
	});
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_minres_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, const smm_hip_precond* M, int* solver_status, int* iterations,
                       float* resnorm2) {
	return minresHost<float>(a, b, x, maxIterations, eps, M, solver_status, iterations, resnorm2);
}
int smm_hip_minres_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, const smm_hip_precond* M, int* solver_status, int* iterations,
                       double* resnorm2) {
	return minresHost<double>(a, b, x, maxIterations, eps, M, solver_status, iterations, resnorm2);
}
int smm_hip_minres_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M, smm_hip_stream stream,
                           int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return minresDev<float>(a, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_minres_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M, smm_hip_stream stream,
                           int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return minresDev<double>(a, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm2);
}

}  // extern "C"
