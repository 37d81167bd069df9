// smm_solvers.hip -- device-resident Krylov loops: ConjugateGradient (ref:2316-2398, IC0 overload ref:2414-2505),
// BiCGStab (ref:2191-2303), BiCGSymmetric (ref:2021-2102).
//
// Design (MI355X-first, not a translation of the CPU loop):
//   * every vector and every scalar (alpha, beta, omega, ||r||^2, the convergence flag, the iteration count)
//     lives in HBM; the host only enqueues kernels.  No per-iteration host round trip: the host peeks at the
//     `done` flag through a pinned mailbox every few iterations, and every kernel of the loop starts by testing
//     the flag, so iterations enqueued past convergence are no-ops and x / iterations / status are exactly
//     those of the iteration at which the reference would have returned.
//   * the dot products that follow an SpMV are fused into the SpMV epilogue (p.Ap; ap.r0; as.as + as.s), the
//     ||r||^2 and r.r0 sums are fused into the x/r update, exactly the fusions the reference's serial loops
//     do (ref:2371-2375, 2263-2267) plus the SpMV ones.  Partial sums are combined in a fixed order.
//   * update loops keep the reference's expression shapes (_smm_fma nesting), so given the same scalars they
//     are bit-identical to the CPU loops.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_krylov_steps.h"
#include "smm_solver_host.h"

namespace smm {

constexpr int TPB = 256;

// ---- scalar stages (one workgroup each) ----------------------------------------------------------------
// CG start: rr = r.r ; if eps^2 > rr -> done, SUCCESS, x untouched (ref:2341-2344)
template <typename T>
__global__ __launch_bounds__(TPB) void cgInitScal(const T* __restrict__ partials, Scal<T>* sc, T eps, int pcg, const T* __restrict__ partials2) {
	__shared__ T red[4];
	const T rr = sumParts(partials, red);
	T rz = T(0);
	if (pcg) rz = sumParts(partials2, red);
	if (threadIdx.x == 0) {
		sc->rr = pcg ? rz : rr;
		sc->rrPing[0] = sc->rr;
		sc->res = rr;
		sc->iters = 0;
		sc->status = SMM_SOLVER_MAX_ITERATIONS_REACHED;
		sc->done = 0;
		sc->pad = 0;
		sc->flushIter = -1;
		if (eps * eps > rr) {
			sc->done = 1;
			sc->status = SMM_SOLVER_SUCCESS;
		}
	}
}

// alpha = rr / (Ap.p)  (ref:2354-2358)
template <typename T>
__global__ __launch_bounds__(TPB) void cgAlphaScal(const T* __restrict__ partials, Scal<T>* sc) {
	__shared__ T red[4];
	if (sc->done) return;
	const T pAp = sumParts(partials, red);
	if (threadIdx.x == 0) {
		sc->denom = pAp;
		sc->alpha = sc->rr / pAp;
	}
}

// after the x/r update: convergence test, beta (ref:2377-2382); for PCG partials hold r.r and partials2 r.z (ref:2483-2488)
template <typename T>
__global__ __launch_bounds__(TPB) void cgBetaScal(const T* __restrict__ partials, const T* __restrict__ partials2, Scal<T>* sc, T eps, int pcg) {
	__shared__ T red[4];
	if (sc->done) return;
	const T rrNew = sumParts(partials, red);
	T rzNew = T(0);
	if (pcg) rzNew = sumParts(partials2, red);
	if (threadIdx.x == 0) {
		sc->iters += 1;
		sc->res = rrNew;
		if (eps * eps > rrNew) {
			sc->done = 1;
			sc->status = SMM_SOLVER_SUCCESS;
		} else if (pcg) {
			sc->beta = rzNew / sc->rr;
			sc->rr = rzNew;
		} else {
			sc->beta = rrNew / sc->rr;
			sc->rr = rrNew;
		}
	}
}

// ---- vector stages -------------------------------------------------------------------------------------
// x = alpha p + xcur ; r = -alpha Ap + r ; partial ||r||^2   (ref:2371-2375)
template <typename T>
__global__ __launch_bounds__(TPB) void cgUpdateXR(int n, const Scal<T>* __restrict__ sc, const T* p, const T* Ap, const T* xcur, T* x, T* r,
                                                  T* __restrict__ partials, int wantNorm) {
	__shared__ T red[4];
	if (sc->done) return;
	const T alpha = sc->alpha;
	T acc = T(0);
	const T* const in[4] = {p, xcur, Ap, r};
	T* const out[2] = {x, r};
	streamMap<T, false, 4, 2>(n, in, out, [&](const T(&v)[4], T(&o)[2]) {
		o[0] = smmFma(alpha, v[0], v[1]);
		const T ri = smmFma(-alpha, v[2], v[3]);
		o[1] = ri;
		acc += ri * ri;
	});
	if (wantNorm) {
		const T s = blockSum256(acc, red);
		if (threadIdx.x == 0) partials[blockIdx.x] = s;
	}
}

// p = beta p + z   (ref:2391-2393 with z = r; ref:2497-2499 with z = M^-1 r)
template <typename T>
__global__ __launch_bounds__(TPB) void cgUpdateP(int n, const Scal<T>* __restrict__ sc, T* p, const T* z) {
	if (sc->done) return;
	const T beta = sc->beta;
	const T* const in[2] = {p, z};
	T* const out[1] = {p};
	streamMap<T, false, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(beta, v[0], v[1]); });
}

// ---- fused forms: the scalar stage is folded into the vector kernel that consumes it --------------------------------------
// Every workgroup re-adds the NPART partial sums itself (same order => same bits in every workgroup), so alpha / beta / omega
// need no kernel of their own: two launches per CG iteration and three per BiCGStab iteration disappear.  State that must
// survive a kernel (rr, alpha, omega, done, iterations) is written by workgroup 0 only; rr is double-buffered by iteration
// parity because workgroup 0 writes the next value while the others still read the current one.
// The two update kernels of a CG iteration (ref:2354-2394), split so that every vector is passed as few times as the data flow
// allows: the first needs only Ap and r (r = -alpha Ap + r and ||r||^2 -- the next reduction point), the second reads p once for
// BOTH of its uses (x = alpha p + xcur, the reference's :2362-2366, and p = beta p + r): 8 vector passes per iteration instead of
// the 9 of "x and r, then p" (r03; config 4's iteration is two thirds vector updates since its SpMV reads no values[]).  Same
// expressions on the same operands: same bits.
// alpha = rr / (Ap.p) ; r = -alpha Ap + r ; partial ||r||^2.  sc->pad = the done flag as this iteration found it: the second kernel
// decides by it (its own workgroup 0 raises `done` while other workgroups of the same launch may not have started yet).
// (the vector loops of the fused kernels go through streamMap, smm_device.h: 16-byte accesses, 4 packs per lane in flight)
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgFusedR(int n, Scal<T>* sc, int par, const T* __restrict__ partsA, const T* Ap, T* r,
                                                T* __restrict__ partsC, int alphaSlot) {
	__shared__ T red[5];
	if (cgSnapshotDone(sc)) return;
	const T rr = sc->rrPing[par];
	cgStepR<T, NT>(n, sc, rr, sumPartsAll(partsA, red), red, Ap, r, partsC, alphaSlot);
}

// x = alpha p + xcur ; convergence test ; beta ; p = beta p + r   (ref:2362-2394: x is updated before the test, p only when the loop goes on)
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgFusedXP(int n, Scal<T>* sc, int par, const T* __restrict__ partsC, T eps, T* p, const T* r, const T* xcur,
                                                 T* x) {
	__shared__ T red[5];
	if (sc->pad) return;
	const T rrNew = sumPartsAll(partsC, red);
	const T rrOld = sc->rrPing[par];
	const T alpha = sc->alpha;
	const bool converged = eps * eps > rrNew;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		sc->iters += 1;
		sc->res = rrNew;
		if (converged) {
			sc->done = 1;
			sc->status = SMM_SOLVER_SUCCESS;
		} else {
			sc->rrPing[par ^ 1] = rrNew;
		}
	}
	if (converged) {
		const T* const in[2] = {p, xcur};
		T* const out[1] = {x};
		streamMap<T, NT, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(alpha, v[0], v[1]); });
		return;
	}
	const T beta = rrNew / rrOld;
	const T* const in[3] = {p, xcur, r};
	T* const out[2] = {x, p};
	streamMap<T, NT, 3, 2>(n, in, out, [&](const T(&v)[3], T(&o)[2]) {
		o[0] = smmFma(alpha, v[0], v[1]);
		o[1] = smmFma(beta, v[0], v[2]);
	});
}

// ---- the x update deferred (r05) ------------------------------------------------------------------------------------------------
// For vectors that do not fit the caches an iteration of CG is 10 vector passes, 5 of them in cgFusedXP (read p, x, r; write x, p).  With
// the last LAZY_M directions kept in a ring (LazyRing, cgLazyStep: smm_krylov_steps.h) x is brought up to date every LAZY_M-th iteration in
// the launch that forms the next p anyway: (3 (M - 1) + M + 4) / M = 4 + 1 / M passes per iteration instead of 5 (M = 8: 4.125; with p formed
// inside the SpMV the flush is a launch of its own, (M + 2) / M = 1.25), at the price of M more vectors of device memory.
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgLazyXP(int n, Scal<T>* sc, int par, const T* __restrict__ partsC, T eps, LazyRing<T> ring, int cur, int pending, int flush,
                                                int alphaSlot, const T* r, const T* xcur, T* x) {
	__shared__ T red[5];
	if (sc->pad) return;
	cgLazyStep<T, NT>(WholeRows{n}, true, sc, par, sumPartsAll(partsC, red), eps, ring, cur, pending, flush, alphaSlot, r, xcur, x);
}

template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void cgLazyFlushOnly(int n, const Scal<T>* __restrict__ sc, LazyRing<T> ring, int cur, int pending, int scheduled, int iter,
                                                       int alphaSlot, const T* xcur, T* x) {
	cgFlushOnlyStep<T, NT>(WholeRows{n}, sc, ring, cur, pending, scheduled, iter, alphaSlot, xcur, x);
}

// the three update kernels of a BiCGStab iteration (bicgStepS / XR / P, smm_krylov_steps.h); partsA = [ap.r0]
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void bicgFusedS(int n, Scal<T>* sc, int par, const T* __restrict__ partsA, const T* ap, const T* r, T* sv) {
	__shared__ T red[5];
	if (sc->done) return;
	const T rr0 = sc->rrPing[par];
	bicgStepS<T, NT>(WholeRows{n}, true, sc, rr0, sumPartsAll(partsA, red), ap, r, sv);
}

// partsB = [as.as | as.s], partsC = [r.r | r.r0]
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void bicgFusedXR(int n, Scal<T>* sc, const T* __restrict__ partsB, const T* p, const T* sv, const T* as,
                                                   const T* r0, T* x, T* r, T* __restrict__ partsC) {
	__shared__ T red[5];
	if (sc->done) return;
	const T asas = sumPartsAll(partsB, red);
	const T ass = sumPartsAll(partsB + NPART, red);
	bicgStepXR<T, NT, true>(n, sc, asas, ass, red, p, sv, as, r0, x, r, partsC);
}

template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void bicgFusedP(int n, Scal<T>* sc, int par, const T* __restrict__ partsC, T eps, const T* ap, const T* r, T* p) {
	__shared__ T red[5];
	if (sc->done) return;
	const T rr = sumPartsAll(partsC, red);
	const T newRR0 = sumPartsAll(partsC + NPART, red);
	bicgStepP<T, NT>(WholeRows{n}, true, sc, par, rr, newRR0, eps, ap, r, p);
}

// two dot products that share an operand: partials = a.a, partials2 = a.b
template <typename T>
__global__ __launch_bounds__(TPB) void dot2Partials(int n, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ partials,
                                                    T* __restrict__ partials2, const int* __restrict__ doneFlag) {
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	T acc0 = T(0), acc1 = T(0);
	const T* const in[2] = {a, b};
	streamMap<T, false, 2, 0>(n, in, nullptr, [&](const T(&v)[2], T(&)[1]) {
		acc0 += v[0] * v[0];
		acc1 += v[0] * v[1];
	});
	const T s0 = blockSum256(acc0, red);
	const T s1 = blockSum256(acc1, red);
	if (threadIdx.x == 0) {
		partials[blockIdx.x] = s0;
		partials2[blockIdx.x] = s1;
	}
}

// ---- BiCGSymmetric stages (ref:2021-2102) ----------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(TPB) void bsymInitScal(const T* __restrict__ partials, Scal<T>* sc) {
	__shared__ T red[4];
	const T rr = sumParts(partials, red);  // ref:2043
	if (threadIdx.x == 0) {
		sc->rr = rr;
		sc->iters = 0;
		sc->done = 0;
		sc->status = SMM_SOLVER_SUCCESS;
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void bsymAlphaScal(const T* __restrict__ partials, Scal<T>* sc, T eps) {
	__shared__ T red[4];
	if (sc->done) return;
	const T denom = sumParts(partials, red);
	if (threadIdx.x == 0) {
		if (eps > (denom < T(0) ? -denom : denom) && sc->rr > T(1)) {  // ref:2056-2058
			sc->done = 1;
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->alpha = sc->rr / denom;
		}
	}
}

// x += alpha p ; r -= alpha ap  (ref:2068-2071: plain += / -= forms, not _smm_fma)
template <typename T>
__global__ __launch_bounds__(TPB) void bsymUpdateXR(int n, const Scal<T>* __restrict__ sc, const T* p, const T* ap, T* x, T* r,
                                                    T* __restrict__ partials) {
	__shared__ T red[4];
	if (sc->done) return;
	const T alpha = sc->alpha;
	T acc = T(0);
	const T* const in[4] = {p, x, ap, r};
	T* const out[2] = {x, r};
	streamMap<T, false, 4, 2>(n, in, out, [&](const T(&v)[4], T(&o)[2]) {
		const T pa = alpha * v[0];
		o[0] = v[1] + pa;
		const T qa = alpha * v[2];
		const T ri = v[3] - qa;
		o[1] = ri;
		acc += ri * ri;
	});
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <typename T>
__global__ __launch_bounds__(TPB) void bsymBetaScal(const T* __restrict__ partials, Scal<T>* sc, T eps) {
	__shared__ T red[4];
	if (sc->done) return;
	const T newRR = sumParts(partials, red);  // ref:2075
	if (threadIdx.x == 0) {
		if (newRR > T(1) && sc->rr < eps) {  // ref:2079-2081
			sc->done = 1;
			sc->status = SMM_SOLVER_DIVERGED;
		} else {
			sc->beta = newRR / sc->rr;
			sc->rr = newRR;
			sc->iters += 1;
			if (!(newRR > eps * eps)) sc->done = 1;  // ref:2096
		}
	}
}

// p = r + beta p  (ref:2090-2092)
template <typename T>
__global__ __launch_bounds__(TPB) void bsymUpdateP(int n, const Scal<T>* __restrict__ sc, const T* r, T* p) {
	if (sc->done) return;
	const T beta = sc->beta;
	const T* const in[2] = {p, r};
	T* const out[1] = {p};
	streamMap<T, false, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) {
		const T bp = beta * v[0];
		o[0] = v[1] + bp;
	});
}

// ---------------------------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------------------------
// Non-temporal loads / stores for an update kernel whose vectors cannot stay in the 256 MB Infinity Cache until the next kernel
// reads them anyway; cache-resident problems keep the default policy.  SMM_HIP_UPDATE_NT=0/1 overrides (measurements).
bool updateNT(long long n, size_t elemBytes, int vectors) {
	const int forced = env::intOr(env::UPDATE_NT, -1);
	if (forced >= 0) return forced != 0;
	return static_cast<double>(n) * static_cast<double>(elemBytes) * vectors > 192.0 * 1024 * 1024;
}

// from how many bytes per vector CG defers its x update (cgLazyXP): where five vectors no longer fit the 256 MB Infinity Cache the passes
// are what an iteration costs; below, the extra ring of directions buys nothing.  smm_hip_set_cg_lazy_x_min_bytes (tests) / SMM_HIP_CG_LAZY_X=0
static std::atomic<long long> g_lazyMinBytes{-1};
long long cgLazyMinBytes() {
	const long long forced = g_lazyMinBytes.load(std::memory_order_relaxed);
	if (forced >= 0) return forced;
	return env::flagOr(env::CG_LAZY_X, true) ? (64LL << 20) : (1LL << 62);
}

template <typename T>
int cgDev(const smm_hip_csr* a, const T* b, const T* x0, T* x, int maxIterations, T eps, const smm_hip_precond* M, hipStream_t s, int* status,
          int* iterations, T* resnorm2) {
	SMM_TRY(solverCheck<T>("cg", a, b, x0, x));
	const int pcg = M != nullptr;
	// the reference only has the IC0 overload (ref:2414-2422); the Chebyshev polynomial and the multigrid V-cycle are symmetric positive definite for such a matrix too
	// (MULTICOLOR_IC0 and MULTICOLOR_SGS are IC0 / SGS of P A Pᵀ carried back by P: symmetric positive definite when A is)
	SMM_TRY(precondAdmissible("cg", M, a, SOLVER_CG));
	const int n = a->rows;
	if (!pcg) {
		// a matrix that fits the chip's register file is solved in one launch (smm_resident.hip)
		bool handled = false;
		SMM_TRY(ensureCsrReady(a, s, true));
		SMM_TRY(cgResidentTry<T>(a, b, x0, x, maxIterations, eps, s, status, iterations, resnorm2, &handled));
		if (handled) return SMM_HIP_OK;
	}
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));  // many SpMVs ahead: a mid-size banded / stencil matrix takes the index-free family
	DevBuf<T> r, p, Ap, z, parts, parts2;
	DevBuf<T> ringBuf[LAZY_M];
	DevBuf<Scal<T>> sc;
	// the deferred x update (cgLazyXP): unpreconditioned CG on vectors too large for the caches; LAZY_M more vectors for the ring of directions
	bool lazy = !pcg && static_cast<long long>(n) * static_cast<long long>(sizeof(T)) >= cgLazyMinBytes();
	LazyRing<T> ring{};
	SMM_TRY(r.alloc(n));
	SMM_TRY(p.alloc(n));
	if (lazy) {
		ring.p[0] = p;
		for (int k = 0; k < LAZY_M && lazy; ++k) {
			if (ringBuf[k].alloc(n) != SMM_HIP_OK) lazy = false;  // no room for the ring: the eager loop needs none
			ring.p[k + 1] = ringBuf[k];
		}
		if (!lazy) {
			for (int k = 0; k < LAZY_M; ++k) ringBuf[k].release();
			(void)hipGetLastError();
		}
	}
	const bool fuseP = lazy && constMarchFusable(a, sizeof(T));  // (decided once per solve: the two loop forms do their bookkeeping in different launches)
	SMM_TRY(Ap.alloc(n));
	if (pcg) SMM_TRY(z.alloc(n));
	SMM_TRY(parts.alloc(2 * NPART));
	SMM_TRY(parts2.alloc(NPART));
	SMM_TRY(sc.alloc(1));
	const int g = solverGrid(n);

	const int* doneFlag = &sc.p->done;
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 0, 0, maxIterations == -1 ? n : maxIterations));
	bool fromZero = false;  // x0 = 0 and finite values: r = b without an SpMV (zeroStart, smm_solver_host.h)
	SMM_TRY(zeroStart<T>(a, x0, watch, s, &fromZero));
	if (!fromZero) SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x0, r, 0, nullptr, nullptr, nullptr, s));  // r = b - A x0, ref:2337
	if (pcg) {
		if (fromZero) SMM_TRY(launchCopy2<T>(n, b, r, nullptr, s));
		SMM_TRY(precondApplyDev<T>(M, r, z, nullptr, s));           // z = M^-1 r, ref:2441
		SMM_TRY(launchCopy2<T>(n, z, p, nullptr, s));               // p = z, ref:2447
		SMM_TRY(launchDotPartials<T>(n, r, r, parts, nullptr, s));  // ||r||^2
		SMM_TRY(launchDotPartials<T>(n, r, z, parts2, nullptr, s)); // r.z
	} else {
		if (fromZero) SMM_TRY(launchCopy2<T>(n, b, r, p, s));       // r = p = b in one pass over b
		else SMM_TRY(launchCopy2<T>(n, r, p, nullptr, s));          // p = r, ref:2340
		SMM_TRY(launchDotPartials<T>(n, r, r, parts, nullptr, s));  // ref:2341
	}
	cgInitScal<T><<<1, TPB, 0, s>>>(parts, sc, eps, pcg, parts2);
	if (maxIterations == -1) maxIterations = n;  // ref:2345-2347 (no clamp otherwise)

	for (int i = 0; i < maxIterations && !watch.leave(i); ++i) {
		if (lazy && fuseP) {
			// the direction is formed INSIDE the SpMV (2.5-D constant-diagonal kernel): SpMV' (bookkeeping of iteration i - 1, p_i, A p_i, p.Ap),
			// the flush of x behind it (scheduled every LAZY_M-th iteration; or because SpMV' found iteration i - 1 converged), the r update
			const int cur = i % (LAZY_M + 1);
			if (i == 0) {
				SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, ring.p[0], Ap, 1, ring.p[0], parts, doneFlag, s, SPMV_HALF_TILES));
			} else {
				const int prev = (i - 1) % (LAZY_M + 1);
				const CgFuseBook<T> bk{&sc.p->pad, sc.p->rrPing, &sc.p->res, &sc.p->iters, &sc.p->done, &sc.p->status, &sc.p->flushIter};
				const CgFuseArgs<T> f{r, ring.p[cur], bk, parts2, eps, (i - 1) & 1, i};
				if (!launchConstMarchFusedP<T>(a, ring.p[prev], Ap, parts, doneFlag, f, s)) {
					setError("cg: the fused SpMV could not be launched");
					return SMM_HIP_ERR_HIP;
				}
				SMM_LAUNCH_UPDATE(cgLazyFlushOnly, updateNT(n, sizeof(T), 5), g, s, n, sc, ring, prev, (i - 1) % LAZY_M + 1, i % LAZY_M == 0 ? 1 : 0, i, (i - 1) % LAZY_M,
				                  i <= LAZY_M ? x0 : x, x);
			}
			SMM_LAUNCH_UPDATE(cgFusedR, updateNT(n, sizeof(T), 3), NPART, s, n, sc, i & 1, parts, Ap, r, parts2, i % LAZY_M);
			if (i == maxIterations - 1) {  // the last planned iteration has no SpMV' behind it: its bookkeeping and the rest of x
				SMM_LAUNCH_UPDATE(cgLazyXP, updateNT(n, sizeof(T), 5), g, s, n, sc, i & 1, parts2, eps, ring, cur, i % LAZY_M + 1, 1, i % LAZY_M, r, i < LAZY_M ? x0 : x, x);
			}
			continue;
		}
		if (lazy) {
			// the direction of iteration i lives in ring slot i % (LAZY_M + 1); x is brought up to date every LAZY_M-th iteration, in the last
			// planned one, and by whichever launch finds the iteration converged
			const int cur = i % (LAZY_M + 1);
			const T* pc = ring.p[cur];
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, pc, Ap, 1, pc, parts, doneFlag, s, SPMV_HALF_TILES));
			SMM_LAUNCH_UPDATE(cgFusedR, updateNT(n, sizeof(T), 3), NPART, s, n, sc, i & 1, parts, Ap, r, parts2, i % LAZY_M);
			const int pending = i % LAZY_M + 1;
			const int flush = (pending == LAZY_M || i == maxIterations - 1) ? 1 : 0;
			const T* xc = i < LAZY_M ? x0 : x;  // (until the first scheduled flush x has not been written: ref:2351, 2395)
			SMM_LAUNCH_UPDATE(cgLazyXP, updateNT(n, sizeof(T), 5), g, s, n, sc, i & 1, parts2, eps, ring, cur, pending, flush, i % LAZY_M, r, xc, x);
			continue;
		}
		// Ap = A p with the p.Ap partial sums fused into the epilogue (ref:2353-2354)
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, Ap, 1, p, parts, doneFlag, s, pcg ? 0 : SPMV_HALF_TILES));
		const T* xcur = i == 0 ? x0 : x;  // ref:2351, 2395
		if (pcg) {
			cgAlphaScal<T><<<1, TPB, 0, s>>>(parts, sc);
			// NPART workgroups: every partial slot is (re)written each iteration, idle workgroups write 0
			cgUpdateXR<T><<<NPART, TPB, 0, s>>>(n, sc, p, Ap, xcur, x, r, parts, 0);
			SMM_TRY(precondApplyDev<T>(M, r, z, doneFlag, s));         // ref:2482
			dot2Partials<T><<<NPART, TPB, 0, s>>>(n, r, z, parts, parts2, doneFlag);  // r.r and r.z, ref:2483-2484
			cgBetaScal<T><<<1, TPB, 0, s>>>(parts, parts2, sc, eps, 1);
			cgUpdateP<T><<<g, TPB, 0, s>>>(n, sc, p, z);
		} else {
			// alpha and beta are formed inside the two update kernels (no scalar launches)
			SMM_LAUNCH_UPDATE(cgFusedR, updateNT(n, sizeof(T), 3), NPART, s, n, sc, i & 1, parts, Ap, r, parts2, 0);
			SMM_LAUNCH_UPDATE(cgFusedXP, updateNT(n, sizeof(T), 5), g, s, n, sc, i & 1, parts2, eps, p, r, xcur, x);
		}
	}
	Scal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	if (status) *status = h.status;
	if (iterations) *iterations = h.iters;
	if (resnorm2) *resnorm2 = h.res;
	return pcg ? precondTakeError(M, s) : SMM_HIP_OK;
}

// M^-1 of the preconditioned loop: the library's device-resident preconditioners, or a HOST functor of the caller (the reference's
// BiCGStab template takes any type with `int apply(const T* rhs, T* x) const`, ref:2191-2199, 2218, 2235, 2251)
template <typename T>
struct DevApplier {
	const smm_hip_precond* M;
	static constexpr bool hostSide = false;
	int operator()(const T* in, T* out, const int* doneFlag, hipStream_t s) const { return precondApplyDev<T>(M, in, out, doneFlag, s); }
};

// The vector goes to the host, the caller's functor runs there, the result comes back: two PCIe copies and two stream drains per
// apply.  Everything else of the iteration stays on the device.  A non-zero return of the functor ends the solve with
// SMM_HIP_ERR_PRECOND (the reference ignores apply()'s return value inside the loop; a failing apply leaves x undefined there).
template <typename T>
struct HostApplier {
	int (*fn)(void* user, const T* rhs, T* x);
	void* user;
	int n;
	T* hostIn;   // pinned
	T* hostOut;  // pinned
	static constexpr bool hostSide = true;
	int operator()(const T* in, T* out, const int* /*doneFlag*/, hipStream_t s) const {
		if (n == 0) return SMM_HIP_OK;
		SMM_HIP_TRY(hipMemcpyAsync(hostIn, in, sizeof(T) * n, hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (fn(user, hostIn, hostOut) != 0) {
			setError("bicgstab: the caller's preconditioner apply() returned non-zero");
			return SMM_HIP_ERR_PRECOND;
		}
		SMM_HIP_TRY(hipMemcpyAsync(out, hostOut, sizeof(T) * n, hipMemcpyHostToDevice, s));
		return SMM_HIP_OK;
	}
};

template <typename T, typename Applier>
static int bicgstabLoop(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, const bool precondition, const Applier& apply, hipStream_t s,
                        int* status, int* iterations, T* resnorm, const T* jacobiDiag = nullptr, const smm_hip_precond* blockM = nullptr) {
	// jacobiDiag: M is the library's Jacobi preconditioner and its apply (x = rhs / diag, smm_precond.hip) is folded into the rows of the
	// SpMV that precedes it -- the same division on the same operands, so the same bits as SpMV + apply -- which lets the preconditioned
	// loop use the fused dots of the unpreconditioned one: no apply launches, no dot launches, no extra vector passes.
	// blockM: M is a block preconditioner (smm_precond_block.hip): its one-launch apply forms the dot products of its result in its
	// own epilogue, so the loop needs no dot launches either.
	const int n = a->rows;
	maxIterations = std::min(maxIterations, n);  // ref:2200
	if (maxIterations == -1) maxIterations = n;  // ref:2201-2203
	DevBuf<T> r, r0, p, ap, sv, as, scratch, parts, parts2;
	DevBuf<Scal<T>> sc;
	{
		SetupTrace trace("bicgstab loop:   allocate the temporaries");
		SMM_TRY(r.alloc(n));
		SMM_TRY(r0.alloc(n));
		SMM_TRY(p.alloc(n));
		SMM_TRY(ap.alloc(n));
		SMM_TRY(sv.alloc(n));
		SMM_TRY(as.alloc(n));
		if (precondition) SMM_TRY(scratch.alloc(n));
		SMM_TRY(parts.alloc(2 * NPART));   // [ap.r0] then [as.as | as.s]
		SMM_TRY(parts2.alloc(2 * NPART));  // [r.r | r.r0]
		SMM_TRY(sc.alloc(1));
	}
	SetupTrace traceLoop("bicgstab loop:   enqueue + run + read back");
	const int g = NPART;  // update kernels that write partials use the full partial grid
	// block preconditioner of THIS matrix: A p and A s are formed inside the apply's launch, row by row in the order of the stored entries
	const bool fuseBlk = blockM && blockM->a == a && blockFuseSpmv(blockM, false);

	const int* doneFlag = &sc.p->done;
	const int planned = std::max(1, maxIterations);  // do { } while: the body always runs once (ref:2232, 2277)
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, planned));
	bool fromZero = false;  // x = 0 and finite values: b - A x is b, no SpMV is launched for it (zeroStart, smm_solver_host.h)
	SMM_TRY(zeroStart<T>(a, x, watch, s, &fromZero));
	if (precondition) {
		if (fromZero) SMM_TRY(launchCopy2<T>(n, b, scratch, nullptr, s));
		else SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, scratch, 0, nullptr, nullptr, nullptr, s));  // ref:2215
		SMM_TRY(apply(scratch, r, nullptr, s));                                                       // ref:2217-2224
	} else if (!fromZero) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, nullptr, s));
	}
	if (fromZero && !precondition) SMM_TRY(launchCopyMany<T>(n, b, r, r0, p, nullptr, s));  // r = r0 = p = b in one pass over b
	else SMM_TRY(launchCopy2<T>(n, r, r0, p, s));                                           // ref:2225-2226
	SMM_TRY(launchDotPartials<T>(n, r, r0, parts, nullptr, s));  // ref:2231
	rr0InitScal<T><<<1, TPB, 0, s>>>(parts, sc);  // (smm_solver_scal.h)

	for (int i = 0; i < planned; ++i) {
		if (Applier::hostSide && i > 0) {
			// a host functor drains the stream at every apply anyway: test the flag directly so that it is never called for an
			// iteration the loop has already left
			int done = 0;
			SMM_HIP_TRY(hipMemcpyAsync(&done, doneFlag, sizeof(int), hipMemcpyDeviceToHost, s));
			SMM_HIP_TRY(hipStreamSynchronize(s));
			if (done) break;
		} else if (watch.leave(i)) {
			break;
		}
		if (jacobiDiag) {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, jacobiDiag, p, ap, 1, r0, parts, doneFlag, s, SPMV_DIV_LHS));  // ref:2234-2235 + 2243 fused
		} else if (blockM) {
			if (fuseBlk) {
				SMM_TRY(blockApplySpmvDev<T>(blockM, p, ap, 1, r0, parts, doneFlag, s));  // ref:2234 + 2235 + 2243 in one launch
			} else {
				SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, scratch, 0, nullptr, nullptr, doneFlag, s));  // ref:2234
				SMM_TRY(blockApplyDev<T>(blockM, scratch, ap, 1, r0, parts, doneFlag, s));                         // ref:2235 + 2243 fused
			}
		} else if (precondition) {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, scratch, 0, nullptr, nullptr, doneFlag, s));  // ref:2234
			SMM_TRY(apply(scratch, ap, doneFlag, s));                                                          // ref:2235
			SMM_TRY(launchDotPartials<T>(n, ap, r0, parts, doneFlag, s));                                      // ref:2243
		} else {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, ap, 1, r0, parts, doneFlag, s));  // ref:2240 + 2243 fused
		}
		// alpha, omega and beta are formed inside the three update kernels that consume them (no scalar launches)
		SMM_LAUNCH_UPDATE(bicgFusedS, updateNT(n, sizeof(T), 3), solverGrid(n), s, n, sc, i & 1, parts, ap, r, sv);
		if (jacobiDiag) {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, jacobiDiag, sv, as, 2, sv, parts, doneFlag, s, SPMV_DIV_LHS));  // ref:2250-2251 + 2256-2261 fused
		} else if (blockM) {
			if (fuseBlk) {
				SMM_TRY(blockApplySpmvDev<T>(blockM, sv, as, 2, sv, parts, doneFlag, s));  // ref:2250 + 2251 + 2259, 2261 in one launch
			} else {
				SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, sv, scratch, 0, nullptr, nullptr, doneFlag, s));  // ref:2250
				SMM_TRY(blockApplyDev<T>(blockM, scratch, as, 2, sv, parts, doneFlag, s));                          // ref:2251 + 2259, 2261 fused
			}
		} else if (precondition) {
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, sv, scratch, 0, nullptr, nullptr, doneFlag, s));  // ref:2250
			SMM_TRY(apply(scratch, as, doneFlag, s));                                                           // ref:2251
			dot2Partials<T><<<NPART, TPB, 0, s>>>(n, as, sv, parts, parts.p + NPART, doneFlag);                 // ref:2259, 2261
		} else {
			// as = A s with as.as -> parts[0..NPART) and as.s -> parts[NPART..2 NPART) fused (ref:2256-2261)
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, sv, as, 2, sv, parts, doneFlag, s));
		}
		SMM_LAUNCH_UPDATE(bicgFusedXR, updateNT(n, sizeof(T), 7), g, s, n, sc, parts, p, sv, as, r0, x, r, parts2);
		SMM_LAUNCH_UPDATE(bicgFusedP, updateNT(n, sizeof(T), 4), solverGrid(n), s, n, sc, i & 1, parts2, eps, ap, r, p);
	}
	Scal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	if (status) *status = h.iters > maxIterations ? SMM_SOLVER_MAX_ITERATIONS_REACHED : SMM_SOLVER_SUCCESS;  // ref:2279-2282
	if (iterations) *iterations = h.iters;
	if (resnorm) *resnorm = h.res;
	return SMM_HIP_OK;
}

template <typename T>
int bicgstabDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, hipStream_t s, int* status,
                int* iterations, T* resnorm) {
	SMM_TRY(solverCheck<T>("bicgstab", a, b, x));
	const bool precondition = M != nullptr && M->kind != SMM_PRECOND_NONE;  // ref:2209
	SMM_TRY(precondAdmissible("bicgstab", M, a, SOLVER_GENERAL));
	const DevApplier<T> apply{M};
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	const T* jacobiDiag = precondition && M->kind == SMM_PRECOND_JACOBI ? static_cast<const T*>(M->d_values) : nullptr;
	const smm_hip_precond* blockM = precondition && isBlockKind(M->kind) ? M : nullptr;
	if (!precondition || jacobiDiag) {
		// a matrix in the row-mask encoding whose vectors fit the register file is solved in ONE launch (smm_resident_bicg.hip)
		bool handled = false;
		SMM_TRY(bicgstabResidentTry<T>(a, b, x, maxIterations, eps, jacobiDiag, s, status, iterations, resnorm, &handled));
		if (handled) return SMM_HIP_OK;
	}
	SMM_TRY((bicgstabLoop<T, DevApplier<T>>(a, b, x, maxIterations, eps, precondition, apply, s, status, iterations, resnorm, jacobiDiag, blockM)));
	return precondition ? precondTakeError(M, s) : SMM_HIP_OK;
}

// host vectors, host functor: the generic form of the reference's template (ref:2191-2199)
template <typename T>
static int bicgstabFunctorHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, int (*fn)(void*, const T*, T*), void* user, int* status,
                               int* iterations, T* resnorm) {
	if (!fn) {
		setError("bicgstab_functor: null apply function");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(solverCheck<T>("bicgstab", a, b, x));
	const int n = a->rows;
	return solveFromHost<T>(n, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		T* pinned = nullptr;
		SMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pinned), sizeof(T) * 2 * static_cast<size_t>(std::max(1, n)), hipHostMallocDefault));
		struct Unpin {
			T* p;
			~Unpin() { hipHostFree(p); }
		} unpin{pinned};
		const HostApplier<T> apply{fn, user, n, pinned, pinned + std::max(1, n)};
		const int rc = bicgstabLoop<T, HostApplier<T>>(a, db, dx, maxIterations, eps, true, apply, s, status, iterations, resnorm);
		if (rc != SMM_HIP_OK) (void)hipStreamSynchronize(s);  // an apply's copy out of `pinned` may still be queued
		return rc;
	});
}

template <typename T>
int bicgsymmetricDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, hipStream_t s, int* status, int* iterations) {
	SMM_TRY(solverCheck<T>("bicgsymmetric", a, b, x));
	const int n = a->rows;
	maxIterations = std::min(maxIterations, n);  // ref:2030-2033
	if (maxIterations == -1) maxIterations = n;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	DevBuf<T> r, p, ap, parts;
	DevBuf<Scal<T>> sc;
	SMM_TRY(r.alloc(n));
	SMM_TRY(p.alloc(n));
	SMM_TRY(ap.alloc(n));
	SMM_TRY(parts.alloc(2 * NPART));
	SMM_TRY(sc.alloc(1));
	SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, nullptr, s));  // ref:2036
	SMM_TRY(launchCopy2<T>(n, r, p, nullptr, s));
	SMM_TRY(launchDotPartials<T>(n, r, r, parts, nullptr, s));
	bsymInitScal<T><<<1, TPB, 0, s>>>(parts, sc);
	const int* doneFlag = &sc.p->done;
	const int planned = std::max(1, maxIterations);
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1, 0, planned));
	for (int i = 0; i < planned && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, p, ap, 1, p, parts, doneFlag, s));  // ref:2048-2049
		bsymAlphaScal<T><<<1, TPB, 0, s>>>(parts, sc, eps);
		bsymUpdateXR<T><<<NPART, TPB, 0, s>>>(n, sc, p, ap, x, r, parts);
		bsymBetaScal<T><<<1, TPB, 0, s>>>(parts, sc, eps);
		bsymUpdateP<T><<<solverGrid(n), TPB, 0, s>>>(n, sc, r, p);
	}
	Scal<T> h;
	SMM_TRY(loopFinish(watch, &h, sc.p, sizeof(h), s));
	int st = h.status;
	if (st == SMM_SOLVER_SUCCESS && h.iters > maxIterations) st = SMM_SOLVER_MAX_ITERATIONS_REACHED;  // ref:2098-2100
	if (status) *status = st;
	if (iterations) *iterations = h.iters;
	return SMM_HIP_OK;
}

// ---- host-pointer wrappers: the reference's calling convention -----------------------------------------
template <typename T>
static int cgHost(const smm_hip_csr* a, const T* b, const T* x0, T* x, int maxIterations, T eps, const smm_hip_precond* M, int* status,
                  int* iterations, T* resnorm2) {
	SMM_TRY(solverCheck<T>("cg", a, b, x0, x));
	// x is only written once the loop runs (ref:2342-2344): the device copy starts from the caller's x and comes back only then
	int it = 0;
	SMM_TRY(solveFromHost<T>(a->rows, b, x0, x, [&](const T* db, const T* dx0, T* dx, hipStream_t s) {
		return cgDev<T>(a, db, dx0, dx, maxIterations, eps, M, s, status, &it, resnorm2);
	}, &it));
	if (iterations) *iterations = it;
	return SMM_HIP_OK;
}

template <typename T>
static int bicgstabHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, int* status, int* iterations,
                        T* resnorm) {
	SMM_TRY(solverCheck<T>("bicgstab", a, b, x));
	const HostTrace trace{"bicgstab (host pointers): whole call", "bicgstab (host pointers):   allocate b, x", "bicgstab (host pointers):   copy b, x in",
	                      "bicgstab (host pointers):   device loop", "bicgstab (host pointers):   copy x out"};
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return bicgstabDev<T>(a, db, dx, maxIterations, eps, M, s, status, iterations, resnorm);
	}, nullptr, trace);
}

template <typename T>
static int bicgsymmetricHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, int* status, int* iterations) {
	SMM_TRY(solverCheck<T>("bicgsymmetric", a, b, x));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return bicgsymmetricDev<T>(a, db, dx, maxIterations, eps, s, status, iterations);
	});
}

// every translation unit of the library is a code object of its own, built for the device at the FIRST launch of any of its kernels
// (5-9 ms each, measured: profiles/r04/first_spmv_setup_trace.txt); smm_hip_init touches one kernel of each hot-path unit so that
// the first SpMV of a process does not pay for it (SMM_HIP_PRELOAD=0: load lazily as before)
void preloadSolversUnit() {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(cgAlphaScal<float>));
	(void)hipGetLastError();
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_cg_f32(const smm_hip_csr* a, const float* b, const float* x0, float* x, int maxIterations, float eps, const smm_hip_precond* M,
                   int* solver_status, int* iterations, float* resnorm2) {
	return cgHost<float>(a, b, x0, x, maxIterations, eps, M, solver_status, iterations, resnorm2);
}
int smm_hip_cg_f64(const smm_hip_csr* a, const double* b, const double* x0, double* x, int maxIterations, double eps, const smm_hip_precond* M,
                   int* solver_status, int* iterations, double* resnorm2) {
	return cgHost<double>(a, b, x0, x, maxIterations, eps, M, solver_status, iterations, resnorm2);
}
int smm_hip_cg_dev_f32(const smm_hip_csr* a, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps,
                       const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return cgDev<float>(a, d_b, d_x0, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_cg_dev_f64(const smm_hip_csr* a, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                       const smm_hip_precond* M, smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return cgDev<double>(a, d_b, d_x0, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm2);
}

int smm_hip_bicgstab_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, const smm_hip_precond* M, int* solver_status,
                         int* iterations, float* resnorm) {
	return bicgstabHost<float>(a, b, x, maxIterations, eps, M, solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, const smm_hip_precond* M, int* solver_status,
                         int* iterations, double* resnorm) {
	return bicgstabHost<double>(a, b, x, maxIterations, eps, M, solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M,
                             smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm) {
	SMM_TRY(ensureInit());
	return bicgstabDev<float>(a, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M,
                             smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm) {
	SMM_TRY(ensureInit());
	return bicgstabDev<double>(a, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm);
}

int smm_hip_bicgstab_functor_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, smm_hip_apply_fn_f32 apply, void* user,
                                 int* solver_status, int* iterations, float* resnorm) {
	return bicgstabFunctorHost<float>(a, b, x, maxIterations, eps, apply, user, solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_functor_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, smm_hip_apply_fn_f64 apply, void* user,
                                 int* solver_status, int* iterations, double* resnorm) {
	return bicgstabFunctorHost<double>(a, b, x, maxIterations, eps, apply, user, solver_status, iterations, resnorm);
}

int smm_hip_set_cg_lazy_x_min_bytes(long long bytes) {
	g_lazyMinBytes.store(bytes, std::memory_order_relaxed);
	return SMM_HIP_OK;
}

int smm_hip_bicgsymmetric_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int* solver_status, int* iterations) {
	return bicgsymmetricHost<float>(a, b, x, maxIterations, eps, solver_status, iterations);
}
int smm_hip_bicgsymmetric_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int* solver_status, int* iterations) {
	return bicgsymmetricHost<double>(a, b, x, maxIterations, eps, solver_status, iterations);
}

}  // extern "C"
