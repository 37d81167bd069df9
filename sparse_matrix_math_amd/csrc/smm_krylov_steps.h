// smm_krylov_steps.h -- the steps of the device-resident ConjugateGradient (ref:2354-2394) and BiCGStab (ref:2243-2277) loops, written
// once for the single-GPU loop (smm_solvers.hip) and the row-partitioned one (smm_dist.hip).  The kernels of the two units are shells:
// a shell obtains the reduced scalars -- every workgroup re-adds NPART partials (sumPartsAll) on one GPU, reads the all-reduced totals[k]
// in the row-partitioned loop -- and says which rows its launch covers; the recurrence arithmetic, the bookkeeping in Scal<T> and the
// deferred-x ring are here, so the two loops round alike by construction.
#pragma once
#include "smm_solver_scal.h"

namespace smm {

// ---- which rows a launch covers ------------------------------------------------------------------------------------------------
// the whole vector: one streamMap (smm_device.h: 16-byte accesses, 4 packs per lane in flight)
struct WholeRows {
	int n;
	template <typename T, int NIN, int NOUT, bool NT, typename F>
	__device__ __forceinline__ void map(const T* const* in, T* const* out, F&& f) const {
		streamMap<T, NT, NIN, NOUT>(n, in, out, f);
	}
};

// up to four [lo, hi) runs of rows, passed to the update kernels by value (the boundary rows some peer receives / the rest: halo first)
struct RowRanges {
	int n = 0;
	int lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
	long long rows() const {
		long long t = 0;
		for (int i = 0; i < n; ++i) t += hi[i] - lo[i];
		return t;
	}
	template <typename T, int NIN, int NOUT, bool NT, typename F>
	__device__ __forceinline__ void map(const T* const* in, T* const* out, F&& f) const {
		for (int i = 0; i < n; ++i) {
			const T* in2[NIN];
			T* out2[NOUT];
#pragma unroll
			for (int k = 0; k < NIN; ++k) in2[k] = in[k] + lo[i];
#pragma unroll
			for (int k = 0; k < NOUT; ++k) out2[k] = out[k] + lo[i];
			streamMap<T, NT, NIN, NOUT>(hi[i] - lo[i], in2, out2, f);
		}
	}
};
inline RowRanges wholeRange(int n) {  // rows [0, n) as one run
	RowRanges all{};
	all.n = 1;
	all.hi[0] = n;
	return all;
}

// `book` in the steps below: this launch records the scalars.  Of a boundary / bulk pair of launches both form them from the same
// operands, one writes them; a launch over the whole vector passes true.
// rr0 / rr of bicgStepS / cgStepR: rrPing[par], which the kernel loads BEFORE it sums partials (the load's latency hides behind the sums).

// ---- BiCGStab --------------------------------------------------------------------------------------------------------------------
// alpha = rr0 / (ap.r0) ; s = -alpha ap + r   (ref:2243-2247)
template <typename T, bool NT, typename Rows>
__device__ __forceinline__ void bicgStepS(const Rows& rows, bool book, Scal<T>* sc, T rr0, T apr0, const T* ap, const T* r, T* sv) {
	const T alpha = rr0 / apr0;
	if (book && blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;
	const T* const in[2] = {ap, r};
	T* const out[1] = {sv};
	rows.template map<T, 2, 1, NT>(in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(-alpha, v[0], v[1]); });
}

// omega = (as.s)/(as.as) ; r = -omega as + s ; partial ||r||^2 -> partsC[0..NPART) and r.r0 -> partsC[NPART..2 NPART)   (ref:2259-2269);
// WITHX: x = alpha p + (omega s + x) (ref:2264) in the same pass over s.  red: 4 words of LDS
template <typename T, bool NT, bool WITHX>
__device__ __forceinline__ void bicgStepXR(int n, Scal<T>* sc, T asas, T ass, T* red, const T* p, const T* sv, const T* as, const T* r0, T* x, T* r,
                                           T* __restrict__ partsC) {
	const T omega = ass / asas;
	const T alpha = WITHX ? sc->alpha : T(0);
	if (blockIdx.x == 0 && threadIdx.x == 0) sc->omega = omega;
	T acc0 = T(0), acc1 = T(0);
	// inputs: s [, x, p], as, r0; outputs: [x,] r
	constexpr int NIN = WITHX ? 5 : 3, NOUT = WITHX ? 2 : 1;
	const T* const in[5] = {sv, WITHX ? x : as, WITHX ? p : r0, as, r0};
	T* const out[2] = {WITHX ? x : r, r};
	streamMap<T, NT, NIN, NOUT>(n, in, out, [&](const T(&v)[NIN], T(&o)[NOUT]) {
		const T si = v[0];
		if constexpr (WITHX) o[0] = smmFma(alpha, v[2], smmFma(omega, si, v[1]));
		const T ri = smmFma(-omega, v[NIN - 2], si);
		o[NOUT - 1] = ri;
		acc0 += ri * ri;
		acc1 += ri * v[NIN - 1];
	});
	const T s0 = blockSum256(acc0, red);
	const T s1 = blockSum256(acc1, red);
	if (threadIdx.x == 0) {
		partsC[blockIdx.x] = s0;
		partsC[NPART + blockIdx.x] = s1;
	}
}

// resL2Norm, loop test, beta, p = beta (-omega ap + p) + r   (ref:2268-2277)
template <typename T, bool NT, typename Rows>
__device__ __forceinline__ void bicgStepP(const Rows& rows, bool book, Scal<T>* sc, int par, T rr, T newRR0, T eps, const T* ap, const T* r, T* p) {
	const T res = sqrtRn(rr);
	const T alpha = sc->alpha;
	const T omega = sc->omega;
	const T rr0 = sc->rrPing[par];
	const bool leave = !(res > eps);  // while (resL2Norm > eps ...): NaN leaves the loop too
	if (book && blockIdx.x == 0 && threadIdx.x == 0) {
		sc->res = res;
		sc->rrPing[par ^ 1] = newRR0;
		sc->iters += 1;
		if (leave) sc->done = 1;
	}
	if (leave) return;
	const T beta = (newRR0 * alpha) / (rr0 * omega);  // ref:2271
	const T* const in[3] = {ap, p, r};
	T* const out[1] = {p};
	rows.template map<T, 3, 1, NT>(in, out, [&](const T(&v)[3], T(&o)[1]) { o[0] = smmFma(beta, smmFma(-omega, v[0], v[1]), v[2]); });
}

// ---- ConjugateGradient -----------------------------------------------------------------------------------------------------------
// the first launch of an iteration leaves `done` as it found it in sc->pad: the launches behind it decide by that (workgroup 0 of one of them
// raises `done` while other workgroups of the same launch may not have started yet)
template <typename T>
__device__ __forceinline__ int cgSnapshotDone(Scal<T>* sc) {
	const int done = sc->done;
	if (blockIdx.x == 0 && threadIdx.x == 0) sc->pad = done;
	return done;
}

// alpha = rr / (Ap.p) ; r = -alpha Ap + r ; partial ||r||^2   (ref:2354-2375).  red: 4 words of LDS
template <typename T, bool NT>
__device__ __forceinline__ void cgStepR(int n, Scal<T>* sc, T rr, T pAp, T* red, const T* Ap, T* r, T* __restrict__ partsC, int alphaSlot) {
	const T alpha = rr / pAp;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		sc->alpha = alpha;
		sc->alphaRing[alphaSlot] = alpha;
	}
	T acc = T(0);
	const T* const in[2] = {Ap, r};
	T* const out[1] = {r};
	streamMap<T, NT, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) {
		const T ri = smmFma(-alpha, v[0], v[1]);
		o[0] = ri;
		acc += ri * ri;
	});
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) partsC[blockIdx.x] = s;
}

// ---- the x update deferred -------------------------------------------------------------------------------------------------------
// x is only an accumulator: x_{k+1} = alpha_k p_k + x_k (ref:2362-2366).  Keeping the last LAZY_M directions in a ring, x is brought up to
// date every LAZY_M-th iteration -- x = alpha_k p_k + (... + (alpha_{k-M+1} p_{k-M+1} + x)): the reference's roundings in the reference's
// order, bit for bit.  The launch that finds the iteration converged -- or is told it is the last -- flushes whatever is pending, so x
// is complete whenever the loop ends.
template <typename T>
struct LazyRing {
	T* p[LAZY_M + 1];  // (row-partitioned loop: the owned part of every halo-extended ring vector)
};

// alpha[LAZY_M - 1] = the alpha at ring position alphaSlot (the newest), alpha[LAZY_M - 2] the one before, ...
template <typename T>
__device__ __forceinline__ void cgLazyAlphas(const Scal<T>* sc, int alphaSlot, T (&alpha)[LAZY_M]) {
#pragma unroll
	for (int k = 0; k < LAZY_M; ++k) alpha[LAZY_M - 1 - k] = sc->alphaRing[(alphaSlot + LAZY_M - k) % LAZY_M];
}

// PENDING directions (the one in slot `cur` included) are applied to x; PUPD: p_next = beta p_cur + r as well
template <typename T, bool NT, int PENDING, bool PUPD, typename Rows>
__device__ __forceinline__ void cgLazyFlush(const Rows& rows, const LazyRing<T>& ring, int cur, const T (&alpha)[LAZY_M], T beta, const T* r, const T* xcur, T* x) {
	// inputs: x, p_cur-PENDING+1 .. p_cur (oldest first) [, r]; outputs: x [, p_next]
	const T* in[PENDING + 2];
	in[0] = xcur;
#pragma unroll
	for (int k = 0; k < PENDING; ++k) in[1 + k] = ring.p[(cur + (LAZY_M + 1) - (PENDING - 1 - k)) % (LAZY_M + 1)];
	in[PENDING + 1] = PUPD ? r : xcur;  // (without the p update r is not read: any valid vector)
	T* out[2] = {x, ring.p[(cur + 1) % (LAZY_M + 1)]};
	rows.template map<T, PENDING + 2, PUPD ? 2 : 1, NT>(in, out, [&](const T(&v)[PENDING + 2], T(&o)[PUPD ? 2 : 1]) {
		T xv = v[0];
#pragma unroll
		for (int k = 0; k < PENDING; ++k) xv = smmFma(alpha[LAZY_M - PENDING + k], v[1 + k], xv);  // oldest direction first, ref:2372
		o[0] = xv;
		if constexpr (PUPD) o[1] = smmFma(beta, v[PENDING], v[PENDING + 1]);
	});
}

// the flush for a `pending` (1 .. LAZY_M) known only when the launch runs
template <typename T, bool NT, typename Rows>
__device__ __forceinline__ void cgLazyFlushPending(const Rows& rows, const LazyRing<T>& ring, int cur, int pending, bool pupd, const T (&alpha)[LAZY_M], T beta, const T* r,
                                                   const T* xcur, T* x) {
	static_assert(LAZY_M == 8, "the cases below");
#define SMM_LAZY_CASE(P)                                                                      \
	case P:                                                                                   \
		if (pupd) cgLazyFlush<T, NT, P, true>(rows, ring, cur, alpha, beta, r, xcur, x);      \
		else cgLazyFlush<T, NT, P, false>(rows, ring, cur, alpha, beta, r, xcur, x);          \
		break;
	switch (pending) {
		SMM_LAZY_CASE(1)
		SMM_LAZY_CASE(2)
		SMM_LAZY_CASE(3)
		SMM_LAZY_CASE(4)
		SMM_LAZY_CASE(5)
		SMM_LAZY_CASE(6)
		SMM_LAZY_CASE(7)
		SMM_LAZY_CASE(8)
	default: break;
	}
#undef SMM_LAZY_CASE
}

// convergence test ; beta ; p_next = beta p_cur + r (ref:2377-2394) ; x brought up to date when `flush` (host: every LAZY_M-th iteration and
// the last planned one) or when the iteration converged.  pending = directions not yet applied to x, this iteration's included (1 .. LAZY_M).
// The caller has tested sc->pad (cgSnapshotDone), not `done`: workgroup 0 of this very launch may be raising `done` while others start,
// and their rows still need the flush.
template <typename T, bool NT, typename Rows>
__device__ __forceinline__ void cgLazyStep(const Rows& rows, bool book, Scal<T>* sc, int par, T rrNew, T eps, const LazyRing<T>& ring, int cur, int pending, int flush,
                                           int alphaSlot, const T* r, const T* xcur, T* x) {
	const T rrOld = sc->rrPing[par];
	const bool converged = eps * eps > rrNew;
	T alpha[LAZY_M];
	cgLazyAlphas(sc, alphaSlot, alpha);
	if (book && blockIdx.x == 0 && threadIdx.x == 0) {
		sc->iters += 1;
		sc->res = rrNew;
		if (converged) {
			sc->done = 1;
			sc->status = SMM_SOLVER_SUCCESS;
		} else {
			sc->rrPing[par ^ 1] = rrNew;
		}
	}
	const T beta = rrNew / rrOld;
	if (!(flush || converged)) {
		const T* const in[2] = {ring.p[cur], r};
		T* const out[1] = {ring.p[(cur + 1) % (LAZY_M + 1)]};
		rows.template map<T, 2, 1, NT>(in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(beta, v[0], v[1]); });
		return;
	}
	cgLazyFlushPending<T, NT>(rows, ring, cur, pending, !converged, alpha, beta, r, xcur, x);
}

// With the next direction formed inside the SpMV (launchConstMarchFusedP) nothing is left of cgLazyStep but x: this launch sits behind every
// such SpMV and completes x when it is scheduled (every LAZY_M-th iteration) or when that SpMV found its predecessor converged (flushIter ==
// iter: one shot -- the launches enqueued behind a finished solve find another number there).  pending directions end at ring slot `cur`;
// alphaSlot: the ring position of the newest one's alpha.
template <typename T, bool NT, typename Rows>
__device__ __forceinline__ void cgFlushOnlyStep(const Rows& rows, const Scal<T>* __restrict__ sc, const LazyRing<T>& ring, int cur, int pending, int scheduled, int iter,
                                                int alphaSlot, const T* xcur, T* x) {
	const bool converged = sc->flushIter == iter;
	if (!converged && (!scheduled || sc->done)) return;
	T alpha[LAZY_M];
	cgLazyAlphas(sc, alphaSlot, alpha);
	cgLazyFlushPending<T, NT>(rows, ring, cur, pending, false, alpha, T(0), nullptr, xcur, x);
}

}  // namespace smm
