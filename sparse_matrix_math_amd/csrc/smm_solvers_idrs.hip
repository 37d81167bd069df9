// smm_solvers_idrs.hip -- IDR(s) in the biorthogonal form (van Gijzen and Sonneveld 2011) with right preconditioning, device-resident.
// An addition: the reference has no IDR(s).  The definition is tests/idrs_restatement.py; the contract is in include/smm_hip.h.
//
// G, U and the shadow space P are ONE allocation each, column-major, s columns, leading dimension rounded up to 64 elements (every column
// starts 16-byte aligned); a caller's P is used as given.  u of step k is formed straight into column k of U and g = A u is written by the
// SpMV straight into column k of G: both columns' old contents have been consumed by then (the sums of a step run over i >= k).
// An inner step k is, besides the SpMV (and, with a preconditioner, its apply and a second form pass):
//   idrsForm            every workgroup: c[k:] by forward substitution from M and f; v = r - sum c_i G_i; U_k = om v + sum c_i U_i
//   multiDot + finish   h_i = p_i . g for all s columns from the same g (smm_multivec.h)
//   idrsOrthoUpdate     every workgroup: a, the new column of M, beta; G_k, U_k made biorthogonal; r, x; the partial sums of r.r
//   idrsStep            one workgroup: r.r, the column of M, f, the tests, the counters and the `done` flag
// five launches whatever k and s are.  The dimension-reduction step is the SpMV with t.t and t.r in its epilogue, idrsReduce (om, x, r,
// the partial sums of r.r) and idrsStep.  A cycle starts with multiDot + finish for f = P^T r.  The host never sees M.  ONE device flag:
// `done`, written by idrsStep alone (one workgroup, so no launch races with its own test) and read first by every kernel; a cycle never
// ends early otherwise, so there is no second flag.  A breakdown is noticed by every workgroup of idrsOrthoUpdate / idrsReduce alike (they
// write nothing then); workgroup 0 leaves a note (`bad`) for idrsStep.  No floating-point atomics, every sum in a fixed order: two runs of
// one solve give the same bits.
#include <algorithm>
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_multivec.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;
constexpr int MAXS = SMM_IDRS_MAX_S;
// columns of G / U loaded before the first of them is consumed
constexpr int ID_C = 4;

template <typename T>
struct IdrsState {
	T M[MAXS * MAXS];  // P^T G, lower triangular: M[i][j] at i + j * MAXS
	T f[MAXS];         // P^T r, kept up to date inside a cycle
	T h[MAXS], coef[MAXS];  // P^T g of the step ; the shadow space's Gram-Schmidt: the products and their negatives
	T col[MAXS];       // the new column of M, from idrsOrthoUpdate to idrsStep
	T om, beta, rr;
	int done, iters, status, bad;
};

// the set-up: iterations = 0, M = I, om = 1, r.r and the loop's first test
template <typename T>
__global__ __launch_bounds__(TPB) void idrsInit(IdrsState<T>* st, const T* __restrict__ rrParts, int maxIterations, T eps) {
	__shared__ T red[4];
	const T rr = sumParts(rrParts, red);
	if (threadIdx.x < MAXS * MAXS) st->M[threadIdx.x] = threadIdx.x % MAXS == threadIdx.x / MAXS ? T(1) : T(0);
	if (threadIdx.x != 0) return;
	st->om = T(1);
	st->beta = T(0);
	st->rr = rr;
	st->iters = 0;
	st->status = SMM_SOLVER_SUCCESS;
	st->bad = 0;
	st->done = (rr > eps * eps && 0 < maxIterations) ? 0 : 1;  // (a NaN residual leaves too)
}

// acc = _smm_fma(+-coef_i, V_i, acc) for i = lo .. hi - 1 ascending, on the MV_U packs of a lane; ID_C columns are loaded before the first
// is consumed (a short last chunk re-reads the last column)
template <typename T, bool NEG>
__device__ __forceinline__ void foldColumns(typename Pack16<T>::V (&acc)[MV_U], const T* V, long long ld, const T* coef, int lo, int hi, const long long (&li)[MV_U]) {
	using P = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	for (int c0 = lo; c0 < hi; c0 += ID_C) {
		P vv[ID_C][MV_U];
		T cf[ID_C];
#pragma unroll
		for (int c = 0; c < ID_C; ++c) {
			const int col = min(c0 + c, hi - 1);
			cf[c] = NEG ? -coef[col] : coef[col];
#pragma unroll
			for (int u = 0; u < MV_U; ++u) vv[c][u] = reinterpret_cast<const P*>(V + static_cast<long long>(col) * ld)[li[u]];
		}
#pragma unroll
		for (int c = 0; c < ID_C; ++c) {
			if (c0 + c < hi) {
#pragma unroll
				for (int u = 0; u < MV_U; ++u) {
#pragma unroll
					for (int e = 0; e < N; ++e) acc[u][e] = smmFma(cf[c], vv[c][u][e], acc[u][e]);
				}
			}
		}
	}
}

// MODE 0 (no preconditioner): v = r - sum_{i>=k} c_i G_i (never stored); U_k = om v + sum_{i>=k} c_i U_i
// MODE 1: out = v                        MODE 2: U_k = om in + sum_{i>=k} c_i U_i  (in = M^-1 v)
// c[k:] = solve(lower(M[k:, k:]), f[k:]) is redone by every workgroup (and by both passes) from the same M and f: the same bits everywhere.
template <typename T, int MODE>
__global__ __launch_bounds__(TPB) void idrsForm(long long n, int k, int s, const IdrsState<T>* __restrict__ st, const T* r, const T* G, T* U, long long ld, const T* in, T* out) {
	using P = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	__shared__ T sc[MAXS];
	if (st->done) return;
	if (threadIdx.x == 0) {
		for (int i = k; i < s; ++i) {
			T sum = st->f[i];
			for (int j = k; j < i; ++j) sum = sum - st->M[i + j * MAXS] * sc[j];
			sc[i] = sum / st->M[i + i * MAXS];
		}
	}
	__syncthreads();
	const T om = st->om;
	T* uk = U + static_cast<long long>(k) * ld;
	const bool vec = aligned16(r) && aligned16(G) && aligned16(U) && ld % N == 0 && (MODE == 0 || (MODE == 1 ? aligned16(out) : aligned16(in)));
	const long long nvec = vec ? n / N : 0;
	const long long tile = static_cast<long long>(MV_U) * TPB;
	for (long long base = static_cast<long long>(blockIdx.x) * tile; base < nvec; base += static_cast<long long>(gridDim.x) * tile) {
		P acc[MV_U];
		long long li[MV_U];
		bool live[MV_U];
#pragma unroll
		for (int u = 0; u < MV_U; ++u) {
			const long long i = base + u * TPB + threadIdx.x;
			live[u] = i < nvec;
			li[u] = live[u] ? i : nvec - 1;
			acc[u] = reinterpret_cast<const P*>(MODE == 2 ? in : r)[li[u]];
		}
		if (MODE != 2) foldColumns<T, true>(acc, G, ld, sc, k, s, li);
		if (MODE != 1) {
#pragma unroll
			for (int u = 0; u < MV_U; ++u) {
#pragma unroll
				for (int e = 0; e < N; ++e) acc[u][e] = om * acc[u][e];
			}
			foldColumns<T, false>(acc, U, ld, sc, k, s, li);
		}
#pragma unroll
		for (int u = 0; u < MV_U; ++u) {
			if (live[u]) reinterpret_cast<P*>(MODE == 1 ? out : uk)[li[u]] = acc[u];
		}
	}
	for (long long i = nvec * N + static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		T acc = MODE == 2 ? in[i] : r[i];
		if (MODE != 2) {
			for (int c = k; c < s; ++c) acc = smmFma(-sc[c], G[static_cast<long long>(c) * ld + i], acc);
		}
		if (MODE != 1) {
			acc = om * acc;
			for (int c = k; c < s; ++c) acc = smmFma(sc[c], U[static_cast<long long>(c) * ld + i], acc);
			uk[i] = acc;
		} else {
			out[i] = acc;
		}
	}
}

// a_i = (h_i - sum_{j<i} M[i][j] a_j) / M[i][i], i < k ; col_i = h_i - sum_{j<k} M[i][j] a_j, i >= k ; beta = f_k / col_k -- by every
// workgroup from the same device scalars.  col_k == 0 or not finite: the breakdown, nothing is written (x and r stay as they are).
// g -= sum_{i<k} a_i G_i ; u -= sum_{i<k} a_i U_i (columns k of G and U, in place) ; r -= beta g ; x += beta u ; rrParts[block] = r . r
template <typename T>
__global__ __launch_bounds__(TPB) void idrsOrthoUpdate(long long n, int k, int s, IdrsState<T>* st, T* G, T* U, long long ld, T* r, T* x, T* __restrict__ rrParts) {
	using P = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	__shared__ T red[4];
	__shared__ T sa[MAXS];
	__shared__ T sbeta;
	__shared__ int sbad;
	if (st->done) return;
	if (threadIdx.x == 0) {
		T col[MAXS];
		for (int i = 0; i < k; ++i) {
			T sum = st->h[i];
			for (int j = 0; j < i; ++j) sum = sum - st->M[i + j * MAXS] * sa[j];
			sa[i] = sum / st->M[i + i * MAXS];
		}
		for (int i = k; i < s; ++i) {
			T sum = st->h[i];
			for (int j = 0; j < k; ++j) sum = sum - st->M[i + j * MAXS] * sa[j];
			col[i] = sum;
		}
		const T d = col[k];
		const int bad = (d == T(0) || !isfinite(d)) ? 1 : 0;
		const T beta = st->f[k] / d;
		sbeta = beta;
		sbad = bad;
		if (blockIdx.x == 0) {  // (fields no workgroup reads in this launch)
			for (int i = k; i < s; ++i) st->col[i] = col[i];
			st->beta = beta;
			st->bad = bad;
		}
	}
	__syncthreads();
	if (sbad) return;
	const T beta = sbeta;
	T* gk = G + static_cast<long long>(k) * ld;
	T* uk = U + static_cast<long long>(k) * ld;
	const bool vec = aligned16(G) && aligned16(U) && aligned16(r) && aligned16(x) && ld % N == 0;
	const long long nvec = vec ? n / N : 0;
	const long long tile = static_cast<long long>(MV_U) * TPB;
	T rr = T(0);
	for (long long base = static_cast<long long>(blockIdx.x) * tile; base < nvec; base += static_cast<long long>(gridDim.x) * tile) {
		P g[MV_U], u[MV_U], rv[MV_U], xv[MV_U];
		long long li[MV_U];
		bool live[MV_U];
#pragma unroll
		for (int q = 0; q < MV_U; ++q) {
			const long long i = base + q * TPB + threadIdx.x;
			live[q] = i < nvec;
			li[q] = live[q] ? i : nvec - 1;
			g[q] = reinterpret_cast<const P*>(gk)[li[q]];
			u[q] = reinterpret_cast<const P*>(uk)[li[q]];
			rv[q] = reinterpret_cast<const P*>(r)[li[q]];
			xv[q] = reinterpret_cast<const P*>(x)[li[q]];
		}
		foldColumns<T, true>(g, G, ld, sa, 0, k, li);
		foldColumns<T, true>(u, U, ld, sa, 0, k, li);
#pragma unroll
		for (int q = 0; q < MV_U; ++q) {
			if (live[q]) {
#pragma unroll
				for (int e = 0; e < N; ++e) {
					rv[q][e] = smmFma(-beta, g[q][e], rv[q][e]);
					xv[q][e] = smmFma(beta, u[q][e], xv[q][e]);
					rr += rv[q][e] * rv[q][e];
				}
				if (k > 0) {
					reinterpret_cast<P*>(gk)[li[q]] = g[q];
					reinterpret_cast<P*>(uk)[li[q]] = u[q];
				}
				reinterpret_cast<P*>(r)[li[q]] = rv[q];
				reinterpret_cast<P*>(x)[li[q]] = xv[q];
			}
		}
	}
	for (long long i = nvec * N + static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		T g = gk[i], u = uk[i];
		for (int c = 0; c < k; ++c) {
			g = smmFma(-sa[c], G[static_cast<long long>(c) * ld + i], g);
			u = smmFma(-sa[c], U[static_cast<long long>(c) * ld + i], u);
		}
		if (k > 0) {
			gk[i] = g;
			uk[i] = u;
		}
		const T rn = smmFma(-beta, g, r[i]);
		r[i] = rn;
		x[i] = smmFma(beta, u, x[i]);
		rr += rn * rn;
	}
	const T sum = blockSum256(rr, red);
	if (threadIdx.x == 0) rrParts[blockIdx.x] = sum;
}

// The dimension-reduction step: t.t and t.r from the SpMV's epilogue (ttr = [t.t | t.r], NPART partials each), rho = |t.r| / sqrt(t.t r.r),
// om = t.r / t.t, scaled up by 0.7 / rho when rho < 0.7; x += om z ; r -= om t ; rrParts[block] = r . r.  z = M^-1 r (r itself without a
// preconditioner).  t.t == 0 or not finite: the breakdown, nothing is written.
template <typename T>
__global__ __launch_bounds__(TPB) void idrsReduce(long long n, IdrsState<T>* st, const T* __restrict__ ttr, const T* z, const T* t, T* r, T* x, T* __restrict__ rrParts) {
	__shared__ T red[5];
	if (st->done) return;
	const T tt = sumPartsAll(ttr, red);
	const T tr = sumPartsAll(ttr + NPART, red);
	const int bad = (tt == T(0) || !isfinite(tt)) ? 1 : 0;
	const T rho = fabs(tr) / sqrt(tt * st->rr);
	T om = tr / tt;
	if (rho < T(0.7)) om = om * (T(0.7) / rho);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		st->bad = bad;
		if (!bad) st->om = om;
	}
	if (bad) return;
	T acc = T(0);
	const T* const in[4] = {x, z, t, r};
	T* const out[2] = {x, r};
	streamMap<T, false, 4, 2>(n, in, out, [&](const T(&v)[4], T(&o)[2]) {
		o[0] = smmFma(om, v[1], v[0]);
		const T rn = smmFma(-om, v[2], v[3]);
		o[1] = rn;
		acc += rn * rn;
	});
	const T sum = blockSum256(acc, red);
	if (threadIdx.x == 0) rrParts[blockIdx.x] = sum;
}

// One workgroup after every step (k == s: the dimension-reduction step): r.r from the nb partials, the column of M and f -= beta M[:, k],
// iterations++, the tests.  The only writer of `done`.
template <typename T>
__global__ __launch_bounds__(TPB) void idrsStep(IdrsState<T>* st, const T* __restrict__ rrParts, int nb, int k, int s, int maxIterations, T eps) {
	__shared__ T red[4];
	if (st->done) return;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) acc += rrParts[i];
	const T rr = blockSum256(acc, red);
	if (threadIdx.x != 0) return;
	if (st->bad) {  // x, r and the counters as they are
		st->status = SMM_SOLVER_DIVERGED;
		st->done = 1;
		return;
	}
	if (k < s) {
		for (int i = 0; i < k; ++i) st->M[i + k * MAXS] = T(0);
		for (int i = k; i < s; ++i) st->M[i + k * MAXS] = st->col[i];
	}
	const int iters = st->iters + 1;
	st->iters = iters;
	st->rr = rr;
	if (!(rr > eps * eps) || iters >= maxIterations) {  // (a NaN residual leaves too)
		st->done = 1;
		return;
	}
	if (k < s) {
		const T beta = st->beta;
		for (int i = k + 1; i < s; ++i) st->f[i] = st->f[i] - beta * st->col[i];
	}
}

// P = the hash, then classical Gram-Schmidt applied twice and a division by the norm, column by column (all of it smm_multivec.h's).
// parts: MAXS * NPART elements, parts1: NPART, prod / neg: MAXS device scalars each.
template <typename T>
static int shadowFill(int n, int S, unsigned long long seed, T* P, long long ld, T* parts, T* parts1, T* prod, T* neg, hipStream_t s) {
	if (n <= 0) return SMM_HIP_OK;
	const int gmv = gridMV(n, sizeof(T));
	hashFillKernel<T><<<dim3(solverGrid(n), S), TPB, 0, s>>>(n, seed, 0, P, ld);
	for (int j = 0; j < S; ++j) {
		T* pj = P + static_cast<long long>(j) * ld;
		orthogonaliseTwice<T>(P, ld, n, gmv, j, pj, parts, parts1, prod, prod, neg, nullptr, s);
		normaliseKernel<T><<<solverGrid(n), TPB, 0, s>>>(n, pj, parts1, gmv, nullptr, nullptr);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

static int sCheck(const char* who, int S) {
	if (S < 1 || S > MAXS) {
		setError("%s: s must be 1 .. %d", who, MAXS);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int idrsCheck(const smm_hip_csr* a, const T* b, const T* x, int S, const T* d_P, long long ldP) {
	SMM_TRY(solverCheck<T>("idrs", a, b, x));
	SMM_TRY(sCheck("idrs", S));
	if (d_P && ldP < a->rows) {
		setError("idrs: the leading dimension of P is smaller than rows");
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int idrsDev(const smm_hip_csr* a, const T* b, T* x, int maxIterations, T eps, int S, const smm_hip_precond* M, const T* d_P, long long ldP,
                   unsigned long long seed, hipStream_t s, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(idrsCheck<T>(a, b, x, S, d_P, ldP));
	const bool precondition = M != nullptr && M->kind != SMM_PRECOND_NONE;
	SMM_TRY(precondAdmissible("idrs", M, a, SOLVER_GENERAL));
	if (precondition && M->dtype != dtypeOf<T>()) {
		setError("idrs: the preconditioner holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	const int n = a->rows;
	if (maxIterations < 0) maxIterations = n;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	const long long ld = std::max<long long>(64, (static_cast<long long>(n) + 63) / 64 * 64);
	DevBuf<T> G, U, Pown, r, tv, vw, zv, parts, parts1, parts2;
	DevBuf<IdrsState<T>> st;
	SMM_TRY(G.alloc(static_cast<size_t>(ld) * S));
	SMM_TRY(U.alloc(static_cast<size_t>(ld) * S));
	if (!d_P) SMM_TRY(Pown.alloc(static_cast<size_t>(ld) * S));
	SMM_TRY(r.alloc(n));
	SMM_TRY(tv.alloc(n));
	if (precondition) {
		SMM_TRY(vw.alloc(n));
		SMM_TRY(zv.alloc(n));
	}
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXS) * NPART));
	SMM_TRY(parts1.alloc(NPART));      // r.r
	SMM_TRY(parts2.alloc(2 * NPART));  // [t.t | t.r]
	SMM_TRY(st.alloc(1));
	IdrsState<T>* sp = st.p;
	const int* done = &sp->done;
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(IdrsState<T>), s));
	SMM_HIP_TRY(hipMemsetAsync(G.p, 0, sizeof(T) * static_cast<size_t>(ld) * S, s));
	SMM_HIP_TRY(hipMemsetAsync(U.p, 0, sizeof(T) * static_cast<size_t>(ld) * S, s));
	const T* P = d_P;
	if (!d_P) {
		SMM_TRY(shadowFill<T>(n, S, seed, Pown.p, ld, parts, parts1, sp->h, sp->coef, s));
		P = Pown.p;
		ldP = ld;
	}
	const int gmv = gridMV(n, sizeof(T));
	const int gup = solverGrid(n);

	SMM_TRY(launchSpmv<T>(a, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, nullptr, s));
	SMM_TRY(launchDotPartials<T>(n, r, r, parts1, nullptr, s));
	idrsInit<T><<<1, TPB, 0, s>>>(sp, parts1, maxIterations, eps);

	LoopWatch watch;
	SMM_TRY(watch.begin(s, done, 1, 1));  // asked before every cycle but the first
	// while the loop is live every queued step is taken, so `queued` is the iteration count the next step starts from
	int queued = 0;
	for (int c = 0; queued < maxIterations && !watch.leave(c); ++c) {
		multiDotKernel<T><<<gmv, TPB, 0, s>>>(n, S, P, ldP, r.p, parts, done);
		multiDotFinish<T><<<S, TPB, 0, s>>>(parts, gmv, sp->f, nullptr, done);
		for (int k = 0; k < S && queued < maxIterations; ++k, ++queued) {
			T* gk = G.p + static_cast<long long>(k) * ld;
			T* uk = U.p + static_cast<long long>(k) * ld;
			if (precondition) {
				idrsForm<T, 1><<<gmv, TPB, 0, s>>>(n, k, S, sp, r.p, G.p, U.p, ld, nullptr, vw.p);
				SMM_TRY(precondApplyDev<T>(M, vw, zv, done, s));
				idrsForm<T, 2><<<gmv, TPB, 0, s>>>(n, k, S, sp, r.p, G.p, U.p, ld, zv.p, nullptr);
			} else {
				idrsForm<T, 0><<<gmv, TPB, 0, s>>>(n, k, S, sp, r.p, G.p, U.p, ld, nullptr, nullptr);
			}
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, uk, gk, 0, nullptr, nullptr, done, s));
			multiDotKernel<T><<<gmv, TPB, 0, s>>>(n, S, P, ldP, gk, parts, done);
			multiDotFinish<T><<<S, TPB, 0, s>>>(parts, gmv, sp->h, nullptr, done);
			idrsOrthoUpdate<T><<<gmv, TPB, 0, s>>>(n, k, S, sp, G.p, U.p, ld, r.p, x, parts1);
			idrsStep<T><<<1, TPB, 0, s>>>(sp, parts1, gmv, k, S, maxIterations, eps);
		}
		if (queued < maxIterations) {
			const T* z = r;
			if (precondition) {
				SMM_TRY(precondApplyDev<T>(M, r, zv, done, s));
				z = zv;
			}
			SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, z, tv, 2, r, parts2, done, s));
			idrsReduce<T><<<gup, TPB, 0, s>>>(n, sp, parts2, z, tv.p, r.p, x, parts1);
			idrsStep<T><<<1, TPB, 0, s>>>(sp, parts1, gup, S, S, maxIterations, eps);
			++queued;
		}
	}
	struct {  // IdrsState<T> from `rr` on
		T rr;
		int done, iters, status, bad;
	} tail;
	static_assert(sizeof(tail) == sizeof(IdrsState<T>) - offsetof(IdrsState<T>, rr), "the tail of IdrsState");
	SMM_TRY(loopFinish(watch, &tail, &sp->rr, sizeof(tail), s));
	const T rr = tail.rr;
	int st_out = SMM_SOLVER_MAX_ITERATIONS_REACHED;
	if (rr <= eps * eps) st_out = SMM_SOLVER_SUCCESS;
	else if (tail.status == SMM_SOLVER_DIVERGED) st_out = SMM_SOLVER_DIVERGED;
	if (status) *status = st_out;
	if (iterations) *iterations = tail.iters;
	if (resnorm2) *resnorm2 = rr;
	return precondition ? precondTakeError(M, s) : SMM_HIP_OK;
}

// host vectors (x in / out); the shadow space is the library's own
template <typename T>
static int idrsHost(const smm_hip_csr* a, T* b, T* x, int maxIterations, T eps, int S, const smm_hip_precond* M, unsigned long long seed, int* status, int* iterations,
                    T* resnorm2) {
	SMM_TRY(idrsCheck<T>(a, b, x, S, nullptr, 0));
	return solveFromHost<T>(a->rows, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return idrsDev<T>(a, db, dx, maxIterations, eps, S, M, nullptr, 0, seed, s, status, iterations, resnorm2);
	});
}

template <typename T>
static int shadowDev(int n, int S, unsigned long long seed, T* d_P, long long ld, hipStream_t s) {
	SMM_TRY(sCheck("idrs_shadow", S));
	if (n < 0 || ld < n || (n > 0 && !d_P)) {
		setError("idrs_shadow: bad arguments (n >= 0, ld >= n, no null array)");
		return SMM_HIP_ERR_INVALID;
	}
	DevBuf<T> parts, parts1, scal;
	SyncOnExit drain{s};  // the scratch is released under no queued work
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXS) * NPART));
	SMM_TRY(parts1.alloc(NPART));
	SMM_TRY(scal.alloc(2 * MAXS));
	return shadowFill<T>(n, S, seed, d_P, ld, parts, parts1, scal.p, scal.p + MAXS, s);
}

// (see preloadSolversUnit, smm_solvers.hip)
void preloadIdrsUnit() {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(idrsInit<float>));
	(void)hipGetLastError();
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_idrs_f32(const smm_hip_csr* a, float* b, float* x, int maxIterations, float eps, int s, const smm_hip_precond* M, unsigned long long seed,
                     int* solver_status, int* iterations, float* resnorm2) {
	return idrsHost<float>(a, b, x, maxIterations, eps, s, M, seed, solver_status, iterations, resnorm2);
}
int smm_hip_idrs_f64(const smm_hip_csr* a, double* b, double* x, int maxIterations, double eps, int s, const smm_hip_precond* M, unsigned long long seed,
                     int* solver_status, int* iterations, double* resnorm2) {
	return idrsHost<double>(a, b, x, maxIterations, eps, s, M, seed, solver_status, iterations, resnorm2);
}
int smm_hip_idrs_dev_f32(const smm_hip_csr* a, const float* d_b, float* d_x, int maxIterations, float eps, int s, const smm_hip_precond* M, const float* d_P,
                         long long ldP, unsigned long long seed, smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return idrsDev<float>(a, d_b, d_x, maxIterations, eps, s, M, d_P, ldP, seed, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_idrs_dev_f64(const smm_hip_csr* a, const double* d_b, double* d_x, int maxIterations, double eps, int s, const smm_hip_precond* M, const double* d_P,
                         long long ldP, unsigned long long seed, smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return idrsDev<double>(a, d_b, d_x, maxIterations, eps, s, M, d_P, ldP, seed, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_idrs_shadow_dev_f32(int n, int s, unsigned long long seed, float* d_P, long long ld, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return shadowDev<float>(n, s, seed, d_P, ld, pickStream(stream));
}
int smm_hip_idrs_shadow_dev_f64(int n, int s, unsigned long long seed, double* d_P, long long ld, smm_hip_stream stream) {
	SMM_TRY(ensureInit());
	return shadowDev<double>(n, s, seed, d_P, ld, pickStream(stream));
}

}  // extern "C"
