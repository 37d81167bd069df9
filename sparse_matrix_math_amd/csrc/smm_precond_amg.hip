// smm_precond_amg.hip -- smoothed-aggregation multigrid preconditioner with a symmetric V-cycle on gfx950 (an addition, no counterpart in
// the reference).  include/smm_hip.h (SMM_PRECOND_AMG) states the definition in words, tests/amg_restatement.py line by line.
//
// Set-up, per level A_l (n rows), everything on the device, one lane per row:
//   strength flags    one byte per stored entry: j != i and a_ij^2 >= theta_l^2 |a_ii| |a_jj| in double
//   roots             a distance-2 maximal independent set in synchronous rounds.  A row's key (state, hash, index) is ONE 64-bit word, so a
//                     maximum is an integer maximum; a decided non-root never wins a maximum an undecided row takes part in and is packed as
//                     0, which leaves one bit for the states 1 / 2: (state - 1) << 63 | hash << 31 | index.  A round is two hops (each from
//                     the previous array into another one) and the state update, which also writes the next round's keys and counts the
//                     undecided rows: that one int is what the host reads per round.
//   aggregates        roots numbered by a prefix scan (rocprim); phase 1 (the smallest root number among the strong neighbours), phase 2
//                     (passes from the previous assignment into another array, until a pass assigns nothing), left-over rows numbered by a
//                     second scan.
//   operators         T (one 1 per row) and S = I - omega D^-1 A on A's pattern are written by two kernels; P = S T, R = P^T, A P and
//                     A_{l+1} = R (A P) are the library's own product and transpose, so every level is an ordinary smm_hip_csr.
//   smoother          the Chebyshev preconditioner of A_l (smm_precond_cheb.hip), which also brings the diagonal copy and the Gershgorin bound
//   coarsest level    copied to the host, inverted in double by Gauss-Jordan with partial pivoting, rounded to T once, kept dense
// No result depends on how rows are dealt to lanes: integer maxima / minima and counts only, every pass out of place.
//
// Created with near-null-space candidates B (smm_hip_precond_create_amg_candidates_*; tests/amg_candidates_restatement.py), a level differs in:
//   node graph        block size b > 1: N = Tb^T ((A o A) Tb) by the library's product and transpose, the root of every value; the kernels
//                     above run on N unchanged and a dof inherits its node's aggregate
//   T                 the member dofs of every aggregate in ascending order (one stable radix sort), the thin QR of its block of B_l by
//                     modified Gram-Schmidt (amgQrKernel: one wavefront or 16 / 32 lanes per aggregate, the block in LDS up to 256 rows,
//                     inner products in an order fixed by the aggregate's size alone); Q is T's values, R the rows of B_{l+1}
//   dropped columns   a column dependent on the earlier ones on an aggregate has no entries in T; its coarse dof gets a stored 1:
//                     A_{l+1} = R (A P) + E by the library's sum
// The cycle does not know about candidates.  Byte model and summation order: DESIGN.md section 3.31.
//
// The cycle (amgCycle) is launches only: per level two smoother applies, two residual SpMVs with A_l, one SpMV with R_l, one with P_l and
// one x += d pass; the coarsest level is one launch, one wavefront per row.  Every launch takes the solver's done flag.  All level vectors
// belong to the handle: one handle serves one stream at a time.  Traffic per cycle: DESIGN.md section 3.14.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "smm_csr_build.h"
#include "smm_device.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

struct smm_amg_level {
	const smm_hip_csr* A = nullptr;  // level 0: the caller's matrix; deeper: Anext of the level above (owned there)
	int n = 0, nc = 0;
	bool coarsest = true;
	smm_hip_precond* cheb = nullptr;  // the smoother; its d_values is the diagonal copy
	double lam = 0.0;
	int* d_agg = nullptr;      // [n] aggregate numbers (without candidates: T's positions as well)
	int* d_tstart = nullptr;   // [n + 1] 0 .. n; with candidates: the kept columns of every row's aggregate, scanned
	void* d_tval = nullptr;    // [n] ones; with candidates: [nnz(T)] the columns of Q
	void* d_sval = nullptr;    // [nnz] S on A's pattern
	smm_hip_csr *S = nullptr, *Tm = nullptr, *P = nullptr, *R = nullptr, *AP = nullptr, *Anext = nullptr;
	// created with candidates (k > 0 in the handle): T holds up to k entries per row at d_tpos, B_l is kept for every level
	int nAgg = 0, dropped = 0;  // aggregates (nc = nAgg k coarse dofs); coarse dofs whose column of T is empty
	int* d_tpos = nullptr;      // [nnz(T)]
	void* d_B = nullptr;        // [n x k] column-major, leading dimension n
	smm_hip_csr *E = nullptr, *RAP = nullptr;  // dropped > 0: Anext = RAP + E, E the stored ones of the dropped coarse dofs
	void *x = nullptr, *b = nullptr, *r = nullptr, *d = nullptr;  // level vectors (level 0: r and d only)
};

struct smm_precond_amg {
	double theta = 0.08, eigRatio = 30.0;
	int maxLevels = 10, coarseRows = 256, smoothDegree = 2;
	std::vector<smm_amg_level> lv;
	void* d_inv = nullptr;  // [nL x nL] row-major, T
	int nL = 0;
	int k = 0, dofsPerNode = 1;  // k > 0: created with k candidates (smm_hip_precond_create_amg_candidates_*)
	void* nextB = nullptr;       // during such a create: B_l of the level about to be made (the level takes it over)
};

namespace smm {

namespace {

constexpr int TPB = 256;
constexpr int AMG_DENSE_LIMIT = 1024;

inline int rowGrid(long long n) { return static_cast<int>(std::max<long long>(1, std::min<long long>((n + TPB - 1LL) / TPB, numCUs() * 8LL))); }

__device__ __forceinline__ unsigned amgHash(unsigned i) {  // the 32-bit murmur3 finaliser of i + 1
	unsigned h = i + 1u;
	h ^= h >> 16;
	h *= 0x85ebca6bu;
	h ^= h >> 13;
	h *= 0xc2b2ae35u;
	h ^= h >> 16;
	return h;
}
__device__ __forceinline__ unsigned long long amgKey(int state, long long i) {
	if (state == 0) return 0ull;
	return (static_cast<unsigned long long>(state - 1) << 63) | (static_cast<unsigned long long>(amgHash(static_cast<unsigned>(i))) << 31) | static_cast<unsigned long long>(i);
}

#define AMG_ROWS(row, n) for (long long row = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; row < (n); row += static_cast<long long>(gridDim.x) * TPB)

template <typename T>
__global__ __launch_bounds__(TPB) void amgStrongKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals,
                                                       const T* __restrict__ diag, double th2, unsigned char* __restrict__ strong) {
	AMG_ROWS(row, n) {
		const double di = fabs(static_cast<double>(diag[row]));
		const double left = th2 * di;
		for (int k = start[row]; k < start[row + 1]; ++k) {
			const int j = positions[k];
			bool s = false;
			if (j != row && static_cast<unsigned>(j) < static_cast<unsigned>(n)) {
				const double a = static_cast<double>(vals[k]);
				s = a * a >= left * fabs(static_cast<double>(diag[j]));
			}
			strong[k] = s ? 1 : 0;
		}
	}
}

__global__ __launch_bounds__(TPB) void amgInitKernel(int n, int* __restrict__ state, unsigned long long* __restrict__ key) {
	AMG_ROWS(row, n) {
		state[row] = 1;
		key[row] = amgKey(1, row);
	}
}

// keyOut[i] = max(keyIn[i], max over the strong neighbours j of keyIn[j])
__global__ __launch_bounds__(TPB) void amgHopKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const unsigned char* __restrict__ strong,
                                                    const unsigned long long* __restrict__ keyIn, unsigned long long* __restrict__ keyOut) {
	AMG_ROWS(row, n) {
		unsigned long long top = keyIn[row];
		for (int k = start[row]; k < start[row + 1]; ++k) {
			if (strong[k]) {
				const unsigned long long other = keyIn[positions[k]];
				top = other > top ? other : top;
			}
		}
		keyOut[row] = top;
	}
}

// an undecided row whose two-hop maximum carries its own index becomes a root; otherwise one whose maximum is a root's becomes a non-root.
// Writes the next round's keys and adds the rows still undecided to *undecided.
__global__ __launch_bounds__(TPB) void amgStateKernel(int n, const unsigned long long* __restrict__ k2, const int* __restrict__ stateIn, int* __restrict__ stateOut,
                                                      unsigned long long* __restrict__ keyOut, int* undecided) {
	int open = 0;
	AMG_ROWS(row, n) {
		int s = stateIn[row];
		if (s == 1) {
			const unsigned long long k = k2[row];
			if (static_cast<long long>(k & 0x7fffffffull) == row) s = 2;
			else if (k >> 63) s = 0;
		}
		stateOut[row] = s;
		keyOut[row] = amgKey(s, row);
		open += s == 1 ? 1 : 0;
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) open += __shfl_xor(open, o, WAVE);
	if ((threadIdx.x & (WAVE - 1)) == 0 && open) atomicAdd(undecided, open);
}

// flag[i] = 1 where pick[i] == want (i < n), flag[n] = 0: scanned over n + 1 items, the last sum is the count
__global__ __launch_bounds__(TPB) void amgFlagKernel(int n, const int* __restrict__ pick, int want, bool negative, int* __restrict__ flag) {
	AMG_ROWS(row, n + 1LL) { flag[row] = row < n && (negative ? pick[row] < 0 : pick[row] == want) ? 1 : 0; }
}

// phase 1: a root takes its number, a non-root the smallest number among the roots in N(i), -1 when there is none
__global__ __launch_bounds__(TPB) void amgPhase1Kernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const unsigned char* __restrict__ strong,
                                                       const int* __restrict__ state, const int* __restrict__ number, int* __restrict__ agg) {
	AMG_ROWS(row, n) {
		int best = 0x7fffffff;
		if (state[row] == 2) {
			best = number[row];
		} else {
			for (int k = start[row]; k < start[row + 1]; ++k) {
				if (strong[k]) {
					const int j = positions[k];
					if (state[j] == 2) best = min(best, number[j]);
				}
			}
		}
		agg[row] = best == 0x7fffffff ? -1 : best;
	}
}

// phase 2, one pass: an unassigned row takes the smallest number among the assigned members of N(i) in aggIn; *assigned counts them
__global__ __launch_bounds__(TPB) void amgPhase2Kernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const unsigned char* __restrict__ strong,
                                                       const int* __restrict__ aggIn, int* __restrict__ aggOut, int* assigned) {
	int got = 0;
	AMG_ROWS(row, n) {
		int mine = aggIn[row];
		if (mine < 0) {
			int best = 0x7fffffff;
			for (int k = start[row]; k < start[row + 1]; ++k) {
				if (strong[k]) {
					const int other = aggIn[positions[k]];
					if (other >= 0) best = min(best, other);
				}
			}
			if (best != 0x7fffffff) {
				mine = best;
				got += 1;
			}
		}
		aggOut[row] = mine;
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) got += __shfl_xor(got, o, WAVE);
	if ((threadIdx.x & (WAVE - 1)) == 0 && got) atomicAdd(assigned, got);
}

// rows still unassigned become aggregates of their own, numbered after the roots in ascending row order
__global__ __launch_bounds__(TPB) void amgLeftKernel(int n, int nRoots, const int* __restrict__ number, int* __restrict__ agg) {
	AMG_ROWS(row, n) {
		if (agg[row] < 0) agg[row] = nRoots + number[row];
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void amgTentativeKernel(int n, int* __restrict__ tstart, T* __restrict__ tval) {
	AMG_ROWS(row, n + 1LL) {
		tstart[row] = static_cast<int>(row);
		if (row < n) tval[row] = T(1);
	}
}

// ---- created with candidates: the node graph, the grouping by aggregate and the QR of every aggregate's block of B_l ----------------------
constexpr int AMG_MAX_K = SMM_AMG_MAX_CANDIDATES;
constexpr int AMG_QR_LDS_ROWS = SMM_AMG_QR_LDS_ROWS;

__device__ __forceinline__ float amgSqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double amgSqrt(double x) { return __builtin_sqrt(x); }

#define AMG_ITEMS(i, count) for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < (count); i += static_cast<long long>(gridDim.x) * TPB)

template <typename T>
__global__ __launch_bounds__(TPB) void amgSquareKernel(long long count, const T* __restrict__ in, T* __restrict__ out) {
	AMG_ITEMS(i, count) out[i] = in[i] * in[i];
}

template <typename T>
__global__ __launch_bounds__(TPB) void amgRootKernel(long long count, T* __restrict__ v) {
	AMG_ITEMS(i, count) v[i] = amgSqrt(v[i]);
}

// Tb, the dof -> node map: n x n / b, one 1 per row at column i / b
template <typename T>
__global__ __launch_bounds__(TPB) void amgNodeMapKernel(int n, int b, int* __restrict__ start, int* __restrict__ positions, T* __restrict__ vals) {
	AMG_ROWS(row, n + 1LL) {
		start[row] = static_cast<int>(row);
		if (row < n) {
			positions[row] = static_cast<int>(row / b);
			vals[row] = T(1);
		}
	}
}

// the stored diagonal entry of every row (0 where a row has none)
template <typename T>
__global__ __launch_bounds__(TPB) void amgDiagKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals, T* __restrict__ diag) {
	AMG_ROWS(row, n) {
		T d = T(0);
		for (int k = start[row]; k < start[row + 1]; ++k) {
			if (positions[k] == row) d = vals[k];
		}
		diag[row] = d;
	}
}

// a dof inherits its node's aggregate; also the identity the stable grouping sorts along
__global__ __launch_bounds__(TPB) void amgInheritKernel(int n, int b, const int* __restrict__ nodeAgg, int* __restrict__ agg) {
	AMG_ROWS(row, n) { agg[row] = nodeAgg[row / b]; }
}
__global__ __launch_bounds__(TPB) void amgIotaKernel(int n, int* __restrict__ out) {
	AMG_ROWS(row, n) { out[row] = static_cast<int>(row); }
}

// bounds[a] = the first position of the sorted aggregate numbers that holds a number >= a (a = 0 .. nAgg)
__global__ __launch_bounds__(TPB) void amgBoundsKernel(int nAgg, int n, const int* __restrict__ sorted, int* __restrict__ bounds) {
	AMG_ROWS(a, nAgg + 1LL) {
		int lo = 0, hi = n;
		while (lo < hi) {
			const int mid = lo + (hi - lo) / 2;
			if (sorted[mid] < a) lo = mid + 1;
			else hi = mid;
		}
		bounds[a] = lo;
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void amgFiniteKernel(long long count, const T* __restrict__ v, int* bad) {
	AMG_ITEMS(i, count) {
		if (!isfinite(v[i])) atomicOr(bad, 1);
	}
}

// The thin QR of every aggregate's block of B_l by modified Gram-Schmidt: G lanes per aggregate (G = 16 / 32 where no aggregate of the
// level has more rows than that, else one wavefront).  Rank r of the aggregate -- its member dofs ascend -- belongs to lane r mod G, which
// alone reads and writes that row of the block: the lanes meet in the inner products only.  An inner product: every lane sums its ranks in
// ascending order from +0.0 with smmFma, then the xor butterfly G / 2 .. 1; with m <= G a lane holds one term and the missing lanes +0.0, so
// the sum is what the 64-lane form gives: a function of m alone.  The block (column c at w + c m) sits in LDS while m <= LROWS and in its
// place in qd otherwise.  Column c: norm0 = |v_c| as gathered; v_c = smmFma(-r_jc, q_j, v_c) for the kept j < c ascending, r_jc =
// q_j . v_c; nrm = |v_c|; kept iff nrm > tol norm0: q_c = v_c / nrm, r_cc = nrm; otherwise q_c = 0 and row c of R stays zero.  R goes to
// rows a k .. of Bnext (zeroed by the caller), Q to qd (aggregate a at qd + start_a k, column-major, leading dimension m).
// Every shuffle is reached by all lanes: the loops over aggregates, c and j are uniform, a group without an aggregate runs them with m = 0.
template <typename T, int G>
__global__ __launch_bounds__(TPB) void amgQrKernel(int nAgg, int k, int n, const int* __restrict__ aggStart, const int* __restrict__ members, const T* __restrict__ B,
                                                   T* __restrict__ qd, T* __restrict__ Bnext, int* __restrict__ keptMask, T tol) {
	constexpr int GROUPS = TPB / G;
	constexpr int LROWS = G == WAVE ? AMG_QR_LDS_ROWS : G;
	__shared__ T lds[GROUPS * LROWS * AMG_MAX_K];
	const int t = threadIdx.x % G;
	const int grp = threadIdx.x / G;
	const size_t ldn = static_cast<size_t>(nAgg) * k;
	for (int first = blockIdx.x * GROUPS; first < nAgg; first += gridDim.x * GROUPS) {
		const int a = first + grp;
		const bool live = a < nAgg;
		const int o = live ? aggStart[a] : 0;
		const int m = live ? aggStart[a + 1] - o : 0;
		const bool inLds = m <= LROWS;
		T* const home = qd + static_cast<size_t>(o) * k;
		T* const w = inLds ? lds + grp * (LROWS * AMG_MAX_K) : home;
		for (int c = 0; c < k; ++c) {
			for (int r = t; r < m; r += G) w[c * m + r] = B[static_cast<size_t>(c) * n + members[o + r]];
		}
		unsigned kept = 0;
		for (int c = 0; c < k; ++c) {
			T* const v = w + c * m;
			T acc = T(0);
			for (int r = t; r < m; r += G) acc = smmFma(v[r], v[r], acc);
			const T norm0 = amgSqrt(groupSum<G>(acc));
			for (int j = 0; j < c; ++j) {
				const T* const q = w + j * m;
				acc = T(0);
				for (int r = t; r < m; r += G) acc = smmFma(q[r], v[r], acc);
				const T rjc = groupSum<G>(acc);
				if ((kept >> j) & 1u) {
					for (int r = t; r < m; r += G) v[r] = smmFma(-rjc, q[r], v[r]);
					if (t == 0) Bnext[static_cast<size_t>(c) * ldn + static_cast<size_t>(a) * k + j] = rjc;
				}
			}
			acc = T(0);
			for (int r = t; r < m; r += G) acc = smmFma(v[r], v[r], acc);
			const T nrm = amgSqrt(groupSum<G>(acc));
			if (nrm > tol * norm0) {
				kept |= 1u << c;
				for (int r = t; r < m; r += G) v[r] = v[r] / nrm;
				if (t == 0) Bnext[static_cast<size_t>(c) * ldn + static_cast<size_t>(a) * k + c] = nrm;
			} else {
				for (int r = t; r < m; r += G) v[r] = T(0);
			}
		}
		if (inLds) {
			for (int c = 0; c < k; ++c) {
				for (int r = t; r < m; r += G) home[c * m + r] = w[c * m + r];
			}
		}
		if (live && t == 0) keptMask[a] = static_cast<int>(kept);
	}
}

// count[i] = the kept columns of row i's aggregate (count[n] = 0): scanned, T's row starts
__global__ __launch_bounds__(TPB) void amgRowCountKernel(int n, const int* __restrict__ agg, const int* __restrict__ keptMask, int* __restrict__ count) {
	AMG_ROWS(row, n + 1LL) { count[row] = row < n ? __popc(static_cast<unsigned>(keptMask[agg[row]])) : 0; }
}

// T's positions and values, one lane per place p of the grouping: row members[p] takes q_c of its aggregate at column a k + c, kept c only
template <typename T>
__global__ __launch_bounds__(TPB) void amgTentativeFillKernel(int n, int k, const int* __restrict__ members, const int* __restrict__ sortedAgg, const int* __restrict__ aggStart,
                                                              const int* __restrict__ keptMask, const int* __restrict__ tstart, const T* __restrict__ qd,
                                                              int* __restrict__ tpos, T* __restrict__ tval) {
	AMG_ROWS(p, n) {
		const int a = sortedAgg[p];
		const int o = aggStart[a];
		const int m = aggStart[a + 1] - o;
		const unsigned kept = static_cast<unsigned>(keptMask[a]);
		int e = tstart[members[p]];
		for (int c = 0; c < k; ++c) {
			if ((kept >> c) & 1u) {
				tpos[e] = a * k + c;
				tval[e] = qd[static_cast<size_t>(o) * k + static_cast<size_t>(c) * m + (p - o)];
				++e;
			}
		}
	}
}

// S = I - omega D^-1 A on A's pattern: s = omega / d_i; off the diagonal -(s a_ij), on it 1 - s a_ii; every operation rounds once
template <typename T>
__global__ __launch_bounds__(TPB) void amgSmootherKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals,
                                                         const T* __restrict__ diag, T omega, T* __restrict__ sval) {
	AMG_ROWS(row, n) {
		const T s = omega / diag[row];
		for (int k = start[row]; k < start[row + 1]; ++k) {
			const T t = s * vals[k];
			sval[k] = positions[k] == row ? T(1) - t : -t;
		}
	}
}

// x = Inv b, one wavefront per row: lane k sums columns k, k + 64, ... in ascending order from +0.0, then the xor butterfly of the dot kernels
template <typename T>
__global__ __launch_bounds__(TPB) void amgDenseKernel(int n, const T* __restrict__ inv, const T* __restrict__ b, T* __restrict__ x, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	const int lane = threadIdx.x & (WAVE - 1);
	constexpr int WAVES = TPB / WAVE;
	for (int row = blockIdx.x * WAVES + (threadIdx.x >> 6); row < n; row += gridDim.x * WAVES) {
		const T* __restrict__ line = inv + static_cast<size_t>(row) * n;
		T acc = T(0);
		for (int c = lane; c < n; c += WAVE) acc = smmFma(line[c], b[c], acc);
		acc = groupSum<WAVE>(acc);
		if (lane == 0) x[row] = acc;
	}
}

// x = x + d
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void amgAddKernel(int n, const T* d, T* x, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	const T* const in[2] = {x, d};
	T* const out[1] = {x};
	streamMap<T, NT, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = v[0] + v[1]; });
}

int readInt(const int* d, int* h, hipStream_t s) {
	SMM_HIP_TRY(hipMemcpyAsync(h, d, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// declared behind the scratch buffers of a set-up stage: unless dismissed (the success path has synchronised already) it drains the stream
// before they go back to the allocator, so an error exit never releases memory that kernels still queued may touch
struct DrainOnExit {
	hipStream_t s;
	bool armed = true;
	explicit DrainOnExit(hipStream_t stream) : s(stream) {}
	~DrainOnExit() {
		if (armed) (void)hipStreamSynchronize(s);
	}
};

smm_hip_stream asHandle(hipStream_t s) { return reinterpret_cast<smm_hip_stream>(s); }

template <typename T>
const T* diagOf(const smm_amg_level& L) { return static_cast<const T*>(L.cheb->d_values); }

int makeSmoother(const smm_precond_amg* G, smm_amg_level& L) {
	if (L.cheb) smm_hip_precond_destroy(L.cheb);
	L.cheb = nullptr;
	SMM_TRY(smm_hip_precond_create_chebyshev(L.A, G->smoothDegree, SMM_CHEB_BOUND_GERSHGORIN, G->eigRatio, 10, 0.0, 0.0, &L.cheb));
	return smm_hip_precond_chebyshev_info(L.cheb, nullptr, nullptr, nullptr, &L.lam);
}

// the aggregates of the graph A (n rows, its diagonal in diag): *outAgg (n + 1 ints, the caller's from then on) and *outCount
template <typename T>
int aggregateGraph(const smm_hip_csr* A, const T* diag, double thetaL, int** outAgg, int* outCount, hipStream_t s) {
	const int n = A->rows, g = rowGrid(n);
	const size_t len = static_cast<size_t>(n) + 1;
	DevBuf<unsigned char> strong;
	DevBuf<int> stateA, stateB, flag, number, aggB, word;
	DevBuf<unsigned long long> keyA, keyB, keyC;
	DrainOnExit drain(s);
	SMM_TRY(strong.alloc(static_cast<size_t>(std::max(1, A->nnz))));
	SMM_TRY(stateA.alloc(len));
	SMM_TRY(stateB.alloc(len));
	SMM_TRY(flag.alloc(len));
	SMM_TRY(number.alloc(len));
	SMM_TRY(aggB.alloc(len));
	SMM_TRY(word.alloc(1));
	SMM_TRY(keyA.alloc(len));
	SMM_TRY(keyB.alloc(len));
	SMM_TRY(keyC.alloc(len));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(outAgg), len * sizeof(int)));
	int* const agg = *outAgg;
	amgStrongKernel<T><<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, static_cast<const T*>(A->d_values), diag, thetaL * thetaL, strong);
	amgInitKernel<<<g, TPB, 0, s>>>(n, stateA, keyA);
	int* stIn = stateA;
	int* stOut = stateB;
	unsigned long long* kIn = keyA;
	unsigned long long* kOut = keyC;
	for (long long round = 0;; ++round) {
		if (round > n) {  // (the undecided row with the largest hash is decided in every round)
			setError("amg: the root selection did not end");
			return SMM_HIP_ERR_PRECOND;
		}
		SMM_HIP_TRY(hipMemsetAsync(word, 0, sizeof(int), s));
		amgHopKernel<<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, strong, kIn, keyB);
		amgHopKernel<<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, strong, keyB, kOut);
		amgStateKernel<<<g, TPB, 0, s>>>(n, kOut, stIn, stOut, kIn, word);  // (kIn is free again: both hops have read it)
		SMM_HIP_TRY(hipGetLastError());
		std::swap(stIn, stOut);
		int open = 0;
		SMM_TRY(readInt(word, &open, s));
		if (open == 0) break;
	}
	const int* state = stIn;
	amgFlagKernel<<<rowGrid(len), TPB, 0, s>>>(n, state, 2, false, flag);
	SMM_TRY(scanExclusive(flag.p, number.p, len, s));
	int nRoots = 0;
	SMM_TRY(readInt(number.p + n, &nRoots, s));
	amgPhase1Kernel<<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, strong, state, number, agg);
	int* aIn = agg;
	int* aOut = aggB;
	for (long long pass = 0; pass <= n; ++pass) {
		SMM_HIP_TRY(hipMemsetAsync(word, 0, sizeof(int), s));
		amgPhase2Kernel<<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, strong, aIn, aOut, word);
		SMM_HIP_TRY(hipGetLastError());
		int got = 0;
		SMM_TRY(readInt(word, &got, s));
		if (got == 0) break;  // (aOut equals aIn)
		std::swap(aIn, aOut);
	}
	if (aIn != agg) SMM_HIP_TRY(hipMemcpyAsync(agg, aIn, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToDevice, s));
	amgFlagKernel<<<rowGrid(len), TPB, 0, s>>>(n, agg, 0, true, flag);
	SMM_TRY(scanExclusive(flag.p, number.p, len, s));
	int left = 0;
	SMM_TRY(readInt(number.p + n, &left, s));
	if (left) amgLeftKernel<<<g, TPB, 0, s>>>(n, nRoots, number, agg);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));  // the scratch arrays go back to the allocator when this scope ends
	drain.armed = false;
	*outCount = nRoots + left;
	return SMM_HIP_OK;
}

// the aggregates of level L: L.d_agg and L.nc
template <typename T>
int aggregate(smm_amg_level& L, double thetaL, hipStream_t s) {
	return aggregateGraph<T>(L.A, diagOf<T>(L), thetaL, &L.d_agg, &L.nc, s);
}

template <typename T>
int createDev(int rows, int cols, const int* start, const int* positions, const T* vals, smm_hip_csr** out) {
	if (std::is_same<T, float>::value) return smm_hip_csr_create_dev_f32(rows, cols, start, positions, reinterpret_cast<const float*>(vals), out);
	return smm_hip_csr_create_dev_f64(rows, cols, start, positions, reinterpret_cast<const double*>(vals), out);
}

// handles of a set-up stage that wrap its scratch arrays: destroyed before those arrays are released
struct ScratchHandles {
	std::vector<smm_hip_csr*> h;
	~ScratchHandles() {
		for (smm_hip_csr* m : h) smm_hip_csr_destroy(m);
	}
	smm_hip_csr** add() {
		h.push_back(nullptr);
		return &h.back();
	}
};

// created with candidates: the dof aggregates of level L (block size b) -- L.d_agg, L.nAgg.  b > 1: the aggregates of the node graph
// N = Tb^T ((A o A) Tb) with the root of every value, N_IJ = the Frobenius norm of block (I, J); a dof inherits its node's aggregate
template <typename T>
int nodeAggregates(smm_amg_level& L, int b, double thetaL, hipStream_t s) {
	if (b == 1) return aggregateGraph<T>(L.A, diagOf<T>(L), thetaL, &L.d_agg, &L.nAgg, s);
	const smm_hip_csr* A = L.A;
	const int n = L.n, nodes = n / b;
	DevBuf<int> mapStart, mapPos, nodeAgg;
	DevBuf<T> ones, squared, diag;
	ScratchHandles tmp;
	tmp.h.reserve(5);
	DrainOnExit drain(s);
	SMM_TRY(mapStart.alloc(static_cast<size_t>(n) + 1));
	SMM_TRY(mapPos.alloc(static_cast<size_t>(n)));
	SMM_TRY(ones.alloc(static_cast<size_t>(n)));
	SMM_TRY(squared.alloc(static_cast<size_t>(std::max(1, A->nnz))));
	SMM_TRY(diag.alloc(static_cast<size_t>(nodes)));
	amgNodeMapKernel<T><<<rowGrid(n + 1LL), TPB, 0, s>>>(n, b, mapStart, mapPos, ones);
	amgSquareKernel<T><<<rowGrid(A->nnz), TPB, 0, s>>>(A->nnz, static_cast<const T*>(A->d_values), squared);
	SMM_HIP_TRY(hipGetLastError());
	smm_hip_csr **A2 = tmp.add(), **Tb = tmp.add(), **TbT = tmp.add(), **A2Tb = tmp.add(), **N = tmp.add();
	SMM_TRY(createDev<T>(n, n, A->d_start, A->d_positions, squared.p, A2));
	SMM_TRY(createDev<T>(n, nodes, mapStart, mapPos, ones.p, Tb));
	SMM_TRY(smm_hip_csr_multiply_create(*A2, *Tb, asHandle(s), A2Tb));
	SMM_TRY(smm_hip_csr_transpose_create(*Tb, asHandle(s), TbT));
	SMM_TRY(smm_hip_csr_multiply_create(*TbT, *A2Tb, asHandle(s), N));
	const smm_hip_csr* g = *N;
	amgRootKernel<T><<<rowGrid(g->nnz), TPB, 0, s>>>(g->nnz, static_cast<T*>(g->d_values));
	amgDiagKernel<T><<<rowGrid(nodes), TPB, 0, s>>>(nodes, g->d_start, g->d_positions, static_cast<const T*>(g->d_values), diag);
	SMM_HIP_TRY(hipGetLastError());
	int* perNode = nullptr;
	const int st = aggregateGraph<T>(g, diag.p, thetaL, &perNode, &L.nAgg, s);
	nodeAgg.p = perNode;  // (released with the other scratch arrays)
	SMM_TRY(st);
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_agg), (static_cast<size_t>(n) + 1) * sizeof(int)));
	amgInheritKernel<<<rowGrid(n), TPB, 0, s>>>(n, b, nodeAgg, L.d_agg);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	return SMM_HIP_OK;
}

template <typename T, int G>
void launchQr(int nAgg, int k, int n, const int* aggStart, const int* members, const T* B, T* qd, T* Bnext, int* keptMask, hipStream_t s) {
	constexpr int GROUPS = TPB / G;
	const int grid = static_cast<int>(std::max<long long>(1, std::min<long long>((nAgg + GROUPS - 1LL) / GROUPS, numCUs() * 8LL)));
	amgQrKernel<T, G><<<grid, TPB, 0, s>>>(nAgg, k, n, aggStart, members, B, qd, Bnext, keptMask, static_cast<T>(SMM_AMG_DROP_TOL));
}

// created with candidates: T of level L (d_tstart, d_tpos, d_tval), *Bnext = B_{l+1} (nc x k, the caller's from then on), L.dropped and E
template <typename T>
int buildTentative(const smm_precond_amg* G, smm_amg_level& L, void** Bnext, hipStream_t s) {
	const int n = L.n, k = G->k, nAgg = L.nAgg;
	const size_t nk = static_cast<size_t>(n) * k, nck = static_cast<size_t>(L.nc) * k;
	DevBuf<int> iota, sortedAgg, members, aggStart, keptMask, count;
	DevBuf<T> qd, next;
	DrainOnExit drain(s);
	SMM_TRY(iota.alloc(static_cast<size_t>(n)));
	SMM_TRY(sortedAgg.alloc(static_cast<size_t>(n)));
	SMM_TRY(members.alloc(static_cast<size_t>(n)));
	SMM_TRY(aggStart.alloc(static_cast<size_t>(nAgg) + 1));
	SMM_TRY(keptMask.alloc(static_cast<size_t>(nAgg)));
	SMM_TRY(count.alloc(static_cast<size_t>(n) + 1));
	SMM_TRY(qd.alloc(nk));
	SMM_TRY(next.alloc(nck));
	// the member dofs of every aggregate in ascending order: a stable sort of the dof numbers by aggregate number
	amgIotaKernel<<<rowGrid(n), TPB, 0, s>>>(n, iota);
	SMM_TRY(sortPairs(L.d_agg, sortedAgg.p, iota.p, members.p, static_cast<size_t>(n), 32u, s));
	amgBoundsKernel<<<rowGrid(nAgg + 1LL), TPB, 0, s>>>(nAgg, n, sortedAgg, aggStart);
	SMM_HIP_TRY(hipGetLastError());
	std::vector<int> bounds(static_cast<size_t>(nAgg) + 1);
	SMM_HIP_TRY(hipMemcpyAsync(bounds.data(), aggStart.p, bounds.size() * sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	int longest = 0;
	for (int a = 0; a < nAgg; ++a) longest = std::max(longest, bounds[static_cast<size_t>(a) + 1] - bounds[static_cast<size_t>(a)]);
	SMM_HIP_TRY(hipMemsetAsync(next.p, 0, std::max<size_t>(nck, 1) * sizeof(T), s));
	const T* B = static_cast<const T*>(L.d_B);
	if (longest <= 16) launchQr<T, 16>(nAgg, k, n, aggStart, members, B, qd, next, keptMask, s);
	else if (longest <= 32) launchQr<T, 32>(nAgg, k, n, aggStart, members, B, qd, next, keptMask, s);
	else launchQr<T, WAVE>(nAgg, k, n, aggStart, members, B, qd, next, keptMask, s);
	amgRowCountKernel<<<rowGrid(n + 1LL), TPB, 0, s>>>(n, L.d_agg, keptMask, count);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_tstart), (static_cast<size_t>(n) + 1) * sizeof(int)));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_tpos), std::max<size_t>(nk, 1) * sizeof(int)));
	SMM_TRY(devAlloc(&L.d_tval, std::max<size_t>(nk, 1) * sizeof(T)));
	SMM_TRY(scanExclusive(count.p, L.d_tstart, static_cast<size_t>(n) + 1, s));
	amgTentativeFillKernel<T><<<rowGrid(n), TPB, 0, s>>>(n, k, members, sortedAgg, aggStart, keptMask, L.d_tstart, qd, L.d_tpos, static_cast<T*>(L.d_tval));
	SMM_HIP_TRY(hipGetLastError());
	std::vector<int> kept(static_cast<size_t>(nAgg));
	SMM_HIP_TRY(hipMemcpyAsync(kept.data(), keptMask.p, kept.size() * sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	// E: a stored 1 on the diagonal of every coarse dof whose column of T is empty
	std::vector<int> start(static_cast<size_t>(L.nc) + 1, 0), pos;
	for (int a = 0; a < nAgg; ++a) {
		for (int c = 0; c < k; ++c) {
			const size_t row = static_cast<size_t>(a) * k + c;
			const bool gone = ((kept[static_cast<size_t>(a)] >> c) & 1) == 0;
			if (gone) pos.push_back(static_cast<int>(row));
			start[row + 1] = static_cast<int>(pos.size());
		}
	}
	L.dropped = static_cast<int>(pos.size());
	if (L.dropped) {
		const std::vector<T> ones(pos.size(), T(1));
		if (std::is_same<T, float>::value) SMM_TRY(smm_hip_csr_create_f32(L.nc, L.nc, start.data(), pos.data(), reinterpret_cast<const float*>(ones.data()), &L.E));
		else SMM_TRY(smm_hip_csr_create_f64(L.nc, L.nc, start.data(), pos.data(), reinterpret_cast<const double*>(ones.data()), &L.E));
	}
	*Bnext = next.detach();
	return SMM_HIP_OK;
}

template <typename T>
int fillSmoother(const smm_amg_level& L, hipStream_t s) {
	const smm_hip_csr* A = L.A;
	const double omega = 4.0 / (3.0 * L.lam);
	amgSmootherKernel<T><<<rowGrid(L.n), TPB, 0, s>>>(L.n, A->d_start, A->d_positions, static_cast<const T*>(A->d_values), diagOf<T>(L), static_cast<T>(omega),
	                                                  static_cast<T*>(L.d_sval));
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// T, S and the four derived matrices of a level whose aggregates are known
template <typename T>
int buildOperators(smm_amg_level& L, hipStream_t s) {
	const smm_hip_csr* A = L.A;
	const int n = L.n;
	if (!L.d_tpos) {  // one 1 per row at the aggregate's column; with candidates buildTentative has written T already
		SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_tstart), (static_cast<size_t>(n) + 1) * sizeof(int)));
		SMM_TRY(devAlloc(&L.d_tval, static_cast<size_t>(std::max(1, n)) * sizeof(T)));
	}
	SMM_TRY(devAlloc(&L.d_sval, static_cast<size_t>(std::max(1, A->nnz)) * sizeof(T)));
	if (!L.d_tpos) amgTentativeKernel<T><<<rowGrid(n + 1LL), TPB, 0, s>>>(n, L.d_tstart, static_cast<T*>(L.d_tval));
	SMM_TRY(fillSmoother<T>(L, s));
	SMM_TRY(createDev<T>(n, L.nc, L.d_tstart, L.d_tpos ? L.d_tpos : L.d_agg, static_cast<const T*>(L.d_tval), &L.Tm));
	SMM_TRY(createDev<T>(n, n, A->d_start, A->d_positions, static_cast<const T*>(L.d_sval), &L.S));
	SMM_TRY(smm_hip_csr_multiply_create(L.S, L.Tm, asHandle(s), &L.P));
	SMM_TRY(smm_hip_csr_transpose_create(L.P, asHandle(s), &L.R));
	SMM_TRY(smm_hip_csr_multiply_create(A, L.P, asHandle(s), &L.AP));
	if (!L.E) return smm_hip_csr_multiply_create(L.R, L.AP, asHandle(s), &L.Anext);
	// a coarse dof whose column of T is empty has an empty row and column in R (A P): it becomes a decoupled identity row
	SMM_TRY(smm_hip_csr_multiply_create(L.R, L.AP, asHandle(s), &L.RAP));
	if (std::is_same<T, float>::value) return smm_hip_csr_add_create_f32(L.RAP, 1.0f, L.E, 1.0f, asHandle(s), &L.Anext);
	return smm_hip_csr_add_create_f64(L.RAP, 1.0, L.E, 1.0, asHandle(s), &L.Anext);
}

template <typename T>
int refreshOperators(smm_amg_level& L, hipStream_t s) {
	SMM_TRY(fillSmoother<T>(L, s));
	if (std::is_same<T, float>::value) {
		SMM_TRY(smm_hip_csr_values_changed_f32(L.S, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.P, L.S, L.Tm, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.AP, L.A, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_transpose_refresh_f32(L.R, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.E ? L.RAP : L.Anext, L.R, L.AP, asHandle(s)));
		if (L.E) SMM_TRY(smm_hip_csr_add_into_f32(L.Anext, L.RAP, 1.0f, L.E, 1.0f, asHandle(s)));
	} else {
		SMM_TRY(smm_hip_csr_values_changed_f64(L.S, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.P, L.S, L.Tm, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.AP, L.A, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_transpose_refresh_f64(L.R, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.E ? L.RAP : L.Anext, L.R, L.AP, asHandle(s)));
		if (L.E) SMM_TRY(smm_hip_csr_add_into_f64(L.Anext, L.RAP, 1.0, L.E, 1.0, asHandle(s)));
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// the coarsest matrix copied to the host, inverted in double by Gauss-Jordan with partial pivoting, rounded to T once
template <typename T>
int coarseInverse(smm_precond_amg* G, hipStream_t s) {
	const smm_hip_csr* A = G->lv.back().A;
	const int n = A->rows;
	G->nL = n;
	if (!G->d_inv) SMM_TRY(devAlloc(&G->d_inv, std::max<size_t>(1, static_cast<size_t>(n) * n) * sizeof(T)));
	if (n == 0) return SMM_HIP_OK;
	std::vector<int> start(static_cast<size_t>(n) + 1), pos(static_cast<size_t>(std::max(1, A->nnz)));
	std::vector<T> val(static_cast<size_t>(std::max(1, A->nnz)));
	SMM_TRY(smm_hip_csr_get_pattern(A, start.data(), pos.data()));
	if (std::is_same<T, float>::value) SMM_TRY(smm_hip_csr_get_values_f32(A, reinterpret_cast<float*>(val.data())));
	else SMM_TRY(smm_hip_csr_get_values_f64(A, reinterpret_cast<double*>(val.data())));
	const size_t w = static_cast<size_t>(n);
	std::vector<double> a(w * w, 0.0), inv(w * w, 0.0);
	for (size_t i = 0; i < w; ++i) {
		inv[i * w + i] = 1.0;
		for (int k = start[i]; k < start[i + 1]; ++k) {
			if (pos[static_cast<size_t>(k)] >= 0 && pos[static_cast<size_t>(k)] < n) a[i * w + static_cast<size_t>(pos[static_cast<size_t>(k)])] += static_cast<double>(val[static_cast<size_t>(k)]);
		}
	}
	for (size_t c = 0; c < w; ++c) {
		size_t p = c;
		for (size_t i = c + 1; i < w; ++i) {
			if (std::fabs(a[i * w + c]) > std::fabs(a[p * w + c])) p = i;
		}
		const double pivot = a[p * w + c];
		if (pivot == 0.0 || !std::isfinite(pivot)) {
			setError("amg: the coarsest matrix (%d rows) is singular or not finite at column %zu", n, c);
			return SMM_HIP_ERR_PRECOND;
		}
		if (p != c) {
			std::swap_ranges(a.begin() + static_cast<long>(p * w), a.begin() + static_cast<long>((p + 1) * w), a.begin() + static_cast<long>(c * w));
			std::swap_ranges(inv.begin() + static_cast<long>(p * w), inv.begin() + static_cast<long>((p + 1) * w), inv.begin() + static_cast<long>(c * w));
		}
		const double scale = 1.0 / pivot;
		for (size_t j = 0; j < w; ++j) {
			a[c * w + j] *= scale;
			inv[c * w + j] *= scale;
		}
		for (size_t i = 0; i < w; ++i) {
			const double f = a[i * w + c];
			if (i == c || f == 0.0) continue;
			for (size_t j = 0; j < w; ++j) {
				a[i * w + j] -= f * a[c * w + j];
				inv[i * w + j] -= f * inv[c * w + j];
			}
		}
	}
	std::vector<T> out(w * w);
	for (size_t k = 0; k < w * w; ++k) out[k] = static_cast<T>(inv[k]);
	SMM_TRY(hostToDev(G->d_inv, out.data(), w * w * sizeof(T), s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template <typename T>
int amgCycle(const smm_precond_amg* G, size_t l, const T* b, T* x, const int* doneFlag, hipStream_t s) {
	const smm_amg_level& L = G->lv[l];
	const int n = L.n;
	if (L.coarsest) {
		amgDenseKernel<T><<<std::max(1, (n + TPB / WAVE - 1) / (TPB / WAVE)), TPB, 0, s>>>(n, static_cast<const T*>(G->d_inv), b, x, doneFlag);
		SMM_HIP_TRY(hipGetLastError());
		return SMM_HIP_OK;
	}
	const smm_amg_level& C = G->lv[l + 1];
	T* r = static_cast<T*>(L.r);
	T* d = static_cast<T*>(L.d);
	T* bc = static_cast<T*>(C.b);
	T* xc = static_cast<T*>(C.x);
	SMM_TRY(chebApplyDev<T>(L.cheb, b, x, doneFlag, s));                                                   // x = M b
	SMM_TRY(launchSpmv<T>(L.A, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, doneFlag, s));                    // r = b - A x
	SMM_TRY(launchSpmv<T>(L.R, SMM_OP_ASSIGN, nullptr, r, bc, 0, nullptr, nullptr, doneFlag, s));          // r_c = R r
	SMM_TRY(amgCycle<T>(G, l + 1, bc, xc, doneFlag, s));                                                   // e_c = V(r_c)
	SMM_TRY(launchSpmv<T>(L.P, SMM_OP_ADD, x, xc, x, 0, nullptr, nullptr, doneFlag, s));                   // x = x + P e_c
	SMM_TRY(launchSpmv<T>(L.A, SMM_OP_SUB, b, x, r, 0, nullptr, nullptr, doneFlag, s));                    // r = b - A x
	SMM_TRY(chebApplyDev<T>(L.cheb, r, d, doneFlag, s));                                                   // d = M r
	SMM_LAUNCH_UPDATE(amgAddKernel, updateNT(n, sizeof(T), 3), solverGrid(n), s, n, d, x, doneFlag);        // x = x + d
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

std::string sizesOf(const smm_precond_amg* G) {
	std::string out;
	for (const smm_amg_level& L : G->lv) out += (out.empty() ? "" : " / ") + std::to_string(L.n);
	return out;
}

template <typename T>
int copyDiagonal(smm_hip_precond* M, hipStream_t s) {
	const smm_amg_level& L = M->amg->lv.front();
	const size_t len = static_cast<size_t>(std::max(1, L.n));
	if (!M->d_values) SMM_TRY(devAlloc(&M->d_values, len * sizeof(T)));
	M->n_values = static_cast<size_t>(L.n);
	if (L.n) SMM_HIP_TRY(hipMemcpyAsync(M->d_values, L.cheb->d_values, static_cast<size_t>(L.n) * sizeof(T), hipMemcpyDeviceToDevice, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

}  // namespace

template <typename T>
int amgApplyDev(const smm_hip_precond* M, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_precond_amg* G = M->amg;
	if (!G || G->lv.empty()) {
		setError("precond_apply: the multigrid preconditioner has no hierarchy");
		return SMM_HIP_ERR_INVALID;
	}
	std::lock_guard<std::mutex> whole(M->enqueueMutex);  // every level's x, b, r, d are the handle's: one cycle's launches stay together
	return amgCycle<T>(G, 0, rhs, x, doneFlag, s);
}

template int amgApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int amgApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void amgDestroy(smm_precond_amg* G) {
	if (!G) return;
	for (smm_amg_level& L : G->lv) {
		smm_hip_precond_destroy(L.cheb);
		smm_hip_csr_destroy(L.S);
		smm_hip_csr_destroy(L.Tm);
		smm_hip_csr_destroy(L.P);
		smm_hip_csr_destroy(L.R);
		smm_hip_csr_destroy(L.AP);
		smm_hip_csr_destroy(L.Anext);
		smm_hip_csr_destroy(L.RAP);
		smm_hip_csr_destroy(L.E);
		devFree(L.d_tpos);
		devFree(L.d_B);
		devFree(L.d_agg);
		devFree(L.d_tstart);
		devFree(L.d_tval);
		devFree(L.d_sval);
		devFree(L.x);
		devFree(L.b);
		devFree(L.r);
		devFree(L.d);
	}
	devFree(G->d_inv);
	devFree(G->nextB);
	delete G;
}

template <typename T>
static int amgCreateTyped(const smm_hip_csr* a, smm_hip_precond* M) {
	smm_precond_amg* G = M->amg;
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());  // the matrix may still be being written on a caller's stream
	const smm_hip_csr* A = a;
	G->lv.reserve(static_cast<size_t>(G->maxLevels));
	for (int l = 0;; ++l) {
		G->lv.emplace_back();
		smm_amg_level& L = G->lv.back();
		L.A = A;
		L.n = A->rows;
		SMM_TRY(ensureCsrReady(A, nullptr, false));
		L.d_B = G->nextB;
		G->nextB = nullptr;
		SMM_TRY(makeSmoother(G, L));
		if (L.n <= G->coarseRows || l + 1 == G->maxLevels) break;
		if (G->k) {  // node aggregates, k coarse dofs for each
			SMM_TRY(nodeAggregates<T>(L, l == 0 ? G->dofsPerNode : G->k, std::ldexp(G->theta, -l), s));
			L.nc = L.nAgg * G->k;  // (at most n k, which the create call has checked)
		} else {
			SMM_TRY(aggregate<T>(L, std::ldexp(G->theta, -l), s));
		}
		if (10LL * L.nc >= 9LL * L.n) {  // the level would not shrink: it is the coarsest
			devFree(L.d_agg);
			L.d_agg = nullptr;
			L.nc = L.nAgg = 0;
			break;
		}
		L.coarsest = false;
		if (G->k) SMM_TRY(buildTentative<T>(G, L, &G->nextB, s));
		SMM_TRY(buildOperators<T>(L, s));
		A = L.Anext;
	}
	if (G->lv.back().n > AMG_DENSE_LIMIT) {
		setError("amg: the coarsest level has %d rows, more than %d (rows per level: %s)", G->lv.back().n, AMG_DENSE_LIMIT, sizesOf(G).c_str());
		return SMM_HIP_ERR_PRECOND;
	}
	SMM_TRY(coarseInverse<T>(G, s));
	for (size_t l = 0; l < G->lv.size(); ++l) {
		smm_amg_level& L = G->lv[l];
		const size_t bytes = static_cast<size_t>(std::max(1, L.n)) * sizeof(T);
		if (l > 0) {
			SMM_TRY(devAlloc(&L.x, bytes));
			SMM_TRY(devAlloc(&L.b, bytes));
		}
		if (!L.coarsest) {
			SMM_TRY(devAlloc(&L.r, bytes));
			SMM_TRY(devAlloc(&L.d, bytes));
		}
	}
	SMM_TRY(copyDiagonal<T>(M, s));
	if (a->rows) {  // one cycle on zeros: whatever a level's SpMV builds on first use is built here, not inside a solver's loop
		DevBuf<T> zero, out;
		SMM_TRY(zero.alloc(static_cast<size_t>(a->rows)));
		SMM_TRY(out.alloc(static_cast<size_t>(a->rows)));
		SMM_HIP_TRY(hipMemsetAsync(zero, 0, static_cast<size_t>(a->rows) * sizeof(T), s));
		SMM_TRY(amgCycle<T>(G, 0, zero.p, out.p, nullptr, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	return SMM_HIP_OK;
}

template <typename T>
static int amgRefreshTyped(smm_hip_precond* M) {
	smm_precond_amg* G = M->amg;
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());
	for (smm_amg_level& L : G->lv) {
		SMM_TRY(makeSmoother(G, L));
		if (!L.coarsest) SMM_TRY(refreshOperators<T>(L, s));
	}
	SMM_TRY(coarseInverse<T>(G, s));
	return copyDiagonal<T>(M, s);
}

}  // namespace smm

using namespace smm;

static const smm_precond_amg* amgOf(const smm_hip_precond* M, const char* who) {
	if (!M || M->kind != SMM_PRECOND_AMG || !M->amg || M->amg->lv.empty()) {
		setError("%s: not a multigrid (AMG) preconditioner", who);
		return nullptr;
	}
	return M->amg;
}

// what both ways of creating the kind check, in the order smm_hip_precond_create_amg always had
static int amgCheckParameters(const smm_hip_csr* a, double theta, int max_levels, int coarse_rows, int smooth_degree, double eig_ratio) {
	if (!(theta >= 0.0 && theta < 1.0)) {  // (a NaN fails both)
		setError("precond_create_amg: theta must be in [0, 1)");
		return SMM_HIP_ERR_INVALID;
	}
	if (max_levels < 1 || max_levels > SMM_AMG_MAX_LEVELS) {
		setError("precond_create_amg: max_levels must be 1 .. %d", SMM_AMG_MAX_LEVELS);
		return SMM_HIP_ERR_INVALID;
	}
	if (coarse_rows < 1 || coarse_rows > SMM_AMG_MAX_COARSE_ROWS) {
		setError("precond_create_amg: coarse_rows must be 1 .. %d", SMM_AMG_MAX_COARSE_ROWS);
		return SMM_HIP_ERR_INVALID;
	}
	if (smooth_degree < 0 || smooth_degree > SMM_CHEB_MAX_DEGREE) {
		setError("precond_create_amg: smooth_degree must be 0 .. %d", SMM_CHEB_MAX_DEGREE);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("preconditioner needs a square matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (!(eig_ratio > 1.0 && std::isfinite(eig_ratio))) {
		setError("precond_create_amg: eig_ratio must be finite and > 1");
		return SMM_HIP_ERR_PRECOND;
	}
	return SMM_HIP_OK;
}

static smm_hip_precond* amgNewHandle(const smm_hip_csr* a, double theta, int max_levels, int coarse_rows, int smooth_degree, double eig_ratio) {
	auto* M = new smm_hip_precond();
	M->kind = SMM_PRECOND_AMG;
	M->dtype = a->dtype;
	M->a = a;
	M->amg = new smm_precond_amg();
	M->amg->theta = theta;
	M->amg->maxLevels = max_levels;
	M->amg->coarseRows = coarse_rows;
	M->amg->smoothDegree = smooth_degree;
	M->amg->eigRatio = eig_ratio;
	return M;
}

// B: n x k column-major, on the host or (onDevice) in device memory in use on `stream`
template <typename T>
static int amgCreateWithCandidates(const smm_hip_csr* a, const T* B, bool onDevice, hipStream_t stream, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                   int smooth_degree, double eig_ratio, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_amg_candidates: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (a->dtype != dtypeOf<T>()) {
		setError("precond_create_amg_candidates: the matrix has the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (k < 1 || k > SMM_AMG_MAX_CANDIDATES || dofs_per_node < 1 || dofs_per_node > SMM_AMG_MAX_DOFS_PER_NODE) {
		setError("precond_create_amg_candidates: k must be 1 .. %d and dofs_per_node 1 .. %d", SMM_AMG_MAX_CANDIDATES, SMM_AMG_MAX_DOFS_PER_NODE);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(amgCheckParameters(a, theta, max_levels, coarse_rows, smooth_degree, eig_ratio));
	const size_t count = static_cast<size_t>(a->rows) * static_cast<size_t>(k);
	if (a->rows % dofs_per_node != 0 || count > 0x7fffffffULL || (count && !B)) {
		setError("precond_create_amg_candidates: %d rows with %d dofs per node and %d candidates (the rows must be whole nodes, rows * k below 2^31, B not null)", a->rows,
		         dofs_per_node, k);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	hipStream_t s = libStream();
	DevBuf<T> own;
	DevBuf<int> bad;
	SMM_TRY(own.alloc(count));
	SMM_TRY(bad.alloc(1));
	if (count) {
		if (onDevice) {
			SMM_HIP_TRY(hipMemcpyAsync(own.p, B, count * sizeof(T), hipMemcpyDeviceToDevice, stream));
			SMM_HIP_TRY(hipStreamSynchronize(stream));
		} else {
			SMM_TRY(hostToDev(own.p, B, count * sizeof(T), s));
		}
	}
	SMM_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), s));
	amgFiniteKernel<T><<<rowGrid(static_cast<long long>(count)), TPB, 0, s>>>(static_cast<long long>(count), own.p, bad.p);
	SMM_HIP_TRY(hipGetLastError());
	int notFinite = 0;
	SMM_TRY(readInt(bad.p, &notFinite, s));
	if (notFinite) {
		setError("precond_create_amg_candidates: B holds a value that is not finite");
		return SMM_HIP_ERR_INVALID;
	}
	smm_hip_precond* M = amgNewHandle(a, theta, max_levels, coarse_rows, smooth_degree, eig_ratio);
	M->amg->k = k;
	M->amg->dofsPerNode = dofs_per_node;
	M->amg->nextB = own.detach();
	const int st = amgCreateTyped<T>(a, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

template <typename T>
static int amgCandidatesOf(const smm_hip_precond* M, int level, T* b_l, size_t count, int* k, int* dropped, smm_hip_csr** t_l) {
	const smm_precond_amg* G = amgOf(M, "precond_amg_candidates");
	if (!G) return SMM_HIP_ERR_INVALID;
	if (G->k == 0 || M->dtype != dtypeOf<T>()) {
		setError("precond_amg_candidates: not created with candidates, or the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (level < 0 || static_cast<size_t>(level) >= G->lv.size()) {
		setError("precond_amg_candidates: level %d of %zu", level, G->lv.size());
		return SMM_HIP_ERR_INVALID;
	}
	const smm_amg_level& L = G->lv[static_cast<size_t>(level)];
	if (count > static_cast<size_t>(L.n) * static_cast<size_t>(G->k) || (count && !b_l)) {
		setError("precond_amg_candidates: level %d has %d x %d values", level, L.n, G->k);
		return SMM_HIP_ERR_INVALID;
	}
	if (k) *k = G->k;
	if (dropped) *dropped = L.dropped;
	if (t_l) *t_l = L.Tm;
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	if (count) SMM_HIP_TRY(hipMemcpyAsync(b_l, L.d_B, count * sizeof(T), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

extern "C" {

int smm_hip_precond_create_amg(const smm_hip_csr* a, double theta, int max_levels, int coarse_rows, int smooth_degree, double eig_ratio, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_amg: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(amgCheckParameters(a, theta, max_levels, coarse_rows, smooth_degree, eig_ratio));
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	smm_hip_precond* M = amgNewHandle(a, theta, max_levels, coarse_rows, smooth_degree, eig_ratio);
	const int st = a->dtype == SMM_DTYPE_F32 ? amgCreateTyped<float>(a, M) : amgCreateTyped<double>(a, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

int smm_hip_precond_create_amg_candidates_f32(const smm_hip_csr* a, const float* B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows, int smooth_degree,
                                              double eig_ratio, smm_hip_precond** out) {
	return amgCreateWithCandidates<float>(a, B, false, nullptr, k, dofs_per_node, theta, max_levels, coarse_rows, smooth_degree, eig_ratio, out);
}
int smm_hip_precond_create_amg_candidates_f64(const smm_hip_csr* a, const double* B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows, int smooth_degree,
                                              double eig_ratio, smm_hip_precond** out) {
	return amgCreateWithCandidates<double>(a, B, false, nullptr, k, dofs_per_node, theta, max_levels, coarse_rows, smooth_degree, eig_ratio, out);
}
int smm_hip_precond_create_amg_candidates_dev_f32(const smm_hip_csr* a, const float* d_B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                                  int smooth_degree, double eig_ratio, smm_hip_stream stream, smm_hip_precond** out) {
	return amgCreateWithCandidates<float>(a, d_B, true, reinterpret_cast<hipStream_t>(stream), k, dofs_per_node, theta, max_levels, coarse_rows, smooth_degree, eig_ratio, out);
}
int smm_hip_precond_create_amg_candidates_dev_f64(const smm_hip_csr* a, const double* d_B, int k, int dofs_per_node, double theta, int max_levels, int coarse_rows,
                                                  int smooth_degree, double eig_ratio, smm_hip_stream stream, smm_hip_precond** out) {
	return amgCreateWithCandidates<double>(a, d_B, true, reinterpret_cast<hipStream_t>(stream), k, dofs_per_node, theta, max_levels, coarse_rows, smooth_degree, eig_ratio, out);
}
int smm_hip_precond_amg_candidates_f32(const smm_hip_precond* M, int level, float* b_l, size_t count, int* k, int* dropped, smm_hip_csr** t_l) {
	return amgCandidatesOf<float>(M, level, b_l, count, k, dropped, t_l);
}
int smm_hip_precond_amg_candidates_f64(const smm_hip_precond* M, int level, double* b_l, size_t count, int* k, int* dropped, smm_hip_csr** t_l) {
	return amgCandidatesOf<double>(M, level, b_l, count, k, dropped, t_l);
}

int smm_hip_precond_amg_refresh(smm_hip_precond* M) {
	if (!amgOf(M, "precond_amg_refresh")) return SMM_HIP_ERR_INVALID;
	SMM_TRY(ensureInit());
	return M->dtype == SMM_DTYPE_F32 ? amgRefreshTyped<float>(M) : amgRefreshTyped<double>(M);
}

int smm_hip_precond_amg_info(const smm_hip_precond* M, int* levels, int* rows, int* nnz, size_t count, double* operator_complexity) {
	const smm_precond_amg* G = amgOf(M, "precond_amg_info");
	if (!G) return SMM_HIP_ERR_INVALID;
	if (levels) *levels = static_cast<int>(G->lv.size());
	double total = 0.0;
	for (size_t l = 0; l < G->lv.size(); ++l) {
		if (rows && l < count) rows[l] = G->lv[l].n;
		if (nnz && l < count) nnz[l] = G->lv[l].A->nnz;
		total += static_cast<double>(G->lv[l].A->nnz);
	}
	if (operator_complexity) *operator_complexity = total / static_cast<double>(std::max(1, G->lv[0].A->nnz));
	return SMM_HIP_OK;
}

int smm_hip_precond_amg_level(const smm_hip_precond* M, int level, smm_hip_csr** a_l, smm_hip_csr** p_l, smm_hip_csr** r_l) {
	const smm_precond_amg* G = amgOf(M, "precond_amg_level");
	if (!G) return SMM_HIP_ERR_INVALID;
	if (level < 0 || static_cast<size_t>(level) >= G->lv.size()) {
		setError("precond_amg_level: level %d of %zu", level, G->lv.size());
		return SMM_HIP_ERR_INVALID;
	}
	const smm_amg_level& L = G->lv[static_cast<size_t>(level)];
	if (a_l) *a_l = const_cast<smm_hip_csr*>(L.A);
	if (p_l) *p_l = L.P;
	if (r_l) *r_l = L.R;
	return SMM_HIP_OK;
}

int smm_hip_precond_amg_aggregates(const smm_hip_precond* M, int level, int* agg, size_t count) {
	const smm_precond_amg* G = amgOf(M, "precond_amg_aggregates");
	if (!G) return SMM_HIP_ERR_INVALID;
	if (level < 0 || static_cast<size_t>(level) >= G->lv.size() || G->lv[static_cast<size_t>(level)].coarsest) {
		setError("precond_amg_aggregates: level %d has no aggregates (%zu levels, the coarsest has none)", level, G->lv.size());
		return SMM_HIP_ERR_INVALID;
	}
	const smm_amg_level& L = G->lv[static_cast<size_t>(level)];
	if (!agg || count > static_cast<size_t>(L.n)) {
		setError("precond_amg_aggregates: level %d has %d rows", level, L.n);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	if (count) SMM_HIP_TRY(hipMemcpyAsync(agg, L.d_agg, count * sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

static int amgInverseHost(const smm_hip_precond* M, int dtype, void* out, size_t count, size_t elem) {
	const smm_precond_amg* G = amgOf(M, "precond_amg_coarse_inverse");
	if (!G) return SMM_HIP_ERR_INVALID;
	const size_t have = static_cast<size_t>(G->nL) * static_cast<size_t>(G->nL);
	if (M->dtype != dtype || !out || count > have) {
		setError("precond_amg_coarse_inverse: dtype mismatch, null pointer or more than %zu values asked", have);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	if (count) SMM_HIP_TRY(hipMemcpyAsync(out, G->d_inv, count * elem, hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

int smm_hip_precond_amg_coarse_inverse_f32(const smm_hip_precond* M, float* out, size_t count) { return amgInverseHost(M, SMM_DTYPE_F32, out, count, sizeof(float)); }
int smm_hip_precond_amg_coarse_inverse_f64(const smm_hip_precond* M, double* out, size_t count) { return amgInverseHost(M, SMM_DTYPE_F64, out, count, sizeof(double)); }

}  // extern "C"
