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
// The cycle (amgCycle) is launches only: per level two smoother applies, two residual SpMVs with A_l, one SpMV with R_l, one with P_l and
// one x += d pass; the coarsest level is one launch, one wavefront per row.  Every launch takes the solver's done flag.  All level vectors
// belong to the handle: one handle serves one stream at a time.  Traffic per cycle: DESIGN.md section 3.14.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

struct smm_amg_level {
	const smm_hip_csr* A = nullptr;  // level 0: the caller's matrix; deeper: Anext of the level above (owned there)
	int n = 0, nc = 0;
	bool coarsest = true;
	smm_hip_precond* cheb = nullptr;  // the smoother; its d_values is the diagonal copy
	double lam = 0.0;
	int* d_agg = nullptr;      // [n] aggregate numbers = T's positions
	int* d_tstart = nullptr;   // [n + 1] 0 .. n
	void* d_tval = nullptr;    // [n] ones
	void* d_sval = nullptr;    // [nnz] S on A's pattern
	smm_hip_csr *S = nullptr, *Tm = nullptr, *P = nullptr, *R = nullptr, *AP = nullptr, *Anext = nullptr;
	void *x = nullptr, *b = nullptr, *r = nullptr, *d = nullptr;  // level vectors (level 0: r and d only)
};

struct smm_precond_amg {
	double theta = 0.08, eigRatio = 30.0;
	int maxLevels = 10, coarseRows = 256, smoothDegree = 2;
	std::vector<smm_amg_level> lv;
	void* d_inv = nullptr;  // [nL x nL] row-major, T
	int nL = 0;
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

int scanExclusive(const int* in, int* out, size_t count, hipStream_t s) {
	size_t bytes = 0;
	SMM_HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, count, rocprim::plus<int>(), s));
	DevBuf<unsigned char> temp;
	SMM_TRY(temp.alloc(std::max<size_t>(bytes, 1)));
	SMM_HIP_TRY(rocprim::exclusive_scan(temp.p, bytes, in, out, 0, count, rocprim::plus<int>(), s));
	return SMM_HIP_OK;
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

// the aggregates of level L: L.d_agg and L.nc
template <typename T>
int aggregate(smm_amg_level& L, double thetaL, hipStream_t s) {
	const smm_hip_csr* A = L.A;
	const int n = L.n, g = rowGrid(n);
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
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_agg), len * sizeof(int)));
	amgStrongKernel<T><<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, static_cast<const T*>(A->d_values), diagOf<T>(L), thetaL * thetaL, strong);
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
	SMM_TRY(scanExclusive(flag, number, len, s));
	int nRoots = 0;
	SMM_TRY(readInt(number.p + n, &nRoots, s));
	amgPhase1Kernel<<<g, TPB, 0, s>>>(n, A->d_start, A->d_positions, strong, state, number, L.d_agg);
	int* aIn = L.d_agg;
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
	if (aIn != L.d_agg) SMM_HIP_TRY(hipMemcpyAsync(L.d_agg, aIn, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToDevice, s));
	amgFlagKernel<<<rowGrid(len), TPB, 0, s>>>(n, L.d_agg, 0, true, flag);
	SMM_TRY(scanExclusive(flag, number, len, s));
	int left = 0;
	SMM_TRY(readInt(number.p + n, &left, s));
	if (left) amgLeftKernel<<<g, TPB, 0, s>>>(n, nRoots, number, L.d_agg);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));  // the scratch arrays go back to the allocator when this scope ends
	drain.armed = false;
	L.nc = nRoots + left;
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
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&L.d_tstart), (static_cast<size_t>(n) + 1) * sizeof(int)));
	SMM_TRY(devAlloc(&L.d_tval, static_cast<size_t>(std::max(1, n)) * sizeof(T)));
	SMM_TRY(devAlloc(&L.d_sval, static_cast<size_t>(std::max(1, A->nnz)) * sizeof(T)));
	amgTentativeKernel<T><<<rowGrid(n + 1LL), TPB, 0, s>>>(n, L.d_tstart, static_cast<T*>(L.d_tval));
	SMM_TRY(fillSmoother<T>(L, s));
	if (std::is_same<T, float>::value) {
		SMM_TRY(smm_hip_csr_create_dev_f32(n, L.nc, L.d_tstart, L.d_agg, static_cast<const float*>(L.d_tval), &L.Tm));
		SMM_TRY(smm_hip_csr_create_dev_f32(n, n, A->d_start, A->d_positions, static_cast<const float*>(L.d_sval), &L.S));
	} else {
		SMM_TRY(smm_hip_csr_create_dev_f64(n, L.nc, L.d_tstart, L.d_agg, static_cast<const double*>(L.d_tval), &L.Tm));
		SMM_TRY(smm_hip_csr_create_dev_f64(n, n, A->d_start, A->d_positions, static_cast<const double*>(L.d_sval), &L.S));
	}
	SMM_TRY(smm_hip_csr_multiply_create(L.S, L.Tm, asHandle(s), &L.P));
	SMM_TRY(smm_hip_csr_transpose_create(L.P, asHandle(s), &L.R));
	SMM_TRY(smm_hip_csr_multiply_create(A, L.P, asHandle(s), &L.AP));
	SMM_TRY(smm_hip_csr_multiply_create(L.R, L.AP, asHandle(s), &L.Anext));
	return SMM_HIP_OK;
}

template <typename T>
int refreshOperators(smm_amg_level& L, hipStream_t s) {
	SMM_TRY(fillSmoother<T>(L, s));
	if (std::is_same<T, float>::value) {
		SMM_TRY(smm_hip_csr_values_changed_f32(L.S, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.P, L.S, L.Tm, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.AP, L.A, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_transpose_refresh_f32(L.R, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f32(L.Anext, L.R, L.AP, asHandle(s)));
	} else {
		SMM_TRY(smm_hip_csr_values_changed_f64(L.S, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.P, L.S, L.Tm, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.AP, L.A, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_transpose_refresh_f64(L.R, L.P, asHandle(s)));
		SMM_TRY(smm_hip_csr_multiply_into_f64(L.Anext, L.R, L.AP, asHandle(s)));
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
		SMM_TRY(makeSmoother(G, L));
		if (L.n <= G->coarseRows || l + 1 == G->maxLevels) break;
		SMM_TRY(aggregate<T>(L, std::ldexp(G->theta, -l), s));
		if (10LL * L.nc >= 9LL * L.n) {  // the level would not shrink: it is the coarsest
			devFree(L.d_agg);
			L.d_agg = nullptr;
			L.nc = 0;
			break;
		}
		L.coarsest = false;
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

extern "C" {

int smm_hip_precond_create_amg(const smm_hip_csr* a, double theta, int max_levels, int coarse_rows, int smooth_degree, double eig_ratio, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_amg: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
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
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
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
	const int st = a->dtype == SMM_DTYPE_F32 ? amgCreateTyped<float>(a, M) : amgCreateTyped<double>(a, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
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
