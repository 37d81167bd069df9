// smm_precond_ainv.hip -- FSAI and SPAI: preconditioners that ARE sparse matrices, built on the device (additions, no counterpart in the
// reference).  An apply is the library's SpMV (FSAI: w = G r, z = Gt w; SPAI: z = M r): no dependency chain, no level count.
// include/smm_hip.h (SMM_PRECOND_FSAI) states the definition in words, tests/ainv_restatement.py line by line.
//
// Set-up = one small dense SPD system per row i on the columns J_i of that row of the pattern (a, or the structural power of a):
//   FSAI  a[J, J] y = e_last,            row i of G = y / sqrt(y_last)      (J = the columns <= i)
//   SPAI  (a a^T)[J, J] y = (a^T)[i, J], row i of M = y                     (the normal equations of min || e_i^T - m a[J, :] ||)
// What is new here is ainvSolveKernel: ONE launch over all rows; a system is gathered from CSR into a packed lower triangle in LDS and
// solved there by a right-looking Cholesky factorisation and two substitutions.  Every entry is updated in ascending j and nothing is
// reduced, so spreading the rows i of a system over lanes gives the bits of the sequential loops whatever the lane count.
//   - A system of n unknowns runs on a sub-group of L = 8, 16, 32 or 64 lanes (the smallest L >= the longest row of the pattern), 64 / L
//     systems per wavefront; a workgroup is ONE wavefront, so its barriers cost nothing and LDS per workgroup is at most 17 KB (fp64, L = 64).
//   - Lane i owns row i of the triangle.  The column reads S[i][j] at fixed j hit the addresses i (i + 1) / 2 + j: the stride between
//     neighbouring lanes is i + 1, not a power of two, so the packed layout itself spreads a column over the banks (no padding); the
//     reads S[k][j] of the update and S[j][i] of the back substitution are one address for the whole sub-group / consecutive addresses.
//   - The loops over j run to the longest system of the WAVEFRONT with the shorter sub-groups predicated off, so every barrier and every
//     shuffle sits in wave-uniform control flow.
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <type_traits>

#include "smm_csr_build.h"
#include "smm_device.h"

// the state of one FSAI / SPAI handle, behind the public handle (whose d_values are G's / M's values: nnz of them)
struct smm_precond_ainv {
	int power = 1;
	int maxRow = 0;  // the longest row of the pattern J
	int tier = 8;    // lanes per system of the set-up kernel
	int* d_gstart = nullptr;  // the pattern J as CSR arrays, owned; G wraps them and the handle's d_values
	int* d_gpos = nullptr;
	smm_hip_csr* G = nullptr;   // FSAI: G; SPAI: M
	smm_hip_csr* Gt = nullptr;  // FSAI: G^T; SPAI: null
	smm_hip_csr* At = nullptr;  // SPAI: a^T and N = a a^T, kept for the refresh
	smm_hip_csr* N = nullptr;
	unsigned char* d_asc = nullptr;  // per row of the source (a or N): 1 when its columns ascend strictly (then no column is stored twice)
	void* d_w = nullptr;             // FSAI: w = G r of an apply in flight: ONE per handle, so a handle serves one stream at a time
};

namespace smm {
namespace {

constexpr int TPB = 256;

inline int rowGrid(long long n) { return static_cast<int>(std::max<long long>(1, std::min<long long>((n + TPB - 1LL) / TPB, numCUs() * 8LL))); }
smm_hip_stream asHandle(hipStream_t s) { return reinterpret_cast<smm_hip_stream>(s); }

// the next distinct column of row [b, e) above `last` (and, LOWER, not above `row`); INT_MAX when there is none
template <bool LOWER>
__device__ __forceinline__ int nextColumn(const int* __restrict__ positions, int b, int e, int row, int last) {
	int best = INT_MAX;
	for (int k = b; k < e; ++k) {
		const int c = positions[k];
		if (c > last && c < best && (!LOWER || c <= row)) best = c;
	}
	return best;
}

// words: [0] smallest row with a column outside [0, n), [1] smallest row without its diagonal, [2] smallest row longer than SMM_AINV_MAX_ROW
// (INT_MAX: none), [3] the longest row.  lens[i] = |J_i| (a row whose columns do not ascend and that holds more than 64 distinct ones is
// counted by its stored entries), lens[n] = 0; *total = the sum.  asc[i]: the columns of row i ascend strictly.
template <bool LOWER>
__global__ __launch_bounds__(TPB) void ainvCountKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, int* __restrict__ lens,
                                                       unsigned long long* total, int* words) {
	int longest = 0;
	unsigned long long sum = 0ull;
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i <= n; i += static_cast<long long>(gridDim.x) * TPB) {
		if (i == n) {
			lens[n] = 0;
			continue;
		}
		const int row = static_cast<int>(i);
		const int b = start[row], e = start[row + 1];
		bool ascending = true, inside = true, diag = false;
		int kept = 0, prev = -1;
		for (int k = b; k < e; ++k) {
			const int c = positions[k];
			inside = inside && c >= 0 && c < n;
			ascending = ascending && c > prev;
			prev = c;
			diag = diag || c == row;
			if (!LOWER || c <= row) ++kept;
		}
		int len = kept;
		if (!ascending && inside) {  // distinct columns by selection, at most SMM_AINV_MAX_ROW + 1 rounds
			len = 0;
			int last = -1;
			while (len <= SMM_AINV_MAX_ROW) {
				last = nextColumn<LOWER>(positions, b, e, row, last);
				if (last == INT_MAX) break;
				++len;
			}
			if (len > SMM_AINV_MAX_ROW) len = kept;
		}
		if (!inside) atomicMin(words + 0, row);
		else if (!diag) atomicMin(words + 1, row);
		else if (len > SMM_AINV_MAX_ROW) atomicMin(words + 2, row);
		lens[row] = len;
		longest = max(longest, len);
		sum += static_cast<unsigned long long>(len);
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) {
		longest = max(longest, __shfl_xor(longest, o, WAVE));
		sum += __shfl_xor(sum, o, WAVE);
	}
	if ((threadIdx.x & (WAVE - 1)) == 0 && longest > 0) atomicMax(words + 3, longest);
	if ((threadIdx.x & (WAVE - 1)) == 0 && sum != 0ull) atomicAdd(total, sum);  // (in 64 bits: the int scan that follows is only run when this fits)
}

// gpos[gstart[i] ..) = J_i, ascending and without repetition (every row passed ainvCountKernel: gstart[i + 1] - gstart[i] = |J_i| <= 64)
template <bool LOWER>
__global__ __launch_bounds__(TPB) void ainvFillKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const int* __restrict__ gstart,
                                                      int* __restrict__ gpos) {
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		const int row = static_cast<int>(i);
		const int b = start[row], e = start[row + 1];
		const int gb = gstart[row], len = gstart[row + 1] - gb;
		int last = -1;
		for (int t = 0; t < len; ++t) {
			last = nextColumn<LOWER>(positions, b, e, row, last);
			gpos[gb + t] = last;
		}
	}
}

// asc[i] = 1 when the columns of row i ascend strictly
__global__ __launch_bounds__(TPB) void ainvAscendKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, unsigned char* __restrict__ asc) {
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		bool ascending = true;
		int prev = -1;
		for (int k = start[i]; k < start[i + 1]; ++k) {
			ascending = ascending && positions[k] > prev;
			prev = positions[k];
		}
		asc[i] = ascending ? 1 : 0;
	}
}

// position of column c in J[0 .. n) (ascending, distinct), or -1
__device__ __forceinline__ int findInJ(const int* J, int n, int c) {
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (J[mid] < c) lo = mid + 1;
		else hi = mid;
	}
	return lo < n && J[lo] == c ? lo : -1;
}

__device__ __forceinline__ int tri(int i) { return (i * (i + 1)) >> 1; }

// One system per sub-group of L lanes, 64 / L systems per one-wavefront workgroup.  src = a (FSAI) or N = a a^T (SPAI); at = a^T (SPAI).
// errRow: the smallest row whose factorisation met a pivot that is not > 0 or not finite (atomic min).
template <typename T, int L, bool SPAI>
__global__ __launch_bounds__(WAVE) void ainvSolveKernel(int rows, const int* __restrict__ gstart, const int* __restrict__ gpos, T* __restrict__ gval,
                                                        const int* __restrict__ sStart, const int* __restrict__ sPos, const T* __restrict__ sVal,
                                                        const unsigned char* __restrict__ sAsc, const int* __restrict__ tStart, const int* __restrict__ tPos,
                                                        const T* __restrict__ tVal, int* errRow) {
	constexpr int G = WAVE / L, TRI = L * (L + 1) / 2;
	__shared__ T tile[G][TRI];
	__shared__ int cols[G][L];
	const int g = threadIdx.x / L, l = threadIdx.x % L;
	T* const S = tile[g];
	int* const J = cols[g];
	for (long long base = static_cast<long long>(blockIdx.x) * G; base < rows; base += static_cast<long long>(gridDim.x) * G) {  // (wave-uniform)
		const long long row = base + g;
		const bool live = row < rows;
		const int gb = live ? gstart[row] : 0;
		const int n = live ? min(gstart[row + 1] - gb, L) : 0;  // (the launch's L covers the longest row; the clamp keeps LDS in bounds regardless)
		if (l < n) J[l] = gpos[gb + l];
		for (int t = l; t < tri(n); t += L) S[t] = T(0);  // look() of an entry that is not stored: +0.0
		__syncthreads();
		// gather: row J[p] of the source in stored order, each entry placed by a search in J; the first stored entry of a column wins
		for (int p = 0; p < n; ++p) {
			const int r = J[p];
			const int rb = sStart[r], re = sStart[r + 1];
			if (sAsc[r]) {  // no column twice: the lanes share the row
				for (int k = rb + l; k < re; k += L) {
					const int c = sPos[k];
					if (c > r) break;  // the upper triangle is never read
					const int q = findInJ(J, n, c);
					if (q >= 0) S[tri(p) + q] = sVal[k];
				}
			} else if (l == 0) {  // one lane walks the row and remembers the columns it has placed
				unsigned long long placed = 0ull;
				for (int k = rb; k < re; ++k) {
					const int c = sPos[k];
					if (c > r) continue;
					const int q = findInJ(J, n, c);
					if (q >= 0 && !((placed >> q) & 1ull)) {
						S[tri(p) + q] = sVal[k];
						placed |= 1ull << q;
					}
				}
			}
		}
		// the right-hand side, b[l] in lane l
		T breg = T(0);
		if (SPAI) {
			if (l < n) {
				const int want = J[l];
				for (int k = tStart[row]; k < tStart[row + 1]; ++k) {
					if (tPos[k] == want) {
						breg = tVal[k];
						break;
					}
				}
			}
		} else if (l == n - 1) {
			breg = T(1);
		}
		int nmax = n;
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, WAVE));
		__syncthreads();
		// S = C C^T, right-looking: column j is scaled, then taken out of every later entry of the rows below
		bool failed = false;
		const bool mine = l < n;
		for (int j = 0; j < nmax; ++j) {
			const bool on = j < n;
			const T d = on ? S[tri(j) + j] : T(1);
			if (on && !(d > T(0) && d <= std::numeric_limits<T>::max())) failed = true;
			const T root = sqrt(d);
			T lij = T(0);
			if (on && mine && l > j) {
				lij = S[tri(l) + j] / root;
				S[tri(l) + j] = lij;
			}
			__syncthreads();
			if (on && l == j) S[tri(j) + j] = root;  // (behind the barrier: every lane has read d; nobody reads S[j][j] again before the step's last barrier)
			if (on && mine && l > j) {
				for (int k = j + 1; k <= l; ++k) S[tri(l) + k] = smmFma(-lij, S[tri(k) + j], S[tri(l) + k]);
			}
			__syncthreads();
		}
		const T dl = mine ? S[tri(l) + l] : T(1);
		const int lane0 = g * L;
		// C y = b
		T yreg = T(0);
		for (int j = 0; j < nmax; ++j) {
			const bool on = j < n;
			const T yj = __shfl(breg / dl, lane0 + j, WAVE);
			if (on && l == j) yreg = yj;
			if (on && mine && l > j) breg = smmFma(-S[tri(l) + j], yj, breg);
		}
		// C^T y = y
		for (int j = nmax - 1; j >= 0; --j) {
			const bool on = j < n;
			const T yj = __shfl(yreg / dl, lane0 + j, WAVE);
			if (on && l == j) yreg = yj;
			if (on && l < j) yreg = smmFma(-S[tri(j) + l], yj, yreg);
		}
		const T ylast = __shfl(yreg, lane0 + max(n - 1, 0), WAVE);
		if (mine) gval[gb + l] = SPAI ? yreg : yreg / sqrt(ylast);
		if (failed && l == 0 && live) atomicMin(errRow, static_cast<int>(row));
		__syncthreads();  // the tile is zeroed again by the next round
	}
}

template <typename T, int L>
void launchSolveTier(const smm_hip_precond* M, hipStream_t s, int* errRow) {
	const smm_precond_ainv* A = M->ainv;
	const int rows = M->a->rows;
	constexpr int G = WAVE / L;
	const int grid = static_cast<int>(std::max<long long>(1, std::min<long long>((rows + G - 1LL) / G, numCUs() * 64LL)));
	T* gval = static_cast<T*>(M->d_values);
	if (M->kind == SMM_PRECOND_SPAI) {
		ainvSolveKernel<T, L, true><<<grid, WAVE, 0, s>>>(rows, A->d_gstart, A->d_gpos, gval, A->N->d_start, A->N->d_positions, static_cast<const T*>(A->N->d_values), A->d_asc,
		                                                  A->At->d_start, A->At->d_positions, static_cast<const T*>(A->At->d_values), errRow);
	} else {
		ainvSolveKernel<T, L, false><<<grid, WAVE, 0, s>>>(rows, A->d_gstart, A->d_gpos, gval, M->a->d_start, M->a->d_positions, static_cast<const T*>(M->a->d_values), A->d_asc,
		                                                   nullptr, nullptr, nullptr, errRow);
	}
}

// the values of G / M from the present values of the source matrices, and (FSAI) of Gt; synchronises `s`
template <typename T>
int ainvNumeric(smm_hip_precond* M, bool refresh, hipStream_t s) {
	smm_precond_ainv* A = M->ainv;
	const smm_hip_csr* a = M->a;
	const int n = a->rows;
	const bool spai = M->kind == SMM_PRECOND_SPAI;
	constexpr bool F32 = std::is_same<T, float>::value;
	if (refresh && spai) {
		SMM_TRY(F32 ? smm_hip_csr_transpose_refresh_f32(A->At, a, asHandle(s)) : smm_hip_csr_transpose_refresh_f64(A->At, a, asHandle(s)));
		SMM_TRY(F32 ? smm_hip_csr_multiply_into_f32(A->N, a, A->At, asHandle(s)) : smm_hip_csr_multiply_into_f64(A->N, a, A->At, asHandle(s)));
	}
	if (n > 0) {
		DevBuf<int> err;
		SMM_TRY(err.alloc(1));
		int herr = INT_MAX;
		SMM_TRY(hostToDev(err, &herr, sizeof(int), s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		SetupTrace trace(spai ? "ainv: solve kernel (SPAI)" : "ainv: solve kernel (FSAI)");  // SMM_HIP_TRACE_SETUP=1: the set-up launch alone, wall clock to its read-back
		if (A->tier == 8) launchSolveTier<T, 8>(M, s, err);
		else if (A->tier == 16) launchSolveTier<T, 16>(M, s, err);
		else if (A->tier == 32) launchSolveTier<T, 32>(M, s, err);
		else launchSolveTier<T, 64>(M, s, err);
		SMM_HIP_TRY(hipGetLastError());
		SMM_HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (herr != INT_MAX) {
			setError("%s: row %d: a pivot of its system is not positive or not finite (%s)", spai ? "spai" : "fsai", herr,
			         spai ? "the matrix has dependent rows on the pattern, or a a^T is too ill-conditioned for this precision" : "the matrix is not symmetric positive definite");
			return SMM_HIP_ERR_PRECOND;
		}
	}
	if (refresh) SMM_TRY(F32 ? smm_hip_csr_values_changed_f32(A->G, asHandle(s)) : smm_hip_csr_values_changed_f64(A->G, asHandle(s)));
	if (refresh && !spai) SMM_TRY(F32 ? smm_hip_csr_transpose_refresh_f32(A->Gt, A->G, asHandle(s)) : smm_hip_csr_transpose_refresh_f64(A->Gt, A->G, asHandle(s)));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// the pattern J of every row as CSR arrays of the handle; *nnz its entries
template <bool LOWER>
int ainvPattern(const smm_hip_csr* pat, int power, smm_precond_ainv* A, size_t* nnz, hipStream_t s) {
	const int n = pat->rows;
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&A->d_gstart), (static_cast<size_t>(n) + 1) * sizeof(int)));
	DevBuf<int> lens, words;
	DevBuf<unsigned long long> total;
	SMM_TRY(lens.alloc(static_cast<size_t>(n) + 1));
	SMM_TRY(words.alloc(4));
	SMM_TRY(total.alloc(1));
	int h[4] = {INT_MAX, INT_MAX, INT_MAX, 0};
	unsigned long long sum = 0ull;
	SMM_TRY(hostToDev(words, h, sizeof(h), s));
	SMM_HIP_TRY(hipMemsetAsync(total, 0, sizeof(unsigned long long), s));
	ainvCountKernel<LOWER><<<rowGrid(n + 1LL), TPB, 0, s>>>(n, pat->d_start, pat->d_positions, lens, total, words);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(&sum, total, sizeof(sum), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (h[0] != INT_MAX) {
		setError("precond_create_ainv: row %d holds a column outside the matrix", h[0]);
		return SMM_HIP_ERR_INVALID;
	}
	if (h[1] != INT_MAX && (h[2] == INT_MAX || h[1] <= h[2])) {
		setError("precond_create_ainv: row %d has no stored diagonal entry", h[1]);
		return SMM_HIP_ERR_PRECOND;
	}
	if (h[2] != INT_MAX) {
		int len = 0;
		SMM_HIP_TRY(hipMemcpyAsync(&len, lens.p + h[2], sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		setError("precond_create_ainv: row %d of the pattern has %d entries at power %d; a row may have at most %d (use a lower power)", h[2], len, power, SMM_AINV_MAX_ROW);
		return SMM_HIP_ERR_PRECOND;
	}
	if (sum > static_cast<unsigned long long>(INT_MAX)) {
		setError("precond_create_ainv: the pattern would hold %llu entries (limit 2^31 - 1)", sum);
		return SMM_HIP_ERR_INVALID;
	}
	A->maxRow = h[3];
	A->tier = h[3] <= 8 ? 8 : h[3] <= 16 ? 16 : h[3] <= 32 ? 32 : 64;
	*nnz = static_cast<size_t>(sum);
	SMM_TRY(scanExclusive(lens.p, A->d_gstart, static_cast<size_t>(n) + 1, s));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&A->d_gpos), std::max<size_t>(1, *nnz) * sizeof(int)));
	if (n) ainvFillKernel<LOWER><<<rowGrid(n), TPB, 0, s>>>(n, pat->d_start, pat->d_positions, A->d_gstart, A->d_gpos);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template <typename T>
int ainvCreateTyped(const smm_hip_csr* a, int power, smm_hip_precond* M) {
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());  // the matrix may still be being written on a caller's stream
	smm_precond_ainv* A = M->ainv;
	const int n = a->rows;
	const bool spai = M->kind == SMM_PRECOND_SPAI;
	constexpr bool F32 = std::is_same<T, float>::value;
	// Pat = the structural product of `power` copies of a (only its pattern is used)
	smm_hip_csr* pat = nullptr;
	for (int p = 2; p <= power; ++p) {
		smm_hip_csr* next = nullptr;
		const int st = smm_hip_csr_multiply_create(pat ? pat : a, a, asHandle(s), &next);
		smm_hip_csr_destroy(pat);
		SMM_TRY(st);
		pat = next;
	}
	size_t nnz = 0;
	const int st = spai ? ainvPattern<false>(pat ? pat : a, power, A, &nnz, s) : ainvPattern<true>(pat ? pat : a, power, A, &nnz, s);
	smm_hip_csr_destroy(pat);
	SMM_TRY(st);
	SMM_TRY(devAlloc(&M->d_values, std::max<size_t>(1, nnz) * sizeof(T)));
	M->n_values = nnz;
	SMM_HIP_TRY(hipMemsetAsync(M->d_values, 0, std::max<size_t>(1, nnz) * sizeof(T), s));
	SMM_TRY(F32 ? smm_hip_csr_create_dev_f32(n, n, A->d_gstart, A->d_gpos, static_cast<const float*>(M->d_values), &A->G)
	            : smm_hip_csr_create_dev_f64(n, n, A->d_gstart, A->d_gpos, static_cast<const double*>(M->d_values), &A->G));
	if (spai) {
		SMM_TRY(smm_hip_csr_transpose_create(a, asHandle(s), &A->At));
		SMM_TRY(smm_hip_csr_multiply_create(a, A->At, asHandle(s), &A->N));
	}
	const smm_hip_csr* src = spai ? A->N : a;
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&A->d_asc), static_cast<size_t>(std::max(1, n))));
	if (n) ainvAscendKernel<<<rowGrid(n), TPB, 0, s>>>(n, src->d_start, src->d_positions, A->d_asc);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(ainvNumeric<T>(M, false, s));
	SMM_TRY(ensureCsrReady(A->G, nullptr, false));
	if (!spai) {
		SMM_TRY(smm_hip_csr_transpose_create(A->G, asHandle(s), &A->Gt));
		SMM_TRY(ensureCsrReady(A->Gt, nullptr, false));
		SMM_TRY(devAlloc(&A->d_w, static_cast<size_t>(std::max(1, n)) * sizeof(T)));
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

const smm_precond_ainv* ainvOf(const smm_hip_precond* M, const char* who) {
	if (!M || (M->kind != SMM_PRECOND_FSAI && M->kind != SMM_PRECOND_SPAI) || !M->ainv || !M->ainv->G) {
		setError("%s: not an FSAI / SPAI preconditioner", who);
		return nullptr;
	}
	return M->ainv;
}

}  // namespace

template <typename T>
int ainvApplyDev(const smm_hip_precond* M, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_precond_ainv* A = M->ainv;
	if (!A || !A->G || (M->kind == SMM_PRECOND_FSAI && !A->Gt)) {
		setError("precond_apply: the approximate-inverse preconditioner was not set up");
		return SMM_HIP_ERR_INVALID;
	}
	if (M->kind == SMM_PRECOND_SPAI) return launchSpmv<T>(A->G, SMM_OP_ASSIGN, nullptr, rhs, x, 0, nullptr, nullptr, doneFlag, s);  // z = M r
	T* w = static_cast<T*>(A->d_w);
	std::lock_guard<std::mutex> whole(M->enqueueMutex);  // d_w is the handle's: the two SpMVs stay together
	SMM_TRY(launchSpmv<T>(A->G, SMM_OP_ASSIGN, nullptr, rhs, w, 0, nullptr, nullptr, doneFlag, s));  // w = G r
	return launchSpmv<T>(A->Gt, SMM_OP_ASSIGN, nullptr, w, x, 0, nullptr, nullptr, doneFlag, s);     // z = Gt w
}
template int ainvApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int ainvApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void ainvDestroy(smm_precond_ainv* A) {
	if (!A) return;
	smm_hip_csr_destroy(A->G);  // (wraps d_gstart / d_gpos and the handle's d_values: does not own them)
	smm_hip_csr_destroy(A->Gt);
	smm_hip_csr_destroy(A->N);
	smm_hip_csr_destroy(A->At);
	devFree(A->d_gstart);
	devFree(A->d_gpos);
	devFree(A->d_asc);
	devFree(A->d_w);
	delete A;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_precond_create_ainv(const smm_hip_csr* a, int kind, int power, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_ainv: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (kind != SMM_PRECOND_FSAI && kind != SMM_PRECOND_SPAI) {
		setError("precond_create_ainv: kind must be SMM_PRECOND_FSAI or SMM_PRECOND_SPAI");
		return SMM_HIP_ERR_INVALID;
	}
	if (power < 1 || power > SMM_AINV_MAX_POWER) {
		setError("precond_create_ainv: power must be 1 .. %d", SMM_AINV_MAX_POWER);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("preconditioner needs a square matrix");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));  // a set-up call without a stream: drains the device once
	auto* M = new smm_hip_precond();
	M->kind = kind;
	M->dtype = a->dtype;
	M->a = a;
	M->ainv = new smm_precond_ainv();
	M->ainv->power = power;
	const int st = a->dtype == SMM_DTYPE_F32 ? ainvCreateTyped<float>(a, power, M) : ainvCreateTyped<double>(a, power, M);
	if (st != SMM_HIP_OK) {
		(void)hipDeviceSynchronize();  // nothing queued may still touch what the destroy releases
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

int smm_hip_precond_ainv_refresh(smm_hip_precond* M) {
	if (!ainvOf(M, "precond_ainv_refresh")) return SMM_HIP_ERR_INVALID;
	SMM_TRY(ensureInit());
	SMM_HIP_TRY(hipDeviceSynchronize());
	hipStream_t s = libStream();
	const int st = M->dtype == SMM_DTYPE_F32 ? ainvNumeric<float>(M, true, s) : ainvNumeric<double>(M, true, s);
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return st;
}

int smm_hip_precond_ainv_info(const smm_hip_precond* M, int* power, int* max_row, size_t* nnz) {
	const smm_precond_ainv* A = ainvOf(M, "precond_ainv_info");
	if (!A) return SMM_HIP_ERR_INVALID;
	if (power) *power = A->power;
	if (max_row) *max_row = A->maxRow;
	if (nnz) *nnz = M->n_values;
	return SMM_HIP_OK;
}

int smm_hip_precond_ainv_matrix(const smm_hip_precond* M, smm_hip_csr** g, smm_hip_csr** gt) {
	const smm_precond_ainv* A = ainvOf(M, "precond_ainv_matrix");
	if (!A) return SMM_HIP_ERR_INVALID;
	if (g) *g = A->G;
	if (gt) *gt = A->Gt;
	return SMM_HIP_OK;
}

}  // extern "C"
