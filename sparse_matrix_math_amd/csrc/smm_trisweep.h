// smm_trisweep.h -- what a triangular sweep IS, once, for the exact kinds (smm_precond.hip) and their multicolour forms (smm_precond_mc.hip).
//
// The arithmetic of one row (sweepStart / sweepTerm / sweepFinish) is the reference's, entry for entry (ref:1673-1711, 1806-1835): whoever
// walks a row's triangular part in the stored order with these three and starts only when the rows it reads are final gives the bits of the
// sequential sweep.  Two walkers do: sweepRow (one lane per row, below) and the windowed loop of the synchronisation-free sweeps
// (sweepFreeKernel, smm_precond.hip).
// A level-scheduled sweep: the rows are cut into dependency levels (a LevelSchedule), a level of more than SMALL_LEVEL rows gets a launch of
// its own, runs of smaller levels are chained inside one SMALL_LEVEL-lane workgroup with a workgroup barrier between levels.  The rows of a
// level are order[bounds[l] .. bounds[l+1]) (exact kinds: rows sorted by level) or that range itself (multicolour kinds: a colour is a level of
// both sweeps and a contiguous range of P A Pᵀ, so the upper sweep walks the same bounds backwards).  An IO policy says where a row's input
// comes from and where its result goes: NaturalIO for vectors in the matrix's numbering, PermutedIO with the permutation folded into the first
// read and the last write.
#pragma once
#include <type_traits>
#include <vector>

#include "smm_csr_build.h"
#include "smm_device.h"
#include "smm_internal.h"

namespace smm {

constexpr int SWEEP_TPB = 256;
constexpr int SMALL_LEVEL = 1024;  // levels up to this many rows are chained inside one workgroup

enum SweepMode { SGS_LO = 0, SGS_UP = 1, ILU_LO = 2, ILU_UP = 3, IC_LO = 4, IC_UP = 5 };
constexpr bool isLower(int mode) { return mode == SGS_LO || mode == ILU_LO || mode == IC_LO; }

// ---- the arithmetic of one row: `own` is the row's input (the right-hand side of a lower sweep, the lower sweep's result in an upper one)
template <typename T, int MODE>
__device__ __forceinline__ T sweepStart(T own) {
	return MODE == SGS_UP ? T(0) : own;  // ref:1698: the upper SGS sweep sums from zero
}
template <typename T, int MODE>
__device__ __forceinline__ T sweepTerm(T acc, T value, T xv) {
	if (MODE == SGS_UP) return smmFma(value, xv, acc);                        // ref:1702-1706
	if (MODE == SGS_LO || MODE == ILU_LO || MODE == ILU_UP) return smmFma(-value, xv, acc);  // ref:1677-1681; ILU: L y = rhs (unit diagonal), U x = y
	const T prod = value * xv;  // IC, ref:1812-1813, 1828-1829: multiply, then subtract
	return acc - prod;
}
template <typename T, int MODE>
__device__ __forceinline__ T sweepFinish(T acc, T own, T diagValue) {
	if (MODE == SGS_UP) return own - acc / diagValue;  // ref:1710
	if (MODE == ILU_LO) return acc;
	return acc / diagValue;  // SGS_LO (ref:1695), ILU_UP, IC_LO (ref:1818), IC_UP (ref:1834)
}

// ---- where a row's input comes from and where its result goes.  Lower sweeps read `in` and write y; upper sweeps read and write y.
// (The policy carries its vectors: with NaturalIO the level kernel's arguments stay within one 64-byte line, as before the two were one.)
template <typename T>
struct NaturalIO {
	const T* in;
	T* y;
	template <int MODE>
	__device__ __forceinline__ T own(int row) const {
		return isLower(MODE) ? in[row] : y[row];
	}
	template <int MODE>
	__device__ __forceinline__ void put(int row, T r) const {
		y[row] = r;
	}
};
// the caller's vectors are in A's numbering, the sweeps run on B = P A Pᵀ: the lower sweep reads in[perm[row]], the upper sweep's write also
// stores out[perm[row]] -- no gather or scatter pass over a vector
template <typename T>
struct PermutedIO {
	const int* perm;
	const T* in;
	T* y;
	T* out;
	template <int MODE>
	__device__ __forceinline__ T own(int row) const {
		return isLower(MODE) ? in[perm[row]] : y[row];
	}
	template <int MODE>
	__device__ __forceinline__ void put(int row, T r) const {
		y[row] = r;
		if (!isLower(MODE)) out[perm[row]] = r;
	}
};

// One row by one lane: the entries of the triangular part in the stored order, up to the diagonal -- every row holds its diagonal (checked at
// create time), which ends the walk.
template <typename T, int MODE, typename IO>
__device__ __forceinline__ void sweepRow(int row, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals, const IO& io) {
	constexpr bool LOWER = isLower(MODE);
	constexpr bool OWN_LAST = MODE == SGS_UP;  // the one sweep that sums from zero: its input is read where it is needed, after the walk
	int k = LOWER ? start[row] : start[row + 1] - 1;
	T own = T(0);
	if (!OWN_LAST) own = io.template own<MODE>(row);
	T acc = sweepStart<T, MODE>(own);
	int col = positions[k];
	T value = vals[k];
	while (LOWER ? col < row : col > row) {
		acc = sweepTerm<T, MODE>(acc, value, io.y[col]);
		k += LOWER ? 1 : -1;
		col = positions[k];
		value = vals[k];
	}
	if (OWN_LAST) own = io.template own<MODE>(row);
	io.template put<MODE>(row, sweepFinish<T, MODE>(acc, own, value));
}

// ORDERED: position i of the schedule is row order[i]; otherwise it is row i
// one large level: positions [begin, begin + count)
template <typename T, int MODE, typename IO, bool ORDERED>
__global__ __launch_bounds__(SWEEP_TPB) void sweepLevelKernel(const int* __restrict__ order, int begin, int count, const int* __restrict__ start,
                                                              const int* __restrict__ positions, const T* __restrict__ vals, IO io, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	const unsigned i = blockIdx.x * SWEEP_TPB + threadIdx.x;
	if (i < static_cast<unsigned>(count)) {
		const int at = begin + static_cast<int>(i);
		sweepRow<T, MODE, IO>(ORDERED ? order[at] : at, start, positions, vals, io);
	}
}

// a run of small levels inside one workgroup: l0, l0 + step, ... up to (not including) l1; bounds is the device copy of the level bounds
template <typename T, int MODE, typename IO, bool ORDERED>
__global__ __launch_bounds__(SMALL_LEVEL) void sweepChainKernel(const int* __restrict__ order, const int* __restrict__ bounds, int l0, int l1, int step,
                                                                const int* __restrict__ start, const int* __restrict__ positions,
                                                                const T* __restrict__ vals, IO io, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	for (int l = l0; l != l1; l += step) {
		const int begin = bounds[l];
		const int count = bounds[l + 1] - begin;
		if (static_cast<int>(threadIdx.x) < count) {
			const int at = begin + static_cast<int>(threadIdx.x);
			sweepRow<T, MODE, IO>(ORDERED ? order[at] : at, start, positions, vals, io);
		}
		// rows of the next level read y[] written above by other wavefronts of this workgroup
		__threadfence_block();
		__syncthreads();
	}
}

// launch groups: a chain of small levels [l0, l1), or a single large level
struct Group {
	int l0, l1;
	bool chain;
};
struct LevelSchedule {
	int* d_order = nullptr;    // rows sorted by level (owned); null: the rows of a level are the range itself
	int* d_bounds = nullptr;   // device copy of `bounds` (owned)
	std::vector<int> bounds;   // level l covers positions bounds[l] .. bounds[l+1]
	std::vector<Group> groups;
	int levels() const { return bounds.empty() ? 0 : static_cast<int>(bounds.size()) - 1; }
	void release() {
		devFree(d_order);
		devFree(d_bounds);
		d_order = d_bounds = nullptr;
	}
};

inline void planGroups(const std::vector<int>& bounds, std::vector<Group>& groups) {
	groups.clear();
	const int nl = static_cast<int>(bounds.size()) - 1;
	int l = 0;
	while (l < nl) {
		if (bounds[l + 1] - bounds[l] > SMALL_LEVEL) {
			groups.push_back({l, l + 1, false});
			++l;
		} else {
			int e = l + 1;
			while (e < nl && bounds[e + 1] - bounds[e] <= SMALL_LEVEL) ++e;
			groups.push_back({l, e, true});
			l = e;
		}
	}
}

// enqueues one sweep of matrix `m` (values `vals` on its pattern) over the schedule's groups, first to last or (backwards) last to first;
// ORDERED as the schedule is (d_order set or null)
template <typename T, int MODE, typename IO, bool ORDERED>
int runLevelSweep(const LevelSchedule& sch, bool backwards, const smm_hip_csr* m, const T* vals, const IO& io, const int* doneFlag, hipStream_t s) {
	const size_t ng = sch.groups.size();
	for (size_t i = 0; i < ng; ++i) {
		const Group& g = sch.groups[backwards ? ng - 1 - i : i];
		const int begin = sch.bounds[g.l0], count = sch.bounds[g.l1] - begin;
		const int from = backwards ? g.l1 - 1 : g.l0, to = backwards ? g.l0 - 1 : g.l1, step = backwards ? -1 : 1;
		const int grid = (count + SWEEP_TPB - 1) / SWEEP_TPB;
		if (g.chain) sweepChainKernel<T, MODE, IO, ORDERED><<<1, SMALL_LEVEL, 0, s>>>(sch.d_order, sch.d_bounds, from, to, step, m->d_start, m->d_positions, vals, io, doneFlag);
		else sweepLevelKernel<T, MODE, IO, ORDERED><<<grid, SWEEP_TPB, 0, s>>>(sch.d_order, begin, count, m->d_start, m->d_positions, vals, io, doneFlag);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// ---- rows sorted by an integer key
static __global__ __launch_bounds__(SWEEP_TPB) void iotaKernel(int n, int* out) {
	for (long long i = static_cast<long long>(blockIdx.x) * SWEEP_TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * SWEEP_TPB) out[i] = static_cast<int>(i);
}
inline int sweepGrid(long long work) { return static_cast<int>(std::max<long long>(1, std::min<long long>((work + SWEEP_TPB - 1) / SWEEP_TPB, numCUs() * 8LL))); }

// bounds[k] = the first position of the sorted keys whose key is >= k (k = 0 .. nKeys); a key no row holds gives an empty range
static __global__ __launch_bounds__(SWEEP_TPB) void keyBoundsKernel(int n, int nKeys, const int* __restrict__ sortedKeys, int* __restrict__ bounds) {
	for (long long k = static_cast<long long>(blockIdx.x) * SWEEP_TPB + threadIdx.x; k <= nKeys; k += static_cast<long long>(gridDim.x) * SWEEP_TPB) {
		int lo = 0, hi = n;
		while (lo < hi) {
			const int mid = lo + ((hi - lo) >> 1);
			if (sortedKeys[mid] < k) lo = mid + 1;
			else hi = mid;
		}
		bounds[k] = lo;
	}
}

// d_order[n] = the rows sorted by d_keys[row] (0 <= key < nKeys), stably: the row index ascends inside a key; d_bounds[nKeys + 1] and
// hostBounds = where each key's rows begin in that order.  Both device arrays are the caller's.  Synchronises `s`.
inline int sortRowsByKey(const int* d_keys, int n, int nKeys, hipStream_t s, int* d_order, int* d_bounds, std::vector<int>& hostBounds) {
	hostBounds.assign(static_cast<size_t>(nKeys) + 1, 0);
	if (n == 0) {
		SMM_HIP_TRY(hipMemsetAsync(d_bounds, 0, hostBounds.size() * sizeof(int), s));
		return SMM_HIP_OK;
	}
	DevBuf<int> rowsIn, sorted;
	SMM_TRY(rowsIn.alloc(n));
	SMM_TRY(sorted.alloc(n));
	iotaKernel<<<sweepGrid(n), SWEEP_TPB, 0, s>>>(n, rowsIn);
	int bits = 1;
	while (bits < 31 && (1ll << bits) < nKeys) ++bits;
	SMM_TRY(sortPairs(d_keys, sorted.p, rowsIn.p, d_order, static_cast<size_t>(n), static_cast<unsigned>(bits), s));
	keyBoundsKernel<<<sweepGrid(nKeys + 1LL), SWEEP_TPB, 0, s>>>(n, nKeys, sorted, d_bounds);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(hostBounds.data(), d_bounds, hostBounds.size() * sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));  // the scratch buffers go back to the allocator when this scope ends
	return SMM_HIP_OK;
}

// ---- the three exact kinds: f(lower mode, upper mode) with the pair as std::integral_constant<int, ...>
template <typename F>
int withSweepModes(int baseKind, F&& f) {
	switch (baseKind) {
	case SMM_PRECOND_SGS: return f(std::integral_constant<int, SGS_LO>{}, std::integral_constant<int, SGS_UP>{});
	case SMM_PRECOND_ILU0: return f(std::integral_constant<int, ILU_LO>{}, std::integral_constant<int, ILU_UP>{});
	case SMM_PRECOND_IC0: return f(std::integral_constant<int, IC_LO>{}, std::integral_constant<int, IC_UP>{});
	default: setError("precond_apply: kind %d has no apply", baseKind); return SMM_HIP_ERR_INVALID;
	}
}

// what a failed ILU0 / IC0 factorisation reports: herr as the factor kernels leave it (smm_precond.hip)
inline int factorErrorFor(int baseKind, int herr) {
	if (!herr) return SMM_HIP_OK;
	if (baseKind == SMM_PRECOND_ILU0) setError("ilu0: zero / missing pivot (reordering would be needed, ref:1741-1746)");
	else setError(herr & 1 ? "ic0: matrix is not symmetric positive definite on its pattern (ref:1871-1878)" : "ic0: the pattern of the matrix is not symmetric");
	return SMM_HIP_ERR_PRECOND;
}

}  // namespace smm
