// smm_spgemm.hip -- C = A B for two CSR matrices ON THE DEVICE: the structural product as an ordinary smm_hip_csr handle
// (smm_hip_csr_multiply_create) and the numeric phase alone into an existing pattern (smm_hip_csr_multiply_into_*).
//   check: one lane per row / stored entry of each operand: start[] ascends from 0, every column lies inside its matrix.  A failure raises
//     a bit of a device word before anything is used as an address (the upper-bound pass below guards its own reads the same way, so it
//     is queued behind the check without a synchronisation in between).
//   upper bounds: ub_i = sum over the stored (i, p) of len(B_p), 8 lanes per row of A, 64 bits per row.
//   symbolic: rows are binned by ub_i (two counting passes over one list of rows: count, 5-word scan, fill).  A group of lanes per row of C
//     inserts the columns of the gathered rows of B into a hash set of int keys (integer atomicCAS, linear probing):
//       ub <= 32      a sub-wavefront group (8 or 32 lanes, from B's mean row length) and 64 slots of LDS per row, 256 lanes per workgroup
//       ub <= 256     one wavefront = one workgroup per row, 512 slots of LDS
//       ub <= 1024    ... 2048 slots
//       ub <= 4096    ... 8192 slots (32 KiB)
//       beyond        a workgroup of 256 lanes per row and a table in GLOBAL memory of 2^ceil(log2(2 min(ub, n))) slots (at most 2^31) -- correct for any size
//     Pass one counts the distinct columns (a 64-bit scan gives start[] and nnz, refused beyond 2^31 - 1); pass two hashes again (the LDS
//     tables) or walks the table pass one left behind (the global ones), writes the row's columns in table order, and one segmented radix
//     sort (rocprim, a set-up pass) leaves them ascending in positions[].
//   numeric (create and into alike): rows of C binned by their stored length.  The row's sorted columns and one accumulator per stored
//     entry sit in LDS (<= 32 entries: sub-wavefront groups; <= 512 and <= 4096: a wavefront per row); A's entries of the row are taken ONE
//     AFTER ANOTHER in stored order, the lanes of the group spread over B's row p -- its columns are distinct, so no two lanes of a step
//     meet in one accumulator --, the slot of column j is a binary search of the row's columns, acc = smmFma(a, b, acc).  The steps of a
//     row are program-ordered inside ONE wavefront (DS operations complete in order), so the sum of an entry is the row sum of rMult in
//     A's stored order: no floating-point atomics, no tree sums, nothing depends on the launch geometry.  Rows longer than 4096 entries:
//     256 lanes per row, the accumulators are the output array itself (global memory), one workgroup barrier per step.
//     A product whose column is not stored in the row raises the row number (atomicMin) -- multiply_into's refusal.
//   into: computed into scratch; the flag is read (the call synchronises); on success the scratch becomes the values array (owned arrays:
//     pointer swap) or is copied into it (caller-owned arrays), then the path of every value edit (csrValuesEdited).
//   Bytes beside the set-up passes: A once per phase, sum ub_i (s + 4) gathered from B (4 in the symbolic passes), nnz(C) (s + 4) written.
#include <algorithm>
#include <climits>

#include "smm_csr_build.h"
#include "smm_device.h"

namespace smm {
namespace {

constexpr int GTPB = BUILD_TPB;
constexpr int MAXBINS = 5;
// symbolic bins by ub (the last bin: global table) and the LDS slots per row of the first four
constexpr long long SYM_UP[MAXBINS - 1] = {32, 256, 1024, 4096};
constexpr int SYM_SLOTS[MAXBINS - 1] = {64, 512, 2048, 8192};
// numeric bins by the row's stored length (the last bin: accumulators in global memory) = entries of LDS per row
constexpr int NUM_BINS = 4;
constexpr long long NUM_UP[NUM_BINS - 1] = {32, 512, 4096};

// bits of the check word
constexpr int NO_ROW = INT_MAX;  // the "smallest row with a product outside the pattern" word when there is none (a row number is below it)
constexpr int BAD_A_START = 1, BAD_A_COL = 2, BAD_B_START = 4, BAD_B_COL = 8, BAD_C_START = 16;

struct BinCuts {
	long long upTo[MAXBINS - 1];
	int bins;
};

// the two words of a call: [0] the check word, [1] the smallest row with a product outside the pattern
__global__ void flagsInitKernel(int* flags) {
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		flags[0] = 0;
		flags[1] = NO_ROW;
	}
}

// Slots of the global-memory set of a row that can hold at most min(ub, n) distinct columns: a power of two, at least 64 and at least
// twice that number, but never more than 2^31 -- n < 2^31, so the set still has more slots than keys and every probe ends.  *shift: what
// brings the 32-bit hash down to a slot number.
__host__ __device__ inline unsigned globalSlots(long long ub, int n, int* shift) {
	const unsigned long long distinctMost = static_cast<unsigned long long>(ub < n ? ub : n);
	unsigned slots = 64;
	int sh = 26;
	while (slots < (1u << 31) && slots < 2ull * distinctMost) {
		slots <<= 1;
		--sh;
	}
	if (shift) *shift = sh;
	return slots;
}

__global__ __launch_bounds__(GTPB) void checkKernel(int rows, int cols, int nnz, const int* __restrict__ start, const int* __restrict__ positions, int badStart,
                                                    int badCol, int* bad) {
	const long long i = static_cast<long long>(blockIdx.x) * GTPB + threadIdx.x;
	if (i < rows && (start[i] > start[i + 1] || (i == 0 && start[0] != 0))) atomicOr(bad, badStart);
	if (positions && i < nnz) {
		const int c = positions[i];
		if (c < 0 || c >= cols) atomicOr(bad, badCol);
	}
}

// ub[i] = sum of len(B_p) over the stored (i, p): 8 lanes per row of A.  Safe on unchecked input: a row is read only inside [0, nnzA), a
// column is used only inside [0, k); B's start[] is read at checked places and its values are used as numbers only
__global__ __launch_bounds__(GTPB) void upperBoundKernel(int m, int k, int nnzA, const int* __restrict__ aStart, const int* __restrict__ aPos,
                                                         const int* __restrict__ bStart, long long* __restrict__ ub, int* bad) {
	const long long gid = static_cast<long long>(blockIdx.x) * GTPB + threadIdx.x;
	const long long row = gid >> 3;
	const int lane = static_cast<int>(gid & 7);
	if (row >= m) return;  // (the 8 lanes of a row leave together)
	const int s0 = aStart[row], s1 = aStart[row + 1];
	long long sum = 0;
	if (s0 < 0 || s1 > nnzA || s0 > s1) {
		atomicOr(bad, BAD_A_START);
	} else {
		for (int e = s0 + lane; e < s1; e += 8) {
			const int p = aPos[e];
			if (p >= 0 && p < k) sum += static_cast<long long>(bStart[p + 1]) - bStart[p];
			else atomicOr(bad, BAD_A_COL);
		}
	}
#pragma unroll
	for (int o = 4; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 8);
	if (lane == 0) ub[row] = sum;
}

template <bool FROM_START>
__device__ __forceinline__ int binOf(const BinCuts& cuts, const long long* __restrict__ key, const int* __restrict__ start, long long i) {
	const long long v = FROM_START ? static_cast<long long>(start[i + 1]) - start[i] : key[i];
	if (v <= 0) return FROM_START ? 0 : -1;  // ub == 0: nothing lands in this row; a row of c without entries is still looked at (multiply_into)
	int b = 0;
	while (b < cuts.bins - 1 && v > cuts.upTo[b]) ++b;
	return b;
}

// counts[b] = rows of bin b: counted per workgroup in LDS, one global atomic per bin and workgroup (a million lanes adding to one word
// queue up behind each other).  The last bin of the symbolic phase (global tables) also reserves the row's table: tableOff[i], *tableSlots
template <bool FROM_START>
__global__ __launch_bounds__(GTPB) void binCountKernel(int m, BinCuts cuts, const long long* __restrict__ key, const int* __restrict__ start, int* counts,
                                                       int n, long long* __restrict__ tableOff, unsigned long long* tableSlots) {
	__shared__ int ldsCount[MAXBINS];
	if (threadIdx.x < MAXBINS) ldsCount[threadIdx.x] = 0;
	__syncthreads();
	const long long i = static_cast<long long>(blockIdx.x) * GTPB + threadIdx.x;
	const int b = i < m ? binOf<FROM_START>(cuts, key, start, i) : -1;
	if (b >= 0) {
		atomicAdd(&ldsCount[b], 1);
		if (!FROM_START && tableOff && b == cuts.bins - 1) {
			tableOff[i] = static_cast<long long>(atomicAdd(tableSlots, static_cast<unsigned long long>(globalSlots(key[i], n, nullptr))));
		}
	}
	__syncthreads();
	if (threadIdx.x < MAXBINS && ldsCount[threadIdx.x] > 0) atomicAdd(&counts[threadIdx.x], ldsCount[threadIdx.x]);
}

// base[b] = rows in the bins before b; cursor[b] = 0 (one lane)
__global__ void binScanKernel(int bins, const int* __restrict__ counts, int* __restrict__ base, int* __restrict__ cursor) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	int sum = 0;
	for (int b = 0; b < bins; ++b) {
		base[b] = sum;
		cursor[b] = 0;
		sum += counts[b];
	}
}

// list[base[b] ...] = the rows of bin b (in any order: every row is worked on for itself, its result does not depend on its place).  A
// workgroup ranks its rows per bin in LDS and takes its share of every bin's range with one global atomic
template <bool FROM_START>
__global__ __launch_bounds__(GTPB) void binFillKernel(int m, BinCuts cuts, const long long* __restrict__ key, const int* __restrict__ start,
                                                      const int* __restrict__ base, int* cursor, int* __restrict__ list) {
	__shared__ int ldsCount[MAXBINS], ldsFirst[MAXBINS];
	if (threadIdx.x < MAXBINS) ldsCount[threadIdx.x] = 0;
	__syncthreads();
	const long long i = static_cast<long long>(blockIdx.x) * GTPB + threadIdx.x;
	const int b = i < m ? binOf<FROM_START>(cuts, key, start, i) : -1;
	const int rank = b >= 0 ? atomicAdd(&ldsCount[b], 1) : 0;
	__syncthreads();
	if (threadIdx.x < MAXBINS && ldsCount[threadIdx.x] > 0) ldsFirst[threadIdx.x] = base[threadIdx.x] + atomicAdd(&cursor[threadIdx.x], ldsCount[threadIdx.x]);
	__syncthreads();
	if (b >= 0) list[ldsFirst[b] + rank] = static_cast<int>(i);
}

// true: col was not in the set.  slots is a power of two larger than the number of distinct keys the set will ever hold
__device__ __forceinline__ bool setInsert(int* table, unsigned slots, int shift, int col) {
	unsigned h = (static_cast<unsigned>(col) * 2654435761u) >> shift;
	for (;;) {
		const int seen = table[h];
		if (seen == col) return false;
		if (seen == -1) {
			const int old = atomicCAS(&table[h], -1, col);
			if (old == -1) return true;
			if (old == col) return false;
		}
		h = (h + 1) & (slots - 1);
	}
}

// The columns of the rows of B that row `row` of A names, into `table`; returns how many this lane added.  G lanes work on the row.
template <int G>
__device__ __forceinline__ int gatherColumns(int row, int lane, const int* __restrict__ aStart, const int* __restrict__ aPos, const int* __restrict__ bStart,
                                             const int* __restrict__ bPos, int* table, unsigned slots, int shift) {
	int added = 0;
	const int s0 = aStart[row], s1 = aStart[row + 1];
	if (G <= WAVE) {
		for (int base = s0; base < s1; base += G) {
			const int e = base + lane;
			int bs = 0, be = 0;
			if (e < s1) {
				const int p = aPos[e];
				bs = bStart[p];
				be = bStart[p + 1];
			}
			const int steps = min(G, s1 - base);
			for (int t = 0; t < steps; ++t) {
				const int rs = __shfl(bs, t, G), re = __shfl(be, t, G);
				for (int q = rs + lane; q < re; q += G) added += setInsert(table, slots, shift, bPos[q]) ? 1 : 0;
			}
		}
	} else {
		for (int e = s0; e < s1; ++e) {
			const int p = aPos[e];
			const int rs = bStart[p], re = bStart[p + 1];
			for (int q = rs + lane; q < re; q += G) added += setInsert(table, slots, shift, bPos[q]) ? 1 : 0;
		}
	}
	return added;
}

// LDS hash sets: TPB / G rows per workgroup, `slots` ints each.  FILL = false: count[row] = distinct columns.  FILL = true: the same set
// again, then its keys to cols[cStart[row] ...] in table order (the segmented sort orders them)
template <int G, int TPB, bool FILL>
__global__ __launch_bounds__(TPB) void symbolicLdsKernel(int nList, const int* __restrict__ list, int slots, int shift, const int* __restrict__ aStart,
                                                         const int* __restrict__ aPos, const int* __restrict__ bStart, const int* __restrict__ bPos,
                                                         int* __restrict__ count, const int* __restrict__ cStart, int* __restrict__ cols) {
	extern __shared__ int ldsTables[];
	__shared__ int ldsCursor[TPB / G];
	constexpr int ROWS = TPB / G;
	const int grp = threadIdx.x / G, lane = threadIdx.x % G;
	const long long item = static_cast<long long>(blockIdx.x) * ROWS + grp;
	const bool active = item < nList;
	int* table = ldsTables + static_cast<size_t>(grp) * slots;
	for (int t = lane; t < slots; t += G) table[t] = -1;
	if (lane == 0) ldsCursor[grp] = 0;
	__syncthreads();
	int row = 0, added = 0;
	if (active) {
		row = list[item];
		added = gatherColumns<G>(row, lane, aStart, aPos, bStart, bPos, table, static_cast<unsigned>(slots), shift);
	}
	if (!FILL) {
#pragma unroll
		for (int o = G / 2; o > 0; o >>= 1) added += __shfl_xor(added, o, G);
		if (active && lane == 0) count[row] = added;
		return;
	}
	__syncthreads();
	if (!active) return;
	const int out0 = cStart[row];
	for (int t = lane; t < slots; t += G) {
		const int key = table[t];
		if (key != -1) cols[out0 + atomicAdd(&ldsCursor[grp], 1)] = key;
	}
}

// the long rows: a workgroup per row, the set in global memory at tables[tableOff[row]] (filled with -1 beforehand), count[row] by integer atomics
__global__ __launch_bounds__(GTPB) void symbolicGlobalCountKernel(int nList, const int* __restrict__ list, int n, const long long* __restrict__ ub,
                                                                  const long long* __restrict__ tableOff, int* tables, const int* __restrict__ aStart,
                                                                  const int* __restrict__ aPos, const int* __restrict__ bStart, const int* __restrict__ bPos, int* count) {
	const int row = list[blockIdx.x];
	int shift = 0;
	const unsigned slots = globalSlots(ub[row], n, &shift);
	const int added = gatherColumns<GTPB>(row, threadIdx.x, aStart, aPos, bStart, bPos, tables + tableOff[row], slots, shift);
	if (added) atomicAdd(&count[row], added);
}

// ... and the keys of its table to cols[cStart[row] ...]; cursor[row] starts at 0
__global__ __launch_bounds__(GTPB) void symbolicGlobalFillKernel(int nList, const int* __restrict__ list, int n, const long long* __restrict__ ub,
                                                                 const long long* __restrict__ tableOff, const int* __restrict__ tables,
                                                                 const int* __restrict__ cStart, int* cursor, int* __restrict__ cols) {
	const int row = list[blockIdx.x];
	const unsigned slots = globalSlots(ub[row], n, nullptr);
	const int* table = tables + tableOff[row];
	const int out0 = cStart[row];
	for (unsigned t = threadIdx.x; t < slots; t += GTPB) {
		const int key = table[t];
		if (key != -1) cols[out0 + atomicAdd(&cursor[row], 1)] = key;
	}
}

// the place of col in the ascending cols[0 .. len), -1 when it is not there
__device__ __forceinline__ int slotOf(const int* cols, int len, int col) {
	int lo = 0, hi = len;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (cols[mid] < col) lo = mid + 1;
		else hi = mid;
	}
	return lo < len && cols[lo] == col ? lo : -1;
}

// between two steps of a row inside one wavefront: the compiler keeps the LDS accesses of the step before in front of those of the step
// after (the hardware completes a wavefront's DS operations in order); no instruction is emitted
__device__ __forceinline__ void stepFence() {
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// Rows of C of at most `cap` stored entries: TPB / G rows per workgroup, G <= 64 lanes of ONE wavefront per row.  LDS: TPB / G * cap
// accumulators, then as many columns.  out[] receives every stored entry of the row; *badRow the smallest row with a product outside it.
template <typename T, int G, int TPB>
__global__ __launch_bounds__(TPB) void numericLdsKernel(int nList, const int* __restrict__ list, int cap, const int* __restrict__ aStart, const int* __restrict__ aPos,
                                                        const T* __restrict__ aVal, const int* __restrict__ bStart, const int* __restrict__ bPos,
                                                        const T* __restrict__ bVal, const int* __restrict__ cStart, const int* __restrict__ cPos, T* __restrict__ out,
                                                        int* badRow) {
	extern __shared__ double ldsNumeric[];
	constexpr int ROWS = TPB / G;
	const int grp = threadIdx.x / G, lane = threadIdx.x % G;
	const long long item = static_cast<long long>(blockIdx.x) * ROWS + grp;
	if (item >= nList) return;  // (no workgroup barrier below: a group meets only itself, inside one wavefront)
	T* acc = reinterpret_cast<T*>(ldsNumeric) + static_cast<size_t>(grp) * cap;
	int* cols = reinterpret_cast<int*>(reinterpret_cast<T*>(ldsNumeric) + static_cast<size_t>(ROWS) * cap) + static_cast<size_t>(grp) * cap;
	const int row = list[item];
	const int c0 = cStart[row], len = cStart[row + 1] - c0;
	for (int t = lane; t < len; t += G) {
		cols[t] = cPos[c0 + t];
		acc[t] = T(0);
	}
	stepFence();
	bool missed = false;
	const int s0 = aStart[row], s1 = aStart[row + 1];
	for (int base = s0; base < s1; base += G) {
		const int e = base + lane;
		int bs = 0, be = 0;
		T a = T(0);
		if (e < s1) {
			const int p = __builtin_nontemporal_load(aPos + e);
			a = __builtin_nontemporal_load(aVal + e);
			bs = bStart[p];
			be = bStart[p + 1];
		}
		const int steps = min(G, s1 - base);
		for (int t = 0; t < steps; ++t) {  // A's entries one after another, in stored order
			const int rs = __shfl(bs, t, G), re = __shfl(be, t, G);
			const T at = __shfl(a, t, G);
			for (int q = rs + lane; q < re; q += G) {
				const int slot = slotOf(cols, len, bPos[q]);
				if (slot >= 0) acc[slot] = smmFma(at, bVal[q], acc[slot]);
				else missed = true;
			}
			stepFence();
		}
	}
	if (missed) atomicMin(badRow, row);
	for (int t = lane; t < len; t += G) out[c0 + t] = acc[t];
}

// Rows of C of any length: a workgroup per row, out[] (zeroed by the caller) holds the accumulators, one barrier per step
template <typename T>
__global__ __launch_bounds__(GTPB) void numericGlobalKernel(int nList, const int* __restrict__ list, const int* __restrict__ aStart, const int* __restrict__ aPos,
                                                            const T* __restrict__ aVal, const int* __restrict__ bStart, const int* __restrict__ bPos,
                                                            const T* __restrict__ bVal, const int* __restrict__ cStart, const int* __restrict__ cPos, T* out,
                                                            int* badRow) {
	const int row = list[blockIdx.x];
	const int c0 = cStart[row], len = cStart[row + 1] - c0;
	const int* cols = cPos + c0;
	T* acc = out + c0;
	bool missed = false;
	const int s0 = aStart[row], s1 = aStart[row + 1];
	for (int e = s0; e < s1; ++e) {  // (uniform over the workgroup: every lane meets every barrier)
		const int p = __builtin_nontemporal_load(aPos + e);  // (A is read once: the policy of the LDS kernel)
		const T a = __builtin_nontemporal_load(aVal + e);
		const int rs = bStart[p], re = bStart[p + 1];
		for (int q = rs + static_cast<int>(threadIdx.x); q < re; q += GTPB) {
			const int slot = slotOf(cols, len, bPos[q]);
			if (slot >= 0) acc[slot] = smmFma(a, bVal[q], acc[slot]);
			else missed = true;
		}
		__syncthreads();  // (workgroup-scope fence: the next step's lanes, in any wavefront of this workgroup, see this step's sums)
	}
	if (missed) atomicMin(badRow, row);
}

// the rows of a matrix dealt to bins: list[] bin after bin, hostCounts[] once the caller has synchronised
struct RowBins {
	DevBuf<int> list, words;  // words: counts[MAXBINS], base[MAXBINS], cursor[MAXBINS]
	int counts[MAXBINS] = {0, 0, 0, 0, 0};
	int* dCounts() const { return words.p; }
	int* dBase() const { return words.p + MAXBINS; }
	int* dCursor() const { return words.p + 2 * MAXBINS; }
	int base(int b) const {
		int s = 0;
		for (int i = 0; i < b; ++i) s += counts[i];
		return s;
	}
};

template <bool FROM_START>
int enqueueBins(RowBins& bins, int m, const BinCuts& cuts, const long long* key, const int* start, int n, long long* tableOff, unsigned long long* tableSlots,
                hipStream_t s) {
	SMM_TRY(bins.list.alloc(static_cast<size_t>(m)));
	SMM_TRY(bins.words.alloc(3 * MAXBINS));
	SMM_HIP_TRY(hipMemsetAsync(bins.words.p, 0, 3 * MAXBINS * sizeof(int), s));
	binCountKernel<FROM_START><<<gridOf(m), GTPB, 0, s>>>(m, cuts, key, start, bins.dCounts(), n, tableOff, tableSlots);
	binScanKernel<<<1, 64, 0, s>>>(cuts.bins, bins.dCounts(), bins.dBase(), bins.dCursor());
	binFillKernel<FROM_START><<<gridOf(m), GTPB, 0, s>>>(m, cuts, key, start, bins.dBase(), bins.dCursor(), bins.list);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(bins.counts, bins.dCounts(), MAXBINS * sizeof(int), hipMemcpyDeviceToHost, s));
	return SMM_HIP_OK;
}

// lanes per row of the sub-wavefront kernels, from the mean length of B's rows (what one step spreads its lanes over)
int smallGroup(const smm_hip_csr* b) { return b->rows > 0 && static_cast<long long>(b->nnz) > 12LL * b->rows ? 32 : 8; }

int describeBad(int bad, const char* what, const smm_hip_csr* a, const smm_hip_csr* b) {
	if (bad & (BAD_A_START | BAD_B_START | BAD_C_START)) {
		setError("%s: start[] of %s does not ascend from 0", what, bad & BAD_A_START ? "a" : bad & BAD_B_START ? "b" : "c");
	} else if (bad & BAD_A_COL) {
		setError("%s: a column of a lies outside [0, %d)", what, a->cols);
	} else {
		setError("%s: a column of b lies outside [0, %d)", what, b->cols);
	}
	return SMM_HIP_ERR_INVALID;
}

int enqueueCheck(const smm_hip_csr* m, int badStart, int badCol, int* d_bad, hipStream_t s) {
	const long long work = std::max<long long>(m->rows, badCol ? m->nnz : 0);
	if (work > 0) checkKernel<<<gridOf(work), GTPB, 0, s>>>(m->rows, m->cols, m->nnz, m->d_start, badCol ? m->d_positions : nullptr, badStart, badCol, d_bad);
	return SMM_HIP_OK;
}

// the numeric phase for the pattern (cStart, cPos) of an m-row matrix whose rows were binned by length into `bins` (counts on the host)
template <typename T>
int enqueueNumeric(const RowBins& bins, const smm_hip_csr* a, const smm_hip_csr* b, const int* cStart, const int* cPos, long long nnzC, T* out, int* d_badRow,
                   hipStream_t s) {
	const int* aS = a->d_start;
	const int* aP = a->d_positions;
	const T* aV = static_cast<const T*>(a->d_values);
	const int* bS = b->d_start;
	const int* bP = b->d_positions;
	const T* bV = static_cast<const T*>(b->d_values);
	// (every entry of the long rows starts from +0.0, their accumulators are out[] itself; the other rows' entries are all written by their
	// kernels afterwards: the whole array is zeroed in one pass, first)
	if (bins.counts[3] > 0) SMM_HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(nnzC) * sizeof(T), s));
	if (bins.counts[0] > 0) {
		const int cap = static_cast<int>(NUM_UP[0]);
		const int* list = bins.list.p + bins.base(0);
		if (smallGroup(b) == 8) {
			numericLdsKernel<T, 8, GTPB><<<gridOf(bins.counts[0], GTPB / 8), GTPB, (GTPB / 8) * cap * (sizeof(T) + sizeof(int)), s>>>(bins.counts[0], list, cap, aS, aP, aV, bS, bP, bV, cStart, cPos, out, d_badRow);
		} else {
			numericLdsKernel<T, 32, GTPB><<<gridOf(bins.counts[0], GTPB / 32), GTPB, (GTPB / 32) * cap * (sizeof(T) + sizeof(int)), s>>>(bins.counts[0], list, cap, aS, aP, aV, bS, bP, bV, cStart, cPos, out, d_badRow);
		}
	}
	for (int bin = 1; bin <= 2; ++bin) {
		if (bins.counts[bin] == 0) continue;
		const int cap = static_cast<int>(NUM_UP[bin]);
		numericLdsKernel<T, WAVE, WAVE><<<bins.counts[bin], WAVE, cap * (sizeof(T) + sizeof(int)), s>>>(bins.counts[bin], bins.list.p + bins.base(bin), cap, aS, aP, aV, bS, bP, bV, cStart, cPos, out, d_badRow);
	}
	if (bins.counts[3] > 0) {
		numericGlobalKernel<T><<<bins.counts[3], GTPB, 0, s>>>(bins.counts[3], bins.list.p + bins.base(3), aS, aP, aV, bS, bP, bV, cStart, cPos, out, d_badRow);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

BinCuts numericCuts() {
	BinCuts c{};
	for (int i = 0; i < NUM_BINS - 1; ++i) c.upTo[i] = NUM_UP[i];
	c.bins = NUM_BINS;
	return c;
}

BinCuts symbolicCuts() {
	BinCuts c{};
	for (int i = 0; i < MAXBINS - 1; ++i) c.upTo[i] = SYM_UP[i];
	c.bins = MAXBINS;
	return c;
}

template <bool FILL>
int enqueueSymbolicLds(const RowBins& bins, const smm_hip_csr* a, const smm_hip_csr* b, int* count, const int* cStart, int* cols, hipStream_t s) {
	const int* aS = a->d_start;
	const int* aP = a->d_positions;
	const int* bS = b->d_start;
	const int* bP = b->d_positions;
	if (bins.counts[0] > 0) {
		const int slots = SYM_SLOTS[0], shift = 32 - bitsFor(slots);
		const int* list = bins.list.p + bins.base(0);
		if (smallGroup(b) == 8) {
			symbolicLdsKernel<8, GTPB, FILL><<<gridOf(bins.counts[0], GTPB / 8), GTPB, (GTPB / 8) * slots * sizeof(int), s>>>(bins.counts[0], list, slots, shift, aS, aP, bS, bP, count, cStart, cols);
		} else {
			symbolicLdsKernel<32, GTPB, FILL><<<gridOf(bins.counts[0], GTPB / 32), GTPB, (GTPB / 32) * slots * sizeof(int), s>>>(bins.counts[0], list, slots, shift, aS, aP, bS, bP, count, cStart, cols);
		}
	}
	for (int bin = 1; bin <= 3; ++bin) {
		if (bins.counts[bin] == 0) continue;
		const int slots = SYM_SLOTS[bin], shift = 32 - bitsFor(slots);
		symbolicLdsKernel<WAVE, WAVE, FILL><<<bins.counts[bin], WAVE, slots * sizeof(int), s>>>(bins.counts[bin], bins.list.p + bins.base(bin), slots, shift, aS, aP, bS, bP, count, cStart, cols);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template <typename T>
int multiplyCreateTyped(const smm_hip_csr* a, const smm_hip_csr* b, hipStream_t s, smm_hip_csr** out) {
	SetupTrace trace("multiply: create");
	const int m = a->rows, k = a->cols, n = b->cols;
	if (a->nnz < 0 || b->nnz < 0 || (m == 0 && a->nnz != 0) || (k == 0 && b->nnz != 0)) {
		setError("csr_multiply_create: start[] of %s does not ascend from 0", a->nnz < 0 || (m == 0 && a->nnz != 0) ? "a" : "b");
		return SMM_HIP_ERR_INVALID;
	}
	OwnedCsr c;
	SMM_TRY(newOwnedCsr(m, n, a->dtype, &c));
	DevBuf<int> d_bad;  // [0] the check word, [1] the smallest row with a product outside the pattern
	SMM_TRY(d_bad.alloc(2));
	flagsInitKernel<<<1, 64, 0, s>>>(d_bad.p);
	SMM_TRY(enqueueCheck(a, BAD_A_START, BAD_A_COL, d_bad, s));
	SMM_TRY(enqueueCheck(b, BAD_B_START, BAD_B_COL, d_bad, s));
	long long nnzC = 0;
	if (m > 0 && a->nnz > 0 && b->nnz > 0) {
		DevBuf<long long> ub, tableOff;
		DevBuf<unsigned long long> tableSlots;
		SMM_TRY(ub.alloc(static_cast<size_t>(m)));
		SMM_TRY(tableOff.alloc(static_cast<size_t>(m)));
		SMM_TRY(tableSlots.alloc(1));
		SMM_HIP_TRY(hipMemsetAsync(tableSlots.p, 0, sizeof(unsigned long long), s));
		upperBoundKernel<<<gridOf(8LL * m), GTPB, 0, s>>>(m, k, a->nnz, a->d_start, a->d_positions, b->d_start, ub, d_bad);
		RowBins sym;
		SMM_TRY(enqueueBins<false>(sym, m, symbolicCuts(), ub, nullptr, n, tableOff, tableSlots, s));
		int bad = 0;
		unsigned long long slotsTotal = 0;
		SMM_HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipMemcpyAsync(&slotsTotal, tableSlots.p, sizeof(slotsTotal), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (bad) return describeBad(bad, "csr_multiply_create", a, b);
		// ---- symbolic, pass one: the distinct columns of every row
		DevBuf<int> count, tables, cursor;  // count[m + 1]: the last word stays 0, so that the scan's last output is nnz
		SMM_TRY(count.alloc(static_cast<size_t>(m) + 1));
		SMM_HIP_TRY(hipMemsetAsync(count.p, 0, (static_cast<size_t>(m) + 1) * sizeof(int), s));
		SMM_TRY((enqueueSymbolicLds<false>(sym, a, b, count, nullptr, nullptr, s)));
		const int nLong = sym.counts[MAXBINS - 1];
		const int* longList = sym.list.p + sym.base(MAXBINS - 1);
		if (nLong > 0) {
			SMM_TRY(tables.alloc(static_cast<size_t>(slotsTotal)));
			SMM_HIP_TRY(hipMemsetAsync(tables.p, 0xFF, static_cast<size_t>(slotsTotal) * sizeof(int), s));
			symbolicGlobalCountKernel<<<nLong, GTPB, 0, s>>>(nLong, longList, n, ub, tableOff, tables, a->d_start, a->d_positions, b->d_start, b->d_positions, count);
			SMM_HIP_TRY(hipGetLastError());
		}
		SMM_TRY(startsFromCounts("csr_multiply_create", "product", count.p, m, c.get(), &nnzC, s));
		SMM_TRY(allocCsrEntries(c.get(), nnzC, false));
		if (nnzC > 0) {
			// ---- symbolic, pass two: the columns in table order, then ascending
			DevBuf<int> unsorted;
			SMM_TRY(unsorted.alloc(static_cast<size_t>(nnzC)));
			SMM_TRY((enqueueSymbolicLds<true>(sym, a, b, nullptr, c->d_start, unsorted, s)));
			if (nLong > 0) {
				SMM_TRY(cursor.alloc(static_cast<size_t>(m)));
				SMM_HIP_TRY(hipMemsetAsync(cursor.p, 0, static_cast<size_t>(m) * sizeof(int), s));
				symbolicGlobalFillKernel<<<nLong, GTPB, 0, s>>>(nLong, longList, n, ub, tableOff, tables, c->d_start, cursor, unsorted);
				SMM_HIP_TRY(hipGetLastError());
			}
			SMM_TRY(sortKeysSegmented(reinterpret_cast<unsigned*>(unsorted.p), reinterpret_cast<unsigned*>(c->d_positions), static_cast<unsigned>(nnzC),
			                          static_cast<unsigned>(m), c->d_start, c->d_start + 1, static_cast<unsigned>(std::max(1, bitsFor(n))), s));
			// ---- numeric: the same code as multiply_into
			RowBins num;
			SMM_TRY(enqueueBins<true>(num, m, numericCuts(), nullptr, c->d_start, n, nullptr, nullptr, s));
			SMM_HIP_TRY(hipStreamSynchronize(s));
			SMM_TRY(enqueueNumeric<T>(num, a, b, c->d_start, c->d_positions, nnzC, static_cast<T*>(c->d_values), d_bad.p + 1, s));
			int badRow = NO_ROW;
			SMM_HIP_TRY(hipMemcpyAsync(&badRow, d_bad.p + 1, sizeof(int), hipMemcpyDeviceToHost, s));
			SMM_HIP_TRY(hipStreamSynchronize(s));
			if (badRow != NO_ROW) {  // (the symbolic phase stored every product's place: this would be a defect of the library)
				setError("csr_multiply_create: internal error, a product of row %d has no place in the pattern", badRow);
				return SMM_HIP_ERR_INVALID;
			}
		}
	} else {
		int bad = 0;
		SMM_HIP_TRY(hipGetLastError());
		SMM_HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (bad) return describeBad(bad, "csr_multiply_create", a, b);
		SMM_HIP_TRY(hipMemsetAsync(c->d_start, 0, (static_cast<size_t>(m) + 1) * sizeof(int), s));
	}
	if (!c->d_positions) SMM_TRY(allocCsrEntries(c.get(), 0, false));
	SMM_TRY(ensureCsrReady(c.get(), s, true));  // nnz, the first active row, the typical row and the kernel choice as for caller-owned device arrays
	*out = c.release();
	return SMM_HIP_OK;
}

template <typename T>
int multiplyIntoTyped(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b, hipStream_t s) {
	const char* what = "csr_multiply_into";
	if (!c || !a || !b) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (c == a || c == b) {
		setError("%s: c must not be a or b", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (c->dtype != dtypeOf<T>() || a->dtype != dtypeOf<T>() || b->dtype != dtypeOf<T>()) {
		setError("%s: a matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->cols != b->rows || c->rows != a->rows || c->cols != b->cols) {
		setError("%s: shapes %d x %d, %d x %d and c %d x %d do not fit", what, a->rows, a->cols, b->rows, b->cols, c->rows, c->cols);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	SMM_TRY(ensureCsrReady(c, s, true));
	const int m = c->rows;
	if (a->nnz < 0 || b->nnz < 0 || c->nnz < 0 || (m == 0 && (a->nnz != 0 || c->nnz != 0)) || (b->rows == 0 && b->nnz != 0)) {
		setError("%s: a start[] does not ascend from 0", what);
		return SMM_HIP_ERR_INVALID;
	}
	DevBuf<int> d_bad;
	SMM_TRY(d_bad.alloc(2));
	flagsInitKernel<<<1, 64, 0, s>>>(d_bad.p);
	SMM_TRY(enqueueCheck(a, BAD_A_START, BAD_A_COL, d_bad, s));
	SMM_TRY(enqueueCheck(b, BAD_B_START, BAD_B_COL, d_bad, s));
	SMM_TRY(enqueueCheck(c, BAD_C_START, 0, d_bad, s));  // (c's columns are only compared with, never used as an address)
	RowBins num;
	if (m > 0) SMM_TRY(enqueueBins<true>(num, m, numericCuts(), nullptr, c->d_start, c->cols, nullptr, nullptr, s));
	int bad = 0;
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (bad) return describeBad(bad, what, a, b);
	// (the bins were cut from c's start[] before the check's verdict was known: they only counted)
	DevBuf<T> scratch;
	SMM_TRY(scratch.alloc(static_cast<size_t>(c->nnz)));
	if (a->nnz > 0 && b->nnz > 0) {
		// (also when c stores nothing: its rows are all in the first bin, no entry is read or written, and a product that lands raises the row)
		SMM_TRY(enqueueNumeric<T>(num, a, b, c->d_start, c->d_positions, c->nnz, scratch.p, d_bad.p + 1, s));
	} else if (c->nnz > 0) {
		SMM_HIP_TRY(hipMemsetAsync(scratch.p, 0, static_cast<size_t>(c->nnz) * sizeof(T), s));
	}
	int badRow = NO_ROW;
	SMM_HIP_TRY(hipMemcpyAsync(&badRow, d_bad.p + 1, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (badRow != NO_ROW) {
		setError("%s: a product of row %d falls on an entry that c does not store", what, badRow);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(adoptValues(c, scratch, s));
	return csrValuesEdited(c, s);
}

}  // namespace
}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_multiply_create(const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream, smm_hip_csr** out) {
	if (!out) {
		setError("csr_multiply_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!a || !b) {
		setError("csr_multiply_create: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->dtype != b->dtype) {
		setError("csr_multiply_create: the matrices hold different element types");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->cols != b->rows) {
		setError("csr_multiply_create: a has %d columns, b has %d rows", a->cols, b->rows);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	return a->dtype == SMM_DTYPE_F32 ? multiplyCreateTyped<float>(a, b, s, out) : multiplyCreateTyped<double>(a, b, s, out);
}

int smm_hip_csr_multiply_into_f32(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream) {
	return multiplyIntoTyped<float>(c, a, b, pickStream(stream));
}
int smm_hip_csr_multiply_into_f64(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b, smm_hip_stream stream) {
	return multiplyIntoTyped<double>(c, a, b, pickStream(stream));
}

}  // extern "C"
