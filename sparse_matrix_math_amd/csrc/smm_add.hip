// smm_add.hip -- C = alpha A + beta B for two CSR matrices of one shape ON THE DEVICE: the union of the two patterns as an ordinary
// smm_hip_csr handle (smm_hip_csr_add_create_*) and the numeric phase alone into an existing pattern (smm_hip_csr_add_into_*).
// Both operands hold their columns ascending strictly inside every row, so nothing is sorted and nothing needs an atomic: the union is a
// MERGE BY RANKING -- the place of an entry in C's row is its rank in its own row plus the number of the other operand's entries of that
// row that come before it and are not stored twice.
//   lanes and work: every kernel deals STORED ENTRIES flat over lanes, 256 per workgroup, whatever the row lengths -- a 7-entry stencil row
//     and a 5 000-entry row both read their entries coalesced and keep every lane of the wavefront busy; no lane walks a row.  The row of an
//     entry is found from start[]: a small kernel searches all of start[] for the rows of every workgroup's first and last entry, every lane
//     then searches between those two.  The columns of the OTHER matrix that the workgroup's rows can meet -- positions[start[first row] ..
//     start[last row + 1]) -- are what every lane searches: when they are at most ADD_SEG = 1024 they are staged in LDS (4 KiB per searched
//     matrix) and searched there, beyond that (a workgroup inside or across rows longer than that) in global memory.  That is the one
//     threshold of this unit.
//   check (an operand not yet known to be good; the verdict is kept in the handle): one lane per row and per stored entry: start[] ascends
//     from 0 to nnz, columns lie in [0, cols), positions[k] < positions[k + 1] inside a row.  A failure raises a bit of a device word and the
//     smallest offending row (integer atomicMin); the host reads the word before any other kernel of the call is queued.
//   symbolic: one lane per stored entry of b: a binary search of a's row; isNew[q] = 1 when the column is not there, where[q] = the index in
//     a's arrays of the first entry of the row with a larger column.  One exclusive scan (rocprim, a set-up pass) turns isNew[] into
//     N[q] = new entries before q, N[nnz_b] = all of them.  nnz_c = nnz_a + N[nnz_b] is formed in 64 bits on the host (refused beyond
//     2^31 - 1), start_c[i] = start_a[i] + N[start_b[i]].
//   fill (create): an entry of a at index e lands at e + N[lb], lb = the index in b's arrays of the first entry of the row with a column not
//     smaller -- its own rank, a's rows before it, and the new entries of b before it --, with the value u + v when b stores the column and
//     u when not; a NEW entry of b at index q lands at where[q] + N[q] with the value v.  Every slot of C is written once, by one lane.
//   numeric (into): one lane per stored entry of c looks its column up in a's row and in b's row and writes u + v, u, v or +0.0 into
//     scratch: coalesced, no conflicts.  That an operand stores nothing outside c is proved from the operand's side: one lane per stored
//     entry of a (of b) looks its column up in c's row; a miss raises the smallest such row (integer atomicMin).  Columns are distinct, so
//     every entry found is the count the header asks for.  Skipped for an operand that IS c.  Then as smm_hip_csr_multiply_into_*: the word
//     is read (the call synchronises), the scratch becomes c's values (owned arrays: pointer swap; caller-owned: one copy), csrValuesEdited.
//   values: u = alpha * a_ij and v = beta * b_ij are one rounding each, u + v one more (the build has -ffp-contract=off; no smmFma): both
//     library flavours give the same bits, which are those of the assembly of a's scaled triplets followed by b's.
//   Bytes (s = sizeof(T)): check (nnz + rows) 4 per operand, once per handle; symbolic (nnz_a + nnz_b) 4 read, nnz_b 8 written and scanned;
//     fill / numeric (nnz_a + nnz_b)(s + 4) read plus the probes of the searches (LDS or cache), nnz_c (s + 4) written (create) or
//     nnz_c s (into, plus nnz_c 4 of c's columns read).
#include <climits>

#include "smm_csr_build.h"
#include "smm_device.h"

namespace smm {
namespace {

constexpr int ATPB = BUILD_TPB;
constexpr int ADD_SEG = 1024;  // columns of a searched row segment a workgroup stages in LDS; longer segments are searched in global memory

// the words of a call
constexpr int W_BITS = 0;       // what the check found: (BAD_START | BAD_COL | BAD_ORDER) << (3 * operand), operand 0 = a, 1 = b, 2 = c
constexpr int W_START_ROW = 1;  // + operand: the smallest row whose start[] is wrong
constexpr int W_ENTRY_ROW = 4;  // + operand: the smallest row with a column out of range or out of order
constexpr int W_MISS_ROW = 7;   // + operand (0, 1): the smallest row of the operand with an entry c does not store
constexpr int N_WORDS = 9;
constexpr int NO_ROW = INT_MAX;
constexpr int BAD_START = 1, BAD_COL = 2, BAD_ORDER = 4;

__global__ void wordsInitKernel(int* words) {
	if (blockIdx.x == 0 && threadIdx.x < N_WORDS) words[threadIdx.x] = threadIdx.x == W_BITS ? 0 : NO_ROW;
}

// the row r of lo .. hi with start[r] <= e < start[r + 1], given start[lo] <= e < start[hi + 1].  On a start[] that does not ascend it
// still ends and still returns a row of lo .. hi
__device__ __forceinline__ int rowOfEntry(const int* __restrict__ start, int lo, int hi, int e) {
	while (lo < hi) {
		const int mid = lo + ((hi - lo + 1) >> 1);
		if (start[mid] <= e) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

// range[2 k], range[2 k + 1] = the rows of the first and the last entry of workgroup k (entries k ATPB .. min((k + 1) ATPB, nnz) - 1): one lane
// per word, so that the two searches of all of start[] are not at the head of every workgroup of every kernel
__global__ __launch_bounds__(ATPB) void blockRowsKernel(int rows, int nnz, const int* __restrict__ start, int blocks, int* __restrict__ range) {
	const long long t = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (t >= 2LL * blocks) return;
	const long long k = t >> 1;
	const long long e = (t & 1) ? min((k + 1) * ATPB, static_cast<long long>(nnz)) - 1 : k * ATPB;
	range[t] = rowOfEntry(start, 0, rows - 1, static_cast<int>(e));
}

// the row of this lane's entry, searched between the rows of the workgroup's first and last entry (range[0], range[1]); a lane whose entry
// lies beyond nnz gets the last one's
__device__ __forceinline__ int laneRow(const int* __restrict__ start, int nnz, long long first, const int* range) {
	const long long e = min(first + threadIdx.x, static_cast<long long>(nnz) - 1);
	return rowOfEntry(start, range[0], range[1], static_cast<int>(e));
}

// the first index of lo .. hi - 1 whose column is not below col (hi when there is none); cols[] is indexed by index - base
__device__ __forceinline__ int lowerBound(const int* cols, int base, int lo, int hi, int col) {
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (cols[mid - base] < col) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// The columns of the rows range[0] .. range[1] of a matrix, staged in lds[ADD_SEG] when they fit: returns whether they were, *seg0 the index
// of the first.  All lanes of the workgroup call this (a barrier inside).
__device__ __forceinline__ bool stageSegment(const int* __restrict__ start, const int* __restrict__ positions, const int* range, int* lds, int* seg0) {
	const int s0 = start[range[0]], s1 = start[range[1] + 1];
	const bool staged = s1 - s0 <= ADD_SEG;
	if (staged) {
		for (int t = s0 + static_cast<int>(threadIdx.x); t < s1; t += ATPB) lds[t - s0] = positions[t];
	}
	__syncthreads();
	*seg0 = s0;
	return staged;
}

// col in the row lo .. hi - 1 of the staged / global columns: *hit whether it is stored, the lower bound either way
__device__ __forceinline__ int findColumn(bool staged, const int* lds, int seg0, const int* __restrict__ positions, int lo, int hi, int col, bool* hit) {
	int lb;
	if (staged) {
		lb = lowerBound(lds, seg0, lo, hi, col);
		*hit = lb < hi && lds[lb - seg0] == col;
	} else {
		lb = lowerBound(positions, 0, lo, hi, col);
		*hit = lb < hi && positions[lb] == col;
	}
	return lb;
}

__device__ __forceinline__ void raise(int* words, int bit, int operand, int rowWord, int row) {
	atomicOr(&words[W_BITS], bit << (3 * operand));
	atomicMin(&words[rowWord + operand], row);
}

// One lane per row and per stored entry.  Reads start[0 .. rows] and positions[0 .. nnz) only, whatever they hold.
__global__ __launch_bounds__(ATPB) void checkKernel(int rows, int cols, int nnz, const int* __restrict__ start, const int* __restrict__ positions, int operand,
                                                    int* words) {
	__shared__ int range[2];
	const long long first = static_cast<long long>(blockIdx.x) * ATPB;
	const long long i = first + threadIdx.x;
	if (i < rows) {
		const int s0 = start[i], s1 = start[i + 1];
		if (s0 > s1 || (i == 0 && s0 != 0) || (i == rows - 1 && s1 != nnz)) raise(words, BAD_START, operand, W_START_ROW, static_cast<int>(i));
	}
	if (first >= nnz) return;  // (the whole workgroup)
	if (threadIdx.x < 2) {  // (start[] is not known to ascend yet: searched here, on whatever it holds)
		const long long e = threadIdx.x == 0 ? first : min(first + ATPB, static_cast<long long>(nnz)) - 1;
		range[threadIdx.x] = rowOfEntry(start, 0, rows - 1, static_cast<int>(e));
	}
	__syncthreads();
	const int r = laneRow(start, nnz, first, range);
	if (i >= nnz) return;
	const int c = positions[i];
	if (c < 0 || c >= cols) raise(words, BAD_COL, operand, W_ENTRY_ROW, r);
	if (i + 1 < nnz && i + 1 < start[r + 1] && positions[i + 1] <= c) raise(words, BAD_ORDER, operand, W_ENTRY_ROW, r);
}

// one lane per stored entry of b: isNew[q], where[q] (see the head of the file)
__global__ __launch_bounds__(ATPB) void symbolicKernel(const int* __restrict__ ranges, int nnzB, const int* __restrict__ aStart, const int* __restrict__ aPos,
                                                       const int* __restrict__ bStart, const int* __restrict__ bPos, int* __restrict__ isNew, int* __restrict__ where) {
	__shared__ int ldsA[ADD_SEG];
	const long long first = static_cast<long long>(blockIdx.x) * ATPB;
	const int* range = ranges + 2 * static_cast<size_t>(blockIdx.x);
	const int row = laneRow(bStart, nnzB, first, range);
	int seg0;
	const bool staged = stageSegment(aStart, aPos, range, ldsA, &seg0);
	const long long q = first + threadIdx.x;
	if (q >= nnzB) return;
	bool hit;
	const int lb = findColumn(staged, ldsA, seg0, aPos, aStart[row], aStart[row + 1], bPos[q], &hit);
	isNew[q] = hit ? 0 : 1;
	where[q] = lb;
}

// start_c[i] = start_a[i] + N[start_b[i]] for i <= rows (N null: b stores nothing)
__global__ __launch_bounds__(ATPB) void startKernel(int rows, const int* __restrict__ aStart, const int* __restrict__ bStart, const int* __restrict__ N,
                                                    int* __restrict__ cStart) {
	const long long i = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (i <= rows) cStart[i] = aStart[i] + (N ? N[bStart[i]] : 0);
}

// one lane per stored entry of a: its place in C, its column, u + v or u
template <typename T>
__global__ __launch_bounds__(ATPB) void fillFromAKernel(const int* __restrict__ ranges, int nnzA, const int* __restrict__ aStart, const int* __restrict__ aPos, const T* __restrict__ aVal,
                                                        T alpha, const int* __restrict__ bStart, const int* __restrict__ bPos, const T* __restrict__ bVal, T beta,
                                                        const int* __restrict__ N, int* __restrict__ cPos, T* __restrict__ cVal) {
	__shared__ int ldsB[ADD_SEG];
	const long long first = static_cast<long long>(blockIdx.x) * ATPB;
	const int* range = ranges + 2 * static_cast<size_t>(blockIdx.x);
	const int row = laneRow(aStart, nnzA, first, range);
	int seg0;
	const bool staged = stageSegment(bStart, bPos, range, ldsB, &seg0);
	const long long e = first + threadIdx.x;
	if (e >= nnzA) return;
	const int col = aPos[e];
	bool hit;
	const int lb = findColumn(staged, ldsB, seg0, bPos, bStart[row], bStart[row + 1], col, &hit);
	const T u = alpha * aVal[e];
	T c = u;
	if (hit) {
		const T v = beta * bVal[lb];
		c = u + v;
	}
	const long long dest = e + (N ? N[lb] : 0);
	cPos[dest] = col;
	cVal[dest] = c;
}

// one lane per stored entry of b: a new one lands at where[q] + N[q] with the value v
template <typename T>
__global__ __launch_bounds__(ATPB) void fillFromBKernel(int nnzB, const int* __restrict__ bPos, const T* __restrict__ bVal, T beta, const int* __restrict__ N,
                                                        const int* __restrict__ where, int* __restrict__ cPos, T* __restrict__ cVal) {
	const long long q = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (q >= nnzB) return;
	const int before = N[q];
	if (N[q + 1] == before) return;
	const long long dest = static_cast<long long>(where[q]) + before;
	cPos[dest] = bPos[q];
	cVal[dest] = beta * bVal[q];
}

// one lane per stored entry of c: out[e] = u + v, u, v or +0.0
template <typename T>
__global__ __launch_bounds__(ATPB) void numericKernel(const int* __restrict__ ranges, int nnzC, const int* __restrict__ cStart, const int* __restrict__ cPos, const int* __restrict__ aStart,
                                                      const int* __restrict__ aPos, const T* __restrict__ aVal, T alpha, const int* __restrict__ bStart,
                                                      const int* __restrict__ bPos, const T* __restrict__ bVal, T beta, T* __restrict__ out) {
	__shared__ int ldsA[ADD_SEG], ldsB[ADD_SEG];
	const long long first = static_cast<long long>(blockIdx.x) * ATPB;
	const int* range = ranges + 2 * static_cast<size_t>(blockIdx.x);
	const int row = laneRow(cStart, nnzC, first, range);
	int segA, segB;
	const bool stagedA = stageSegment(aStart, aPos, range, ldsA, &segA);
	const bool stagedB = stageSegment(bStart, bPos, range, ldsB, &segB);
	const long long e = first + threadIdx.x;
	if (e >= nnzC) return;
	const int col = cPos[e];
	bool hitA, hitB;
	const int ia = findColumn(stagedA, ldsA, segA, aPos, aStart[row], aStart[row + 1], col, &hitA);
	const int ib = findColumn(stagedB, ldsB, segB, bPos, bStart[row], bStart[row + 1], col, &hitB);
	T c = T(0);
	if (hitA) {
		const T u = alpha * aVal[ia];
		c = u;
		if (hitB) {
			const T v = beta * bVal[ib];
			c = u + v;
		}
	} else if (hitB) {
		c = beta * bVal[ib];
	}
	out[e] = c;
}

// one lane per stored entry of an operand: is its column stored in c's row?
__global__ __launch_bounds__(ATPB) void coveredKernel(const int* __restrict__ ranges, int nnzO, const int* __restrict__ oStart, const int* __restrict__ oPos, const int* __restrict__ cStart,
                                                      const int* __restrict__ cPos, int operand, int* words) {
	__shared__ int ldsC[ADD_SEG];
	const long long first = static_cast<long long>(blockIdx.x) * ATPB;
	const int* range = ranges + 2 * static_cast<size_t>(blockIdx.x);
	const int row = laneRow(oStart, nnzO, first, range);
	int seg0;
	const bool staged = stageSegment(cStart, cPos, range, ldsC, &seg0);
	const long long e = first + threadIdx.x;
	if (e >= nnzO) return;
	bool hit;
	(void)findColumn(staged, ldsC, seg0, cPos, cStart[row], cStart[row + 1], oPos[e], &hit);
	if (!hit) atomicMin(&words[W_MISS_ROW + operand], row);
}

int enqueueBlockRows(const smm_hip_csr* m, DevBuf<int>& ranges, hipStream_t s) {
	const int blocks = gridOf(m->nnz);
	SMM_TRY(ranges.alloc(2 * static_cast<size_t>(blocks)));
	if (m->nnz > 0) blockRowsKernel<<<gridOf(2LL * blocks), ATPB, 0, s>>>(m->rows, m->nnz, m->d_start, blocks, ranges.p);
	return SMM_HIP_OK;
}

// What the host can tell without the device, then the check of every operand not yet known to be good; the word is read before the caller
// queues anything else.  ops[k] may repeat a handle (a == b, c == a): it is checked once, under its first name.
int checkOperands(const char* what, const smm_hip_csr* const* ops, int count, int* d_words, hipStream_t s, const char* const* names = nullptr) {
	static const char* const ABC[3] = {"a", "b", "c"};
	const char* const* NAMES = names ? names : ABC;
	bool queued = false;
	for (int k = 0; k < count; ++k) {
		const smm_hip_csr* m = ops[k];
		if (m->nnz < 0 || (m->rows == 0 && m->nnz != 0)) {
			setError("%s: start[] of %s does not ascend from 0 (row 0)", what, NAMES[k]);
			return SMM_HIP_ERR_INVALID;
		}
		bool seen = m->sorted_ok.load(std::memory_order_acquire) == 1;
		for (int j = 0; j < k; ++j) seen = seen || ops[j] == m;
		const long long work = std::max<long long>(m->rows, m->nnz);
		if (seen || work == 0) continue;
		checkKernel<<<gridOf(work), ATPB, 0, s>>>(m->rows, m->cols, m->nnz, m->d_start, m->d_positions, k, d_words);
		queued = true;
	}
	if (!queued) return SMM_HIP_OK;
	int words[N_WORDS];
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	for (int k = 0; k < count; ++k) {
		const int bad = (words[W_BITS] >> (3 * k)) & 7;
		if (bad & BAD_START) {
			setError("%s: start[] of %s does not ascend from 0 to its entry count, first at row %d ", what, NAMES[k], words[W_START_ROW + k]);
			return SMM_HIP_ERR_INVALID;
		}
		if (bad) {
			setError("%s: the columns of %s must lie in [0, %d) and ascend strictly inside a row, first broken in row %d %s", what, NAMES[k], ops[k]->cols,
			         words[W_ENTRY_ROW + k], bad & BAD_COL ? "(a column lies outside)" : "(out of order or repeated)");
			return SMM_HIP_ERR_INVALID;
		}
	}
	for (int k = 0; k < count; ++k) ops[k]->sorted_ok.store(1, std::memory_order_release);
	return SMM_HIP_OK;
}

template <typename T>
int addCreateTyped(const smm_hip_csr* a, T alpha, const smm_hip_csr* b, T beta, hipStream_t s, smm_hip_csr** out) {
	SetupTrace trace("add: create");
	const char* what = "csr_add_create";
	const int m = a->rows;
	DevBuf<int> d_words;
	SMM_TRY(d_words.alloc(N_WORDS));
	wordsInitKernel<<<1, 64, 0, s>>>(d_words.p);
	const smm_hip_csr* ops[2] = {a, b};
	SMM_TRY(checkOperands(what, ops, 2, d_words, s));
	OwnedCsr c;
	SMM_TRY(newOwnedCsr(m, a->cols, a->dtype, &c));
	const int nnzA = a->nnz, nnzB = b->nnz;
	DevBuf<int> rangesA, rangesB, N, where;  // N[nnzB + 1]: isNew[] before the scan (the last word 0), the new entries before q after it
	int newTotal = 0;
	if (nnzB > 0) {
		SMM_TRY(N.alloc(static_cast<size_t>(nnzB) + 1));
		SMM_TRY(where.alloc(static_cast<size_t>(nnzB)));
		SMM_HIP_TRY(hipMemsetAsync(N.p + nnzB, 0, sizeof(int), s));
		SMM_TRY(enqueueBlockRows(b, rangesB, s));
		symbolicKernel<<<gridOf(nnzB), ATPB, 0, s>>>(rangesB.p, nnzB, a->d_start, a->d_positions, b->d_start, b->d_positions, N.p, where.p);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(scanExclusive(N.p, N.p, static_cast<size_t>(nnzB) + 1, s));
		SMM_HIP_TRY(hipMemcpyAsync(&newTotal, N.p + nnzB, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	const long long nnzC = static_cast<long long>(nnzA) + newTotal;  // (newTotal <= nnzB fits 32 bits; the sum may not)
	if (nnzC > INT_MAX) {
		setError("%s: the sum holds %lld entries, more than 2^31 - 1", what, nnzC);
		return SMM_HIP_ERR_INVALID;
	}
	startKernel<<<gridOf(m + 1LL), ATPB, 0, s>>>(m, a->d_start, b->d_start, nnzB > 0 ? N.p : nullptr, c->d_start);
	SMM_TRY(allocCsrEntries(c.get(), nnzC, false));
	T* cVal = static_cast<T*>(c->d_values);
	if (nnzA > 0) {
		SMM_TRY(enqueueBlockRows(a, rangesA, s));
		fillFromAKernel<T><<<gridOf(nnzA), ATPB, 0, s>>>(rangesA.p, nnzA, a->d_start, a->d_positions, static_cast<const T*>(a->d_values), alpha, b->d_start, b->d_positions,
		                                                 static_cast<const T*>(b->d_values), beta, nnzB > 0 ? N.p : nullptr, c->d_positions, cVal);
	}
	if (newTotal > 0) fillFromBKernel<T><<<gridOf(nnzB), ATPB, 0, s>>>(nnzB, b->d_positions, static_cast<const T*>(b->d_values), beta, N.p, where.p, c->d_positions, cVal);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(ensureCsrReady(c.get(), s, true));  // nnz, the first active row, the typical row and the kernel choice as for caller-owned device arrays
	c->sorted_ok.store(1, std::memory_order_release);  // (by construction)
	*out = c.release();
	return SMM_HIP_OK;
}

template <typename T>
int addIntoTyped(smm_hip_csr* c, const smm_hip_csr* a, T alpha, const smm_hip_csr* b, T beta, hipStream_t s) {
	const char* what = "csr_add_into";
	if (!c || !a || !b) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (c->dtype != dtypeOf<T>() || a->dtype != dtypeOf<T>() || b->dtype != dtypeOf<T>()) {
		setError("%s: a matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != b->rows || a->cols != b->cols || c->rows != a->rows || c->cols != a->cols) {
		setError("%s: shapes %d x %d, %d x %d and c %d x %d differ", what, a->rows, a->cols, b->rows, b->cols, c->rows, c->cols);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	SMM_TRY(ensureCsrReady(c, s, true));
	const int m = c->rows;
	DevBuf<int> d_words;
	SMM_TRY(d_words.alloc(N_WORDS));
	wordsInitKernel<<<1, 64, 0, s>>>(d_words.p);
	const smm_hip_csr* ops[3] = {a, b, c};
	SMM_TRY(checkOperands(what, ops, 3, d_words, s));
	DevBuf<T> scratch;
	SMM_TRY(scratch.alloc(static_cast<size_t>(c->nnz)));
	DevBuf<int> rangesC, rangesA, rangesB;
	if (c->nnz > 0) {
		SMM_TRY(enqueueBlockRows(c, rangesC, s));
		numericKernel<T><<<gridOf(c->nnz), ATPB, 0, s>>>(rangesC.p, c->nnz, c->d_start, c->d_positions, a->d_start, a->d_positions, static_cast<const T*>(a->d_values), alpha,
		                                                 b->d_start, b->d_positions, static_cast<const T*>(b->d_values), beta, scratch.p);
	}
	if (a != c && a->nnz > 0) {
		SMM_TRY(enqueueBlockRows(a, rangesA, s));
		coveredKernel<<<gridOf(a->nnz), ATPB, 0, s>>>(rangesA.p, a->nnz, a->d_start, a->d_positions, c->d_start, c->d_positions, 0, d_words);
	}
	if (b != c && b != a && b->nnz > 0) {
		SMM_TRY(enqueueBlockRows(b, rangesB, s));
		coveredKernel<<<gridOf(b->nnz), ATPB, 0, s>>>(rangesB.p, b->nnz, b->d_start, b->d_positions, c->d_start, c->d_positions, 1, d_words);
	}
	int miss[2] = {NO_ROW, NO_ROW};
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(miss, d_words.p + W_MISS_ROW, sizeof(miss), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (miss[0] != NO_ROW || miss[1] != NO_ROW) {
		const int op = miss[0] <= miss[1] ? 0 : 1;
		setError("%s: row %d of %s holds an entry that c does not store", what, miss[op], op == 0 ? "a" : "b");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(adoptValues(c, scratch, s));
	return csrValuesEdited(c, s);
}

template <typename T>
int addCreate(const smm_hip_csr* a, T alpha, const smm_hip_csr* b, T beta, smm_hip_stream stream, smm_hip_csr** out) {
	const char* what = "csr_add_create";
	if (!out) {
		setError("%s: out is null", what);
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!a || !b) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->dtype != dtypeOf<T>() || b->dtype != dtypeOf<T>()) {
		setError("%s: a matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != b->rows || a->cols != b->cols) {
		setError("%s: a is %d x %d, b is %d x %d", what, a->rows, a->cols, b->rows, b->cols);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	return addCreateTyped<T>(a, alpha, b, beta, s, out);
}

}  // namespace

int csrCheckSorted(const char* what, const char* name, const smm_hip_csr* m, hipStream_t s) {
	if (m->sorted_ok.load(std::memory_order_acquire) == 1) return SMM_HIP_OK;
	DevBuf<int> d_words;
	SMM_TRY(d_words.alloc(N_WORDS));
	wordsInitKernel<<<1, 64, 0, s>>>(d_words.p);
	return checkOperands(what, &m, 1, d_words, s, &name);
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_add_create_f32(const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta, smm_hip_stream stream, smm_hip_csr** out) {
	return addCreate<float>(a, alpha, b, beta, stream, out);
}
int smm_hip_csr_add_create_f64(const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta, smm_hip_stream stream, smm_hip_csr** out) {
	return addCreate<double>(a, alpha, b, beta, stream, out);
}
int smm_hip_csr_add_into_f32(smm_hip_csr* c, const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta, smm_hip_stream stream) {
	return addIntoTyped<float>(c, a, alpha, b, beta, pickStream(stream));
}
int smm_hip_csr_add_into_f64(smm_hip_csr* c, const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta, smm_hip_stream stream) {
	return addIntoTyped<double>(c, a, alpha, b, beta, pickStream(stream));
}

}  // extern "C"
