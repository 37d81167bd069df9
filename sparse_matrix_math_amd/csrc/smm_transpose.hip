// smm_transpose.hip -- Aᵀ built ON THE DEVICE as an ordinary smm_hip_csr handle, the gather that carries a value edit of A over to it, and
// the symmetry check on top of both.
//   create (smm_hip_csr_transpose_create): one lane per stored entry e finds its row by a binary search of start[] and checks its column
//     against [0, cols) -- a bad index raises a device flag before anything is addressed with it --; a STABLE radix sort of (column, e)
//     over the bits cols needs (rocprim, as in smm_assembly.hip) puts the entries of one column together, source rows ascending: the
//     sorted payload is perm[].  start_T[j] is a binary search of the sorted columns, one lane per row of Aᵀ; one more pass writes
//     positions_T[k] = row(perm[k]) and values_T[k] = values[perm[k]].  Values travel as raw 32- / 64-bit words: no arithmetic, -0.0 and
//     NaN payloads are kept.  No atomics besides the flag (every writer stores the same word): the result depends on the matrix alone.
//     Bytes beside the sort's own passes (nnz 8 per radix digit read and written): nnz (4 + 4 + 4) for keys, payload and rows,
//     nnz (4 + 4 + 2 s) + the gather for the last pass.  perm[nnz] stays with the handle (4 bytes per entry).
//   refresh (smm_hip_csr_transpose_refresh_*): values_T[k] = a.values[perm[k]], asynchronous: nnz (2 s + 4) bytes plus the locality of the
//     gather (a banded matrix's perm[k] stays within the band's width of k).  Then the path of every value edit (csrValuesEdited).
//   symmetric (smm_hip_csr_is_symmetric): a temporary transpose, start[] / positions[] compared into a flag, then one pass of IEEE == into a flag.
#include <algorithm>

#include "smm_csr_build.h"

namespace smm {
namespace {

constexpr int XTPB = BUILD_TPB;

// one lane per stored entry: key = its column (0 for a column outside [0, cols): *bad is raised and the caller stops), seq = e, row = its row
__global__ __launch_bounds__(XTPB) void keyRowKernel(int nnz, int rows, int cols, const int* __restrict__ start, const int* __restrict__ positions,
                                                     unsigned* __restrict__ key, int* __restrict__ seq, int* __restrict__ rowOf, int* bad) {
	const long long e = static_cast<long long>(blockIdx.x) * XTPB + threadIdx.x;
	if (e >= nnz) return;
	const int col = positions[e];
	const bool ok = col >= 0 && col < cols;
	key[e] = ok ? static_cast<unsigned>(col) : 0u;
	seq[e] = static_cast<int>(e);
	rowOf[e] = rowOfEntry(rows, start, static_cast<int>(e));
	if (!ok) *bad = 1;
}

// startT[j] = number of entries in the columns before j: the first sorted key >= j (j = 0 .. cols)
__global__ __launch_bounds__(XTPB) void colStartKernel(int cols, int nnz, const unsigned* __restrict__ key, int* __restrict__ startT) {
	const long long j = static_cast<long long>(blockIdx.x) * XTPB + threadIdx.x;
	if (j > cols) return;
	int lo = 0, hi = nnz;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (key[mid] < static_cast<unsigned>(j)) lo = mid + 1;
		else hi = mid;
	}
	startT[j] = lo;
}

// perm[] holds each of 0 .. nnz - 1 once (the sort's payload): every read below is in range
template <typename W>
__global__ __launch_bounds__(XTPB) void gatherKernel(int nnz, const int* __restrict__ perm, const int* __restrict__ rowOf, const W* __restrict__ values,
                                                     int* __restrict__ positionsT, W* __restrict__ valuesT) {
	const long long k = static_cast<long long>(blockIdx.x) * XTPB + threadIdx.x;
	if (k >= nnz) return;
	const int e = perm[k];
	if (positionsT) positionsT[k] = rowOf[e];
	valuesT[k] = values[e];
}

// Is `a` a matrix with the pattern `at` was built from?  Entry k of at sits in at's row j and names column i; it came from entry e = perm[k]:
// a must hold e in its row i (start[i] <= e < start[i + 1]) with column j.  perm[] is a bijection, so when this holds for every k (and
// rows, cols, nnz agree) every entry of a has the source's row and column: start[] and positions[] are the source's.
__global__ __launch_bounds__(XTPB) void sourceCheckKernel(int nnz, int rowsT, const int* __restrict__ startT, const int* __restrict__ positionsT,
                                                          const int* __restrict__ perm, int rowsA, const int* __restrict__ startA,
                                                          const int* __restrict__ positionsA, int* differs) {
	const long long k = static_cast<long long>(blockIdx.x) * XTPB + threadIdx.x;
	if (k >= nnz) return;
	const int j = rowOfEntry(rowsT, startT, static_cast<int>(k));
	const int i = positionsT[k];  // (in [0, rowsA): written by gatherKernel from rowOfEntry)
	const int e = perm[k];
	if (i < 0 || i >= rowsA || positionsA[e] != j || startA[i] > e || startA[i + 1] <= e) *differs = 1;
}

// IEEE ==: -0.0 equals +0.0, a NaN equals nothing
template <typename T>
__global__ __launch_bounds__(XTPB) void valuesDifferKernel(int nnz, const T* __restrict__ a, const T* __restrict__ b, int* differs) {
	bool d = false;
	for (long long i = static_cast<long long>(blockIdx.x) * XTPB + threadIdx.x; i < nnz; i += static_cast<long long>(gridDim.x) * XTPB) d |= !(a[i] == b[i]);
	if (d) *differs = 1;
}

template <typename T>
int transposeTyped(const smm_hip_csr* a, hipStream_t s, smm_hip_csr** out) {
	using W = typename Word<T>::type;
	SetupTrace trace("transpose: create");
	const int rows = a->rows, cols = a->cols, nnz = a->nnz;
	if (nnz < 0) {
		setError("csr_transpose: start[rows] is negative");
		return SMM_HIP_ERR_INVALID;
	}
	OwnedCsr t;
	SMM_TRY(newOwnedCsr(cols, rows, a->dtype, &t));
	SMM_TRY(allocCsrEntries(t.get(), nnz, true));
	DevBuf<int> d_bad;
	SMM_TRY(d_bad.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
	if (rows > 0) startCheckKernel<<<gridOf(rows), XTPB, 0, s>>>(rows, a->d_start, d_bad);
	if (nnz > 0 && rows > 0) {
		DevBuf<unsigned> keyIn, keyOut;
		DevBuf<int> seqIn, rowOf;
		SMM_TRY(keyIn.alloc(nnz));
		SMM_TRY(seqIn.alloc(nnz));
		SMM_TRY(rowOf.alloc(nnz));
		keyRowKernel<<<gridOf(nnz), XTPB, 0, s>>>(nnz, rows, cols, a->d_start, a->d_positions, keyIn, seqIn, rowOf, d_bad);
		SMM_HIP_TRY(hipGetLastError());
		int bad = 0;
		SMM_TRY(readFlag(d_bad, s, &bad));
		if (bad) {
			setError("csr_transpose: start[] does not ascend from 0 or a column lies outside [0, %d)", cols);
			return SMM_HIP_ERR_INVALID;
		}
		SMM_TRY(keyOut.alloc(nnz));
		SMM_TRY(sortPairs(keyIn.p, keyOut.p, seqIn.p, t->d_tperm, static_cast<size_t>(nnz), static_cast<unsigned>(std::max(1, bitsFor(cols))), s));
		colStartKernel<<<gridOf(cols + 1LL), XTPB, 0, s>>>(cols, nnz, keyOut, t->d_start);
		gatherKernel<W><<<gridOf(nnz), XTPB, 0, s>>>(nnz, t->d_tperm, rowOf, static_cast<const W*>(a->d_values), t->d_positions, static_cast<W*>(t->d_values));
		SMM_HIP_TRY(hipGetLastError());
		// (the temporaries go back to the allocator stream-ordered: a block is handed out again only behind the work that was using it)
	} else {
		SMM_HIP_TRY(hipGetLastError());
		int bad = 0;
		SMM_TRY(readFlag(d_bad, s, &bad));
		if (bad || nnz != 0) {  // (rows == 0 with entries: start[0] != 0)
			setError("csr_transpose: start[] does not ascend from 0");
			return SMM_HIP_ERR_INVALID;
		}
		SMM_HIP_TRY(hipMemsetAsync(t->d_start, 0, (static_cast<size_t>(cols) + 1) * sizeof(int), s));
	}
	t->transposeOf = csrUid(a);
	SMM_TRY(ensureCsrReady(t.get(), s, true));  // nnz, the first active row, the typical row and the kernel choice as for caller-owned device arrays
	*out = t.release();
	return SMM_HIP_OK;
}

int checkCreate(const smm_hip_csr* a, smm_hip_csr** out, const char* what) {
	if (!out) {
		setError("%s: out is null", what);
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!a) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

template <typename T>
int refreshTyped(smm_hip_csr* at, const smm_hip_csr* a, hipStream_t s) {
	using W = typename Word<T>::type;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(at, s, true));
	if (a->rows != at->cols || a->cols != at->rows || a->nnz != at->nnz) {
		setError("csr_transpose_refresh: the matrix has not the shape or the entry count of the transpose's source");
		return SMM_HIP_ERR_INVALID;
	}
	const int nnz = at->nnz;
	bool same = false;
	SMM_TRY(refreshVerdict(a, at->transposeOf, s, [&](int* d_diff) {
		sourceCheckKernel<<<gridOf(nnz), XTPB, 0, s>>>(nnz, at->rows, at->d_start, at->d_positions, at->d_tperm, a->rows, a->d_start, a->d_positions, d_diff);
	}, &same));
	if (!same) {
		setError("csr_transpose_refresh: the matrix has another nonzero pattern than the transpose's source");
		return SMM_HIP_ERR_INVALID;
	}
	if (nnz > 0) {
		gatherKernel<W><<<gridOf(nnz), XTPB, 0, s>>>(nnz, at->d_tperm, nullptr, static_cast<const W*>(a->d_values), nullptr, static_cast<W*>(at->d_values));
		SMM_HIP_TRY(hipGetLastError());
	}
	return csrValuesEdited(at, s);
}

int refreshChecked(smm_hip_csr* at, const smm_hip_csr* a, int dtype, hipStream_t s) {
	if (!at || !a) {
		setError("csr_transpose_refresh: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (at->dtype != dtype || a->dtype != dtype) {
		setError("csr_transpose_refresh: a matrix holds the other element type");
		return SMM_HIP_ERR_INVALID;
	}
	if (at->transposeOf == 0 || (!at->d_tperm && at->nnz != 0)) {
		setError("csr_transpose_refresh: the handle was not made by smm_hip_csr_transpose_create");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	return dtype == SMM_DTYPE_F32 ? refreshTyped<float>(at, a, s) : refreshTyped<double>(at, a, s);
}

int passGrid(long long work) { return static_cast<int>(std::min<long long>(gridOf(work), numCUs() * 8LL)); }

// t is a's transpose (square, so the shapes and nnz agree): do start[] / positions[] differ?
int patternsDiffer(const smm_hip_csr* a, const smm_hip_csr* t, hipStream_t s, int* differ) {
	DevBuf<int> d_diff;
	SMM_TRY(d_diff.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), s));
	intsDifferKernel<<<passGrid(a->rows + 1LL), XTPB, 0, s>>>(a->rows + 1LL, a->d_start, t->d_start, d_diff);
	if (a->nnz > 0) intsDifferKernel<<<passGrid(a->nnz), XTPB, 0, s>>>(a->nnz, a->d_positions, t->d_positions, d_diff);
	SMM_HIP_TRY(hipGetLastError());
	return readFlag(d_diff, s, differ);
}

template <typename T>
int valuesDiffer(const smm_hip_csr* a, const smm_hip_csr* t, hipStream_t s, int* differ) {
	*differ = 0;
	if (a->nnz == 0) return SMM_HIP_OK;
	DevBuf<int> d_diff;
	SMM_TRY(d_diff.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), s));
	valuesDifferKernel<T><<<passGrid(a->nnz), XTPB, 0, s>>>(a->nnz, static_cast<const T*>(a->d_values), static_cast<const T*>(t->d_values), d_diff);
	SMM_HIP_TRY(hipGetLastError());
	return readFlag(d_diff, s, differ);
}

}  // namespace

int csrTransposeCreate(const smm_hip_csr* a, hipStream_t s, smm_hip_csr** out) {
	SMM_TRY(ensureCsrReady(a, s, true));
	return a->dtype == SMM_DTYPE_F32 ? transposeTyped<float>(a, s, out) : transposeTyped<double>(a, s, out);
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_transpose_create(const smm_hip_csr* a, smm_hip_stream stream, smm_hip_csr** out) {
	SMM_TRY(checkCreate(a, out, "csr_transpose_create"));
	return csrTransposeCreate(a, pickStream(stream), out);
}

int smm_hip_csr_transpose_refresh_f32(smm_hip_csr* at, const smm_hip_csr* a, smm_hip_stream stream) {
	return refreshChecked(at, a, SMM_DTYPE_F32, pickStream(stream));
}
int smm_hip_csr_transpose_refresh_f64(smm_hip_csr* at, const smm_hip_csr* a, smm_hip_stream stream) {
	return refreshChecked(at, a, SMM_DTYPE_F64, pickStream(stream));
}

int smm_hip_csr_is_symmetric(const smm_hip_csr* a, int* pattern_symmetric, int* values_symmetric) {
	if (pattern_symmetric) *pattern_symmetric = 0;
	if (values_symmetric) *values_symmetric = 0;
	if (!a) {
		setError("csr_is_symmetric: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	if (a->rows != a->cols) return SMM_HIP_OK;
	SMM_HIP_TRY(hipDeviceSynchronize());  // (no stream: the arrays may still be being written on any of the caller's streams)
	hipStream_t s = libStream();
	smm_hip_csr* raw = nullptr;
	SMM_TRY(csrTransposeCreate(a, s, &raw));
	OwnedCsr t(raw);
	int differ = 0;
	SMM_TRY(patternsDiffer(a, t.get(), s, &differ));
	if (differ) return SMM_HIP_OK;
	if (pattern_symmetric) *pattern_symmetric = 1;
	if (a->dtype == SMM_DTYPE_F32) SMM_TRY(valuesDiffer<float>(a, t.get(), s, &differ));
	else SMM_TRY(valuesDiffer<double>(a, t.get(), s, &differ));
	if (values_symmetric) *values_symmetric = differ ? 0 : 1;
	return SMM_HIP_OK;
}

int smm_hip_csr_get_pattern(const smm_hip_csr* m, int* start, int* positions) {
	if (!m) {
		setError("csr_get_pattern: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	hipStream_t s = libStream();
	if (start) SMM_TRY(devToHost(start, m->d_start, (static_cast<size_t>(m->rows) + 1) * sizeof(int), s));
	if (positions && m->nnz > 0) SMM_TRY(devToHost(positions, m->d_positions, static_cast<size_t>(m->nnz) * sizeof(int), s));
	return SMM_HIP_OK;
}

}  // extern "C"
