// smm_color.hip -- a colouring of the adjacency graph of a square matrix and the symmetric permutation B = P A Pᵀ of a handle, both ON THE
// DEVICE.  Together they are the set-up of the multicolour preconditioners (smm_precond_mc.hip); each is also an entry point of its own.
//   colour (smm_hip_csr_color*): vertices are the rows; i != j are adjacent when (i, j) or (j, i) is stored (explicit zeros count).  The
//     in-neighbours come from the library's own transpose (smm_transpose.hip), which is dropped again when its pattern equals A's.
//     key(i) = splitmix64(i + 1) is a bijection, so no two vertices tie.  A round is two launches, one lane per row: PICK marks every
//     uncoloured vertex whose key exceeds the keys of all its uncoloured neighbours and counts the uncoloured vertices it did not mark;
//     ASSIGN gives every marked vertex the smallest colour none of its coloured neighbours holds.  Nothing writes a colour during PICK,
//     and the marked vertices are pairwise non-adjacent, so ASSIGN reads only colours of earlier rounds: the result is what sequential
//     greedy colouring in descending key order gives, whatever the scheduling.  The forbidden set is searched in windows of 64 colours
//     (base, base + 64, ...), so the number of colours is bounded by `rows` alone.  The host reads ONE word per round (the count).
//   permute (smm_hip_csr_permute_create*): perm[] is checked on the device (every value in range, none twice: an exchange on inv[] finds a
//     repeat) before anything is addressed with it.  One lane per stored entry e forms the 64-bit key (inv[row] << 32) | inv[column]; a
//     radix sort of (key, e) over the bits 2 x rows need (rocprim, as in smm_transpose.hip) orders the entries by new row, then new column;
//     the payload is the entry map.  start_B[i] is a binary search of the sorted keys, positions_B[k] the key's low word, values_B[k] =
//     values[map[k]] as raw words.  Keys are distinct, so the result depends on the matrix and the permutation alone.
//   refresh (smm_hip_csr_permute_refresh_*): values_B[k] = a.values[map[k]], asynchronous, then the path of every value edit.
#include <algorithm>

#include "smm_csr_build.h"

namespace smm {
namespace {

constexpr int CTPB = BUILD_TPB;

// one step of the splitmix64 generator from the state x: the golden-ratio increment, then the finalizer
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
	unsigned long long z = x + 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long colorKey(int i) { return splitmix64(static_cast<unsigned long long>(i) + 1ULL); }

// is vertex i beaten by an uncoloured neighbour among positions[b .. e)?  (columns were checked against [0, rows) when the transpose was built)
__device__ __forceinline__ bool beaten(int i, unsigned long long key, const int* __restrict__ positions, int b, int e, const int* __restrict__ colors) {
	bool lost = false;
	for (int k = b; k < e; ++k) {
		const int j = positions[k];
		if (j != i && colors[j] < 0 && colorKey(j) > key) lost = true;
	}
	return lost;
}

// startT == null: the pattern is symmetric, A's rows hold every neighbour
__global__ __launch_bounds__(CTPB) void colorPickKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const int* __restrict__ startT,
                                                        const int* __restrict__ positionsT, const int* __restrict__ colors, unsigned char* __restrict__ pick,
                                                        int* left) {
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	bool waits = false;
	if (i < n) {
		bool take = false;
		if (colors[i] < 0) {
			const int v = static_cast<int>(i);
			const unsigned long long key = colorKey(v);
			bool lost = beaten(v, key, positions, start[i], start[i + 1], colors);
			if (!lost && startT) lost = beaten(v, key, positionsT, startT[i], startT[i + 1], colors);
			take = !lost;
			waits = lost;
		}
		pick[i] = take ? 1 : 0;
	}
	const unsigned long long w = __ballot(waits);
	if ((threadIdx.x & 63) == 0 && w != 0ull) atomicAdd(left, __popcll(w));
}

// the colours of [base, base + 64) held by the neighbours among positions[b .. e), as a mask
__device__ __forceinline__ unsigned long long heldColors(int i, int base, const int* __restrict__ positions, int b, int e, const int* __restrict__ colors) {
	unsigned long long mask = 0ull;
	for (int k = b; k < e; ++k) {
		const int j = positions[k];
		const int c = j != i ? colors[j] : -1;
		if (c >= base && c - base < 64) mask |= 1ull << (c - base);
	}
	return mask;
}

__global__ __launch_bounds__(CTPB) void colorAssignKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const int* __restrict__ startT,
                                                          const int* __restrict__ positionsT, const unsigned char* __restrict__ pick, int* colors, int* top) {
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (i >= n || !pick[i]) return;
	const int v = static_cast<int>(i);
	int color = 0;
	// a vertex of degree d finds a free colour among the first d + 1: at most d / 64 + 1 windows
	for (int base = 0;; base += 64) {
		unsigned long long mask = heldColors(v, base, positions, start[i], start[i + 1], colors);
		if (startT) mask |= heldColors(v, base, positionsT, startT[i], startT[i + 1], colors);
		if (~mask != 0ull) {
			color = base + __builtin_ctzll(~mask);
			break;
		}
	}
	colors[i] = color;  // (read by no marked vertex of this round: they are not adjacent)
	atomicMax(top, color);
}

// ---- permutation -----------------------------------------------------------------------------------------
// inv[perm[i]] = i; *bad when a value lies outside [0, n) or comes twice (inv[] starts as -1 everywhere)
__global__ __launch_bounds__(CTPB) void invertPermKernel(int n, const int* __restrict__ perm, int* inv, int* bad) {
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (i >= n) return;
	const int p = perm[i];
	if (p < 0 || p >= n) {
		*bad = 1;
		return;
	}
	if (atomicExch(inv + p, static_cast<int>(i)) != -1) *bad = 1;
}

__global__ __launch_bounds__(CTPB) void permKeyKernel(int nnz, int n, const int* __restrict__ start, const int* __restrict__ positions, const int* __restrict__ inv,
                                                      unsigned long long* __restrict__ key, int* __restrict__ seq, int* bad) {
	const long long e = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (e >= nnz) return;
	const int col = positions[e];
	const bool ok = col >= 0 && col < n;
	const int row = rowOfEntry(n, start, static_cast<int>(e));
	key[e] = (static_cast<unsigned long long>(static_cast<unsigned>(inv[row])) << 32) | static_cast<unsigned long long>(static_cast<unsigned>(ok ? inv[col] : 0));
	seq[e] = static_cast<int>(e);
	if (!ok) *bad = 1;
}

// startB[i] = the first sorted key of new row i or later (i = 0 .. n)
__global__ __launch_bounds__(CTPB) void permStartKernel(int n, int nnz, const unsigned long long* __restrict__ key, int* __restrict__ startB) {
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (i > n) return;
	const unsigned long long want = static_cast<unsigned long long>(i) << 32;
	int lo = 0, hi = nnz;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (key[mid] < want) lo = mid + 1;
		else hi = mid;
	}
	startB[i] = lo;
}

// map[] holds each of 0 .. nnz - 1 once (the sort's payload): every read below is in range
template <typename W>
__global__ __launch_bounds__(CTPB) void permGatherKernel(int nnz, const int* __restrict__ map, const unsigned long long* __restrict__ key, const W* __restrict__ values,
                                                         int* __restrict__ positionsB, W* __restrict__ valuesB) {
	const long long k = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (k >= nnz) return;
	if (positionsB) positionsB[k] = static_cast<int>(key[k] & 0xFFFFFFFFull);
	valuesB[k] = values[map[k]];
}

// Is `a` a matrix with the pattern `b` was permuted from?  Entry k of b sits in b's row i and names column j; it came from entry e = map[k]:
// a must hold e in its row perm[i] with column perm[j].  map[] is a bijection, so when this holds for every k (and rows, nnz agree) a's
// start[] and positions[] are the source's.
__global__ __launch_bounds__(CTPB) void permSourceCheckKernel(int nnz, int n, const int* __restrict__ startB, const int* __restrict__ positionsB,
                                                              const int* __restrict__ map, const int* __restrict__ perm, const int* __restrict__ startA,
                                                              const int* __restrict__ positionsA, int* differs) {
	const long long k = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (k >= nnz) return;
	const int i = rowOfEntry(n, startB, static_cast<int>(k));
	const int r = perm[i];
	const int c = perm[positionsB[k]];  // (positionsB holds values of inv[]: in [0, n))
	const int e = map[k];
	if (positionsA[e] != c || startA[r] > e || startA[r + 1] <= e) *differs = 1;
}

template <typename T>
int permuteTyped(const smm_hip_csr* a, const int* d_perm, hipStream_t s, smm_hip_csr** out) {
	using W = typename Word<T>::type;
	SetupTrace trace("permute: create");
	const int n = a->rows, nnz = a->nnz;
	if (nnz < 0) {
		setError("csr_permute: start[rows] is negative");
		return SMM_HIP_ERR_INVALID;
	}
	OwnedCsr b;
	SMM_TRY(newOwnedCsr(n, n, a->dtype, &b));
	SMM_TRY(allocCsrEntries(b.get(), nnz, true));
	SMM_TRY(allocArray(&b->d_pperm, static_cast<size_t>(n)));
	DevBuf<int> d_bad, inv;
	SMM_TRY(d_bad.alloc(1));
	SMM_TRY(inv.alloc(std::max(1, n)));
	SMM_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
	SMM_HIP_TRY(hipMemsetAsync(inv, 0xFF, static_cast<size_t>(std::max(1, n)) * sizeof(int), s));  // -1: not named yet
	if (n > 0) {
		invertPermKernel<<<gridOf(n), CTPB, 0, s>>>(n, d_perm, inv, d_bad);
		startCheckKernel<<<gridOf(n), CTPB, 0, s>>>(n, a->d_start, d_bad);
	}
	SMM_HIP_TRY(hipGetLastError());
	int bad = 0;
	SMM_TRY(readFlag(d_bad, s, &bad));
	if (bad || (n == 0 && nnz != 0)) {
		setError("csr_permute: perm[] is not a permutation of 0 .. %d (or start[] does not ascend from 0)", n - 1);
		return SMM_HIP_ERR_INVALID;
	}
	if (n > 0) SMM_HIP_TRY(hipMemcpyAsync(b->d_pperm, d_perm, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToDevice, s));
	if (nnz > 0) {
		DevBuf<unsigned long long> keyIn, keyOut;
		DevBuf<int> seqIn;
		SMM_TRY(keyIn.alloc(nnz));
		SMM_TRY(keyOut.alloc(nnz));
		SMM_TRY(seqIn.alloc(nnz));
		permKeyKernel<<<gridOf(nnz), CTPB, 0, s>>>(nnz, n, a->d_start, a->d_positions, inv, keyIn, seqIn, d_bad);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(readFlag(d_bad, s, &bad));
		if (bad) {
			setError("csr_permute: a column lies outside [0, %d)", n);
			return SMM_HIP_ERR_INVALID;
		}
		const unsigned endBit = 32u + static_cast<unsigned>(std::max(1, bitsFor(n)));
		SMM_TRY(sortPairs(keyIn.p, keyOut.p, seqIn.p, b->d_tperm, static_cast<size_t>(nnz), endBit, s));
		permStartKernel<<<gridOf(n + 1LL), CTPB, 0, s>>>(n, nnz, keyOut, b->d_start);
		permGatherKernel<W><<<gridOf(nnz), CTPB, 0, s>>>(nnz, b->d_tperm, keyOut, static_cast<const W*>(a->d_values), b->d_positions, static_cast<W*>(b->d_values));
		SMM_HIP_TRY(hipGetLastError());
		SMM_HIP_TRY(hipStreamSynchronize(s));  // the temporaries go back to the allocator when this scope ends
	} else {
		SMM_HIP_TRY(hipMemsetAsync(b->d_start, 0, (static_cast<size_t>(n) + 1) * sizeof(int), s));
	}
	b->permuteOf = csrUid(a);
	SMM_TRY(ensureCsrReady(b.get(), s, true));
	*out = b.release();
	return SMM_HIP_OK;
}

template <typename T>
int permuteRefreshTyped(smm_hip_csr* b, const smm_hip_csr* a, hipStream_t s) {
	using W = typename Word<T>::type;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	if (a->rows != b->rows || a->cols != b->cols || a->nnz != b->nnz) {
		setError("csr_permute_refresh: the matrix has not the shape or the entry count of the permutation's source");
		return SMM_HIP_ERR_INVALID;
	}
	const int nnz = b->nnz;
	bool same = false;
	SMM_TRY(refreshVerdict(a, b->permuteOf, s, [&](int* d_diff) {
		permSourceCheckKernel<<<gridOf(nnz), CTPB, 0, s>>>(nnz, b->rows, b->d_start, b->d_positions, b->d_tperm, b->d_pperm, a->d_start, a->d_positions, d_diff);
	}, &same));
	if (!same) {
		setError("csr_permute_refresh: the matrix has another nonzero pattern than the permutation's source");
		return SMM_HIP_ERR_INVALID;
	}
	if (nnz > 0) {
		permGatherKernel<W><<<gridOf(nnz), CTPB, 0, s>>>(nnz, b->d_tperm, nullptr, static_cast<const W*>(a->d_values), nullptr, static_cast<W*>(b->d_values));
		SMM_HIP_TRY(hipGetLastError());
	}
	return csrValuesEdited(b, s);
}

int squareChecked(const smm_hip_csr* a, const char* what) {
	if (!a) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("%s: the matrix is not square", what);
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

}  // namespace

int csrColor(const smm_hip_csr* a, hipStream_t s, int* d_colors, int* ncolors) {
	const int n = a->rows;
	*ncolors = 0;
	if (n == 0) return SMM_HIP_OK;
	// the in-neighbours: the transpose, dropped again when its pattern is A's own (it also checks start[] and the columns)
	smm_hip_csr* raw = nullptr;
	SMM_TRY(csrTransposeCreate(a, s, &raw));
	OwnedCsr t(raw);
	DevBuf<int> words;  // [0] the patterns differ, [1] uncoloured vertices left, [2] the largest colour
	DevBuf<unsigned char> pick;
	SMM_TRY(words.alloc(4));
	SMM_TRY(pick.alloc(n));
	SMM_HIP_TRY(hipMemsetAsync(words, 0, 4 * sizeof(int), s));
	const int passGrid = static_cast<int>(std::min<long long>(gridOf(n + 1LL), numCUs() * 8LL));
	intsDifferKernel<<<passGrid, CTPB, 0, s>>>(n + 1LL, a->d_start, t->d_start, words);
	if (a->nnz > 0) intsDifferKernel<<<passGrid, CTPB, 0, s>>>(a->nnz, a->d_positions, t->d_positions, words);
	SMM_HIP_TRY(hipGetLastError());
	int differ = 0;
	SMM_TRY(readFlag(words, s, &differ));
	if (!differ) t.reset();
	const int* startT = t ? t->d_start : nullptr;
	const int* positionsT = t ? t->d_positions : nullptr;
	SMM_HIP_TRY(hipMemsetAsync(d_colors, 0xFF, static_cast<size_t>(n) * sizeof(int), s));  // -1: uncoloured
	// every round colours at least the uncoloured vertex of the largest key: at most n rounds
	for (int round = 0; round < n; ++round) {
		SMM_HIP_TRY(hipMemsetAsync(words.p + 1, 0, sizeof(int), s));
		colorPickKernel<<<gridOf(n), CTPB, 0, s>>>(n, a->d_start, a->d_positions, startT, positionsT, d_colors, pick, words.p + 1);
		colorAssignKernel<<<gridOf(n), CTPB, 0, s>>>(n, a->d_start, a->d_positions, startT, positionsT, pick, d_colors, words.p + 2);
		SMM_HIP_TRY(hipGetLastError());
		int left = 0;
		SMM_TRY(readFlag(words.p + 1, s, &left));
		if (left == 0) break;
	}
	int top = 0;
	SMM_TRY(readFlag(words.p + 2, s, &top));
	*ncolors = top + 1;
	return SMM_HIP_OK;
}

int csrPermuteCreate(const smm_hip_csr* a, const int* d_perm, hipStream_t s, smm_hip_csr** out) {
	SMM_TRY(ensureCsrReady(a, s, true));
	return a->dtype == SMM_DTYPE_F32 ? permuteTyped<float>(a, d_perm, s, out) : permuteTyped<double>(a, d_perm, s, out);
}

int csrPermuteRefresh(smm_hip_csr* b, const smm_hip_csr* a, int dtype, hipStream_t s) {
	if (!b || !a) {
		setError("csr_permute_refresh: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (b->dtype != dtype || a->dtype != dtype) {
		setError("csr_permute_refresh: a matrix holds the other element type");
		return SMM_HIP_ERR_INVALID;
	}
	if (b->permuteOf == 0 || !b->d_pperm || !b->d_tperm) {
		setError("csr_permute_refresh: the handle was not made by smm_hip_csr_permute_create");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	return dtype == SMM_DTYPE_F32 ? permuteRefreshTyped<float>(b, a, s) : permuteRefreshTyped<double>(b, a, s);
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_color_dev(const smm_hip_csr* a, int* d_colors, size_t count, smm_hip_stream stream, int* ncolors) {
	if (ncolors) *ncolors = 0;
	SMM_TRY(squareChecked(a, "csr_color"));
	if (!ncolors || count != static_cast<size_t>(a->rows) || (!d_colors && a->rows > 0)) {
		setError("csr_color: null output, or count is not the number of rows (%d)", a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	return csrColor(a, s, d_colors, ncolors);
}

int smm_hip_csr_color(const smm_hip_csr* a, int* colors, size_t count, int* ncolors) {
	if (ncolors) *ncolors = 0;
	SMM_TRY(squareChecked(a, "csr_color"));
	if (!ncolors || count != static_cast<size_t>(a->rows) || (!colors && a->rows > 0)) {
		setError("csr_color: null output, or count is not the number of rows (%d)", a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureCsrReady(a, nullptr, false));  // a set-up call without a stream: drains the device once
	hipStream_t s = libStream();
	DevBuf<int> d;
	SMM_TRY(d.alloc(a->rows));
	SMM_TRY(csrColor(a, s, d, ncolors));
	if (a->rows > 0) SMM_TRY(devToHost(colors, d, static_cast<size_t>(a->rows) * sizeof(int), s));
	return SMM_HIP_OK;
}

int smm_hip_csr_permute_create_dev(const smm_hip_csr* a, const int* d_perm, size_t count, smm_hip_stream stream, smm_hip_csr** out) {
	if (!out) {
		setError("csr_permute_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(squareChecked(a, "csr_permute_create"));
	if (count != static_cast<size_t>(a->rows) || (!d_perm && a->rows > 0)) {
		setError("csr_permute_create: null perm, or count is not the number of rows (%d)", a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	return csrPermuteCreate(a, d_perm, pickStream(stream), out);
}

int smm_hip_csr_permute_create(const smm_hip_csr* a, const int* perm, size_t count, smm_hip_stream stream, smm_hip_csr** out) {
	if (!out) {
		setError("csr_permute_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(squareChecked(a, "csr_permute_create"));
	if (count != static_cast<size_t>(a->rows) || (!perm && a->rows > 0)) {
		setError("csr_permute_create: null perm, or count is not the number of rows (%d)", a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	hipStream_t s = pickStream(stream);
	DevBuf<int> d;
	SMM_TRY(d.alloc(a->rows));
	if (a->rows > 0) SMM_TRY(hostToDev(d, perm, static_cast<size_t>(a->rows) * sizeof(int), s));
	return csrPermuteCreate(a, d, s, out);
}

int smm_hip_csr_permute_refresh_f32(smm_hip_csr* b, const smm_hip_csr* a, smm_hip_stream stream) { return csrPermuteRefresh(b, a, SMM_DTYPE_F32, pickStream(stream)); }
int smm_hip_csr_permute_refresh_f64(smm_hip_csr* b, const smm_hip_csr* a, smm_hip_stream stream) { return csrPermuteRefresh(b, a, SMM_DTYPE_F64, pickStream(stream)); }

}  // extern "C"
