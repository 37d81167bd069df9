// smm_rcm.hip -- the reverse Cuthill-McKee ordering of a square matrix's adjacency graph, computed ON THE DEVICE, and the bandwidth /
// distinct-offset count of any handle.  include/smm_hip.h ("a BANDWIDTH-REDUCING ORDERING") states the rule; tests/rcm_restatement.py
// is its definition line by line.
//   graph    a's own start[] / positions[] when its pattern equals its transpose's (decided on the device, as smm_hip_csr_is_symmetric
//            does), else the union pattern a + aᵀ from the library's transpose and add.  The transpose checks start[] and every column
//            before anything is addressed with them.  deg(v) counts the distinct neighbours (columns ascend: a repeat is adjacent).
//   start    the vertices sorted once by key = (deg, index) (rocprim, stable, by deg); a device cursor walks that list, so finding the
//            unnumbered vertex of smallest key costs rows / 256 steps over the WHOLE run.  The deg == 0 prefix of the list is the
//            isolated vertices in index order: one launch numbers them all.
//   root     George-Liu.  A search needs no order: bfsStepKernel claims a vertex by an exchange on mark[] (the stamp of this search),
//            appends it to the next frontier and lowers the level's smallest key (64-bit atomicMin).  The host reads one 16-byte record
//            per level: the new frontier's size and that key.
//   number   level-synchronous Cuthill-McKee.  cmExpandKernel gives every unnumbered neighbour w of the frontier parent[w] = the smallest
//            rank among its frontier neighbours (32-bit atomicMin; the lane that finds the initial value appends w).  The new level is
//            then sorted by (parent, deg, index) -- <= 1024 vertices by one workgroup in LDS (bitonic; the keys are distinct), more by
//            two stable rocprim radix sorts, first by index, then by parent << 32 | deg -- and written behind the frontier in order[]:
//            the next frontier IS that slice of order[].  Integer atomics only; nothing depends on which lane arrives first.
//   lanes    a frontier vertex gets 8 lanes; a row of more than 64 entries is walked by its whole wavefront.
// Work per level is proportional to the frontier's edges; the host waits once per level (plus once per component), so the cost is at
// least (levels x searches) round trips: long thin graphs are slow.
#include <algorithm>
#include <climits>

#include "smm_csr_build.h"

namespace smm {
namespace {

constexpr int RTPB = BUILD_TPB;
constexpr int SORT_CAP = 1024;       // the largest level one workgroup sorts in LDS
constexpr int SORT_TPB = 512;        // one lane per compare-exchange of 1024 keys
constexpr int WAVE_ROW = 64;         // rows longer than this are walked by the whole wavefront
constexpr int NO_PARENT = INT_MAX;   // parent[] of a vertex no frontier has reached
constexpr unsigned long long NO_KEY = ~0ull;

struct LevelRec {  // what the host reads per level
	int count;     // vertices of the level
	int pad;
	unsigned long long minKey;  // the smallest (deg << 32 | index) among them
};

template <typename V>
int readBack(V* host, const V* dev, hipStream_t s) {
	SMM_HIP_TRY(hipMemcpyAsync(host, dev, sizeof(V), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

__device__ __forceinline__ unsigned long long keyOf(int deg, int v) {
	return (static_cast<unsigned long long>(static_cast<unsigned>(deg)) << 32) | static_cast<unsigned long long>(static_cast<unsigned>(v));
}

__global__ __launch_bounds__(RTPB) void fillKernel(int n, int value, int* __restrict__ out) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i < n) out[i] = value;
}

// deg[v] = the distinct neighbours of v (the columns of a row ascend: a repeated column sits beside its twin); the sort's key and
// payload; *iso counts the vertices without a neighbour.  The adjacency arrays were checked when the transpose was built.
__global__ __launch_bounds__(RTPB) void degreeKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, int* __restrict__ deg,
                                                     unsigned* __restrict__ key, int* __restrict__ seq, int* iso) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i >= n) return;
	const int v = static_cast<int>(i);
	const int b = start[i], e = start[i + 1];
	int d = 0, last = -1;
	for (int k = b; k < e; ++k) {
		const int j = positions[k];
		if (j != v && j != last) ++d;
		last = j;
	}
	deg[i] = d;
	key[i] = static_cast<unsigned>(d);
	seq[i] = v;
	if (d == 0) atomicAdd(iso, 1);
}

// the isolated vertices are the first `iso` of the list sorted by key, in index order
__global__ __launch_bounds__(RTPB) void isolatedKernel(int iso, const int* __restrict__ byKey, int* __restrict__ order, int* __restrict__ rank, int* cursor) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i >= iso) return;
	if (i == 0) *cursor = iso;
	const int v = byKey[i];
	order[i] = v;
	rank[v] = static_cast<int>(i);
}

// level 0 of a search from v: frontier[0] = v, rec[0] describes it, rec[1] is ready for level 1
__device__ __forceinline__ void seedSearch(int v, int stamp, const int* __restrict__ deg, int* mark, int* frontier, LevelRec* rec) {
	frontier[0] = v;
	mark[v] = stamp;
	rec[0].count = 1;
	rec[0].minKey = keyOf(deg[v], v);
	rec[1].count = 0;
	rec[1].minKey = NO_KEY;
}

// ONE workgroup: moves *cursor to the first vertex of byKey[] that has no rank yet and seeds a search from it (rec[0].count = 0 when
// none is left).  The cursor only moves forward: rows / 256 steps over the whole ordering.
__global__ __launch_bounds__(RTPB) void findStartKernel(int n, const int* __restrict__ byKey, const int* __restrict__ rank, int* cursor, int stamp,
                                                        const int* __restrict__ deg, int* mark, int* frontier, LevelRec* rec) {
	__shared__ int best;
	int c = *cursor;
	__syncthreads();  // (every lane has read the cursor before lane 0 may move it)
	for (;;) {
		if (threadIdx.x == 0) best = INT_MAX;
		__syncthreads();
		const long long at = static_cast<long long>(c) + threadIdx.x;
		if (at < n && rank[byKey[at]] < 0) atomicMin(&best, static_cast<int>(at));
		__syncthreads();
		const int found = best;
		__syncthreads();
		if (found != INT_MAX) {
			if (threadIdx.x == 0) {
				*cursor = found + 1;
				seedSearch(byKey[found], stamp, deg, mark, frontier, rec);
			}
			return;
		}
		if (static_cast<long long>(c) + RTPB >= n) {
			if (threadIdx.x == 0) {
				*cursor = n;
				rec[0].count = 0;
				rec[0].minKey = NO_KEY;
			}
			return;
		}
		c += RTPB;
	}
}

__global__ void seedSearchKernel(int v, int stamp, const int* __restrict__ deg, int* mark, int* frontier, LevelRec* rec) {
	if (blockIdx.x == 0 && threadIdx.x == 0) seedSearch(v, stamp, deg, mark, frontier, rec);
}

// The walk both expansions share: frontier vertex `slot` belongs to 8 consecutive lanes; a row of at most WAVE_ROW entries is walked by
// them, a longer one by the 64 lanes of the wavefront in turn.  visit(w, slot of the vertex w was reached from).
template <typename Visit>
__device__ __forceinline__ void walkFrontier(int f, const int* __restrict__ frontier, const int* __restrict__ start, const int* __restrict__ positions, Visit visit) {
	const long long lane0 = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	const int lane = threadIdx.x & 63, sub = lane & 7;
	const long long slot = lane0 >> 3;
	int b = 0, len = 0;
	if (slot < f) {
		const int u = frontier[slot];
		b = start[u];
		len = start[u + 1] - b;
	}
	if (len <= WAVE_ROW) {
		for (int k = b + sub; k < b + len; k += 8) visit(positions[k], static_cast<int>(slot));
	}
	for (int q = 0; q < 8; ++q) {  // (all 64 lanes take part in the shuffles)
		const int lenQ = __shfl(len, q * 8), bQ = __shfl(b, q * 8);
		if (lenQ > WAVE_ROW) {
			const int slotQ = static_cast<int>((lane0 - lane) >> 3) + q;
			for (int k = bQ + lane; k < bQ + lenQ; k += 64) visit(positions[k], slotQ);
		}
	}
}

// one level of a root search: every vertex next to the frontier that this search (stamp) has not seen is claimed by an exchange and
// appended; the order inside next[] is of no consequence -- the host uses the count and the smallest key alone
__global__ __launch_bounds__(RTPB) void bfsStepKernel(int f, const int* __restrict__ frontier, int* __restrict__ next, const int* __restrict__ start,
                                                      const int* __restrict__ positions, const int* __restrict__ deg, int* mark, int stamp, LevelRec* recNew,
                                                      LevelRec* recOld) {
	if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the host has read the frontier's own record: it becomes the record of the level after next)
		recOld->count = 0;
		recOld->minKey = NO_KEY;
	}
	walkFrontier(f, frontier, start, positions, [&](int w, int) {
		if (mark[w] != stamp && atomicExch(mark + w, stamp) != stamp) {
			next[atomicAdd(&recNew->count, 1)] = w;
			atomicMin(&recNew->minKey, keyOf(deg[w], w));
		}
	});
}

// one level of the numbering: the frontier is order[base .. base + f), its vertex at slot i has rank base + i
__global__ __launch_bounds__(RTPB) void cmExpandKernel(int f, int base, const int* __restrict__ frontier, int* __restrict__ next, const int* __restrict__ start,
                                                       const int* __restrict__ positions, const int* __restrict__ rank, int* parent, int* countNew, int* countOld) {
	if (blockIdx.x == 0 && threadIdx.x == 0) *countOld = 0;
	walkFrontier(f, frontier, start, positions, [&](int w, int slot) {
		if (rank[w] < 0 && atomicMin(parent + w, base + slot) == NO_PARENT) next[atomicAdd(countNew, 1)] = w;
	});
}

// ONE workgroup: the g <= SORT_CAP vertices of level[] sorted by (parent, deg, index) in LDS and numbered from `base`
__global__ __launch_bounds__(SORT_TPB) void sortLevelKernel(int g, int base, const int* __restrict__ level, const int* __restrict__ parent,
                                                            const int* __restrict__ deg, int* __restrict__ order, int* __restrict__ rank) {
	__shared__ unsigned long long hi[SORT_CAP];
	__shared__ int lo[SORT_CAP];
	int m = 2;
	while (m < g) m <<= 1;
	for (int i = threadIdx.x; i < m; i += SORT_TPB) {
		if (i < g) {
			const int w = level[i];
			hi[i] = keyOf(parent[w], deg[w]);
			lo[i] = w;
		} else {
			hi[i] = NO_KEY;
			lo[i] = INT_MAX;
		}
	}
	__syncthreads();
	for (int k = 2; k <= m; k <<= 1) {
		for (int j = k >> 1; j > 0; j >>= 1) {
			for (int t = threadIdx.x; t < (m >> 1); t += SORT_TPB) {
				const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
				const bool ascending = (i & k) == 0;
				const unsigned long long hi0 = hi[i], hi1 = hi[p];
				const int lo0 = lo[i], lo1 = lo[p];
				const bool greater = hi0 > hi1 || (hi0 == hi1 && lo0 > lo1);
				if (greater == ascending) {
					hi[i] = hi1;
					hi[p] = hi0;
					lo[i] = lo1;
					lo[p] = lo0;
				}
			}
			__syncthreads();
		}
	}
	for (int i = threadIdx.x; i < g; i += SORT_TPB) {
		order[base + i] = lo[i];
		rank[lo[i]] = base + i;
	}
}

// the larger levels: the second sort's key of every vertex of the (index-sorted) level
__global__ __launch_bounds__(RTPB) void levelKeyKernel(int g, const int* __restrict__ level, const int* __restrict__ parent, const int* __restrict__ deg,
                                                       unsigned long long* __restrict__ key) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i >= g) return;
	const int w = level[i];
	key[i] = keyOf(parent[w], deg[w]);
}

__global__ __launch_bounds__(RTPB) void numberLevelKernel(int g, int base, const int* __restrict__ order, int* __restrict__ rank) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i < g) rank[order[base + i]] = base + static_cast<int>(i);
}

__global__ __launch_bounds__(RTPB) void seedNumberingKernel(int r, int base, int* order, int* rank, int* counts) {
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		order[base] = r;
		rank[r] = base;
		counts[0] = 0;
		counts[1] = 0;
	}
}

__global__ __launch_bounds__(RTPB) void writePermKernel(int n, int reverse, const int* __restrict__ order, int* __restrict__ perm) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i < n) perm[i] = order[reverse ? n - 1 - i : i];
}

// max |place(i) - place(j)| over the stored entries (place = rank[], or the index itself when rank is null) and, when `bitmap` is given,
// the bit of every j - i + rows - 1.  One lane per row.  Nothing is addressed with a start[] or a column that fails its check: *bad.
__global__ __launch_bounds__(RTPB) void bandwidthKernel(int rows, int cols, int nnz, const int* __restrict__ start, const int* __restrict__ positions,
                                                        const int* __restrict__ rank, unsigned long long* widest, unsigned* bitmap, int* bad) {
	const long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	if (i >= rows) return;
	const int b = start[i], e = start[i + 1];
	if (b < 0 || e < b || e > nnz || (i == 0 && b != 0)) {
		*bad = 1;
		return;
	}
	const long long here = rank ? rank[i] : i;
	long long w = 0;
	for (int k = b; k < e; ++k) {
		const int j = positions[k];
		if (j < 0 || j >= cols) {
			*bad = 1;
			continue;
		}
		const long long d = (rank ? rank[j] : j) - here;
		w = d < 0 ? (-d > w ? -d : w) : (d > w ? d : w);
		if (bitmap) {
			const long long bit = static_cast<long long>(j) - i + rows - 1;
			const unsigned m = 1u << (bit & 31);
			if (!(bitmap[bit >> 5] & m)) atomicOr(bitmap + (bit >> 5), m);
		}
	}
	if (w > 0) atomicMax(widest, static_cast<unsigned long long>(w));
}

__global__ __launch_bounds__(RTPB) void popcountKernel(long long words, const unsigned* __restrict__ bitmap, unsigned long long* total) {
	unsigned long long sum = 0;
	for (long long i = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x; i < words; i += static_cast<long long>(gridDim.x) * RTPB) sum += __popc(bitmap[i]);
	if (sum) atomicAdd(total, sum);
}

int passGrid(long long work) { return static_cast<int>(std::min<long long>(gridOf(work), numCUs() * 8LL)); }

// max |i - j| of `a` (through rank[] when given) and, when asked, its distinct offsets; synchronises `s`
int measureBandwidth(const smm_hip_csr* a, const int* d_rank, hipStream_t s, long long* widest, long long* offsets) {
	*widest = 0;
	if (offsets) *offsets = 0;
	if (a->rows == 0 || a->nnz == 0) return SMM_HIP_OK;
	DevBuf<unsigned long long> words;  // [0] the widest entry, [1] the bits set
	DevBuf<int> d_bad;
	DevBuf<unsigned> bitmap;
	const long long bits = static_cast<long long>(a->rows) + a->cols - 1, mapWords = (bits + 31) / 32;
	SMM_TRY(words.alloc(2));
	SMM_TRY(d_bad.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(words, 0, 2 * sizeof(unsigned long long), s));
	SMM_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), s));
	if (offsets) {
		SMM_TRY(bitmap.alloc(static_cast<size_t>(mapWords)));
		SMM_HIP_TRY(hipMemsetAsync(bitmap, 0, static_cast<size_t>(mapWords) * sizeof(unsigned), s));
	}
	bandwidthKernel<<<gridOf(a->rows), RTPB, 0, s>>>(a->rows, a->cols, a->nnz, a->d_start, a->d_positions, d_rank, words, offsets ? bitmap.p : nullptr, d_bad);
	if (offsets) popcountKernel<<<passGrid(mapWords), RTPB, 0, s>>>(mapWords, bitmap, words.p + 1);
	SMM_HIP_TRY(hipGetLastError());
	int bad = 0;
	SMM_TRY(readBack(&bad, d_bad.p, s));
	if (bad) {
		setError("csr_bandwidth: start[] does not ascend from 0 or a column lies outside [0, %d)", a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	unsigned long long got[2] = {0, 0};
	SMM_HIP_TRY(hipMemcpyAsync(got, words.p, sizeof(got), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	*widest = static_cast<long long>(got[0]);
	if (offsets) *offsets = static_cast<long long>(got[1]);
	return SMM_HIP_OK;
}

// the ordering's working set and its host loop
struct Rcm {
	int n = 0;
	hipStream_t s = nullptr;
	const int* start = nullptr;      // the adjacency: a's own arrays or the union's
	const int* positions = nullptr;
	DevBuf<int> deg, byKey, rank, order, parent, mark, bufA, bufB, cursor, counts;
	DevBuf<LevelRec> rec;
	DevBuf<unsigned> idxOut;  // the larger levels' sorts
	DevBuf<unsigned long long> keyIn, keyOut;
	PrimScratch temp;  // of every sort of the call
	int stamp = 0;

	// a search from `root`, seeded in bufA: its depth and the smallest key of its last level (of which the vertex, the low word, is used)
	int search(int root, int* depth, unsigned long long* lastKey) {
		LevelRec got{1, 0, static_cast<unsigned long long>(static_cast<unsigned>(root))};
		int* frontier = bufA;
		int* next = bufB;
		int f = got.count;
		for (int level = 0;; ++level) {
			*lastKey = got.minKey;
			bfsStepKernel<<<gridOf(8LL * f), RTPB, 0, s>>>(f, frontier, next, start, positions, deg, mark, stamp, rec.p + ((level + 1) & 1), rec.p + (level & 1));
			SMM_HIP_TRY(hipGetLastError());
			SMM_TRY(readBack(&got, rec.p + ((level + 1) & 1), s));
			if (got.count == 0) {
				*depth = level + 1;
				return SMM_HIP_OK;
			}
			f = got.count;
			std::swap(frontier, next);
		}
	}

	// the g vertices of bufA become order[base .. base + g), sorted by (parent, deg, index), and receive their ranks
	int numberLevel(int g, int base) {
		if (g <= SORT_CAP) {
			sortLevelKernel<<<1, SORT_TPB, 0, s>>>(g, base, bufA, parent, deg, order, rank);
			SMM_HIP_TRY(hipGetLastError());
			return SMM_HIP_OK;
		}
		if (!idxOut.p) {
			SMM_TRY(idxOut.alloc(n));
			SMM_TRY(keyIn.alloc(n));
			SMM_TRY(keyOut.alloc(n));
		}
		const unsigned idxBits = static_cast<unsigned>(std::max(1, bitsFor(n)));
		const unsigned* levelIn = reinterpret_cast<const unsigned*>(bufA.p);  // (vertex numbers: never negative)
		SMM_TRY(sortKeys(levelIn, idxOut.p, static_cast<size_t>(g), idxBits, s, &temp));
		const int* sorted = reinterpret_cast<const int*>(idxOut.p);
		levelKeyKernel<<<gridOf(g), RTPB, 0, s>>>(g, sorted, parent, deg, keyIn);
		SMM_HIP_TRY(hipGetLastError());
		// stable: vertices of one (parent, deg) stay in index order
		SMM_TRY(sortPairs(keyIn.p, keyOut.p, sorted, order.p + base, static_cast<size_t>(g), 32u + idxBits, s, &temp));
		numberLevelKernel<<<gridOf(g), RTPB, 0, s>>>(g, base, order, rank);
		SMM_HIP_TRY(hipGetLastError());
		return SMM_HIP_OK;
	}

	// Cuthill-McKee from r, whose rank is `base`: *size vertices appended to order[], *depth levels
	int numberComponent(int r, int base, int* size, int* depth) {
		seedNumberingKernel<<<1, RTPB, 0, s>>>(r, base, order, rank, counts);
		SMM_HIP_TRY(hipGetLastError());
		int lo = base, f = 1;
		for (int level = 0;; ++level) {
			cmExpandKernel<<<gridOf(8LL * f), RTPB, 0, s>>>(f, lo, order.p + lo, bufA, start, positions, rank, parent, counts.p + ((level + 1) & 1), counts.p + (level & 1));
			SMM_HIP_TRY(hipGetLastError());
			int g = 0;
			SMM_TRY(readBack(&g, counts.p + ((level + 1) & 1), s));
			if (g == 0) {
				*size = lo + f - base;
				*depth = level + 1;
				return SMM_HIP_OK;
			}
			SMM_TRY(numberLevel(g, lo + f));
			lo += f;
			f = g;
		}
	}

	int run(int* components, int* levels) {
		*components = 0;
		*levels = 0;
		SMM_TRY(deg.alloc(n));
		SMM_TRY(byKey.alloc(n));
		SMM_TRY(rank.alloc(n));
		SMM_TRY(order.alloc(n));
		SMM_TRY(parent.alloc(n));
		SMM_TRY(mark.alloc(n));
		SMM_TRY(bufA.alloc(n));
		SMM_TRY(bufB.alloc(n));
		SMM_TRY(cursor.alloc(2));  // [0] the cursor in byKey[], [1] the isolated vertices
		SMM_TRY(counts.alloc(2));
		SMM_TRY(rec.alloc(2));
		SMM_HIP_TRY(hipMemsetAsync(cursor, 0, 2 * sizeof(int), s));
		SMM_HIP_TRY(hipMemsetAsync(rank, 0xFF, static_cast<size_t>(n) * sizeof(int), s));  // -1: no rank yet
		SMM_HIP_TRY(hipMemsetAsync(mark, 0, static_cast<size_t>(n) * sizeof(int), s));     // (stamps start at 1)
		fillKernel<<<gridOf(n), RTPB, 0, s>>>(n, NO_PARENT, parent);
		{
			DevBuf<unsigned> degKey, degSorted;
			DevBuf<int> seq;
			SMM_TRY(degKey.alloc(n));
			SMM_TRY(degSorted.alloc(n));
			SMM_TRY(seq.alloc(n));
			degreeKernel<<<gridOf(n), RTPB, 0, s>>>(n, start, positions, deg, degKey, seq, cursor.p + 1);
			SMM_HIP_TRY(hipGetLastError());
			const unsigned endBit = static_cast<unsigned>(std::max(1, bitsFor(n)));  // (deg < n)
			SMM_TRY(sortPairs(degKey.p, degSorted.p, seq.p, byKey.p, static_cast<size_t>(n), endBit, s, &temp));
			SMM_HIP_TRY(hipStreamSynchronize(s));  // the three temporaries go back to the allocator when this scope ends
		}
		int iso = 0;
		SMM_TRY(readBack(&iso, cursor.p + 1, s));
		int numbered = 0;
		if (iso > 0) {
			isolatedKernel<<<gridOf(iso), RTPB, 0, s>>>(iso, byKey, order, rank, cursor);
			SMM_HIP_TRY(hipGetLastError());
			numbered = iso;
			*components = iso;
			*levels = 1;
		}
		while (numbered < n) {
			// step 1: the unnumbered vertex of smallest key, and the search from it
			++stamp;
			findStartKernel<<<1, RTPB, 0, s>>>(n, byKey, rank, cursor, stamp, deg, mark, bufA, rec);
			SMM_HIP_TRY(hipGetLastError());
			LevelRec first{};
			SMM_TRY(readBack(&first, rec.p, s));
			if (first.count != 1) {
				setError("csr_rcm: %d of %d vertices numbered and no start vertex left (was the matrix changed during the call?)", numbered, n);
				return SMM_HIP_ERR_INVALID;
			}
			int r = static_cast<int>(first.minKey & 0xFFFFFFFFull), depth = 0;
			unsigned long long lastKey = 0;
			SMM_TRY(search(r, &depth, &lastKey));
			// step 2: while the vertex of smallest key in the last level starts a deeper search, it becomes the root
			for (;;) {
				const int v = static_cast<int>(lastKey & 0xFFFFFFFFull);
				if (v == r) break;  // (a component of one vertex)
				++stamp;
				seedSearchKernel<<<1, 1, 0, s>>>(v, stamp, deg, mark, bufA, rec);
				SMM_HIP_TRY(hipGetLastError());
				int depthV = 0;
				unsigned long long lastV = 0;
				SMM_TRY(search(v, &depthV, &lastV));
				if (depthV <= depth) break;
				r = v;
				depth = depthV;
				lastKey = lastV;
			}
			// step 3
			int size = 0, depthR = 0;
			SMM_TRY(numberComponent(r, numbered, &size, &depthR));
			if (size <= 0 || depthR != depth || numbered + size > n) {
				setError("csr_rcm: the numbering of a component (%d vertices, %d levels) disagrees with its root search (%d levels; was the matrix changed during the call?)", size, depthR, depth);
				return SMM_HIP_ERR_INVALID;
			}
			numbered += size;
			*components += 1;
			*levels = std::max(*levels, depth);
		}
		return SMM_HIP_OK;
	}
};

int squareChecked(const smm_hip_csr* a, const int* perm, size_t count) {
	if (!a) {
		setError("csr_rcm: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("csr_rcm: the matrix is not square");
		return SMM_HIP_ERR_INVALID;
	}
	if (count != static_cast<size_t>(a->rows) || (!perm && a->rows > 0)) {
		setError("csr_rcm: null perm, or count is not the number of rows (%d)", a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

// the ordering of a square, ready matrix into d_perm[rows] (device); synchronises `s`.  d_perm is written last, after every check.
int csrRcm(const smm_hip_csr* a, hipStream_t s, int reverse, int* d_perm, int* components, int* levels, long long* before, long long* after) {
	SetupTrace trace("rcm");
	const int n = a->rows;
	int comps = 0, depth = 0;
	long long bwBefore = 0, bwAfter = 0;
	if (n > 0) {
		// the in-neighbours: the transpose (it checks start[] and the columns); when its pattern is a's own, a's arrays are the graph
		smm_hip_csr* raw = nullptr;
		SMM_TRY(csrTransposeCreate(a, s, &raw));
		OwnedCsr t(raw), both;
		DevBuf<int> d_diff;
		SMM_TRY(d_diff.alloc(1));
		SMM_HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), s));
		intsDifferKernel<<<passGrid(n + 1LL), RTPB, 0, s>>>(n + 1LL, a->d_start, t->d_start, d_diff);
		if (a->nnz > 0) intsDifferKernel<<<passGrid(a->nnz), RTPB, 0, s>>>(a->nnz, a->d_positions, t->d_positions, d_diff);
		SMM_HIP_TRY(hipGetLastError());
		int differ = 0;
		SMM_TRY(readBack(&differ, d_diff.p, s));
		if (differ) {  // the union pattern a + aᵀ (the values are of no interest); the sum refuses rows whose columns do not ascend strictly
			raw = nullptr;
			if (a->dtype == SMM_DTYPE_F32) SMM_TRY(smm_hip_csr_add_create_f32(a, 1.0f, t.get(), 1.0f, s, &raw));
			else SMM_TRY(smm_hip_csr_add_create_f64(a, 1.0, t.get(), 1.0, s, &raw));
			both.reset(raw);
		}
		t.reset();
		Rcm work;
		work.n = n;
		work.s = s;
		work.start = both ? both->d_start : a->d_start;
		work.positions = both ? both->d_positions : a->d_positions;
		SMM_TRY(work.run(&comps, &depth));
		if (before) SMM_TRY(measureBandwidth(a, nullptr, s, &bwBefore, nullptr));
		if (after) SMM_TRY(measureBandwidth(a, work.rank, s, &bwAfter, nullptr));
		writePermKernel<<<gridOf(n), RTPB, 0, s>>>(n, reverse ? 1 : 0, work.order, d_perm);
		SMM_HIP_TRY(hipGetLastError());
		SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	if (components) *components = comps;
	if (levels) *levels = depth;
	if (before) *before = bwBefore;
	if (after) *after = bwAfter;
	return SMM_HIP_OK;
}

}  // namespace
}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_rcm_dev(const smm_hip_csr* a, int* d_perm, size_t count, int reverse, smm_hip_stream stream, int* components, int* levels,
                        long long* bandwidth_before, long long* bandwidth_after) {
	SMM_TRY(squareChecked(a, d_perm, count));
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	return csrRcm(a, s, reverse, d_perm, components, levels, bandwidth_before, bandwidth_after);
}

int smm_hip_csr_rcm(const smm_hip_csr* a, int* perm, size_t count, int reverse, int* components, int* levels, long long* bandwidth_before,
                    long long* bandwidth_after) {
	SMM_TRY(squareChecked(a, perm, count));
	SMM_TRY(ensureCsrReady(a, nullptr, false));  // a set-up call without a stream: drains the device once
	hipStream_t s = libStream();
	DevBuf<int> d;
	SMM_TRY(d.alloc(a->rows));
	SMM_TRY(csrRcm(a, s, reverse, d, components, levels, bandwidth_before, bandwidth_after));
	if (a->rows > 0) SMM_TRY(devToHost(perm, d, static_cast<size_t>(a->rows) * sizeof(int), s));
	return SMM_HIP_OK;
}

int smm_hip_csr_bandwidth(const smm_hip_csr* a, long long* bandwidth, long long* distinct_offsets) {
	if (bandwidth) *bandwidth = 0;
	if (distinct_offsets) *distinct_offsets = 0;
	if (!a) {
		setError("csr_bandwidth: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	long long widest = 0, offsets = 0;
	SMM_TRY(measureBandwidth(a, nullptr, libStream(), &widest, distinct_offsets ? &offsets : nullptr));
	if (bandwidth) *bandwidth = widest;
	if (distinct_offsets) *distinct_offsets = offsets;
	return SMM_HIP_OK;
}

}  // extern "C"
