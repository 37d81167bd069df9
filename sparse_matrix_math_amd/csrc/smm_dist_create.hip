// smm_dist_create.hip -- building a rank's share of a row-partitioned matrix on the device (overview: smm_dist.hip): the column range, the
// split of the local rows into A_loc / A_rem, the list of a thin remote block's rows, the halo in pieces, the solvers' workspace, the
// halo-first row ranges; smm_hip_dist_csr_create_dev_*, _destroy and the handle's queries.  The only unit of the path that includes rocprim.
#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "smm_dist.h"

namespace smm {

// ---------------------------------------------------------------------------------------------------------
// splitting the local rows into A_loc / A_rem on the device
// ---------------------------------------------------------------------------------------------------------
__global__ void colRangeKernel(long long nnz, const int* __restrict__ positions, int* __restrict__ minmax) {
	int lo = 0x7fffffff, hi = -1;
	for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < nnz; i += static_cast<long long>(gridDim.x) * blockDim.x) {
		const int c = positions[i];
		lo = min(lo, c);
		hi = max(hi, c);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		lo = min(lo, __shfl_xor(lo, o, WAVE));
		hi = max(hi, __shfl_xor(hi, o, WAVE));
	}
	if ((threadIdx.x & 63) == 0 && hi >= 0) {
		atomicMin(minmax, lo);
		atomicMax(minmax + 1, hi);
	}
}

// counts[row] = entries of the row with an owned column; counts[nLocal + 1 + row] = the others.  Both arrays have nLocal + 1
// slots so that an exclusive scan over nLocal + 1 elements ends with the total.
// labWindow (measurements with ONE rank, smm_hip_dist_csr::labWindow).  > 0: an owned column farther than that from its row counts as remote too
// (every row gets a remote part: a rank of MANY); < 0: the last |labWindow| columns of the range count as remote (only rows near that end get a
// remote part: a rank of a FEW)
__device__ __forceinline__ bool labLocal(int c, int row, int ownLo, int ownHi, int labWindow) {
	if (labWindow == 0) return true;
	if (labWindow > 0) return abs(c - row) < labWindow;
	return c < ownHi + labWindow;  // (the last |labWindow| columns are "the neighbour's": the first rank of two)
}

__global__ void splitCountKernel(int nLocal, const int* __restrict__ start, const int* __restrict__ positions, int ownLo, int ownHi, int labWindow,
                                 int* __restrict__ cntLoc, int* __restrict__ cntRem) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row <= nLocal; row += gridDim.x * blockDim.x) {
		int nl = 0, nr = 0;
		if (row < nLocal) {
			const int e = start[row + 1];
			for (int k = start[row]; k < e; ++k) {
				const int c = positions[k];
				if (c >= ownLo && c < ownHi && labLocal(c, ownLo + row, ownLo, ownHi, labWindow)) ++nl;
				else ++nr;
			}
		}
		cntLoc[row] = nl;
		cntRem[row] = nr;
	}
}

constexpr int THIN_SHARE = 8;  // a remote block is thin when rows with a remote entry x THIN_SHARE <= rows
// rows that hold a remote entry: a 0 / 1 flag per row (scanned into the row's index in the list), then the list
__global__ void thinFlagKernel(int nLocal, const int* __restrict__ startRem, int* __restrict__ flag) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row <= nLocal; row += gridDim.x * blockDim.x) {
		flag[row] = row < nLocal && startRem[row + 1] > startRem[row] ? 1 : 0;
	}
}
__global__ void thinListKernel(int nLocal, const int* __restrict__ startRem, const int* __restrict__ index, int* __restrict__ rows) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nLocal; row += gridDim.x * blockDim.x) {
		if (startRem[row + 1] > startRem[row]) rows[index[row]] = row;
	}
}

template <typename T>
__global__ void splitScatterKernel(int nLocal, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ values, int ownLo,
                                   int ownHi, int labWindow, int cmin, const int* __restrict__ startLoc, const int* __restrict__ startRem, int* __restrict__ posLoc,
                                   T* __restrict__ valLoc, int* __restrict__ posRem, T* __restrict__ valRem) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nLocal; row += gridDim.x * blockDim.x) {
		int il = startLoc[row], ir = startRem[row];
		const int e = start[row + 1];
		for (int k = start[row]; k < e; ++k) {  // order inside a row is preserved (columns stay ascending, ref:1247-1249)
			const int c = positions[k];
			const T v = values[k];
			if (c >= ownLo && c < ownHi && labLocal(c, ownLo + row, ownLo, ownHi, labWindow)) {
				posLoc[il] = c - ownLo;
				valLoc[il] = v;
				++il;
			} else {
				posRem[ir] = c - cmin;
				valRem[ir] = v;
				++ir;
			}
		}
	}
}

// piece of the halo a column of A_rem (numbered from the first column of the halo-extended vector) falls into: segment [off, off + cnt)
// is cut at off + floor(k cnt / K), k = 0 .. K; at most MAX_CHUNK_SEGS segments (more: the matrix keeps one piece)
constexpr int MAX_CHUNK_SEGS = 16;
struct ChunkSegs {
	int n, K;
	int off[MAX_CHUNK_SEGS], cnt[MAX_CHUNK_SEGS];
};
__host__ __device__ inline int chunkBound(int cnt, int k, int K) { return static_cast<int>(static_cast<long long>(cnt) * k / K); }
__device__ __forceinline__ int chunkOfColumn(const ChunkSegs& g, int col) {
	for (int i = 0; i < g.n; ++i) {
		const int rel = col - g.off[i];
		if (rel >= 0 && rel < g.cnt[i]) {
			int k = static_cast<int>(static_cast<long long>(rel) * g.K / g.cnt[i]);
			while (k + 1 < g.K && rel >= chunkBound(g.cnt[i], k + 1, g.K)) ++k;  // (the floor of the inverse can land one piece early)
			while (k > 0 && rel < chunkBound(g.cnt[i], k, g.K)) --k;
			return k;
		}
	}
	return g.K - 1;  // (a column outside every received segment cannot occur: A_rem's columns are what the segments were made from)
}

// counts[k * (nLocal + 1) + row] = entries of A_rem's row in piece k
__global__ void chunkCountKernel(int nLocal, const int* __restrict__ start, const int* __restrict__ positions, ChunkSegs segs, int* __restrict__ counts) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row <= nLocal; row += gridDim.x * blockDim.x) {
		int n[MAX_HALO_CHUNKS] = {0, 0, 0, 0};
		if (row < nLocal) {
			const int e = start[row + 1];
			for (int k = start[row]; k < e; ++k) ++n[chunkOfColumn(segs, positions[k])];
		}
		for (int k = 0; k < segs.K; ++k) counts[static_cast<size_t>(k) * (nLocal + 1) + row] = n[k];
	}
}

struct ChunkOut {
	int* pos[MAX_HALO_CHUNKS];
	void* val[MAX_HALO_CHUNKS];
};
template <typename T>
__global__ void chunkScatterKernel(int nLocal, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ values, ChunkSegs segs,
                                   const int* __restrict__ starts, ChunkOut out) {
	for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < nLocal; row += gridDim.x * blockDim.x) {
		int at[MAX_HALO_CHUNKS];
		for (int k = 0; k < segs.K; ++k) at[k] = starts[static_cast<size_t>(k) * (nLocal + 1) + row];
		const int e = start[row + 1];
		for (int i = start[row]; i < e; ++i) {  // order inside a row is preserved
			const int k = chunkOfColumn(segs, positions[i]);
			out.pos[k][at[k]] = positions[i];
			static_cast<T*>(out.val[k])[at[k]] = values[i];
			++at[k];
		}
	}
}

static int exclusiveScan(int* d_inout, int count, hipStream_t s) {
	size_t tempBytes = 0;
	SMM_HIP_TRY(rocprim::exclusive_scan(nullptr, tempBytes, d_inout, d_inout, 0, static_cast<size_t>(count), rocprim::plus<int>(), s));
	void* temp = nullptr;
	SMM_TRY(devAlloc(&temp, tempBytes ? tempBytes : 1));
	const hipError_t e = rocprim::exclusive_scan(temp, tempBytes, d_inout, d_inout, 0, static_cast<size_t>(count), rocprim::plus<int>(), s);
	if (e == hipSuccess) (void)hipStreamSynchronize(s);
	devFree(temp);
	SMM_HIP_TRY(e);
	return SMM_HIP_OK;
}

template <typename T>
static int distWorkspace(smm_hip_dist_csr* D) {
	if (D->r) return SMM_HIP_OK;
	const size_t vb = static_cast<size_t>(std::max(1, D->nLocal)) * sizeof(T);
	const size_t eb = static_cast<size_t>(std::max(1, D->extLen)) * sizeof(T);
	SMM_TRY(devAlloc(&D->r, vb));
	SMM_TRY(devAlloc(&D->r0, vb));
	SMM_TRY(devAlloc(&D->ap, vb));
	SMM_TRY(devAlloc(&D->as, vb));
	SMM_TRY(devAlloc(&D->pExt, eb));
	SMM_TRY(devAlloc(&D->sExt, eb));
	SMM_TRY(devAlloc(&D->xExt, eb));
	SMM_TRY(devAlloc(&D->partsA, PARTS_LEN * sizeof(T)));
	SMM_TRY(devAlloc(&D->partsB, PARTS_LEN * sizeof(T)));
	SMM_TRY(devAlloc(&D->partsC, PARTS_LEN * sizeof(T)));
	SMM_TRY(devAlloc(&D->sc, sizeof(Scal<T>)));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&D->splitSync), (P2P_KINDS + 2) * sizeof(unsigned long long)));
	preloadSplitUnit();  // (its code object is built for the device now, not inside the first iteration)
	preloadDistMatvecUnit();  // (the same for the two units whose first launch would otherwise fall inside the first solve: smm_dist.h)
	preloadDistLoopsUnit();
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipMemsetAsync(D->splitSync, 0, (P2P_KINDS + 2) * sizeof(unsigned long long), s));
	// halo slots outside every recv segment are never read by A_rem; zero keeps them finite.  Tickets start at 0.
	SMM_HIP_TRY(hipMemsetAsync(D->pExt, 0, eb, s));
	SMM_HIP_TRY(hipMemsetAsync(D->sExt, 0, eb, s));
	SMM_HIP_TRY(hipMemsetAsync(D->xExt, 0, eb, s));
	SMM_HIP_TRY(hipMemsetAsync(D->partsA, 0, PARTS_LEN * sizeof(T), s));
	SMM_HIP_TRY(hipMemsetAsync(D->partsB, 0, PARTS_LEN * sizeof(T), s));
	SMM_HIP_TRY(hipMemsetAsync(D->partsC, 0, PARTS_LEN * sizeof(T), s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// halo first: which rows of an updated vector some peer receives
// ---------------------------------------------------------------------------------------------------------
// The send segments in owned-local numbering, merged, clipped and widened to multiples of 16 bytes (the update kernels' fast path needs
// 16-byte aligned runs; a few extra rows in the small launch cost nothing).  No split when (almost) every row is a boundary row.
template <typename T>
static void planHaloFirst(smm_hip_dist_csr* D) {
	D->haloFirst = false;
	D->boundary = RowRanges{};
	D->bulk = RowRanges{};
	const int n = D->nLocal;
	D->bulk.n = 1;
	D->bulk.lo[0] = 0;
	D->bulk.hi[0] = n;
	if (!env::flagOr(env::HALO_FIRST, true) || D->sends.empty() || n <= 0) return;
	constexpr int VEC = 16 / sizeof(T);
	std::vector<std::pair<int, int>> runs;
	for (const Seg& g : D->sends) {
		int lo = g.offset - D->ownOffset, hi = lo + g.count;
		lo = std::max(0, lo / VEC * VEC);
		hi = std::min(n, (hi + VEC - 1) / VEC * VEC);
		if (lo < hi) runs.emplace_back(lo, hi);
	}
	std::sort(runs.begin(), runs.end());
	std::vector<std::pair<int, int>> merged;
	for (const auto& r : runs) {
		if (!merged.empty() && r.first <= merged.back().second) merged.back().second = std::max(merged.back().second, r.second);
		else merged.push_back(r);
	}
	long long total = 0;
	for (const auto& r : merged) total += r.second - r.first;
	if (merged.empty() || merged.size() > 3 || total * 4 > static_cast<long long>(n) * 3) return;  // (too scattered, or nothing left for a bulk launch)
	RowRanges b{}, rest{};
	int at = 0;
	for (const auto& r : merged) {
		b.lo[b.n] = r.first;
		b.hi[b.n] = r.second;
		++b.n;
		if (at < r.first) {
			rest.lo[rest.n] = at;
			rest.hi[rest.n] = r.first;
			++rest.n;
		}
		at = r.second;
	}
	if (at < n) {
		rest.lo[rest.n] = at;
		rest.hi[rest.n] = n;
		++rest.n;
	}
	D->boundary = b;
	D->bulk = rest;
	D->haloFirst = true;
}

template <typename T>
static int distCreate(smm_hip_comm* comm, int nGlobal, const int* bounds, const int* d_start, const int* d_positions, const T* d_values,
                      smm_hip_dist_csr** out) {
	if (!out) {
		setError("dist_csr_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!comm || !bounds || !d_start || nGlobal < 0) {
		setError("dist_csr_create: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	const int world = comm->world, rank = comm->rank;
	if (bounds[0] != 0 || bounds[world] != nGlobal) {
		setError("dist_csr_create: bounds must run from 0 to n_global");
		return SMM_HIP_ERR_INVALID;
	}
	for (int q = 0; q < world; ++q) {
		if (bounds[q] > bounds[q + 1]) {
			setError("dist_csr_create: bounds must be non-decreasing");
			return SMM_HIP_ERR_INVALID;
		}
	}
	struct Guard {
		smm_hip_dist_csr* d;
		~Guard() {
			if (d) smm_hip_dist_csr_destroy(d);
		}
	} guard{new smm_hip_dist_csr()};
	smm_hip_dist_csr* D = guard.d;
	D->comm = comm;
	D->dtype = dtypeOf<T>();
	D->nGlobal = nGlobal;
	D->rowBegin = bounds[rank];
	D->rowEnd = bounds[rank + 1];
	const int nLocal = D->nLocal = D->rowEnd - D->rowBegin;
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());  // the caller's arrays may still be being written on one of its streams (set-up path)
	int nnz = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&nnz, d_start + nLocal, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (nnz < 0 || (nnz > 0 && (!d_positions || !d_values))) {
		setError("dist_csr_create: bad start[] or null positions / values");
		return SMM_HIP_ERR_INVALID;
	}
	// column range this rank's rows touch
	int hmm[2] = {0x7fffffff, -1};
	if (nnz > 0) {
		DevBuf<int> mm;
		SMM_TRY(mm.alloc(2));
		SMM_HIP_TRY(hipMemcpyAsync(mm, hmm, sizeof(hmm), hipMemcpyHostToDevice, s));
		colRangeKernel<<<std::min(2048, (nnz + 255) / 256), 256, 0, s>>>(nnz, d_positions, mm);
		SMM_HIP_TRY(hipMemcpyAsync(hmm, mm, sizeof(hmm), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (hmm[0] < 0 || hmm[1] >= nGlobal) {
			setError("dist_csr_create: column %d outside [0, %d)", hmm[0] < 0 ? hmm[0] : hmm[1], nGlobal);
			return SMM_HIP_ERR_INVALID;
		}
	}
	D->cmin = nnz > 0 ? std::min(hmm[0], D->rowBegin) : D->rowBegin;
	D->cmaxExcl = nnz > 0 ? std::max(hmm[1] + 1, D->rowEnd) : D->rowEnd;
	D->extLen = std::max(1, D->cmaxExcl - D->cmin);
	D->ownOffset = D->rowBegin - D->cmin;
	// every rank learns every rank's range (an all-gather written as a sum of disjoint contributions)
	std::vector<long long> needs(2 * static_cast<size_t>(world), 0);
	needs[2 * rank] = D->cmin;
	needs[2 * rank + 1] = D->cmaxExcl;
	SMM_TRY(commAllreduceI64(comm, needs.data(), 2 * world));
	D->needs = needs;
	D->bounds.assign(bounds, bounds + world + 1);
	for (int q = 0; q < world; ++q) {
		if (q == rank) continue;
		long long lo = std::max<long long>(needs[2 * rank], bounds[q]), hi = std::min<long long>(needs[2 * rank + 1], bounds[q + 1]);
		if (lo < hi) {
			D->recvs.push_back({q, static_cast<int>(lo - D->cmin), static_cast<int>(hi - lo)});
			D->haloElements += static_cast<int>(hi - lo);
		}
		lo = std::max<long long>(needs[2 * q], D->rowBegin);
		hi = std::min<long long>(needs[2 * q + 1], D->rowEnd);
		if (lo < hi) D->sends.push_back({q, static_cast<int>(lo - D->cmin), static_cast<int>(hi - lo)});
	}
	// split
	int* cnt = nullptr;
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&cnt), 2 * (static_cast<size_t>(nLocal) + 1) * sizeof(int)));
	D->arrays[0] = cnt;  // becomes startLoc | startRem
	int* startLoc = cnt;
	int* startRem = cnt + nLocal + 1;
	const int grid = std::max(1, std::min(8192, (nLocal + 256) / 256));
	{
		const int split = env::intOr(env::SPLIT_SPMV, 1);  // (read at every create, like SMM_HIP_HALO_CHUNKS: a property of the matrix)
		D->splitAllowed = split != 0;
		D->splitForced = split == 2;  // (2: also between ranks that share a GPU -- the tests, whose matrices leave the card half empty)
		D->splitSumsLdsMax = std::max(0, env::intOr(env::SPLIT_SUMS_LDS, D->splitSumsLdsMax));
	}
	if (comm->kind == SMM_COMM_SELF) {
		D->labWindow = env::intOr(env::LAB_SELF_SPLIT, 0);  // (measurement hook: what a rank of a many-GPU run computes, on one GPU -- tools/lab/rank_loop_streams.py)
	}
	splitCountKernel<<<grid, 256, 0, s>>>(nLocal, d_start, d_positions, D->rowBegin, D->rowEnd, D->labWindow, startLoc, startRem);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(exclusiveScan(startLoc, nLocal + 1, s));
	SMM_TRY(exclusiveScan(startRem, nLocal + 1, s));
	int totals[2] = {0, 0};
	SMM_HIP_TRY(hipMemcpyAsync(&totals[0], startLoc + nLocal, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(&totals[1], startRem + nLocal, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	D->nnzLoc = totals[0];
	D->nnzRem = totals[1];
	D->remEmpty = totals[1] == 0;
	SMM_TRY(devAlloc(&D->arrays[1], std::max<size_t>(1, totals[0]) * sizeof(int)));
	SMM_TRY(devAlloc(&D->arrays[2], std::max<size_t>(1, totals[0]) * sizeof(T)));
	SMM_TRY(devAlloc(&D->arrays[4], std::max<size_t>(1, totals[1]) * sizeof(int)));
	SMM_TRY(devAlloc(&D->arrays[5], std::max<size_t>(1, totals[1]) * sizeof(T)));
	if (nLocal > 0) {
		splitScatterKernel<T><<<grid, 256, 0, s>>>(nLocal, d_start, d_positions, d_values, D->rowBegin, D->rowEnd, D->labWindow, D->cmin, startLoc, startRem,
		                                          static_cast<int*>(D->arrays[1]), static_cast<T*>(D->arrays[2]), static_cast<int*>(D->arrays[4]),
		                                          static_cast<T*>(D->arrays[5]));
		SMM_HIP_TRY(hipGetLastError());
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (dtypeOf<T>() == SMM_DTYPE_F32) {
		SMM_TRY(smm_hip_csr_create_dev_f32(nLocal, nLocal, startLoc, static_cast<int*>(D->arrays[1]), static_cast<float*>(D->arrays[2]), &D->aLoc));
		SMM_TRY(smm_hip_csr_create_dev_f32(nLocal, D->extLen, startRem, static_cast<int*>(D->arrays[4]), static_cast<float*>(D->arrays[5]), &D->aRem));
	} else {
		SMM_TRY(smm_hip_csr_create_dev_f64(nLocal, nLocal, startLoc, static_cast<int*>(D->arrays[1]), static_cast<double*>(D->arrays[2]), &D->aLoc));
		SMM_TRY(smm_hip_csr_create_dev_f64(nLocal, D->extLen, startRem, static_cast<int*>(D->arrays[4]), static_cast<double*>(D->arrays[5]), &D->aRem));
	}
	// ---- a thin remote block: the rows with a remote entry, listed (each rank for itself: nothing collective depends on it)
	{
		const bool allowed = env::flagOr(env::THIN_REMOTE, true);  // (read at every create: a property of the matrix; 0: the general second launch)
		if (allowed && nLocal > 0 && totals[1] > 0) {
			DevBuf<int> flag;
			SMM_TRY(flag.alloc(static_cast<size_t>(nLocal) + 1));
			thinFlagKernel<<<grid, 256, 0, s>>>(nLocal, startRem, flag);
			SMM_HIP_TRY(hipGetLastError());
			SMM_TRY(exclusiveScan(flag, nLocal + 1, s));
			int nThin = 0;
			SMM_HIP_TRY(hipMemcpyAsync(&nThin, flag.p + nLocal, sizeof(int), hipMemcpyDeviceToHost, s));
			SMM_HIP_TRY(hipStreamSynchronize(s));
			if (nThin > 0 && static_cast<long long>(nThin) * THIN_SHARE <= nLocal) {
				SMM_TRY(devAlloc(reinterpret_cast<void**>(&D->thinRows), static_cast<size_t>(nThin) * sizeof(int)));
				thinListKernel<<<grid, 256, 0, s>>>(nLocal, startRem, flag, D->thinRows);
				SMM_HIP_TRY(hipGetLastError());
				SMM_TRY(devAlloc(&D->partsThin, PARTS_LEN * sizeof(T)));
				SMM_HIP_TRY(hipMemsetAsync(D->partsThin, 0, PARTS_LEN * sizeof(T), s));
				SMM_HIP_TRY(hipStreamSynchronize(s));
				D->nThin = nThin;
			}
		}
	}
	// ---- the halo in pieces (opt-in): every rank must cut alike, so the ranks agree on the smallest request
	{
		const int wanted = std::max(1, std::min(MAX_HALO_CHUNKS, env::intOr(env::HALO_CHUNKS, 1)));  // (read at every create: a property of the matrix, not of the process)
		std::vector<long long> votes(static_cast<size_t>(world), 0);
		// (a rank whose segments do not fit the cut's table asks for one piece)
		votes[static_cast<size_t>(rank)] = D->recvs.size() > static_cast<size_t>(MAX_CHUNK_SEGS) ? 1 : wanted;
		SMM_TRY(commAllreduceI64(comm, votes.data(), world));
		int K = MAX_HALO_CHUNKS;
		for (long long v : votes) K = std::min<long long>(K, std::max<long long>(1, v));
		D->chunks = K;
	}
	if (D->chunks > 1) {
		const int K = D->chunks;
		auto piece = [K](const Seg& g, int k) {
			const int a = chunkBound(g.count, k, K), b = chunkBound(g.count, k + 1, K);
			return Seg{g.peer, g.offset + a, b - a};
		};
		D->sendsK.assign(static_cast<size_t>(K), {});
		D->recvsK.assign(static_cast<size_t>(K), {});
		for (int k = 0; k < K; ++k) {
			for (const Seg& g : D->sends) {
				const Seg q = piece(g, k);
				if (q.count > 0) D->sendsK[static_cast<size_t>(k)].push_back(q);
			}
			for (const Seg& g : D->recvs) {
				const Seg q = piece(g, k);
				if (q.count > 0) D->recvsK[static_cast<size_t>(k)].push_back(q);
			}
		}
		ChunkSegs segs{};
		segs.n = static_cast<int>(D->recvs.size());
		segs.K = K;
		for (int i = 0; i < segs.n; ++i) {
			segs.off[i] = D->recvs[static_cast<size_t>(i)].offset;
			segs.cnt[i] = D->recvs[static_cast<size_t>(i)].count;
		}
		int* starts = nullptr;
		SMM_TRY(devAlloc(reinterpret_cast<void**>(&starts), static_cast<size_t>(K) * (nLocal + 1) * sizeof(int)));
		D->chunkArrays.push_back(starts);
		chunkCountKernel<<<grid, 256, 0, s>>>(nLocal, startRem, static_cast<const int*>(D->arrays[4]), segs, starts);
		SMM_HIP_TRY(hipGetLastError());
		ChunkOut outs{};
		std::vector<int> totalsK(static_cast<size_t>(K), 0);
		for (int k = 0; k < K; ++k) SMM_TRY(exclusiveScan(starts + static_cast<size_t>(k) * (nLocal + 1), nLocal + 1, s));
		for (int k = 0; k < K; ++k) {
			SMM_HIP_TRY(hipMemcpyAsync(&totalsK[static_cast<size_t>(k)], starts + static_cast<size_t>(k) * (nLocal + 1) + nLocal, sizeof(int), hipMemcpyDeviceToHost, s));
		}
		SMM_HIP_TRY(hipStreamSynchronize(s));
		for (int k = 0; k < K; ++k) {
			void *pp = nullptr, *pv = nullptr;
			SMM_TRY(devAlloc(&pp, std::max<size_t>(1, totalsK[static_cast<size_t>(k)]) * sizeof(int)));
			D->chunkArrays.push_back(pp);
			SMM_TRY(devAlloc(&pv, std::max<size_t>(1, totalsK[static_cast<size_t>(k)]) * sizeof(T)));
			D->chunkArrays.push_back(pv);
			outs.pos[k] = static_cast<int*>(pp);
			outs.val[k] = pv;
		}
		if (nLocal > 0) {
			chunkScatterKernel<T><<<grid, 256, 0, s>>>(nLocal, startRem, static_cast<const int*>(D->arrays[4]), static_cast<const T*>(D->arrays[5]), segs, starts, outs);
			SMM_HIP_TRY(hipGetLastError());
		}
		SMM_HIP_TRY(hipStreamSynchronize(s));
		D->aRemK.assign(static_cast<size_t>(K), nullptr);
		D->nnzRemK.assign(totalsK.begin(), totalsK.end());
		for (int k = 0; k < K; ++k) {
			int* st = starts + static_cast<size_t>(k) * (nLocal + 1);
			if (dtypeOf<T>() == SMM_DTYPE_F32) {
				SMM_TRY(smm_hip_csr_create_dev_f32(nLocal, D->extLen, st, outs.pos[k], static_cast<float*>(outs.val[k]), &D->aRemK[static_cast<size_t>(k)]));
			} else {
				SMM_TRY(smm_hip_csr_create_dev_f64(nLocal, D->extLen, st, outs.pos[k], static_cast<double*>(outs.val[k]), &D->aRemK[static_cast<size_t>(k)]));
			}
		}
	}
	SMM_TRY(distWorkspace<T>(D));
	planHaloFirst<T>(D);
	SMM_TRY(p2pSetup<T>(D));
	guard.d = nullptr;
	*out = D;
	return SMM_HIP_OK;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_dist_csr_create_dev_f32(smm_hip_comm* comm, int n_global, const int* bounds, const int* d_start, const int* d_positions,
                                    const float* d_values, smm_hip_dist_csr** out) {
	SMM_TRY(commUsable(comm));
	return guardComm(comm, distCreate<float>(comm, n_global, bounds, d_start, d_positions, d_values, out));
}
int smm_hip_dist_csr_create_dev_f64(smm_hip_comm* comm, int n_global, const int* bounds, const int* d_start, const int* d_positions,
                                    const double* d_values, smm_hip_dist_csr** out) {
	SMM_TRY(commUsable(comm));
	return guardComm(comm, distCreate<double>(comm, n_global, bounds, d_start, d_positions, d_values, out));
}

int smm_hip_dist_csr_destroy(smm_hip_dist_csr* D) {
	if (!D) return SMM_HIP_OK;
	p2pTeardown(D);
	smm_hip_csr_destroy(D->aLoc);
	smm_hip_csr_destroy(D->aRem);
	for (smm_hip_csr* piece : D->aRemK) smm_hip_csr_destroy(piece);
	for (void* p : D->chunkArrays) devFree(p);
	for (void* p : D->arrays) devFree(p);
	for (void* p : {D->r, D->r0, D->ap, D->as, D->scratch, D->pExt, D->sExt, D->xExt, D->partsA, D->partsB, D->partsC, D->sc}) devFree(p);
	devFree(D->splitSync);
	devFree(D->thinRows);
	devFree(D->partsThin);
	devFree(D->rExt);
	for (void* p : D->lazyExt) devFree(p);
	delete D;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_info(const smm_hip_dist_csr* D, int* n_local, int* ext_len, int* own_offset, int* halo_elements, long long* nnz_loc,
                          long long* nnz_rem) {
	if (!D) {
		setError("dist_csr_info: null handle");
		return SMM_HIP_ERR_INVALID;
	}
	if (n_local) *n_local = D->nLocal;
	if (ext_len) *ext_len = D->extLen;
	if (own_offset) *own_offset = D->ownOffset;
	if (halo_elements) *halo_elements = D->haloElements;
	if (nnz_loc) *nnz_loc = D->nnzLoc;
	if (nnz_rem) *nnz_rem = D->nnzRem;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_halo_chunks(const smm_hip_dist_csr* D, int* chunks) {
	if (!D || !chunks) {
		setError("dist_csr_halo_chunks: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*chunks = D->chunks;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_options(const smm_hip_dist_csr* D, int* p2p, int* relays, int* halo_first, double* direct_share) {
	if (!D) {
		setError("dist_csr_options: null handle");
		return SMM_HIP_ERR_INVALID;
	}
	if (p2p) *p2p = D->p2p ? (D->p2p->haloOn ? 1 : 2) : 0;
	if (relays) *relays = D->p2p ? D->p2p->relays : 0;
	if (halo_first) *halo_first = D->haloFirst ? 1 : 0;
	if (direct_share) *direct_share = D->p2p ? D->p2p->directShare : 1.0;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_matvec_forms(const smm_hip_dist_csr* D, long long* one_launch, long long* two_launches) {
	if (!D) {
		setError("dist_csr_matvec_forms: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (one_launch) *one_launch = D->matvecsSplit;
	if (two_launches) *two_launches = D->matvecsTwo;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_thin_remote(const smm_hip_dist_csr* D, int* rows, long long* matvecs) {
	if (!D) {
		setError("dist_csr_thin_remote: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (rows) *rows = D->nThin;
	if (matvecs) *matvecs = D->matvecsThin;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_cg_fused(const smm_hip_dist_csr* D, long long* matvecs) {
	if (!D || !matvecs) {
		setError("dist_csr_cg_fused: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*matvecs = D->cgFused;
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_split_wait(smm_hip_dist_csr* D, double* waited_ms, int reset) {
	if (!D || !waited_ms) {
		setError("dist_csr_split_wait: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*waited_ms = 0.0;
	if (!D->splitSync) return SMM_HIP_OK;
	unsigned long long ticks = 0;
	SMM_HIP_TRY(hipDeviceSynchronize());
	SMM_HIP_TRY(hipMemcpy(&ticks, D->splitSync + P2P_KINDS + 1, sizeof(ticks), hipMemcpyDeviceToHost));
	if (reset) SMM_HIP_TRY(hipMemset(D->splitSync + P2P_KINDS + 1, 0, sizeof(ticks)));
	*waited_ms = static_cast<double>(ticks) * 1.0e-5;  // (wall_clock64 counts at 100 MHz on gfx9)
	return SMM_HIP_OK;
}

int smm_hip_dist_csr_local_block(const smm_hip_dist_csr* D, smm_hip_csr** a_loc, smm_hip_csr** a_rem) {
	if (!D) {
		setError("dist_csr_local_block: null handle");
		return SMM_HIP_ERR_INVALID;
	}
	if (a_loc) *a_loc = D->aLoc;
	if (a_rem) *a_rem = D->aRem;
	return SMM_HIP_OK;
}

}  // extern "C"
