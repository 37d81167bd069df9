// smm_spmv_blocks.hip -- the BLOCKS SpMV family: matrices that are a sparse matrix of dense b x b blocks (b = 2, 3, 4).
//
// Vector-valued problems on unstructured meshes (elasticity: 3 unknowns per node) have far too many column offsets for the PATTERN
// family, but their structure is simple: the b rows of a block row hold the same number of entries, and those entries come in groups
// of b consecutive columns c .. c + b - 1 with c a multiple of b, the same c in all b rows.  ONE column index per block (4 / b^2 bytes
// per entry instead of 4) then replaces positions[], and the b entries of x a block needs are contiguous and serve all b rows.
//
// Analysis (smm_hip_csr_find_blocks): every stored entry is checked on the device against that rule (blocksVerifyKernel); a matrix
// that passes keeps block_col[nnz / b^2], the block-row starts (start[R b] / b^2) and a tile table cut on block-row boundaries with the
// STREAM family's cutRows.  values[] is NOT copied: the kernel reads the handle's own array, so every value edit is seen at once and
// needs no refresh; positions[] of a handle never changes, so the verification stays valid.
//
// Kernel (spmvBlocksKernel): a workgroup takes a tile of whole block rows; the tile's contiguous ranges of values[] and block_col[]
// are staged into LDS with 16-byte coalesced non-temporal loads; then ONE LANE PER BLOCK ROW walks the blocks in stored order with b
// accumulators: per block it loads the b contiguous x values once and issues the b^2 multiply-adds out of LDS.  Row i's chain is its
// entries in stored order starting from 0 -- the reference's sum (ref:1484-1489), the bits of STREAM at one lane per row.
#include <algorithm>
#include <cstring>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_pattern_dev.h"

namespace smm {

// stored entries of a tile, and so of a block row (the b rows together): what the LDS stage holds.  fp64: 32 KiB of values + <= 4 KiB of
// block columns per workgroup, four workgroups per CU
constexpr int BLK_TILE_ENTRIES = 4096;
constexpr int BLK_STAGE_SLACK = 8;  // the aligned head before a tile and the tail of its last 16-byte piece
constexpr int BLK_G = 4;            // blocks whose x loads a lane keeps in flight together

// blocks a block row may hold / entries a ROW may hold at block size b (smm_hip_csr_blocks_info: max_row_entries)
static int blkMaxRowBlocks(int b) { return BLK_TILE_ENTRIES / (b * b); }
static int blkMaxRowEntries(int b) { return blkMaxRowBlocks(b) * b; }

extern __shared__ __attribute__((aligned(16))) unsigned char smmBlkLds[];

typedef int bi32x4 __attribute__((ext_vector_type(4)));

// ---- analysis ---------------------------------------------------------------------------------------------------------------------
// One thread per row r of block row R = r / B.  *bad is raised when: the row's length differs from the first row's of its block row, is no
// multiple of B or exceeds maxRowBlocks blocks; the k-th entry's column is not c + k % B with c = the first row's column of group k / B;
// that c is no multiple of B or the block leaves [0, cols).
template <int B>
__global__ void blocksVerifyKernel(int rows, int cols, int maxRowBlocks, const int* __restrict__ start, const int* __restrict__ positions, int* __restrict__ bad) {
	const long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (r >= rows) return;
	if (r == 0 && start[0] != 0) atomicOr(bad, 1);
	const int r0 = static_cast<int>(r / B) * B;
	const int s0 = start[r0], len0 = start[r0 + 1] - s0;
	const int s = start[r], len = start[r + 1] - s;
	if (len != len0 || len < 0 || len % B != 0 || len / B > maxRowBlocks) {
		atomicOr(bad, 1);
		return;
	}
	bool ok = true;
	for (int k = 0; k < len; ++k) {
		const int c = positions[s0 + (k / B) * B];
		ok = ok && c >= 0 && c % B == 0 && c + B <= cols && positions[s + k] == c + k % B;
	}
	if (!ok) atomicOr(bad, 1);
}

// blkStart[R] = start[R B] / B^2 (every earlier block row consists of whole blocks), blkCol[block] = c / B
template <int B>
__global__ void blocksBuildKernel(int blockRows, const int* __restrict__ start, const int* __restrict__ positions, int* __restrict__ blkStart, int* __restrict__ blkCol) {
	const long long R = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (R > blockRows) return;
	const int s0 = start[R * B];
	const int bs = s0 / (B * B);
	blkStart[R] = bs;
	if (R == blockRows) return;
	const int nb = (start[R * B + 1] - s0) / B;
	for (int j = 0; j < nb; ++j) blkCol[bs + j] = positions[s0 + j * B] / B;
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------
// tiles[] holds {first block row, blkStart[first block row]} per tile (nTiles + 1 entries, the last one {block rows, blocks}).
// vecOk: values[] starts on a 16-byte boundary (else the stage uses element loads).  x is only read element by element: it may be any
// element-aligned view.
template <typename T, int B>
__global__ __launch_bounds__(TPB) void spmvBlocksKernel(int nTiles, const int2* __restrict__ tiles, const int* __restrict__ blkStart, const int* __restrict__ blkCol,
                                                        const T* __restrict__ values, int nnz, int nBlocks, int vecOk, int opFlags, const T* lhs,
                                                        const T* __restrict__ divisor, const T* __restrict__ x, T* out, int dotMode, const T* __restrict__ w1,
                                                        T* __restrict__ partials, const int* __restrict__ doneFlag) {
	using V = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	constexpr int BB = B * B;
	constexpr int NV = BLK_TILE_ENTRIES / (N * TPB) + 1;                 // 16-byte pieces of values[] a lane stages per tile
	constexpr int NVC = (BLK_TILE_ENTRIES / BB + 4 * TPB - 1) / (4 * TPB) + 1;  // ... of block_col[]
	// LDS (sized by the host): red[4] | sVal[BLK_TILE_ENTRIES + SLACK] | sCol[BLK_TILE_ENTRIES / BB + SLACK]
	T* red = reinterpret_cast<T*>(smmBlkLds);
	T* sVal = red + 4;
	int* sCol = reinterpret_cast<int*>(sVal + BLK_TILE_ENTRIES + BLK_STAGE_SLACK);
	if (doneFlag && *doneFlag) return;
	const int op = opFlags & 0xFF;
	const bool ntOut = (opFlags & SPMV_NT_OUT) != 0;
	const int t = threadIdx.x;
	T acc0 = T(0), acc1 = T(0);

	// XCD-aware work split, as in spmvStreamKernel: each of the 8 groups of workgroups (b, b + 8, ...) walks one contiguous eighth of the tiles
	const int nGroups = min(8, static_cast<int>(gridDim.x));
	const int xcdGroup = blockIdx.x % nGroups;
	const int groupSlots = (static_cast<int>(gridDim.x) - xcdGroup + nGroups - 1) / nGroups;
	const int chunkTiles = (nTiles + nGroups - 1) / nGroups;
	const int tileLo = min(nTiles, xcdGroup * chunkTiles), tileHi = min(nTiles, tileLo + chunkTiles);
	for (int tile = tileLo + blockIdx.x / nGroups; tile < tileHi; tile += groupSlots) {
		const int2 m0 = tiles[tile], m1 = tiles[tile + 1];
		const int r0 = m0.x, nrows = m1.x - m0.x;
		const int e0 = m0.y * BB, e1 = m1.y * BB;  // the tile's entries: e1 - e0 <= BLK_TILE_ENTRIES
		const int a0 = e0 & ~(N - 1);              // 16-byte aligned element index
		const int c0 = m0.y & ~3;
		// ---- stage values[a0 .. e1) and blkCol[c0 .. m1.y): all loads first, then the LDS stores ----
		V rv[NV];
		bi32x4 rc[NVC];
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			const long long i = static_cast<long long>(a0) + N * (t + v * TPB);
			if (i < e1) {
				if (vecOk && i + N <= nnz) {
					rv[v] = __builtin_nontemporal_load(reinterpret_cast<const V*>(values + i));
				} else {
#pragma unroll
					for (int u = 0; u < N; ++u) rv[v][u] = i + u < nnz ? values[i + u] : T(0);
				}
			}
		}
#pragma unroll
		for (int v = 0; v < NVC; ++v) {
			const long long i = static_cast<long long>(c0) + 4 * (t + v * TPB);
			if (i < m1.y) {
				if (i + 4 <= nBlocks) {
					rc[v] = __builtin_nontemporal_load(reinterpret_cast<const bi32x4*>(blkCol + i));
				} else {
#pragma unroll
					for (int u = 0; u < 4; ++u) rc[v][u] = i + u < nBlocks ? blkCol[i + u] : 0;
				}
			}
		}
		int bs = 0, nb = 0;
		if (t < nrows) {
			bs = blkStart[r0 + t];
			nb = blkStart[r0 + t + 1] - bs;
		}
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			const int li = N * (t + v * TPB);
			if (static_cast<long long>(a0) + li < e1) *reinterpret_cast<V*>(sVal + li) = rv[v];
		}
#pragma unroll
		for (int v = 0; v < NVC; ++v) {
			const int li = 4 * (t + v * TPB);
			if (static_cast<long long>(c0) + li < m1.y) *reinterpret_cast<bi32x4*>(sCol + li) = rc[v];
		}
		ldsBarrier();  // the tile is in LDS
		if (t < nrows) {
			const int R = r0 + t;
			const int len = nb * B;
			const T* rowVal = sVal + (bs * BB - a0);  // row i of the block row: rowVal + i * len
			const int* cols = sCol + (bs - c0);
			T acc[B];
#pragma unroll
			for (int i = 0; i < B; ++i) acc[i] = T(0);
			int j = 0;
			for (; j + BLK_G <= nb; j += BLK_G) {  // the x loads of BLK_G blocks are issued before the first multiply-add
				T xv[BLK_G][B];
#pragma unroll
				for (int g = 0; g < BLK_G; ++g) {
					const T* xp = x + static_cast<long long>(cols[j + g]) * B;
#pragma unroll
					for (int c = 0; c < B; ++c) xv[g][c] = xp[c];
				}
#pragma unroll
				for (int g = 0; g < BLK_G; ++g) {
#pragma unroll
					for (int i = 0; i < B; ++i) {
#pragma unroll
						for (int c = 0; c < B; ++c) acc[i] = smmFma(rowVal[i * len + (j + g) * B + c], xv[g][c], acc[i]);
					}
				}
			}
			for (; j < nb; ++j) {
				T xv[B];
				const T* xp = x + static_cast<long long>(cols[j]) * B;
#pragma unroll
				for (int c = 0; c < B; ++c) xv[c] = xp[c];
#pragma unroll
				for (int i = 0; i < B; ++i) {
#pragma unroll
					for (int c = 0; c < B; ++c) acc[i] = smmFma(rowVal[i * len + j * B + c], xv[c], acc[i]);
				}
			}
#pragma unroll
			for (int i = 0; i < B; ++i) {
				const int row = R * B + i;
				const T o = patApplyOp(op, lhs, divisor, row, acc[i]);
				storeOut(out + row, o, ntOut);
				if (dotMode == 2) acc0 += o * o;
				if (dotMode) acc1 += o * w1[row];
			}
		}
		ldsBarrier();  // every lane is done with the LDS copy of this tile
	}
	if (dotMode) {
		if (dotMode == 2) {
			const T s0 = blockSum256(acc0, red);
			if (t == 0) partials[blockIdx.x] = s0;
		}
		const T s1 = blockSum256(acc1, red);
		if (t == 0) partials[(dotMode == 2 ? NPART : 0) + blockIdx.x] = s1;
		// consumers always add NPART slots per quantity: clear the ones no workgroup of this (smaller) grid owns
		for (int i = gridDim.x + blockIdx.x * TPB + t; i < NPART; i += gridDim.x * TPB) {
			partials[i] = T(0);
			if (dotMode == 2) partials[NPART + i] = T(0);
		}
		if (opFlags & SPMV_FINISH) lastBlockSums<T>(partials, NPART, dotMode == 2 ? 2 : 1, partials + PARTS_TOTALS, partsTicket(partials));
	}
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
template <int B>
static int tryBlockSize(smm_hip_csr* m, hipStream_t s, bool* fits) {
	*fits = false;
	const int rows = m->rows, cols = m->cols;
	if (rows % B || cols % B || m->nnz % (B * B)) return SMM_HIP_OK;
	DevBuf<int> bad;
	SMM_TRY(bad.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), s));
	if (rows > 0) blocksVerifyKernel<B><<<(rows + 255) / 256, 256, 0, s>>>(rows, cols, blkMaxRowBlocks(B), m->d_start, m->d_positions, bad);
	int h_bad = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (h_bad) return SMM_HIP_OK;
	const int blockRows = rows / B;
	const int nBlocks = m->nnz / (B * B);
	DevBuf<int> bstart, bcol;
	SMM_TRY(bstart.alloc(static_cast<size_t>(blockRows) + 1));
	SMM_TRY(bcol.alloc(static_cast<size_t>(nBlocks) + 4));
	if (rows > 0) {
		blocksBuildKernel<B><<<(blockRows + 1 + 255) / 256, 256, 0, s>>>(blockRows, m->d_start, m->d_positions, bstart, bcol);
	} else {
		SMM_HIP_TRY(hipMemsetAsync(bstart, 0, sizeof(int), s));
	}
	SMM_HIP_TRY(hipGetLastError());
	int2* tiles = nullptr;
	int nTiles = 0;
	SMM_TRY(cutRows(bstart, blockRows, nBlocks, blkMaxRowBlocks(B), TPB, s, &tiles, &nTiles));  // synchronises s: the two arrays are written
	// a later call with another size replaces the kept analysis; the old arrays go to the allocator's quarantine, so launches already
	// enqueued with them stay valid
	devFree(m->d_blk_col);
	devFree(m->d_blk_start);
	devFree(m->d_blk_tiles);
	m->d_blk_col = bcol.detach();
	m->d_blk_start = bstart.detach();
	m->d_blk_tiles = reinterpret_cast<int*>(tiles);
	m->blk_n_tiles = nTiles;
	m->blk_blocks = nBlocks;
	*fits = true;
	return SMM_HIP_OK;
}

// caller holds tileMutex.  *found: the size kept by THIS call, 0 when none of the sizes tried fits (an earlier analysis then stays)
static int findBlocksLocked(smm_hip_csr* m, int blockSize, int* found) {
	*found = 0;
	SMM_HIP_TRY(hipDeviceSynchronize());  // set-up call without a stream: the matrix may still be being written on a caller's stream
	hipStream_t s = libStream();
	static const int SIZES[] = {4, 3, 2};
	for (int b : SIZES) {
		if (blockSize != 0 && blockSize != b) continue;
		if (m->blk_state.load(std::memory_order_acquire) == b) {  // already kept at this size
			*found = b;
			return SMM_HIP_OK;
		}
		bool fits = false;
		SetupTrace trace("BLOCKS analysis (one size)");
		SMM_TRY(b == 4 ? tryBlockSize<4>(m, s, &fits) : b == 3 ? tryBlockSize<3>(m, s, &fits) : tryBlockSize<2>(m, s, &fits));
		if (fits) {
			m->blk_state.store(b, std::memory_order_release);
			*found = b;
			return SMM_HIP_OK;
		}
	}
	if (m->blk_state.load(std::memory_order_acquire) == 0) m->blk_state.store(-1, std::memory_order_release);
	return SMM_HIP_OK;
}

// smm_hip_csr_set_kernel(m, SMM_SPMV_BLOCKS, ...): the analysis if none is kept; SMM_HIP_ERR_INVALID when nothing fits
int ensureBlocks(smm_hip_csr* m) {
	std::lock_guard<std::mutex> lock(m->tileMutex);
	int found = m->blk_state.load(std::memory_order_acquire);
	if (found == 0) SMM_TRY(findBlocksLocked(m, 0, &found));
	if (found <= 0) {
		setError("blocks SpMV: the matrix is not made of dense 2x2, 3x3 or 4x4 blocks on block-aligned columns with at most %d stored entries per block row",
		         BLK_TILE_ENTRIES);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

const char* blocksKernelDesc(const smm_hip_csr* m, long long* bytes) {
	const long long b = m->blk_state.load(std::memory_order_acquire);
	const long long s = m->dtype == SMM_DTYPE_F32 ? 4 : 8;
	if (b > 0) *bytes = static_cast<long long>(m->nnz) * s + (m->nnz / (b * b)) * 4 + (m->rows / b + 1) * 4 + m->cols * s + m->rows * s;
	return "spmvBlocksKernel";
}

template <typename T, int B>
static void launchBlocksB(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials, const int* doneFlag,
                          hipStream_t s) {
	const size_t lds = 4 * sizeof(T) + static_cast<size_t>(BLK_TILE_ENTRIES + BLK_STAGE_SLACK) * sizeof(T) +
	                   static_cast<size_t>(BLK_TILE_ENTRIES / (B * B) + BLK_STAGE_SLACK) * sizeof(int);
	static std::atomic<int> granted{0};
	static std::atomic<long long> occ{0};
	(void)ensureDynamicLds(granted, spmvBlocksKernel<T, B>, lds);
	int perCU = occupancyCached(occ, spmvBlocksKernel<T, B>, TPB, lds, 4);
	if (forcedWgsPerCU() > 0) perCU = forcedWgsPerCU();
	const int cus = (op & SPMV_LEAVE_ROOM) ? std::max(8, numCUs() - 8) : numCUs();
	const int grid = std::max(1, std::min(std::min(m->blk_n_tiles, cus * perCU), NPART));
	const int vecOk = (reinterpret_cast<uintptr_t>(m->d_values) & 15u) == 0 ? 1 : 0;
	spmvBlocksKernel<T, B><<<grid, TPB, lds, s>>>(m->blk_n_tiles, reinterpret_cast<const int2*>(m->d_blk_tiles), m->d_blk_start, m->d_blk_col,
	                                            static_cast<const T*>(m->d_values), m->nnz, m->blk_blocks, vecOk, (op & ~(SPMV_LEAVE_ROOM | SPMV_HALF_TILES)) | spmvOutFlags(m, sizeof(T)),
	                                            lhs, divisor, x, out, dotMode, w1, partials, doneFlag);
}

// the launch behind launchSpmv; `op` carries the flags
template <typename T>
int launchSpmvBlocks(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials, const int* doneFlag,
                     hipStream_t s) {
	const int b = m->blk_state.load(std::memory_order_acquire);  // every blk_* field was written before the state turned positive
	if (b <= 0) {
		setError("blocks SpMV: the matrix has no block analysis");
		return SMM_HIP_ERR_INVALID;
	}
	if (b == 4) launchBlocksB<T, 4>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	else if (b == 3) launchBlocksB<T, 3>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	else launchBlocksB<T, 2>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template int launchSpmvBlocks<float>(const smm_hip_csr*, int, const float*, const float*, const float*, float*, int, const float*, float*, const int*, hipStream_t);
template int launchSpmvBlocks<double>(const smm_hip_csr*, int, const double*, const double*, const double*, double*, int, const double*, double*, const int*, hipStream_t);

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_find_blocks(smm_hip_csr* m, int block_size, int* found) {
	if (found) *found = 0;
	if (!m) {
		setError("csr_find_blocks: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (block_size != 0 && block_size != 2 && block_size != 3 && block_size != 4) {
		setError("csr_find_blocks: block_size must be 0 (try 4, 3, 2), 2, 3 or 4, not %d", block_size);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	std::lock_guard<std::mutex> lock(m->tileMutex);
	int kept = 0;
	SMM_TRY(findBlocksLocked(m, block_size, &kept));
	if (found) *found = kept;
	return SMM_HIP_OK;
}

int smm_hip_csr_blocks_info(const smm_hip_csr* m, int* block_size, long long* blocks, int* max_row_entries) {
	if (!m) {
		setError("csr_blocks_info: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	const int b = m->blk_state.load(std::memory_order_acquire);
	if (block_size) *block_size = b > 0 ? b : 0;
	if (blocks) *blocks = b > 0 ? m->blk_blocks : 0;
	if (max_row_entries) *max_row_entries = b > 0 ? blkMaxRowEntries(b) : 0;
	return SMM_HIP_OK;
}

}  // extern "C"
