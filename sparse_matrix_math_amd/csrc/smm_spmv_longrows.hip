// smm_spmv_longrows.hip -- the LONGROWS SpMV family: matrices with a few very long rows among ordinary ones.
//
// Every other family gives a row that does not fit a tile to ONE wavefront of one workgroup, which streams it from HBM while the rest of
// the chip has long finished the ordinary rows: a dense constraint row of a KKT system, the dense row that the transpose of a global
// regressor column is, the hub rows of a graph Laplacian.  Here a row of more than split_len entries is cut into segments of
// segment_len entries, counted from the row's own first entry, and an SpMV is two launches:
//
//   spmvLongSegmentsKernel  the unit of work is one SEGMENT, taken by one wavefront: its slices of values[] / positions[] are staged into
//                           the wave's own piece of LDS with 16-byte coalesced non-temporal loads (aligned head, as the STREAM staging),
//                           then lane l walks entries l, l + 64, ... of the segment in batches of 8 x[] gathers; the 64 chains meet in
//                           groupSum<WAVE>'s butterfly and the sum goes to segSums[segment] -- a scratch array of THIS CALL.
//   spmvLongRowsKernel      the row kernel: tiles of short rows through LDS, one lane per row, exactly STREAM's data path at one lane per
//                           row (the reference's order, ref:1484-1489); a long row is a tile of its own: wavefront 0 of the workgroup that
//                           owns the tile adds its segment sums in ascending order and runs the common epilogue (op, divide forms, fused
//                           dots) -- the tile table fixes which workgroup that is, so the dot partials do not depend on arrival order.
//
// The order is stated in include/smm_hip.h (SMM_SPMV_LONGROWS) and restated in numpy in tests/longrows_restatement.py.  It depends on the
// row's entries, split_len and segment_len only.  values[] is read in place; the analysis reads start[] only.
#include <algorithm>
#include <climits>
#include <cstring>

#include "smm_csr_build.h"
#include "smm_device.h"
#include "smm_pattern_dev.h"

namespace smm {

constexpr int LR_PIECE = 4 * TPB;   // entries the row kernel stages per pass: one 16-byte load of positions[] per lane
constexpr int LR_PAD = 16;          // slack a gather batch may read past its row
constexpr int LR_GATHER = 8;        // x[] gathers a lane keeps in flight
constexpr int LR_SEG_SLACK = 8;     // the aligned head before a segment and the tail of its last 16-byte piece
constexpr int LR_WAVES = TPB / WAVE;
template <typename T>
struct LrCfg {
	static constexpr int NVMAX = sizeof(T) == 4 ? 4 : 2;  // staging passes of the row kernel: a tile holds NVMAX * 1024 - 3 entries at most
};
static_assert(SMM_LONGROWS_SPLIT_MAX <= LrCfg<double>::NVMAX * LR_PIECE - 3, "a short row must fit the fp64 tile");
static_assert(SMM_LONGROWS_SEGMENT_MIN == WAVE && SMM_LONGROWS_SEGMENT_MAX % WAVE == 0, "segments are whole rounds of the 64 chains");

typedef int li32x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) unsigned char smmLrLds[];

__device__ __forceinline__ float lrReadLane(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ __forceinline__ double lrReadLane(double v, int j) {
	const long long bits = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_readlane(static_cast<int>(bits), j);
	const int hi = __builtin_amdgcn_readlane(static_cast<int>(bits >> 32), j);
	return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

// the 4 entries of positions[] / values[] from element i (a multiple of 4) on: one (fp64 values: two) 16-byte non-temporal load(s) where
// the array starts on a 16-byte boundary and the piece lies inside it, element loads with the bound checked otherwise
__device__ __forceinline__ li32x4 lrLoadPos(const int* __restrict__ positions, int i, int nnz, int vecOk) {
	li32x4 r;
	if (vecOk && i + 4 <= nnz) {
		r = __builtin_nontemporal_load(reinterpret_cast<const li32x4*>(positions + i));
	} else {
#pragma unroll
		for (int u = 0; u < 4; ++u) r[u] = i + u < nnz ? positions[i + u] : 0;
	}
	return r;
}
template <typename T>
__device__ __forceinline__ void lrLoadVal(typename Pack16<T>::V (&r)[4 / Pack16<T>::N], const T* __restrict__ values, int i, int nnz, int vecOk) {
	using V = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	if (vecOk && i + 4 <= nnz) {
#pragma unroll
		for (int h = 0; h < 4 / N; ++h) r[h] = __builtin_nontemporal_load(reinterpret_cast<const V*>(values + i + h * N));
	} else {
#pragma unroll
		for (int u = 0; u < 4; ++u) r[u / N][u % N] = i + u < nnz ? values[i + u] : T(0);
	}
}
template <typename T>
__device__ __forceinline__ void lrStore(const li32x4& rp, const typename Pack16<T>::V (&rv)[4 / Pack16<T>::N], unsigned* sOff, T* sVal, int li) {
	using V = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	*reinterpret_cast<li32x4*>(sOff + li) = rp * static_cast<int>(sizeof(T));  // byte offsets into x: a gather is base + 32-bit offset
#pragma unroll
	for (int h = 0; h < 4 / N; ++h) *reinterpret_cast<V*>(sVal + li + h * N) = rv[h];
}

// ---- analysis ---------------------------------------------------------------------------------------------------------------------
// One thread per row (and one for the closing element): whether the row is long, the segments it is cut into, and its length as the tile
// cut is to see it -- a long row counts as at least capNnz + 1 entries, so that cutRows makes it a tile of its own.
__global__ void lrMarkKernel(int rows, const int* __restrict__ start, int splitLen, int segLen, int capNnz, int* __restrict__ isLong, int* __restrict__ segs,
                             int* __restrict__ cutLen) {
	const long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (r > rows) return;
	int len = 0;
	if (r < rows) len = start[r + 1] - start[r];
	const bool lng = len > splitLen;
	isLong[r] = lng ? 1 : 0;
	segs[r] = lng ? (len + segLen - 1) / segLen : 0;
	cutLen[r] = lng ? max(len, capNnz + 1) : len;
}

// after the three exclusive scans: lrRows[k] = {row, first segment} of the k-th long row, closed by {rows, segments}
__global__ void lrListKernel(int rows, const int* __restrict__ start, int splitLen, const int* __restrict__ longIdx, const int* __restrict__ segFirst,
                             int2* __restrict__ lrRows) {
	const long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (r > rows) return;
	if (r == rows || start[r + 1] - start[r] > splitLen) lrRows[longIdx[r]] = make_int2(static_cast<int>(r), segFirst[r]);
}

// the tiles were cut on the scanned cutLen[]: put the real start[first row] back
__global__ void lrTileStartKernel(int n, int2* __restrict__ tiles, const int* __restrict__ start) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) tiles[i].y = start[tiles[i].x];
}

// ---- launch 1: one sum per segment --------------------------------------------------------------------------------------------------
// NV: 16-byte pieces of positions[] a lane stages per segment (segLen <= (NV - 1) * 256).  LDS (sized by the host): the four waves'
// sVal[segLen + SLACK], then their sOff[segLen + SLACK].  vecOk: bit 0 positions[], bit 1 values[] start on a 16-byte boundary.
template <typename T, int NV>
__global__ __launch_bounds__(TPB) void spmvLongSegmentsKernel(int nLong, int nSegs, int segLen, const int2* __restrict__ lrRows, const int* __restrict__ start,
                                                              const int* __restrict__ positions, const T* __restrict__ values, int nnz, int vecOk,
                                                              const T* __restrict__ x, T* __restrict__ segSums, const int* __restrict__ doneFlag) {
	using V = typename Pack16<T>::V;
	if (doneFlag && *doneFlag) return;
	const int lane = threadIdx.x & (WAVE - 1);
	const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
	const int region = segLen + LR_SEG_SLACK;
	T* sVal = reinterpret_cast<T*>(smmLrLds) + wave * region;
	unsigned* sOff = reinterpret_cast<unsigned*>(reinterpret_cast<T*>(smmLrLds) + LR_WAVES * region) + wave * region;
	for (int seg = blockIdx.x * LR_WAVES + wave; seg < nSegs; seg += gridDim.x * LR_WAVES) {
		// the long row this segment belongs to: the last one whose first segment is <= seg
		int lo = 0, hi = nLong - 1;
		while (lo < hi) {
			const int mid = lo + (hi - lo + 1) / 2;
			if (lrRows[mid].y <= seg) lo = mid;
			else hi = mid - 1;
		}
		const int2 lr = lrRows[lo];
		const int rowEnd = start[lr.x + 1];
		const int b = start[lr.x] + (seg - lr.y) * segLen;  // counted from the row's own first entry
		const int e = min(rowEnd, b + segLen);
		const int a0 = b & ~3;  // 16-byte aligned element index for both arrays
		// ---- stage [a0, e): all loads first, then the LDS stores ----
		li32x4 rp[NV];
		V rv[NV][4 / Pack16<T>::N];
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			const int i = a0 + 4 * (lane + v * WAVE);
			if (i < e) {
				rp[v] = lrLoadPos(positions, i, nnz, vecOk & 1);
				lrLoadVal<T>(rv[v], values, i, nnz, vecOk & 2);
			}
		}
		__builtin_amdgcn_wave_barrier();  // (the chains of the wave's previous segment are read out of LDS before this one is stored)
#pragma unroll
		for (int v = 0; v < NV; ++v) {
			const int li = 4 * (lane + v * WAVE);
			if (a0 + li < e) lrStore<T>(rp[v], rv[v], sOff, sVal, li);
		}
		__builtin_amdgcn_wave_barrier();  // one wave: its LDS operations complete in order, no s_barrier
		// ---- 64 chains: lane l walks entries l, l + 64, ... of the segment; the gathers of a batch are issued before its multiply-adds ----
		const int h = b - a0, len = e - b;
		T dot = T(0);
		for (int j = lane; j < len; j += WAVE * LR_GATHER) {
			unsigned off[LR_GATHER];
			T xv[LR_GATHER], vv[LR_GATHER];
#pragma unroll
			for (int u = 0; u < LR_GATHER; ++u) {
				const bool ok = j + u * WAVE < len;
				off[u] = ok ? sOff[h + j + u * WAVE] : 0u;
				vv[u] = ok ? sVal[h + j + u * WAVE] : T(0);
			}
#pragma unroll
			for (int u = 0; u < LR_GATHER; ++u) xv[u] = patGather<T>(x, off[u]);
#pragma unroll
			for (int u = 0; u < LR_GATHER; ++u) {
				const T next = smmFma(vv[u], xv[u], dot);
				dot = j + u * WAVE < len ? next : dot;
			}
		}
		dot = groupSum<WAVE>(dot);
		if (lane == 0) segSums[seg] = dot;
	}
}

// ---- launch 2: the row kernel -------------------------------------------------------------------------------------------------------
// tiles[] holds {first row, start[first row]} per tile (nTiles + 1 entries, the last one {rows, nnz}); a tile of one row with more than
// splitLen entries is a long row, every other tile holds at most cap - 3 entries in at most TPB rows.
template <typename T>
__global__ __launch_bounds__(TPB) void spmvLongRowsKernel(int nTiles, int cap, int splitLen, const int2* __restrict__ tiles, int nLong, const int2* __restrict__ lrRows,
                                                          const T* __restrict__ segSums, const int* __restrict__ start, const int* __restrict__ positions,
                                                          const T* __restrict__ values, int nnz, int vecOk, int opFlags, const T* lhs,
                                                          const T* __restrict__ divisor, const T* __restrict__ x, T* out, int dotMode, const T* __restrict__ w1,
                                                          T* __restrict__ partials, const int* __restrict__ doneFlag) {
	using V = typename Pack16<T>::V;
	constexpr int NVMAX = LrCfg<T>::NVMAX;
	// LDS (sized by the host): sVal[cap + PAD] | sOff[cap + PAD] | sStart[TPB + 4] | red[4]
	T* sVal = reinterpret_cast<T*>(smmLrLds);
	unsigned* sOff = reinterpret_cast<unsigned*>(sVal + cap + LR_PAD);
	int* sStart = reinterpret_cast<int*>(sOff + cap + LR_PAD);
	T* red = reinterpret_cast<T*>(sStart + TPB + 4);
	if (doneFlag && *doneFlag) return;
	const int op = opFlags & 0xFF;
	const bool ntOut = (opFlags & SPMV_NT_OUT) != 0;
	const int t = threadIdx.x;
	const int lane = t & (WAVE - 1);
	const int nv = cap / LR_PIECE;
	T acc0 = T(0), acc1 = T(0);
	// every slot must always hold a valid byte offset: a batch may run past the end of its row (those products are discarded)
	for (int i = t; i < cap + LR_PAD; i += TPB) {
		sOff[i] = 0u;
		sVal[i] = T(0);
	}
	// XCD-aware work split, as in spmvStreamKernel: each of the 8 groups of workgroups (b, b + 8, ...) walks one contiguous eighth of the tiles
	const int nGroups = min(8, static_cast<int>(gridDim.x));
	const int xcdGroup = blockIdx.x % nGroups;
	const int groupSlots = (static_cast<int>(gridDim.x) - xcdGroup + nGroups - 1) / nGroups;
	const int chunkTiles = (nTiles + nGroups - 1) / nGroups;
	const int tileLo = min(nTiles, xcdGroup * chunkTiles), tileHi = min(nTiles, tileLo + chunkTiles);
	__syncthreads();  // LDS initialised
	for (int tile = tileLo + blockIdx.x / nGroups; tile < tileHi; tile += groupSlots) {
		const int2 m0 = tiles[tile], m1 = tiles[tile + 1];
		const int r0 = m0.x, n0 = m0.y, n1 = m1.y;
		const int nrows = m1.x - m0.x;
		const bool isLong = nrows == 1 && n1 - n0 > splitLen;
		const int a0 = n0 & ~3;
		if (!isLong) {
			// the tile's slices of positions[] / values[]: 16-byte coalesced non-temporal loads, straight on to LDS
			li32x4 rp[NVMAX];
			V rv[NVMAX][4 / Pack16<T>::N];
#pragma unroll
			for (int v = 0; v < NVMAX; ++v) {
				const int i = a0 + 4 * (t + v * TPB);
				if (v < nv && i < n1) {
					rp[v] = lrLoadPos(positions, i, nnz, vecOk & 1);
					lrLoadVal<T>(rv[v], values, i, nnz, vecOk & 2);
				}
			}
			const int ps = t < nrows ? start[r0 + t] : 0;
#pragma unroll
			for (int v = 0; v < NVMAX; ++v) {
				const int li = 4 * (t + v * TPB);
				if (v < nv && a0 + li < n1) lrStore<T>(rp[v], rv[v], sOff, sVal, li);
			}
			if (t < nrows) sStart[t] = ps - a0;
			if (t == 0) sStart[nrows] = n1 - a0;
		}
		ldsBarrier();  // the tile is in LDS
		if (isLong) {
			// wavefront 0 adds the row's segment sums in ascending order: 64 at a time, folded in lane order (every lane forms the same sum)
			if (t < WAVE) {
				int lo = 0, hi = nLong - 1;
				while (lo < hi) {  // the row's place in the long-row list
					const int mid = lo + (hi - lo) / 2;
					if (lrRows[mid].x >= r0) hi = mid;
					else lo = mid + 1;
				}
				const int first = lrRows[lo].y;
				const int nseg = lrRows[lo + 1].y - first;
				T dot = T(0);
				for (int k0 = 0; k0 < nseg; k0 += WAVE) {
					const T sv = k0 + lane < nseg ? segSums[first + k0 + lane] : T(0);
					const int cnt = min(WAVE, nseg - k0);
					for (int q = 0; q < cnt; ++q) dot = dot + lrReadLane(sv, q);
				}
				if (lane == 0) {
					const T o = patApplyOp(op, lhs, divisor, r0, dot);
					out[r0] = o;
					if (dotMode == 2) acc0 += o * o;
					if (dotMode) acc1 += o * w1[r0];
				}
			}
		} else {
			// ---- one lane per row out of LDS, left to right ----
			T dot = T(0);
			int kb = 0, ke = 0;
			if (t < nrows) {
				kb = sStart[t];
				ke = sStart[t + 1];
			}
			for (int k = kb; k < ke; k += LR_GATHER) {
				unsigned off[LR_GATHER];
				T xv[LR_GATHER], vv[LR_GATHER];
#pragma unroll
				for (int u = 0; u < LR_GATHER; ++u) {
					off[u] = sOff[k + u];
					vv[u] = sVal[k + u];
				}
#pragma unroll
				for (int u = 0; u < LR_GATHER; ++u) xv[u] = patGather<T>(x, off[u]);
				const int nvalid = ke - k;
#pragma unroll
				for (int u = 0; u < LR_GATHER; ++u) {
					const T next = smmFma(vv[u], xv[u], dot);
					dot = u < nvalid ? next : dot;
				}
			}
			if (t < nrows) {
				const int row = r0 + t;
				const T o = patApplyOp(op, lhs, divisor, row, dot);
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
// the analysis, on `s` (caller holds tileMutex); the handle is written last, and only on success.  Reads start[] only.
static int buildLongRowsLocked(smm_hip_csr* m, hipStream_t s) {
	SetupTrace trace("LONGROWS analysis");
	const int rows = m->rows;
	const int splitLen = m->lr_req_split ? m->lr_req_split : SMM_LONGROWS_SPLIT_DEFAULT;
	const int segLen = m->lr_req_seg ? m->lr_req_seg : SMM_LONGROWS_SEGMENT_DEFAULT;
	// the row kernel's tile: 256 average rows, at least one row of split_len entries, whole staging passes, within what a lane holds
	const int nvMax = m->dtype == SMM_DTYPE_F32 ? LrCfg<float>::NVMAX : LrCfg<double>::NVMAX;
	const double avg = rows > 0 ? static_cast<double>(m->nnz) / rows : 1.0;
	const double want = std::min(avg * TPB * 1.04 + 3, static_cast<double>(nvMax) * LR_PIECE);
	const int nv = std::max(1, std::min(nvMax, std::max(static_cast<int>((want + LR_PIECE - 1) / LR_PIECE), (splitLen + 3 + LR_PIECE - 1) / LR_PIECE)));
	const int cap = nv * LR_PIECE;
	const int capNnz = cap - 3;
	const size_t n1 = static_cast<size_t>(rows) + 1;
	DevBuf<int> isLong, segs, cutLen;
	SMM_TRY(isLong.alloc(n1));
	SMM_TRY(segs.alloc(n1));
	SMM_TRY(cutLen.alloc(n1));
	const int grid = static_cast<int>((n1 + 255) / 256);
	lrMarkKernel<<<grid, 256, 0, s>>>(rows, m->d_start, splitLen, segLen, capNnz, isLong, segs, cutLen);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(scanExclusive(isLong.p, isLong.p, n1, s));
	SMM_TRY(scanExclusive(segs.p, segs.p, n1, s));
	int nLong = 0, nSegs = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&nLong, isLong.p + rows, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(&nSegs, segs.p + rows, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	// a long row counts as max(len, capNnz + 1) entries in the cut: at most capNnz more than it holds
	const long long cutTotal = static_cast<long long>(m->nnz) + static_cast<long long>(nLong) * capNnz;
	if (cutTotal > INT_MAX) {
		setError("longrows SpMV: %d long rows in a matrix of %d entries overflow the tile cut's 32-bit row starts", nLong, m->nnz);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(scanExclusive(cutLen.p, cutLen.p, n1, s));
	DevBuf<int2> list;
	SMM_TRY(list.alloc(static_cast<size_t>(nLong) + 1));
	lrListKernel<<<grid, 256, 0, s>>>(rows, m->d_start, splitLen, isLong, segs, list);
	SMM_HIP_TRY(hipGetLastError());
	int cutNnz = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&cutNnz, cutLen.p + rows, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	int2* tiles = nullptr;
	int nTiles = 0;
	SMM_TRY(cutRows(cutLen, rows, cutNnz, capNnz, TPB, s, &tiles, &nTiles));
	lrTileStartKernel<<<(nTiles + 1 + 255) / 256, 256, 0, s>>>(nTiles + 1, tiles, m->d_start);
	const hipError_t le = hipGetLastError();
	const hipError_t se = le == hipSuccess ? hipStreamSynchronize(s) : le;  // published below: a launch on another stream may read the tables at once
	if (se != hipSuccess) {
		devFree(tiles);
		return hipFail(se, "longrows tile table", __FILE__, __LINE__);
	}
	// a replaced analysis: the old arrays go to the allocator's quarantine, so launches already enqueued with them stay valid
	devFree(m->d_lr_rows);
	devFree(m->d_lr_tiles);
	m->d_lr_rows = reinterpret_cast<int*>(list.detach());
	m->d_lr_tiles = reinterpret_cast<int*>(tiles);
	m->lr_split = splitLen;
	m->lr_seg = segLen;
	m->lr_long = nLong;
	m->lr_segments = nSegs;
	m->lr_n_tiles = nTiles;
	m->lr_cap = cap;
	m->lr_state.store(1, std::memory_order_release);
	return SMM_HIP_OK;
}

// smm_hip_csr_set_kernel(m, SMM_SPMV_LONGROWS, ...): the analysis if none is kept
int ensureLongRows(smm_hip_csr* m) {
	std::lock_guard<std::mutex> lock(m->tileMutex);
	if (m->lr_state.load(std::memory_order_acquire) == 1) return SMM_HIP_OK;
	SMM_HIP_TRY(hipDeviceSynchronize());  // set-up call without a stream: the matrix may still be being written on a caller's stream
	return buildLongRowsLocked(m, libStream());
}

const char* longRowsKernelDesc(const smm_hip_csr* m, long long* bytes) {
	const long long s = m->dtype == SMM_DTYPE_F32 ? 4 : 8;
	if (m->lr_state.load(std::memory_order_acquire) == 1) {
		std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(m)->tileMutex);
		*bytes += 2 * static_cast<long long>(m->lr_segments) * s + (static_cast<long long>(m->lr_long) + 1) * 8;
	}
	return "spmvLongRowsKernel";
}

void preloadLongRowsUnit() {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(lrMarkKernel));
	(void)hipGetLastError();
}

template <typename T, int NV>
static void launchSegments(int grid, size_t lds, int nLong, int nSegs, int segLen, const int2* lrRows, const smm_hip_csr* m, int vecOk, const T* x, T* segSums,
                           const int* doneFlag, hipStream_t s) {
	static std::atomic<int> granted{0};
	(void)ensureDynamicLds(granted, spmvLongSegmentsKernel<T, NV>, lds);  // (refused: the launch fails and launchSpmv reports it)
	spmvLongSegmentsKernel<T, NV><<<grid, TPB, lds, s>>>(nLong, nSegs, segLen, lrRows, m->d_start, m->d_positions, static_cast<const T*>(m->d_values), m->nnz, vecOk, x,
	                                                    segSums, doneFlag);
}

// the launches behind launchSpmv; `op` carries the flags
template <typename T>
int launchSpmvLongRows(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials, const int* doneFlag,
                       hipStream_t s) {
	// tileMutex is held until both launches are enqueued, as the STREAM branch of launchSpmv holds it: smm_hip_csr_longrows_configure replaces
	// the tables under the same lock and hands the old ones to the allocator's quarantine, which protects work that is ALREADY enqueued
	smm_hip_csr* mm = const_cast<smm_hip_csr*>(m);
	std::lock_guard<std::mutex> lock(mm->tileMutex);
	if (m->lr_state.load(std::memory_order_acquire) != 1) SMM_TRY(buildLongRowsLocked(mm, s));
	const int2* lrRows = reinterpret_cast<const int2*>(m->d_lr_rows);
	const int2* tiles = reinterpret_cast<const int2*>(m->d_lr_tiles);
	const int nLong = m->lr_long, nSegs = m->lr_segments, nTiles = m->lr_n_tiles, cap = m->lr_cap, splitLen = m->lr_split, segLen = m->lr_seg;
	const int vecOk = ((reinterpret_cast<uintptr_t>(m->d_positions) & 15u) == 0 ? 1 : 0) | ((reinterpret_cast<uintptr_t>(m->d_values) & 15u) == 0 ? 2 : 0);
	const int cus = (op & SPMV_LEAVE_ROOM) ? std::max(8, numCUs() - 8) : numCUs();
	// the segment sums belong to THIS call (two host threads, or two streams, may run SpMVs on one handle at once): taken from the
	// stream-ordered allocator and given back when the call returns -- the block is reusable only once the work enqueued here is done
	DevBuf<T> segSums;
	if (nSegs > 0) {
		SMM_TRY(segSums.alloc(static_cast<size_t>(nSegs)));
		const size_t lds = static_cast<size_t>(LR_WAVES) * (segLen + LR_SEG_SLACK) * (sizeof(T) + 4);
		const int perCU = std::max(1, std::min(8, static_cast<int>((160 * 1024) / lds)));
		const int grid = std::max(1, std::min((nSegs + LR_WAVES - 1) / LR_WAVES, cus * perCU));
		if (segLen <= 512) launchSegments<T, 3>(grid, lds, nLong, nSegs, segLen, lrRows, m, vecOk, x, segSums, doneFlag, s);
		else if (segLen <= 1024) launchSegments<T, 5>(grid, lds, nLong, nSegs, segLen, lrRows, m, vecOk, x, segSums, doneFlag, s);
		else launchSegments<T, 9>(grid, lds, nLong, nSegs, segLen, lrRows, m, vecOk, x, segSums, doneFlag, s);
		SMM_HIP_TRY(hipGetLastError());
	}
	const size_t lds = static_cast<size_t>(cap + LR_PAD) * (sizeof(T) + 4) + (TPB + 4) * sizeof(int) + 4 * sizeof(T) + 16;
	static std::atomic<long long> occ{0};
	int perCU = occupancyCached(occ, spmvLongRowsKernel<T>, TPB, lds, 4);
	if (forcedWgsPerCU() > 0) perCU = forcedWgsPerCU();
	const int grid = std::max(1, std::min(std::min(nTiles, cus * perCU), NPART));
	spmvLongRowsKernel<T><<<grid, TPB, lds, s>>>(nTiles, cap, splitLen, tiles, nLong, lrRows, segSums.p, m->d_start, m->d_positions, static_cast<const T*>(m->d_values),
	                                           m->nnz, vecOk, (op & ~(SPMV_LEAVE_ROOM | SPMV_HALF_TILES)) | spmvOutFlags(m, sizeof(T)), lhs, divisor, x, out, dotMode, w1,
	                                           partials, doneFlag);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template int launchSpmvLongRows<float>(const smm_hip_csr*, int, const float*, const float*, const float*, float*, int, const float*, float*, const int*, hipStream_t);
template int launchSpmvLongRows<double>(const smm_hip_csr*, int, const double*, const double*, const double*, double*, int, const double*, double*, const int*, hipStream_t);

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_longrows_configure(smm_hip_csr* m, int split_len, int segment_len) {
	if (!m) {
		setError("csr_longrows_configure: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (split_len != 0 && (split_len < SMM_LONGROWS_SPLIT_MIN || split_len > SMM_LONGROWS_SPLIT_MAX)) {
		setError("csr_longrows_configure: split_len must be 0 (the default, %d) or lie in %d .. %d, not %d", SMM_LONGROWS_SPLIT_DEFAULT, SMM_LONGROWS_SPLIT_MIN,
		         SMM_LONGROWS_SPLIT_MAX, split_len);
		return SMM_HIP_ERR_INVALID;
	}
	if (segment_len != 0 && (segment_len < SMM_LONGROWS_SEGMENT_MIN || segment_len > SMM_LONGROWS_SEGMENT_MAX || segment_len % 64 != 0)) {
		setError("csr_longrows_configure: segment_len must be 0 (the default, %d) or a multiple of 64 in %d .. %d, not %d", SMM_LONGROWS_SEGMENT_DEFAULT,
		         SMM_LONGROWS_SEGMENT_MIN, SMM_LONGROWS_SEGMENT_MAX, segment_len);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	std::lock_guard<std::mutex> lock(m->tileMutex);
	const int oldSplit = m->lr_req_split, oldSeg = m->lr_req_seg;
	m->lr_req_split = split_len;
	m->lr_req_seg = segment_len;
	if (m->lr_state.load(std::memory_order_acquire) != 1) return SMM_HIP_OK;  // kept for the analysis set_kernel runs
	// the kept analysis stays in force until the new one is complete (buildLongRowsLocked writes the handle last, and only on success; every
	// reader holds tileMutex); a failure leaves it and the earlier request in place
	hipError_t e = hipDeviceSynchronize();
	const int st = e == hipSuccess ? buildLongRowsLocked(m, libStream()) : hipFail(e, "hipDeviceSynchronize", __FILE__, __LINE__);
	if (st != SMM_HIP_OK) {
		m->lr_req_split = oldSplit;
		m->lr_req_seg = oldSeg;
	}
	return st;
}

int smm_hip_csr_longrows_info(const smm_hip_csr* m, int* split_len, int* segment_len, int* long_rows, long long* segments) {
	if (!m) {
		setError("csr_longrows_info: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(m)->tileMutex);
	const bool kept = m->lr_state.load(std::memory_order_acquire) == 1;
	if (split_len) *split_len = kept ? m->lr_split : 0;
	if (segment_len) *segment_len = kept ? m->lr_seg : 0;
	if (long_rows) *long_rows = kept ? m->lr_long : 0;
	if (segments) *segments = kept ? m->lr_segments : 0;
	return SMM_HIP_OK;
}

}  // extern "C"
