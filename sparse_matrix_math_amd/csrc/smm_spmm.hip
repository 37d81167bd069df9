// smm_spmm.hip -- CSR SpMM for gfx950: several right-hand sides at once.
//
//   out(i, j) = op(lhs(i, j), sum_e values[e] * x(positions[e], j))        j = 0 .. k-1,  1 <= k <= SMM_HIP_MAX_RHS
//
// A block of k vectors is one dense n x k array, row-major ("interleaved"): element (i, j) sits at i * k + j.  An addition with no
// counterpart in the reference (its rMult takes one vector, ref:1501-1515); column j of every result is what the single-vector entry
// point gives for column j alone (ref:1484-1490: a row's entries in stored order through _smm_fma).
//
// Why: an SpMV is bound by the matrix stream (values[] + positions[]: 8 / 12 bytes per stored entry against 2 flops).  k SpMVs stream it
// k times; here it is streamed ONCE and every entry is used k times, and with the vectors interleaved the gather of x for an entry is
// ONE load of K * sizeof(T) bytes from one cache line.
//
// Kernel (spmmTileKernel<T, K, G>, compile-time K in {1, 2, 4, 8}): the data path of the STREAM family (smm_spmv.hip) read through the
// SAME tile table (the handle's d_rowblocks, whatever cut the SpMV kernels asked for: a tile is <= 256 whole rows and <= cap stored
// entries).  Per tile: positions[] / values[] slices with 16-byte coalesced non-temporal loads -> LDS; then ONE LANE PER ROW walks its
// row out of LDS in batches of G entries -- G vector gathers in flight per lane (plain, cached loads), K accumulators in registers, the
// sum of every column strictly in stored order: the reference's bits whatever smm_hip_csr_set_kernel says.  A row longer than a tile
// (the table marks it: a tile of its own) is streamed straight from HBM by one wavefront, lanes striding over its entries and meeting in
// a butterfly: such rows are only held to the re-ordering bound.  k = 4 and k = 8 are one launch; other k are covered by column chunks
// of width 4 / 2 / 1 with row stride k, one launch each.
//
// The epilogue can form the solvers' dot products per column like launchSpmv's (dotMode 1: out(:,j).w(:,j); 2: also out(:,j).out(:,j)):
// column j's partial sums go to partials[j * 2 * NPART ...], laid out per column as launchSpmv lays out its single set.
#include <algorithm>
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"

namespace smm {

namespace {

constexpr int TPB = 256;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// K adjacent elements of one row of an interleaved block, loaded / stored as ONE vector access.  The alignment promised to the compiler
// is that of an element: a column chunk of a block with k = 3, 5, 6, 7 starts at any multiple of sizeof(T) (global accesses of gfx950
// need no more than dword alignment)
template <typename T, int K>
struct RowVec {
	typedef T Full __attribute__((ext_vector_type(K)));
	typedef Full V __attribute__((aligned(sizeof(T))));
};

template <typename T, int K>
__device__ __forceinline__ typename RowVec<T, K>::Full loadRow(const T* p) {
	return *reinterpret_cast<const typename RowVec<T, K>::V*>(p);
}
template <typename T, int K>
__device__ __forceinline__ void storeRow(T* p, typename RowVec<T, K>::Full v) {
	*reinterpret_cast<typename RowVec<T, K>::V*>(p) = v;
}

template <typename T>
struct SpmmCfg {
	static constexpr int PIECE = 4 * TPB;                  // entries staged per pass: one 16-byte load per lane and array
	static constexpr int NVMAX = sizeof(T) == 4 ? 7 : 5;   // passes of the largest tile the STREAM family cuts
	static constexpr int PAD = 16;                         // slack a gather batch may read past its row
	// the largest tile: three workgroups per CU (160 KiB of LDS), less the small arrays behind the tile -- the TILE kernel's budget
	static constexpr int CAP_MAX = ((160 * 1024) / 3 - 2048) / static_cast<int>(sizeof(T) + 4) - PAD;
};

// gathers in flight per lane: 64 registers' worth of x at most (fp64 K = 8: 4 x 64 bytes)
template <typename T, int K>
constexpr int gatherBatch() { return K * static_cast<int>(sizeof(T)) >= 64 ? 4 : 8; }

// waves per SIMD the register allocation is held to: 3 (the three workgroups per CU the LDS tile leaves room for: <= 168 VGPRs) wherever
// that costs no spill; rows of 32 bytes and more (fp32 K = 8, fp64 K = 4 / 8) hold 64 registers of gathered x beside their sums and the
// staging registers, and run at 2
template <typename T, int K>
constexpr int wavesPerSimd() { return K * static_cast<int>(sizeof(T)) >= 32 ? 2 : 3; }

extern __shared__ __attribute__((aligned(16))) unsigned char spmmDynLds[];

// out(row, :) = op(lhs(row, :), dot[:]) and the row's share of the fused dot products.  divisor is ONE vector for all columns (the Jacobi
// diagonal): the same division on the same operands as the single loop's folded apply (applyOp, smm_spmv.hip), so the same bits.
template <typename T, int K>
__device__ __forceinline__ void finishRow(int op, int row, int ld, const T* lhs, const T* __restrict__ divisor, T* out, const T (&dot)[K], int dotMode,
                                          const T* __restrict__ w1, T (&acc0)[K], T (&acc1)[K]) {
	typename RowVec<T, K>::Full o;
	const size_t at = static_cast<size_t>(row) * ld;
	if (op == SMM_OP_ASSIGN) {
#pragma unroll
		for (int j = 0; j < K; ++j) o[j] = dot[j];
	} else if (op == SPMV_OP_DIV) {
		const T d = divisor[row];
#pragma unroll
		for (int j = 0; j < K; ++j) o[j] = dot[j] / d;
	} else {
		const typename RowVec<T, K>::Full l = loadRow<T, K>(lhs + at);
		if (op == SMM_OP_ADD) {
#pragma unroll
			for (int j = 0; j < K; ++j) o[j] = l[j] + dot[j];
		} else if (op == SMM_OP_SUB) {
#pragma unroll
			for (int j = 0; j < K; ++j) o[j] = l[j] - dot[j];
		} else {  // SPMM_OP_SUB_DIV
			const T d = divisor[row];
#pragma unroll
			for (int j = 0; j < K; ++j) o[j] = (l[j] - dot[j]) / d;
		}
	}
	storeRow<T, K>(out + at, o);
	if (dotMode) {
		const typename RowVec<T, K>::Full w = loadRow<T, K>(w1 + at);
#pragma unroll
		for (int j = 0; j < K; ++j) {
			if (dotMode == 2) acc0[j] += o[j] * o[j];
			acc1[j] += o[j] * w[j];
		}
	}
}

// rowBlocks: {first row, start[first row]} per tile, nTiles + 1 entries closed by {rows, nnz} (cutRows, smm_spmv.hip); a tile holds at
// most TPB rows and, unless it is a single over-long row, at most cap - 3 entries.  lhs / x / out / w1 point at the first column of this
// launch's chunk; ld is the row stride (k) of all four.  partials: 2 * NPART elements per column of the chunk.
template <typename T, int K, int G>
__global__ __launch_bounds__(TPB, (wavesPerSimd<T, K>())) void spmmTileKernel(int nTiles, int cap, int chunkTiles, const int2* __restrict__ rowBlocks, const int* __restrict__ start,
                                                      const int* __restrict__ positions, const T* __restrict__ values, int op, const T* lhs,
                                                      const T* __restrict__ divisor, const T* __restrict__ x, T* out, int ld, int dotMode, const T* __restrict__ w1,
                                                      T* __restrict__ partials, const int* __restrict__ doneFlag) {
	using Cfg = SpmmCfg<T>;
	using XV = typename RowVec<T, K>::Full;
	static_assert(G <= Cfg::PAD, "a batch may read G - 1 slots past its row");
	constexpr int NVMAX = Cfg::NVMAX;
	// LDS (sized by the host): sVal[cap + PAD] | sCol[cap + PAD] | sStart[TPB + 4] | red[4]
	T* sVal = reinterpret_cast<T*>(spmmDynLds);
	int* sCol = reinterpret_cast<int*>(sVal + cap + Cfg::PAD);
	int* sStart = sCol + cap + Cfg::PAD;
	T* red = reinterpret_cast<T*>(sStart + TPB + 4);
	if (doneFlag && *doneFlag) return;

	const int t = threadIdx.x;
	const int lane = t & (WAVE - 1);
	const int nv = (cap + Cfg::PIECE - 1) / Cfg::PIECE;
	T acc0[K], acc1[K];
#pragma unroll
	for (int j = 0; j < K; ++j) acc0[j] = acc1[j] = T(0);
	// every slot must always hold a valid column: a batch may run past the end of its row (those products are discarded)
	for (int i = t; i < cap + Cfg::PAD; i += TPB) {
		sCol[i] = 0;
		sVal[i] = T(0);
	}
	// XCD-aware work split, as in spmvStreamKernel: workgroups b, b + 8, ... share an XCD and walk consecutive tiles of one chunk
	const int nGroups = min(8, static_cast<int>(gridDim.x));
	const int xcdGroup = blockIdx.x % nGroups;
	const int groupSlots = (static_cast<int>(gridDim.x) - xcdGroup + nGroups - 1) / nGroups;
	auto tileOf = [&](int j) {
		const int c = j / chunkTiles;
		const long long tIdx = (static_cast<long long>(c) * nGroups + xcdGroup) * chunkTiles + (j - c * chunkTiles);
		return tIdx < nTiles ? static_cast<int>(tIdx) : nTiles;
	};
	// a tile is staged in whole 16-byte pieces from its aligned start: those may run (cap + 3 at most) past the tile, never past the arrays
	const int stageLimit = (rowBlocks[nTiles].y & ~3) - (cap + 4);
	int j = blockIdx.x / nGroups;
	int tile = tileOf(j);
	int2 m0 = make_int2(0, 0), m1 = make_int2(0, 0);
	if (tile < nTiles) {
		m0 = rowBlocks[tile];
		m1 = rowBlocks[tile + 1];
	}
	__syncthreads();  // LDS initialised
	while (tile < nTiles) {
		const int r0 = m0.x, n0 = m0.y, r1 = m1.x, n1 = m1.y;
		const int nrows = r1 - r0;
		const int a0 = n0 & ~3;
		const bool direct = n1 - n0 > cap - 3 || a0 > stageLimit;
		if (!direct) {
			// the tile's slices of positions[] / values[]: 16-byte coalesced non-temporal loads, all issued before the first LDS store
			i32x4 rp[NVMAX];
			typename Pack16<T>::V rv[NVMAX * (sizeof(T) == 4 ? 1 : 2)];
#pragma unroll
			for (int v = 0; v < NVMAX; ++v) {
				const int i = a0 + 4 * (t + v * TPB);
				if (v < nv && i < n1) {
					rp[v] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(positions + i));
					if constexpr (sizeof(T) == 4) {
						rv[v] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(values + i));
					} else {
						rv[2 * v] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(values + i));
						rv[2 * v + 1] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(values + i + 2));
					}
				}
			}
			const int ps = t < nrows ? start[r0 + t] : 0;
#pragma unroll
			for (int v = 0; v < NVMAX; ++v) {
				const int li = 4 * (t + v * TPB);
				if (v < nv && a0 + li < n1) {
					*reinterpret_cast<i32x4*>(sCol + li) = rp[v];
					if constexpr (sizeof(T) == 4) {
						*reinterpret_cast<f32x4*>(sVal + li) = rv[v];
					} else {
						*reinterpret_cast<f64x2*>(sVal + li) = rv[2 * v];
						*reinterpret_cast<f64x2*>(sVal + li + 2) = rv[2 * v + 1];
					}
				}
			}
			if (t < nrows) sStart[t] = ps - a0;
			if (t == 0) sStart[nrows] = n1 - a0;
		}
		ldsBarrier();  // the tile is in LDS
		// descriptors of this workgroup's next tile (two short loads, in flight during the gathers)
		j += groupSlots;
		const int ntile = tileOf(j);
		int2 m0n = make_int2(0, 0), m1n = make_int2(0, 0);
		if (ntile < nTiles) {
			m0n = rowBlocks[ntile];
			m1n = rowBlocks[ntile + 1];
		}
		if (direct && nrows == 1 && n1 - n0 > cap - 3) {
			// an over-long row: wavefront 0 streams it straight from HBM, lanes striding over its entries; the 64 partial sums of every
			// column meet in a butterfly (re-ordered: such a row is held to the rounding bound of a re-ordered sum, not to the reference's bits)
			if (t < WAVE) {
				T dot[K];
#pragma unroll
				for (int c = 0; c < K; ++c) dot[c] = T(0);
				for (int e = n0 + lane; e < n1; e += WAVE) {
					const T v = values[e];
					const XV xv = loadRow<T, K>(x + static_cast<size_t>(positions[e]) * ld);
#pragma unroll
					for (int c = 0; c < K; ++c) dot[c] = smmFma(v, static_cast<T>(xv[c]), dot[c]);
				}
#pragma unroll
				for (int c = 0; c < K; ++c) dot[c] = groupSum<WAVE>(dot[c]);
				if (lane == 0) finishRow<T, K>(op, r0, ld, lhs, divisor, out, dot, dotMode, w1, acc0, acc1);
			}
		} else if (direct) {
			// one of the last tiles of the matrix (its 16-byte pieces could run past the arrays): one lane per row, in stored order, from HBM
			if (t < nrows) {
				const int row = r0 + t;
				const int e1 = start[row + 1];
				T dot[K];
#pragma unroll
				for (int c = 0; c < K; ++c) dot[c] = T(0);
				for (int e = start[row]; e < e1; ++e) {
					const T v = values[e];
					const XV xv = loadRow<T, K>(x + static_cast<size_t>(positions[e]) * ld);
#pragma unroll
					for (int c = 0; c < K; ++c) dot[c] = smmFma(v, static_cast<T>(xv[c]), dot[c]);
				}
				finishRow<T, K>(op, row, ld, lhs, divisor, out, dot, dotMode, w1, acc0, acc1);
			}
		} else if (t < nrows) {
			// ---- one lane per row out of LDS: batches of G entries, the G gathers all issued before the first multiply-add; every
			// column's sum stays strictly in stored order (ref:1484-1490) ----
			const int kb = sStart[t];
			const int ke = sStart[t + 1];
			T dot[K];
#pragma unroll
			for (int c = 0; c < K; ++c) dot[c] = T(0);
			for (int e = kb; e < ke; e += G) {
				int col[G];
				T vv[G];
				XV xv[G];
#pragma unroll
				for (int u = 0; u < G; ++u) {
					col[u] = sCol[e + u];
					vv[u] = sVal[e + u];
				}
#pragma unroll
				for (int u = 0; u < G; ++u) xv[u] = loadRow<T, K>(x + static_cast<size_t>(static_cast<unsigned>(col[u])) * ld);
				const int nvalid = ke - e;
#pragma unroll
				for (int u = 0; u < G; ++u) {
#pragma unroll
					for (int c = 0; c < K; ++c) {
						const T next = smmFma(vv[u], static_cast<T>(xv[u][c]), dot[c]);
						dot[c] = u < nvalid ? next : dot[c];
					}
				}
			}
			finishRow<T, K>(op, r0 + t, ld, lhs, divisor, out, dot, dotMode, w1, acc0, acc1);
		}
		ldsBarrier();  // every lane is done with the LDS copy of this tile
		tile = ntile;
		m0 = m0n;
		m1 = m1n;
	}
	if (dotMode) {
#pragma unroll
		for (int c = 0; c < K; ++c) {
			T* colParts = partials + static_cast<size_t>(c) * 2 * NPART;
			if (dotMode == 2) {
				const T s0 = blockSum256(acc0[c], red);
				if (t == 0) colParts[blockIdx.x] = s0;
			}
			const T s1 = blockSum256(acc1[c], red);
			if (t == 0) colParts[(dotMode == 2 ? NPART : 0) + blockIdx.x] = s1;
			// consumers always add NPART slots per quantity: clear the ones no workgroup of this (smaller) grid owns
			for (int i = gridDim.x + blockIdx.x * TPB + t; i < NPART; i += gridDim.x * TPB) {
				colParts[i] = T(0);
				if (dotMode == 2) colParts[NPART + i] = T(0);
			}
		}
	}
}

// what one launch needs of the handle's tile table, read under tileMutex
struct TileTable {
	const int2* blocks;
	int nTiles, cap, chunkTiles;
};

// The STREAM family's table as it is (any cut of at most TPB rows per tile serves the one-lane-per-row kernel); a matrix that has none yet
// -- no STREAM SpMV has run on it -- gets the cut of the one-lane-per-row TILE kernel: TPB typical rows, within the LDS of three workgroups
// per CU.  A later SpMV that wants another cut rebuilds the table (launchSpmv) and this file reads that one from then on.
template <typename T>
int tileTableFor(const smm_hip_csr* m, hipStream_t s, TileTable* tt) {
	smm_hip_csr* mm = const_cast<smm_hip_csr*>(m);
	std::lock_guard<std::mutex> lock(mm->tileMutex);
	if (!m->d_rowblocks || m->stream_max_rows > TPB || m->stream_nnz_cap + 3 > SpmmCfg<T>::CAP_MAX + 3) {
		const double avg = m->rows > 0 ? static_cast<double>(m->nnz) / m->rows : 1.0;
		const double len = std::max(avg, static_cast<double>(m->stream_mid_len));
		int cap = static_cast<int>(std::min(len * TPB + 8, static_cast<double>(SpmmCfg<T>::CAP_MAX)));
		cap = (std::max(256, cap) + 3) & ~3;
		SMM_TRY(buildRowBlocks(mm, cap - 3, TPB, s));
	}
	tt->blocks = reinterpret_cast<const int2*>(m->d_rowblocks);
	tt->nTiles = m->n_rowblocks;
	tt->cap = m->stream_nnz_cap + 3;
	tt->chunkTiles = m->stream_chunk_tiles;
	return SMM_HIP_OK;
}

template <typename T, int K>
int launchChunk(const smm_hip_csr* m, const TileTable& tt, int op, int ld, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1,
                T* partials, const int* doneFlag, hipStream_t s) {
	constexpr int G = gatherBatch<T, K>();
	const size_t lds = static_cast<size_t>(tt.cap + SpmmCfg<T>::PAD) * (sizeof(T) + 4) + (TPB + 4) * sizeof(int) + 4 * sizeof(T) + 32;
	static std::atomic<int> granted{0};
	static std::atomic<long long> occ{0};
	(void)ensureDynamicLds(granted, spmmTileKernel<T, K, G>, lds);  // (refused: the launch below fails and the caller reports it)
	int perCU = occupancyCached(occ, spmmTileKernel<T, K, G>, TPB, lds, 3);
	if (forcedWgsPerCU() > 0) perCU = forcedWgsPerCU();
	// persistent grid = the workgroups resident together; with fused dots every column still gets NPART partial slots (the rest are cleared)
	const int grid = std::max(1, std::min(std::min(tt.nTiles, numCUs() * perCU), NPART));
	const int nGroups = std::min(8, grid);
	const int chunkTiles = tt.chunkTiles > 0 ? tt.chunkTiles : std::max(1, (tt.nTiles + nGroups - 1) / nGroups);
	spmmTileKernel<T, K, G><<<grid, TPB, lds, s>>>(tt.nTiles, tt.cap, chunkTiles, tt.blocks, m->d_start, m->d_positions, static_cast<const T*>(m->d_values), op, lhs,
	                                             divisor, x, out, ld, dotMode, w1, partials, doneFlag);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

}  // namespace

template <typename T>
int launchSpmm(const smm_hip_csr* m, int op, int k, const T* lhs, const T* x, T* out, int dotMode, const T* w1, T* partials, const int* doneFlag,
               hipStream_t s, const T* divisor) {
	if (m->dtype != dtypeOf<T>()) {
		setError("spmm: matrix dtype does not match the _f32/_f64 entry point");
		return SMM_HIP_ERR_INVALID;
	}
	if (k < 1 || k > SMM_HIP_MAX_RHS) {
		setError("spmm: k = %d, must be 1 .. %d", k, SMM_HIP_MAX_RHS);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureCsrReady(m, s, true));
	const bool divides = op == SPMV_OP_DIV || op == SPMM_OP_SUB_DIV;
	if (!(op >= SMM_OP_ASSIGN && op <= SMM_OP_SUB) && !divides) {
		setError("spmm: bad op %d", op);
		return SMM_HIP_ERR_INVALID;
	}
	const bool readsLhs = op == SMM_OP_ADD || op == SMM_OP_SUB || op == SPMM_OP_SUB_DIV;
	if (m->rows > 0 && (!x || !out || (readsLhs && !lhs) || (divides && !divisor))) {
		setError("spmm: null array");
		return SMM_HIP_ERR_INVALID;
	}
	if (x == out && m->rows > 0) {  // assert(mult != res), ref:1503
		setError("spmm: x must not alias out");
		return SMM_HIP_ERR_INVALID;
	}
	if (dotMode < 0 || dotMode > 2 || (dotMode && (!w1 || !partials))) {
		setError("spmm: fused dots need w1 and partials");
		return SMM_HIP_ERR_INVALID;
	}
	if (m->rows == 0 && !dotMode) return SMM_HIP_OK;
	TileTable tt;
	SMM_TRY(tileTableFor<T>(m, s, &tt));
	int st = SMM_HIP_OK;
	// k = 8 and k = 4 are one launch; the rest is covered by column chunks of width 4 / 2 / 1 (row stride k)
	for (int c0 = 0; c0 < k && st == SMM_HIP_OK;) {
		const int left = k - c0;
		const int w = left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
		const T* l = lhs ? lhs + c0 : nullptr;
		const T* ww = w1 ? w1 + c0 : nullptr;
		T* pp = partials ? partials + static_cast<size_t>(c0) * 2 * NPART : nullptr;
		switch (w) {
		case 8: st = launchChunk<T, 8>(m, tt, op, k, l, divisor, x + c0, out + c0, dotMode, ww, pp, doneFlag, s); break;
		case 4: st = launchChunk<T, 4>(m, tt, op, k, l, divisor, x + c0, out + c0, dotMode, ww, pp, doneFlag, s); break;
		case 2: st = launchChunk<T, 2>(m, tt, op, k, l, divisor, x + c0, out + c0, dotMode, ww, pp, doneFlag, s); break;
		default: st = launchChunk<T, 1>(m, tt, op, k, l, divisor, x + c0, out + c0, dotMode, ww, pp, doneFlag, s); break;
		}
		c0 += w;
	}
	return st;
}

template int launchSpmm<float>(const smm_hip_csr*, int, int, const float*, const float*, float*, int, const float*, float*, const int*, hipStream_t, const float*);
template int launchSpmm<double>(const smm_hip_csr*, int, int, const double*, const double*, double*, int, const double*, double*, const int*, hipStream_t,
                                const double*);

namespace {

template <typename T>
int spmmCheck(const smm_hip_csr* m, int op, int k) {
	if (!m) {
		setError("spmm: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (op < SMM_OP_ASSIGN || op > SMM_OP_SUB) {
		setError("spmm: bad op %d", op);
		return SMM_HIP_ERR_INVALID;
	}
	if (k < 1 || k > SMM_HIP_MAX_RHS) {
		setError("spmm: k = %d, must be 1 .. %d", k, SMM_HIP_MAX_RHS);
		return SMM_HIP_ERR_INVALID;
	}
	if (m->dtype != dtypeOf<T>()) {
		setError("spmm: matrix dtype does not match the _f32/_f64 entry point");
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

// host-pointer entry: copy in, run, copy out (the calling convention of smm_hip_spmv_*)
template <typename T>
int spmmHost(const smm_hip_csr* m, int op, int k, const T* lhs, const T* x, T* out) {
	SMM_TRY(spmmCheck<T>(m, op, k));
	SMM_TRY(ensureInit());
	if (m->rows > 0 && (!x || !out || (op != SMM_OP_ASSIGN && !lhs))) {
		setError("spmm: null array");
		return SMM_HIP_ERR_INVALID;
	}
	if (m->rows > 0 && x == out) {
		setError("spmm: x must not alias out");
		return SMM_HIP_ERR_INVALID;
	}
	hipStream_t s = libStream();
	const size_t nx = static_cast<size_t>(m->cols) * k, no = static_cast<size_t>(m->rows) * k;
	DevBuf<T> dx, dl, dout;
	SMM_TRY(dx.alloc(nx));
	SMM_TRY(dout.alloc(no));
	if (nx) SMM_TRY(hostToDev(dx, x, sizeof(T) * nx, s));
	const T* dlhs = nullptr;
	if (op != SMM_OP_ASSIGN) {
		SMM_TRY(dl.alloc(no));
		if (no) SMM_TRY(hostToDev(dl, lhs, sizeof(T) * no, s));
		dlhs = dl;
	}
	SMM_TRY(launchSpmm<T>(m, op, k, dlhs, dx, dout, 0, nullptr, nullptr, nullptr, s));
	if (no) SMM_TRY(devToHost(out, dout, sizeof(T) * no, s));
	return SMM_HIP_OK;
}

template <typename T>
int spmmDev(const smm_hip_csr* m, int op, int k, const T* lhs, const T* x, T* out, smm_hip_stream stream) {
	SMM_TRY(spmmCheck<T>(m, op, k));
	SMM_TRY(ensureInit());
	return launchSpmm<T>(m, op, k, lhs, x, out, 0, nullptr, nullptr, nullptr, pickStream(stream));
}

}  // namespace

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_spmm_f32(const smm_hip_csr* m, int op, int k, const float* lhs, const float* x, float* out) { return spmmHost<float>(m, op, k, lhs, x, out); }
int smm_hip_spmm_f64(const smm_hip_csr* m, int op, int k, const double* lhs, const double* x, double* out) { return spmmHost<double>(m, op, k, lhs, x, out); }
int smm_hip_spmm_dev_f32(const smm_hip_csr* m, int op, int k, const float* d_lhs, const float* d_x, float* d_out, smm_hip_stream stream) {
	return spmmDev<float>(m, op, k, d_lhs, d_x, d_out, stream);
}
int smm_hip_spmm_dev_f64(const smm_hip_csr* m, int op, int k, const double* d_lhs, const double* d_x, double* d_out, smm_hip_stream stream) {
	return spmmDev<double>(m, op, k, d_lhs, d_x, d_out, stream);
}

}  // extern "C"
