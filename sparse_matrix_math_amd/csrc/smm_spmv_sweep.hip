// smm_spmv_sweep.hip -- the PATTERN family's SWEEP kernel: the slots kernel's copy and the slots kernel's bits, walked offset-major.
//
// The slots kernel (smm_spmv_slots.hip) finishes one 64-row wave before it starts the next, so an XCD's front passes every line of x once
// per offset, and two passes are far enough apart (the gap between two offsets, in rows) that the line has left the L2 in between.  Here a
// hardware wave keeps up to R consecutive 64-row waves of the matrix open at once, their accumulators in registers, and the OUTER loop runs
// over the offsets: step e of a super-block (all the rows the workgroups of one XCD hold open together) reads the window
// x[block + off[e]], step e + 1 the same window shifted by off[e + 1] - off[e], which the L2 still holds.  Nothing goes through memory
// between the steps and no row is cut: a row's products, their order and its pieces are the slots kernel's, hence the same bits.
//
// Per step and 64-row wave j, from wave-uniform quantities only: if bit e of the wave's mask is set, the entry is
// popcount(mask & ((1 << e) - 1)), its value slots[base_j + entry * 64 + lane], its column row + off[e]; a wave whose bit is clear issues
// no load and no multiply-add.  The entries of a piece are consecutive, so one piece per row is open at a time: acc[j] is the open piece,
// sum[j] the finished ones, added ((p0 + p1) + p2) + p3 when a piece closes.
#include <algorithm>

#include "smm_pattern_dev.h"

namespace smm {

constexpr int SWEEP_WAVES = TPB / WAVE;  // hardware waves per workgroup

// lane j's 64-bit value, held as two registers, as a wave-uniform number (v_readlane returns int: the low half must not sign-extend)
__device__ __forceinline__ unsigned long long sweepLane64(unsigned hi, unsigned lo, int j) {
	const unsigned h = __builtin_amdgcn_readlane(hi, j), l = __builtin_amdgcn_readlane(lo, j);
	return (static_cast<unsigned long long>(h) << 32) | l;
}

// R: 64-row waves a hardware wave holds open; the masks and slot bases of its R waves sit in lanes 0..R-1 of three registers and come out
// with v_readlane (3 R scalar registers would not fit beside the rest at R = 32)
template <typename T, int L, int R>
__global__ __launch_bounds__(TPB) void spmvPatternSweepKernel(int rows, int nWaves, int chunkWaves, const int* __restrict__ offs,
                                                              const long long* __restrict__ base, const unsigned long long* __restrict__ masks,
                                                              const T* __restrict__ slots, const int* __restrict__ start, const int* __restrict__ positions,
                                                              const T* __restrict__ values, int opFlags, const T* lhs, const T* __restrict__ divisor,
                                                              const T* __restrict__ x, T* out, int dotMode, const T* __restrict__ w1,
                                                              T* __restrict__ partials, const int* __restrict__ doneFlag) {
	static_assert(L == 2 || L == 4, "pieces per row");
	static_assert(R >= 1 && R <= 32, "rows of waves held open");
	constexpr int JB = R < 16 ? R : 16;  // waves whose loads are issued together, ahead of their multiply-adds
	static_assert(R % JB == 0, "whole batches");
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	const int op = opFlags & 0xFF;
	const bool ntOut = (opFlags & SPMV_NT_OUT) != 0;
	const int t = threadIdx.x;
	const unsigned lane = t & (WAVE - 1);
	const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
	const int nGroups = min(8, static_cast<int>(gridDim.x));
	const int xcdGroup = blockIdx.x % nGroups;
	const int groupWgs = (static_cast<int>(gridDim.x) - xcdGroup + nGroups - 1) / nGroups;
	const int hwWaves = groupWgs * SWEEP_WAVES;                                       // hardware waves of this XCD group
	const int hw = static_cast<int>(blockIdx.x / nGroups) * SWEEP_WAVES + wave;       // this one among them
	const int gBegin = min(nWaves, xcdGroup * chunkWaves), gEnd = min(nWaves, (xcdGroup + 1) * chunkWaves);
	// the group's eighth in equal super-blocks of at most hwWaves * R waves; inside one, hardware wave h owns `per` consecutive waves
	const int gWaves = gEnd - gBegin;
	const int nSuper = (gWaves + hwWaves * R - 1) / (hwWaves * R);
	const int superWaves = nSuper ? (gWaves + nSuper - 1) / nSuper : 0;
	const int per = (superWaves + hwWaves - 1) / hwWaves;  // <= R
	T acc0 = T(0), acc1 = T(0);
	for (int sb = 0; sb < nSuper; ++sb) {
		const int sBegin = gBegin + sb * superWaves, sEnd = min(gEnd, sBegin + superWaves);
		const int first = sBegin + hw * per;
		const int cnt = max(0, min(per, sEnd - first));
		if (cnt == 0) continue;
		// lane j < cnt: wave first + j's mask and block; a wave without a block (not uniform, or the last partial one) has mask 0 here
		long long bj = -1;
		unsigned long long mj = 0ULL;
		if (static_cast<int>(lane) < cnt) {
			bj = base[first + static_cast<int>(lane)];
			if (bj >= 0) mj = masks[static_cast<long long>(first + static_cast<int>(lane)) * WAVE];
		}
		const unsigned long long have = __builtin_amdgcn_ballot_w64(bj >= 0);
		// those waves first, row by row from CSR (the same pieces: the same bits)
		for (unsigned long long rest = ~have & ((1ULL << cnt) - 1ULL); rest; rest &= rest - 1ULL) {
			const int row = (first + __builtin_ctzll(rest)) * WAVE + static_cast<int>(lane);
			if (row < rows) {
				const T dot = patRowDirect<T, L>(start[row], start[row + 1], values, positions, x);
				const T o = patApplyOp(op, lhs, divisor, row, dot);
				storeOut(out + row, o, ntOut);
				if (dotMode == 2) acc0 += o * o;
				if (dotMode) acc1 += o * w1[row];
			}
		}
		if (have == 0ULL) continue;
		const int ref = __builtin_ctzll(have);
		const long long bRef = static_cast<long long>(sweepLane64(static_cast<unsigned>(bj >> 32), static_cast<unsigned>(bj), ref));
		const unsigned vLo = static_cast<unsigned>(mj), vHi = static_cast<unsigned>(mj >> 32);
		const int vRel = bj >= 0 ? static_cast<int>(bj - bRef) : 0;  // (< R * 64 * 64)
		unsigned long long todo = 0ULL;                              // the offsets any of the waves holds
		for (unsigned long long h = have; h; h &= h - 1ULL) {
			const int j = __builtin_ctzll(h);
			todo |= sweepLane64(vHi, vLo, j);
		}
		const T* const sv = slots + bRef;
		const int row0 = first * WAVE;
		T acc[R], sum[R];
#pragma unroll
		for (int j = 0; j < R; ++j) acc[j] = sum[j] = T(0);
		// The common block: every wave has a block and they all hold the same offsets.  Entry, piece and column are then the same for the
		// whole step, and the waves' blocks follow each other at len x 64 elements (slotsBuild lays the blocks of consecutive waves end to
		// end, without padding): a value load, a gather and a multiply-add per wave.  All of a step's loads are issued before its
		// multiply-adds; R is the batch.
		const unsigned long long lead0 = sweepLane64(vHi, vLo, 0);
		if (have == (1ULL << cnt) - 1ULL && __builtin_amdgcn_ballot_w64(static_cast<int>(lane) < cnt && mj != lead0) == 0ULL) {
			const int len = __builtin_popcountll(lead0);
			const int pl = (len + L - 1) / L;
			const unsigned stride = static_cast<unsigned>(len) * WAVE;
			int done = 0;
			for (todo = lead0; todo; todo &= todo - 1ULL) {
				const T* const ve = sv + static_cast<unsigned>(done) * WAVE;
				const T* const xe = x + (row0 + offs[__builtin_ctzll(todo)]);
				T vv[R], xv[R];
#pragma unroll
				for (int j = 0; j < R; ++j) {
					if (j < cnt) {
						vv[j] = __builtin_nontemporal_load(ve + j * stride + lane);
						xv[j] = xe[j * WAVE + lane];
					}
				}
#pragma unroll
				for (int j = 0; j < R; ++j) {
					if (j < cnt) acc[j] = smmFma(vv[j], xv[j], acc[j]);
				}
				++done;
				if (done == len || done == pl || (L == 4 && (done == 2 * pl || done == 3 * pl))) {
#pragma unroll
					for (int j = 0; j < R; ++j) {
						sum[j] = done <= pl ? acc[j] : sum[j] + acc[j];
						acc[j] = T(0);
					}
				}
			}
		}
		for (; todo; todo &= todo - 1ULL) {
			const int e = __builtin_ctzll(todo);
			const unsigned long long below = (1ULL << e) - 1ULL;
			const int off = offs[e];
#pragma unroll
			for (int jb = 0; jb < R; jb += JB) {
				T vv[JB], xv[JB];
#pragma unroll
				for (int u = 0; u < JB; ++u) {
					const int j = jb + u;
					const unsigned long long lead = sweepLane64(vHi, vLo, j);
					if ((lead >> e) & 1ULL) {
						const int entry = __builtin_popcountll(lead & below);
						const int rel = __builtin_amdgcn_readlane(vRel, j) + entry * WAVE;
						vv[u] = __builtin_nontemporal_load(sv + rel + lane);
						xv[u] = x[static_cast<long long>(row0 + j * WAVE + off) + lane];
					}
				}
#pragma unroll
				for (int u = 0; u < JB; ++u) {
					const int j = jb + u;
					const unsigned long long lead = sweepLane64(vHi, vLo, j);
					if ((lead >> e) & 1ULL) {
						acc[j] = smmFma(vv[u], xv[u], acc[j]);
						const int done = __builtin_popcountll(lead & below) + 1;  // entries of the row so far
						const int len = __builtin_popcountll(lead);
						const int pl = (len + L - 1) / L;
						const bool closes = done == len || done == pl || (L == 4 && (done == 2 * pl || done == 3 * pl));
						if (closes) {
							sum[j] = done <= pl ? acc[j] : sum[j] + acc[j];
							acc[j] = T(0);
						}
					}
				}
			}
		}
#pragma unroll
		for (int j = 0; j < R; ++j) {
			if ((have >> j) & 1ULL) {
				const int row = row0 + j * WAVE + static_cast<int>(lane);  // (a wave with a block is whole: row < rows)
				const T o = patApplyOp(op, lhs, divisor, row, sum[j]);
				storeOut(out + row, o, ntOut);
				if (dotMode == 2) acc0 += o * o;
				if (dotMode) acc1 += o * w1[row];
			}
		}
	}
	if (dotMode) {
		if (dotMode == 2) {
			const T s0 = blockSum256(acc0, red);
			if (t == 0) partials[blockIdx.x] = s0;
		}
		const T s1 = blockSum256(acc1, red);
		if (t == 0) partials[(dotMode == 2 ? NPART : 0) + blockIdx.x] = s1;
		for (int i = gridDim.x + blockIdx.x * TPB + t; i < NPART; i += gridDim.x * TPB) {
			partials[i] = T(0);
			if (dotMode == 2) partials[NPART + i] = T(0);
		}
		if (opFlags & SPMV_FINISH) lastBlockSums<T>(partials, NPART, dotMode == 2 ? 2 : 1, partials + PARTS_TOTALS, partsTicket(partials));
	}
}

// workgroups per CU: as many as fit, up to three (r09: one wave per SIMD does not hide the latency of its own loads -- 611 us per launch
// on the benchmark matrix at R = 16, 445 with two, 430 with three); the block of rows an XCD holds open is 32 CUs x that x 4 waves x R x 64
// rows.  SMM_HIP_PATTERN_SWEEP_WGS=1..8 for lab runs.
static int sweepWgsPerCU() { return std::max(1, std::min(8, env::intOr(env::PATTERN_SWEEP_WGS, 3))); }

// workgroups per CU the launch of one variant really gets: the knob, or fewer where the variant's registers allow fewer
template <typename T, int L, int R>
static int sweepWgsOf() {
	static std::atomic<long long> occ{0};
	return std::max(1, std::min(sweepWgsPerCU(), occupancyCached(occ, spmvPatternSweepKernel<T, L, R>, TPB, 0, 1)));
}

template <typename T, int L>
static int sweepWgsOfR(int rowsOpen) {
	return rowsOpen == 8 ? sweepWgsOf<T, L, 8>() : rowsOpen == 16 ? sweepWgsOf<T, L, 16>() : sweepWgsOf<T, L, 32>();
}

int patternSweepGroupWaves(const smm_hip_csr* m, int lanes, int rowsOpen) {
	const int wgs = m->dtype == SMM_DTYPE_F32 ? (lanes == 2 ? sweepWgsOfR<float, 2>(rowsOpen) : sweepWgsOfR<float, 4>(rowsOpen))
	                                          : (lanes == 2 ? sweepWgsOfR<double, 2>(rowsOpen) : sweepWgsOfR<double, 4>(rowsOpen));
	return ((numCUs() * wgs + 7) / 8) * SWEEP_WAVES * rowsOpen;
}

template <typename T, int L, int R>
static void launchSweepR(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials,
                         const int* doneFlag, hipStream_t s) {
	const int perCU = sweepWgsOf<T, L, R>();
	const int cus = (op & SPMV_LEAVE_ROOM) ? std::max(8, numCUs() - 8) : numCUs();
	const int nWaves = m->pat_slots_waves;
	const int grid = std::max(1, std::min(std::min((nWaves + SWEEP_WAVES - 1) / SWEEP_WAVES, cus * perCU), NPART));
	const int nGroups = std::min(8, grid);
	const int chunkWaves = (nWaves + nGroups - 1) / nGroups;
	spmvPatternSweepKernel<T, L, R><<<grid, TPB, 0, s>>>(m->rows, nWaves, chunkWaves, m->d_pat_off, m->d_pat_slot_base, m->d_pat_masks,
	                                                    static_cast<const T*>(m->d_pat_slots), m->d_start, m->d_positions, static_cast<const T*>(m->d_values),
	                                                    (op & ~SPMV_LEAVE_ROOM) | spmvOutFlags(m, sizeof(T)), lhs, divisor, x, out, dotMode, w1, partials,
	                                                    doneFlag);
}

template <typename T, int L>
static void launchSweepL(const smm_hip_csr* m, int rowsOpen, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1,
                         T* partials, const int* doneFlag, hipStream_t s) {
	switch (rowsOpen) {
	case 8: launchSweepR<T, L, 8>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	case 16: launchSweepR<T, L, 16>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	default: launchSweepR<T, L, 32>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	}
}

template <typename T>
void launchPatSweep(const smm_hip_csr* m, int lanes, int rowsOpen, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1,
                    T* partials, const int* doneFlag, hipStream_t s) {
	if (lanes == 2) {
		launchSweepL<T, 2>(m, rowsOpen, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	} else {
		launchSweepL<T, 4>(m, rowsOpen, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	}
}

template void launchPatSweep<float>(const smm_hip_csr*, int, int, int, const float*, const float*, const float*, float*, int, const float*, float*,
                                    const int*, hipStream_t);
template void launchPatSweep<double>(const smm_hip_csr*, int, int, int, const double*, const double*, const double*, double*, int, const double*, double*,
                                     const int*, hipStream_t);

}  // namespace smm
