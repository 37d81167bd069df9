// smm_spmv_slots.hip -- the PATTERN family's SLOTS kernel: the MASKS encoding with values read, 2 or 4 lanes per row, without the tile
// kernel's LDS value stage.
//
// In a UNIFORM wave -- 64 consecutive rows that all hold the same offsets, i.e. everywhere in a band except where a diagonal enters or
// leaves the matrix -- entry e of every row is the same offset.  The values of such a wave are copied once per matrix into a block of
// popcount(mask) x 64 elements, slot-major ([e][lane]): slot e of the wave is one 256-byte (fp32) load straight into registers, and the
// column is x + row + off[e] with a wave-uniform offset.  No start[], no per-row mask, no LDS, no barrier on that path.  Waves that are not
// uniform (and the last, partial wave) keep a base of -1 and read their rows from CSR with patRowDirect.
//
// Bits: a lane sums its row in the tile kernel's L pieces (ceil(len / L) consecutive entries each, left to right, one accumulator per
// piece) and adds them ((p0 + p1) + p2) + p3 -- the products and the order of spmvPatternTileKernel<T, L, G> and of patRowDirect: the same
// bits.  The L accumulators are independent chains (instruction-level parallelism without any cross-lane step).
#include <algorithm>

#include "smm_csr_build.h"
#include "smm_pattern_dev.h"

namespace smm {

constexpr int SLOT_WAVES = TPB / WAVE;  // waves per workgroup

// the sweep kernel under AUTO (DESIGN 3.1 has the measurements these stand on)
constexpr int SWEEP_ROWS_DEFAULT = 16;  // (r09, benchmark matrix: 8 / 16 / 32 -> 439 / 430 / 541 us per launch; 32 leaves two waves per SIMD)
constexpr int SWEEP_MIN_BLOCKS = 3;  // (10 M rows: 3.2 blocks per XCD group, 427 against 479 us; 4 M rows: 1.3 blocks, 240 against 197)
constexpr long long SWEEP_FRONT_REACH = 16384;  // rows between two touches of an x line that a row-major front's L2 still bridges
constexpr double SWEEP_MIN_RATIO = 1.5;         // modelled x fetches, front over sweep, from which the sweep is taken

// per wave: the elements of its block (popcount of the shared mask x 64 lanes) if the wave is uniform and whole, else 0; uniform waves counted
__global__ __launch_bounds__(TPB) void slotsCountKernel(int rows, int nWaves, const unsigned long long* __restrict__ masks, long long* __restrict__ counts,
                                                        int* __restrict__ uniformWaves) {
	const int lane = threadIdx.x & (WAVE - 1);
	int mine = 0;
	for (int w = (blockIdx.x * TPB + threadIdx.x) / WAVE; w < nWaves; w += gridDim.x * SLOT_WAVES) {
		const int row = w * WAVE + lane;
		const unsigned long long mm = row < rows ? masks[row] : ~0ULL;
		const unsigned long long lead = patUniform64(mm);
		const bool uniform = lead != 0ULL && __builtin_amdgcn_ballot_w64(!(row < rows && mm == lead)) == 0ULL;
		if (lane == 0) {
			counts[w] = uniform ? static_cast<long long>(__builtin_popcountll(lead)) * WAVE : 0;
			mine += uniform;
		}
	}
	if (lane == 0 && mine) atomicAdd(uniformWaves, mine);
}

// after the scan: the waves without a block get -1
__global__ __launch_bounds__(TPB) void slotsMarkKernel(int nWaves, const long long* __restrict__ counts, long long* __restrict__ base) {
	for (int w = blockIdx.x * TPB + threadIdx.x; w < nWaves; w += gridDim.x * TPB) {
		if (counts[w] == 0) base[w] = -1;
	}
}

// the copy (at build and after every edit of values[]): lane l of wave w moves row 64 w + l's entries to slots[base + e * 64 + l]
template <typename T>
__global__ __launch_bounds__(TPB) void slotsFillKernel(int nWaves, const long long* __restrict__ base, const unsigned long long* __restrict__ masks,
                                                       const int* __restrict__ start, const T* __restrict__ values, T* __restrict__ slots) {
	const int lane = threadIdx.x & (WAVE - 1);
	for (int w = (blockIdx.x * TPB + threadIdx.x) / WAVE; w < nWaves; w += gridDim.x * SLOT_WAVES) {
		const long long b = base[w];
		if (b < 0) continue;
		const int row = w * WAVE + lane;
		const int len = __builtin_popcountll(masks[w * WAVE]);
		const T* src = values + start[row];
		T* dst = slots + b + lane;
		for (int e = 0; e < len; ++e) dst[static_cast<long long>(e) * WAVE] = src[e];
	}
}

// One lane per row, 64 rows per wave, a persistent grid.  The waves of the matrix are dealt to the XCD groups (workgroup i runs on XCD
// i % 8) in contiguous eighths, so that the x lines of a stretch of rows stay in one XCD's L2; inside a group the workgroups take the
// group's waves in turn, four adjacent waves per workgroup at a time.  G: slots per piece and batch (all L pieces' values and gathers of a
// batch are issued before its multiply-adds).
template <typename T, int L, int G>
__global__ __launch_bounds__(TPB) void spmvPatternSlotsKernel(int rows, int nWaves, int chunkWaves, const int* __restrict__ offs,
                                                              const long long* __restrict__ base, const unsigned long long* __restrict__ masks,
                                                              const T* __restrict__ slots, const int* __restrict__ start, const int* __restrict__ positions,
                                                              const T* __restrict__ values, int opFlags, const T* lhs, const T* __restrict__ divisor,
                                                              const T* __restrict__ x, T* out, int dotMode, const T* __restrict__ w1,
                                                              T* __restrict__ partials, const int* __restrict__ doneFlag) {
	static_assert(L == 2 || L == 4, "pieces per row");
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	const int op = opFlags & 0xFF;
	const bool ntOut = (opFlags & SPMV_NT_OUT) != 0;
	const int t = threadIdx.x;
	const int lane = t & (WAVE - 1);
	const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
	const int nGroups = min(8, static_cast<int>(gridDim.x));
	const int xcdGroup = blockIdx.x % nGroups;
	const int groupSlots = (static_cast<int>(gridDim.x) - xcdGroup + nGroups - 1) / nGroups;
	const int wEnd = min(nWaves, (xcdGroup + 1) * chunkWaves);
	T acc0 = T(0), acc1 = T(0);
	for (int w = xcdGroup * chunkWaves + static_cast<int>(blockIdx.x / nGroups) * SLOT_WAVES + wave; w < wEnd; w += groupSlots * SLOT_WAVES) {
		const int row = w * WAVE + lane;
		const long long b = base[w];
		T dot = T(0);
		if (b >= 0) {
			const unsigned long long lead = masks[w * WAVE];
			const int len = __builtin_popcountll(lead);
			const int pl = (len + L - 1) / L;
			// lane u holds the offset of entry u (a row has at most 64 entries); an entry's offset comes out with v_readlane
			const int offLane = offs[lane < len ? selectBit(lead, lane) : 0];
			const T* const xr = x + row;
			const T* const sv = slots + b + lane;
			T part[L];
#pragma unroll
			for (int q = 0; q < L; ++q) part[q] = T(0);
			for (int i = 0; i < pl; i += G) {
				T vv[L][G], xv[L][G];
#pragma unroll
				for (int q = 0; q < L; ++q) {
#pragma unroll
					for (int u = 0; u < G; ++u) {
						// slots past the piece or the row repeat the row's last one (a valid load); their products are discarded below
						const int e = min(q * pl + i + u, len - 1);
						vv[q][u] = __builtin_nontemporal_load(sv + static_cast<long long>(e) * WAVE);
						xv[q][u] = xr[__builtin_amdgcn_readlane(offLane, e)];
					}
				}
#pragma unroll
				for (int q = 0; q < L; ++q) {
#pragma unroll
					for (int u = 0; u < G; ++u) {
						if (i + u < pl && q * pl + i + u < len) part[q] = smmFma(vv[q][u], xv[q][u], part[q]);
					}
				}
			}
			dot = part[0];
#pragma unroll
			for (int q = 1; q < L; ++q) dot += part[q];
		} else if (row < rows) {
			dot = patRowDirect<T, L>(start[row], start[row + 1], values, positions, x);  // (the same pieces: the same bits)
		}
		if (row < rows) {
			const T o = patApplyOp(op, lhs, divisor, row, dot);
			storeOut(out + row, o, ntOut);
			if (dotMode == 2) acc0 += o * o;
			if (dotMode) acc1 += o * w1[row];
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

// ---- selection ----------------------------------------------------------------------------------------------------------------------
// SMM_HIP_PATTERN_SLOTS=0: never; =1: wherever it applies (also on a kernel set with smm_hip_csr_set_kernel, whatever the share of uniform
// waves); =3: the same, walked by the sweep kernel (smm_spmv_sweep.hip); unset: AUTO.  A handle's own smm_hip_csr_pattern_slots mode wins
// over the variable.
static int slotsEnvMode() {
	if (!env::isSet(env::PATTERN_SLOTS)) return -1;
	const int mode = env::intOr(env::PATTERN_SLOTS, 0);
	return mode == 3 ? 3 : mode != 0 ? 1 : 0;
}

static int slotsMode(const smm_hip_csr* m) { return m->pat_slots_mode >= 0 ? m->pat_slots_mode : slotsEnvMode(); }

// the kernel applies: the MASKS encoding with values read, 2 or 4 lanes per row, the tile kernel's uniform fast path not switched off
static bool slotsApplies(const smm_hip_csr* m, int lanes) {
	if (lanes != 2 && lanes != 4) return false;
	if (m->pat_encoding != 0 || (m->pat_const && !m->pat_const_off)) return false;
	return env::flagOr(env::FULL_ROWS, true) && env::intOr(env::PATTERN_VARIANT, -1) != 0;
}

// AUTO: only where the family was adopted by the library itself, and only with >= 99 % uniform waves
static bool slotsWanted(const smm_hip_csr* m, int lanes, bool* forced) {
	const int mode = slotsMode(m);
	*forced = mode == 1 || mode == 3;
	if (mode == 0 || !slotsApplies(m, lanes)) return false;
	return mode >= 1 || !m->kernelForced;
}

static bool slotsUniformEnough(const smm_hip_csr* m) {
	return static_cast<long long>(m->pat_slots_uniform) * 100 >= static_cast<long long>(m->pat_slots_waves) * 99;
}

bool patternSlotsChosen(const smm_hip_csr* m, int lanes) {
	bool forced = false;
	if (!slotsWanted(m, lanes, &forced) || m->pat_slots_state != 1 || !m->d_pat_slots) return false;
	return forced || slotsUniformEnough(m);
}

// ---- the sweep kernel (smm_spmv_sweep.hip) on the same copy ------------------------------------------------------------------------
// 64-row waves a hardware wave holds open: SMM_HIP_PATTERN_SWEEP_ROWS=8|16|32 for lab runs, smm_hip_set_pattern_sweep_rows for the tests
static std::atomic<int> g_sweepRows{0};

static int sweepRowsOpen() {
	if (const int forced = g_sweepRows.load(std::memory_order_relaxed)) return forced;
	const int r = env::intOr(env::PATTERN_SWEEP_ROWS, 0);
	return r == 8 || r == 16 || r == 32 ? r : SWEEP_ROWS_DEFAULT;
}

// x lines fetched per line of x, from the sorted offsets: a row-major front re-fetches a line at every gap between two
// offsets that its L2 cannot bridge (SWEEP_FRONT_REACH rows); the sweep of blocks of B rows fetches min(gap, B) / B of its window again
static bool sweepSpanWins(const smm_hip_csr* m, long long blockRows) {
	const std::vector<int>& offs = m->pat_offs_host;
	double front = 1.0, sweep = 1.0;
	for (size_t i = 1; i < offs.size(); ++i) {
		const long long gap = static_cast<long long>(offs[i]) - offs[i - 1];
		if (gap > SWEEP_FRONT_REACH) front += 1.0;
		sweep += static_cast<double>(std::min(gap, blockRows)) / static_cast<double>(blockRows);
	}
	return sweep * SWEEP_MIN_RATIO <= front;
}

// 0: the slots kernel; else the sweep kernel with that many waves open.  Mode 3 takes it wherever the slots kernel runs; AUTO (and mode 2)
// only where it was measured to win (profiles/r09/span_and_size.txt): fp32, an XCD group with at least SWEEP_MIN_BLOCKS full super-blocks,
// and offsets that span more than a row-major front keeps in its L2.
int patternSweepRows(const smm_hip_csr* m, int lanes) {
	const int mode = slotsMode(m);
	const int r = sweepRowsOpen();
	if (mode == 3) return r;
	if (mode == 1 || mode == 0) return 0;
	if (m->dtype != SMM_DTYPE_F32) return 0;  // (fp64 at 10 M rows: 1018 us against the slots kernel's 986 -- two waves per SIMD)
	const long long groupWaves = patternSweepGroupWaves(m, lanes, r);  // (at the workgroups per CU the launch will get)
	if (m->pat_slots_waves / 8 < SWEEP_MIN_BLOCKS * groupWaves) return 0;
	return sweepSpanWins(m, groupWaves * WAVE) ? r : 0;
}

template <typename T>
static int slotsFill(smm_hip_csr* m, hipStream_t s) {
	const int nWaves = m->pat_slots_waves;
	const int grid = std::max(1, std::min(4096, (nWaves + SLOT_WAVES - 1) / SLOT_WAVES));
	slotsFillKernel<T><<<grid, TPB, 0, s>>>(nWaves, m->d_pat_slot_base, m->d_pat_masks, m->d_start, static_cast<const T*>(m->d_values),
	                                         static_cast<T*>(m->d_pat_slots));
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// Layout: base[] is the plain inclusive scan of the counts, so the blocks of consecutive uniform waves lie end to end, popcount x 64
// elements apart, without padding -- the sweep kernel's uniform path (smm_spmv_sweep.hip) steps from one wave's block to the next by that
// distance.  A layout that pads or reorders the blocks has to change that path with it.
// the per-wave header (counts, scan, marks) and, when the kernel is to be used, the copy; published only after the stream has finished
// (a launch on another stream may read it at once), like d_res_ell (smm_resident_bicg.hip)
template <typename T>
static int slotsBuild(smm_hip_csr* m, bool forced, hipStream_t s) {
	SetupTrace trace("pattern: slots copy");
	const int nWaves = (m->rows + WAVE - 1) / WAVE;
	DevBuf<long long> counts, base;
	DevBuf<int> uniform;
	SMM_TRY(counts.alloc(nWaves));
	SMM_TRY(base.alloc(static_cast<size_t>(nWaves) + 1));
	SMM_TRY(uniform.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(uniform.p, 0, sizeof(int), s));
	SMM_HIP_TRY(hipMemsetAsync(base.p, 0, sizeof(long long), s));
	const int grid = std::max(1, std::min(4096, (nWaves + SLOT_WAVES - 1) / SLOT_WAVES));
	slotsCountKernel<<<grid, TPB, 0, s>>>(m->rows, nWaves, m->d_pat_masks, counts.p, uniform.p);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(scanInclusive(counts.p, base.p + 1, static_cast<size_t>(nWaves), s));
	slotsMarkKernel<<<std::max(1, std::min(4096, (nWaves + TPB - 1) / TPB)), TPB, 0, s>>>(nWaves, counts.p, base.p);
	SMM_HIP_TRY(hipGetLastError());
	long long total = 0;
	int nUniform = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&total, base.p + nWaves, sizeof(total), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(&nUniform, uniform.p, sizeof(nUniform), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	m->pat_slots_waves = nWaves;
	m->pat_slots_uniform = nUniform;
	m->pat_slots_elems = total;
	if (!forced && !slotsUniformEnough(m)) return SMM_HIP_ERR_INVALID;
	// the copy is about nnz * sizeof(T): only with room to spare (1 GiB, or 1/16 of the device, whichever is more)
	const size_t bytes = static_cast<size_t>(std::max(1LL, total)) * sizeof(T);
	size_t freeB = 0, totalB = 0;
	SMM_HIP_TRY(hipMemGetInfo(&freeB, &totalB));
	if (freeB < bytes + std::max<size_t>(size_t(1) << 30, totalB / 16)) return SMM_HIP_ERR_INVALID;
	void* p = nullptr;
	SMM_TRY(devAlloc(&p, bytes));
	m->d_pat_slots = p;
	m->d_pat_slot_base = base.detach();
	int st = slotsFill<T>(m, s);
	hipError_t e = st == SMM_HIP_OK ? hipStreamSynchronize(s) : hipSuccess;
	if (st != SMM_HIP_OK || e != hipSuccess) {
		devFree(m->d_pat_slots);
		devFree(m->d_pat_slot_base);
		m->d_pat_slots = nullptr;
		m->d_pat_slot_base = nullptr;
		return st != SMM_HIP_OK ? st : hipFail(e, "slotsFillKernel", __FILE__, __LINE__);
	}
	return SMM_HIP_OK;
}

// Any failure (too few uniform waves under AUTO, no memory, a HIP error) leaves the matrix on the tile kernel: the copy is an optimisation,
// the launch would have run fine without it.  A refusal under AUTO is kept (state -1); a forced handle tries again when it has no copy.
bool ensurePatternSlots(smm_hip_csr* m, int lanes, hipStream_t s) {
	bool forced = false;
	if (!slotsWanted(m, lanes, &forced)) return false;
	if (m->pat_slots_state == 1 && m->d_pat_slots) return forced || slotsUniformEnough(m);
	if (m->pat_slots_state < 0 && !forced) return false;
	const int st = m->dtype == SMM_DTYPE_F32 ? slotsBuild<float>(m, forced, s) : slotsBuild<double>(m, forced, s);
	if (st != SMM_HIP_OK) {
		m->pat_slots_state = -1;
		(void)hipGetLastError();
		setError("");
		return false;
	}
	m->pat_slots_state = 1;
	return true;
}

int refreshPatternSlots(smm_hip_csr* m, hipStream_t s) {
	if (!m->d_pat_slots || !m->d_pat_slot_base || m->rows <= 0) return SMM_HIP_OK;
	return m->dtype == SMM_DTYPE_F32 ? slotsFill<float>(m, s) : slotsFill<double>(m, s);
}

// the bytes of one plain launch: the copy, the per-wave header (base and the wave's mask), the other waves' rows from CSR (values,
// positions, start), x and out
long long patternSlotsBytes(const smm_hip_csr* m) {
	const long long s = m->dtype == SMM_DTYPE_F32 ? 4 : 8;
	const long long rows = m->rows, nnz = m->nnz;
	const long long otherRows = std::max(0LL, rows - 64LL * m->pat_slots_uniform);
	const long long otherNnz = std::max(0LL, nnz - m->pat_slots_elems);
	return m->pat_slots_elems * s + static_cast<long long>(m->pat_slots_waves) * 16 + otherNnz * (s + 4) + (otherRows + m->pat_slots_waves) * 4 +
	       static_cast<long long>(m->cols) * s + rows * s;
}

// gathers per piece and batch: ceil(p / 16) equal batches of a piece of p entries, in the three compiled sizes (the tile kernel's rule)
static int slotsBatch(const smm_hip_csr* m, int lanes) {
	const long long len = m->pat_slots_uniform > 0 ? (m->pat_slots_elems + 32LL * m->pat_slots_uniform) / (64LL * m->pat_slots_uniform) : 1;
	const int p = static_cast<int>(std::max(1LL, (len + lanes - 1) / lanes));
	const int nb = (p + 15) / 16;
	const int g = (p + nb - 1) / nb;
	return g <= 8 ? 8 : g <= 13 ? 13 : 16;
}

template <typename T, int L, int G>
static void launchSlotsG(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials,
                         const int* doneFlag, hipStream_t s) {
	static std::atomic<long long> occ{0};
	const int perCU = occupancyCached(occ, spmvPatternSlotsKernel<T, L, G>, TPB, 0, 4);
	const int cus = (op & SPMV_LEAVE_ROOM) ? std::max(8, numCUs() - 8) : numCUs();
	const int nWaves = m->pat_slots_waves;
	const int grid = std::max(1, std::min(std::min((nWaves + SLOT_WAVES - 1) / SLOT_WAVES, cus * perCU), NPART));
	const int nGroups = std::min(8, grid);
	const int chunkWaves = (nWaves + nGroups - 1) / nGroups;
	spmvPatternSlotsKernel<T, L, G><<<grid, TPB, 0, s>>>(m->rows, nWaves, chunkWaves, m->d_pat_off, m->d_pat_slot_base, m->d_pat_masks,
	                                                    static_cast<const T*>(m->d_pat_slots), m->d_start, m->d_positions, static_cast<const T*>(m->d_values),
	                                                    (op & ~SPMV_LEAVE_ROOM) | spmvOutFlags(m, sizeof(T)), lhs, divisor, x, out, dotMode, w1, partials,
	                                                    doneFlag);
}

template <typename T, int L>
static void launchSlotsL(const smm_hip_csr* m, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials,
                         const int* doneFlag, hipStream_t s) {
	switch (slotsBatch(m, L)) {
	case 8: launchSlotsG<T, L, 8>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	case 13: launchSlotsG<T, L, 13>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	default: launchSlotsG<T, L, 16>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s); break;
	}
}

template <typename T>
void launchPatSlots(const smm_hip_csr* m, int lanes, int op, const T* lhs, const T* divisor, const T* x, T* out, int dotMode, const T* w1, T* partials,
                    const int* doneFlag, hipStream_t s) {
	if (const int rowsOpen = patternSweepRows(m, lanes)) {
		launchPatSweep<T>(m, lanes, rowsOpen, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
		return;
	}
	if (lanes == 2) {
		launchSlotsL<T, 2>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	} else {
		launchSlotsL<T, 4>(m, op, lhs, divisor, x, out, dotMode, w1, partials, doneFlag, s);
	}
}

template void launchPatSlots<float>(const smm_hip_csr*, int, int, const float*, const float*, const float*, float*, int, const float*, float*, const int*,
                                    hipStream_t);
template void launchPatSlots<double>(const smm_hip_csr*, int, int, const double*, const double*, const double*, double*, int, const double*, double*,
                                     const int*, hipStream_t);

}  // namespace smm

extern "C" int smm_hip_csr_pattern_slots(smm_hip_csr* m, int mode) {
	if (!m || mode < -1 || mode > 3) {
		smm::setError("csr_pattern_slots: null matrix or a mode other than -1, 0, 1, 2, 3");
		return SMM_HIP_ERR_INVALID;
	}
	std::lock_guard<std::mutex> lock(m->tileMutex);
	m->pat_slots_mode = mode;
	if ((mode == 1 || mode == 3) && m->pat_slots_state < 0) m->pat_slots_state = 0;  // (a forced handle may try again)
	return SMM_HIP_OK;
}

extern "C" int smm_hip_set_pattern_sweep_rows(int rows_open) {
	if (rows_open != 0 && rows_open != 8 && rows_open != 16 && rows_open != 32) {
		smm::setError("set_pattern_sweep_rows: 8, 16, 32, or 0 for the default");
		return SMM_HIP_ERR_INVALID;
	}
	smm::g_sweepRows.store(rows_open, std::memory_order_relaxed);
	return SMM_HIP_OK;
}
