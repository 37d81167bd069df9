// smm_compose.hip -- matrices put together and taken apart ON THE DEVICE: the block matrix of a p x q table of handles, the submatrix of
// chosen rows and columns, the diagonal as a vector, and the scaling of rows and columns by vectors.  Every created matrix is an ordinary
// smm_hip_csr that owns its arrays and holds its columns ascending inside every row.  No floating-point atomics and no sort: the place of
// every output entry is a function of the operands' start[] arrays alone, so two calls give the same bits.
//   operands: every matrix whose start[] / positions[] steer addresses (the blocks, a submatrix's source) first passes the operand check of
//     the sparse sum (csrCheckSorted: start[] ascends from 0 to nnz, columns in range and strictly ascending; kept in the handle).
//   block (smm_hip_csr_block_create_*): the host derives the heights, widths and offsets from the handles' shapes and uploads ONE table
//     of p q slot descriptors (array pointers, row and column offset, coefficient, lanes per row, first workgroup).  count: one lane per
//     output row adds the lengths of its <= q segments; the exclusive scan (rocprim) gives start[]; fill: ONE launch for all slots.  A slot
//     of h rows gets h L lanes, L = the power of two next to a quarter of its mean row length (1 .. 65536): L consecutive lanes copy one
//     segment with stride L, so a 7-entry stencil row takes two lanes and a single row of 100 000 entries 32768 lanes across workgroups.
//     Inside a slot whose mean is short (L < 64) a group copies at most 8 L entries of its segment itself; what is left of a long segment
//     is copied by the whole wavefront, one long row after the other (a ballot finds them).  The place of a segment inside its output row
//     is recomputed from the row pointers of the slots to its left: nothing of size nnz is kept.  value = coef v, one rounding; coef == 1
//     copies the word.  Bytes (s = sizeof(T)): count rows (q + 1) 4, fill nnz (2 s + 8) plus the row pointers.
//   block refresh: the fill alone, values only, into the kept start[]: nnz 2 s plus the row pointers.  A segment is cut at the end of its
//     output row, so a block with other row lengths than at create (the caller's contract) cannot write outside the matrix.
//   submatrix (smm_hip_csr_submatrix_*): the index lists are checked on the device (integer atomicMin of the first bad position, read before
//     anything else is queued); colMap[a.cols] holds the new column or -1 (the range form compares against c0 / c1 instead).  count: L lanes
//     per selected row (L from the source's mean row length, <= 64) count the kept entries, summed through the group's ballot; a 64-bit scan
//     (the selection may repeat rows: the total is checked against 2^31 - 1); fill: the same walk, a kept entry's place is the number of kept
//     entries before it in the row (ballot + popcount, so the order inside a row is the source's); it also writes map[k] = source index.
//   submatrix refresh: values[k] = a.values[map[k]], nnz (2 s + 4) bytes, then the path of every value edit.
//   diagonal: one lane per row i < min(rows, cols), a binary search of the row for column i (start[] clamped to [0, nnz], so the reads stay
//     inside the arrays whatever it holds); the missing ones are counted per workgroup and added with one integer atomic each.
//   scale: one lane per stored entry finds its row by a binary search of start[] (only when there is a row vector) and writes
//     (r_i v) c_j: two roundings in this order (-ffp-contract=off).  Then the path of every value edit (csrValuesEdited).
#include <climits>

#include "smm_csr_build.h"

namespace smm {
namespace {

constexpr int CTPB = BUILD_TPB;
constexpr int MAX_SLOTS = 64;
constexpr int OWN_CHUNK = 8;         // entries per lane a group of L < 64 lanes copies itself; the rest of the segment goes to the whole wavefront
constexpr int MAX_LANES_LOG = 16;    // at most 65536 lanes per row
constexpr int NO_POS = INT_MAX;

__device__ __forceinline__ float fromWord(unsigned w) { return __uint_as_float(w); }
__device__ __forceinline__ double fromWord(unsigned long long w) { return __longlong_as_double(static_cast<long long>(w)); }
__device__ __forceinline__ unsigned toWord(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned long long toWord(double v) { return static_cast<unsigned long long>(__double_as_longlong(v)); }

// ---- block matrix ------------------------------------------------------------------------------------------------------------------------
struct Slot {
	const int* start;      // null: a zero block
	const int* positions;
	const void* values;
	unsigned long long coef;  // the raw word of the coefficient
	int colOff;
	int lanesLog;          // L = 1 << lanesLog lanes per row
	int one;               // coef == 1: copy the word
	int pad;
	long long firstGroup;  // the first workgroup of the slot in the fill launch
};

struct BlockTable {
	int p, q;
	int rowOff[MAX_SLOTS + 1];  // rowOff[I] = first output row of block row I (p + 1 entries)
	Slot slot[MAX_SLOTS];
};

// one lane per output row: start[r] = the sum of the lengths of its segments (start[rows] = 0: the scan's last addend)
__global__ __launch_bounds__(CTPB) void blockCountKernel(const BlockTable* __restrict__ tab, int rows, int* __restrict__ start) {
	const long long r = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (r > rows) return;
	int len = 0;
	if (r < rows) {
		const int p = tab->p, q = tab->q;
		int I = 0;
		while (I + 1 < p && tab->rowOff[I + 1] <= r) ++I;
		const int lr = static_cast<int>(r) - tab->rowOff[I];
		for (int J = 0; J < q; ++J) {
			const int* st = tab->slot[I * q + J].start;
			if (st) len += st[lr + 1] - st[lr];
		}
	}
	start[r] = len;
}

template <typename W, typename T>
__device__ __forceinline__ void copyEntry(const Slot& sl, int k, long long dest, T coef, int* __restrict__ outPos, W* __restrict__ outVal) {
	if (outPos) outPos[dest] = sl.positions[k] + sl.colOff;
	const W w = static_cast<const W*>(sl.values)[k];
	outVal[dest] = sl.one ? w : toWord(coef * fromWord(w));
}

// One launch for every slot: workgroup -> slot (a search of the <= 64 firstGroup words), L lanes per row of the slot.  outPos null: the
// refresh (values only).  Every destination lies in [outStart[row], outStart[row + 1]).
template <typename T>
__global__ __launch_bounds__(CTPB) void blockFillKernel(const BlockTable* __restrict__ tab, const int* __restrict__ outStart, int* __restrict__ outPos,
                                                        typename Word<T>::type* __restrict__ outVal) {
	using W = typename Word<T>::type;
	const int p = tab->p, q = tab->q;
	const int nSlots = p * q;
	int sIdx = 0;
	for (int k = 1; k < nSlots; ++k) {  // (firstGroup ascends; empty slots repeat the next one's: the LAST slot at or below this workgroup that has work)
		if (tab->slot[k].firstGroup <= static_cast<long long>(blockIdx.x)) sIdx = k;
	}
	const Slot sl = tab->slot[sIdx];
	if (!sl.start) return;  // (whole workgroup)
	const int I = sIdx / q, J = sIdx - I * q;
	const int h = tab->rowOff[I + 1] - tab->rowOff[I];
	const int lanesLog = sl.lanesLog;
	const long long t = (static_cast<long long>(blockIdx.x) - sl.firstGroup) * CTPB + threadIdx.x;
	const long long lr64 = t >> lanesLog;
	const int g = static_cast<int>(t & ((1LL << lanesLog) - 1));
	const bool valid = lr64 < h;
	T coef;
	{
		const W cw = static_cast<W>(sl.coef);
		coef = fromWord(cw);
	}
	int b = 0, e = 0;
	long long d = 0;
	if (valid) {
		const int lr = static_cast<int>(lr64);
		const int row = tab->rowOff[I] + lr;
		b = sl.start[lr];
		e = sl.start[lr + 1];
		d = outStart[row];
		for (int J2 = 0; J2 < J; ++J2) {
			const int* st = tab->slot[I * q + J2].start;
			if (st) d += st[lr + 1] - st[lr];
		}
		const long long room = static_cast<long long>(outStart[row + 1]) - d;  // (create: exactly e - b)
		if (e - b > room) e = b + static_cast<int>(room > 0 ? room : 0);
	}
	const int L = 1 << lanesLog;
	int own = e - b;
	if (lanesLog < 6 && own > L * OWN_CHUNK) own = L * OWN_CHUNK;
	for (int k = g; k < own; k += L) copyEntry<W, T>(sl, b + k, d + k, coef, outPos, outVal);
	if (lanesLog >= 6) return;  // (whole wavefronts: L >= 64 lanes share a row)
	// what is left of long segments: the whole wavefront, one row after the other
	unsigned long long longRows = __ballot(valid && g == 0 && e - b > own);
	const int lane = threadIdx.x & 63;
	while (longRows) {
		const int src = __ffsll(static_cast<long long>(longRows)) - 1;
		longRows &= longRows - 1;
		const int bb = __shfl(b + own, src), ee = __shfl(e, src);
		const int dLo = __shfl(static_cast<int>((d + own) & 0xFFFFFFFFLL), src), dHi = __shfl(static_cast<int>((d + own) >> 32), src);
		const long long dd = (static_cast<long long>(dHi) << 32) | static_cast<unsigned>(dLo);
		for (int k = bb + lane; k < ee; k += 64) copyEntry<W, T>(sl, k, dd + (k - bb), coef, outPos, outVal);
	}
}

// ---- submatrix ---------------------------------------------------------------------------------------------------------------------------
// words[0] / words[1]: the first position of rows_idx / cols_idx that is out of range or (columns) not above its predecessor
__global__ void wordsInitKernel(int* words) {
	if (threadIdx.x < 2) words[threadIdx.x] = NO_POS;
}

__global__ __launch_bounds__(CTPB) void indexCheckKernel(const int* __restrict__ idx, long long n, int bound, int ascending, int* word) {
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (i >= n) return;
	const int v = idx[i];
	const bool bad = v < 0 || v >= bound || (ascending && i > 0 && idx[i - 1] >= v);
	if (bad) atomicMin(word, static_cast<int>(i));  // (n <= 2^31 - 1, and a bad last position of such a list is INT_MAX - 1 at most)
}

// (cols_idx has been checked: every write is in range and no two lanes write one word)
__global__ __launch_bounds__(CTPB) void colMapKernel(const int* __restrict__ colsIdx, int nc, int* __restrict__ colMap) {
	const long long j = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (j < nc) colMap[colsIdx[j]] = static_cast<int>(j);
}

// the new column of `col`, -1 when it is not selected
__device__ __forceinline__ int newColumn(const int* __restrict__ colMap, int c0, int c1, int col) {
	if (colMap) return colMap[col];
	return col >= c0 && col < c1 ? col - c0 : -1;
}

// L = 1 << lanesLog <= 64 lanes per selected row i (source row rowsIdx[i], or r0 + i).  FILL false: counts[i] = kept entries (counts[nr] = 0);
// FILL true: the kept entries in the source's order from outStart[i] on, with map[k] = the source index.
template <typename W, bool FILL>
__global__ __launch_bounds__(CTPB) void subKernel(int nr, const int* __restrict__ rowsIdx, int r0, const int* __restrict__ colMap, int c0, int c1, int lanesLog,
                                                  const int* __restrict__ aStart, const int* __restrict__ aPos, const W* __restrict__ aVal, int* __restrict__ counts,
                                                  const int* __restrict__ outStart, int* __restrict__ outPos, W* __restrict__ outVal, int* __restrict__ map) {
	const long long t = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	const long long i = t >> lanesLog;
	const int L = 1 << lanesLog;
	const int g = static_cast<int>(t & (L - 1));
	const int lane = threadIdx.x & 63;
	const int shift = lane - g;  // the group's first lane inside the wavefront
	const unsigned long long groupMask = L == 64 ? ~0ull : ((1ull << L) - 1);
	const bool valid = i < nr;
	int k = 0, e = 0;
	if (valid) {
		const int row = rowsIdx ? rowsIdx[i] : r0 + static_cast<int>(i);
		k = aStart[row];
		e = aStart[row + 1];
	}
	long long d = FILL && valid ? outStart[i] : 0;
	int count = 0;
	while (__any(k < e)) {  // (the wavefront walks together: the ballots below need every lane)
		const int idx = k + g;
		int nj = -1;
		if (idx < e) nj = newColumn(colMap, c0, c1, aPos[idx]);
		const unsigned long long kept = (__ballot(nj >= 0) >> shift) & groupMask;
		if (FILL && nj >= 0) {
			const long long dest = d + __popcll(kept & ((1ull << g) - 1));
			outPos[dest] = nj;
			outVal[dest] = aVal[idx];
			map[dest] = idx;
		}
		const int n = __popcll(kept);
		d += n;
		count += n;
		if (k < e) k += L;
	}
	if (!FILL) {
		if (valid && g == 0) counts[i] = count;
		if (t == 0) counts[nr] = 0;
	}
}

// (map[] holds indices below the source's entry count, which the caller has compared with the matrix it passes)
template <typename W>
__global__ __launch_bounds__(CTPB) void gatherKernel(int nnz, const int* __restrict__ map, const W* __restrict__ values, W* __restrict__ out) {
	const long long k = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (k < nnz) out[k] = values[map[k]];
}

// ---- diagonal and scaling ----------------------------------------------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(CTPB) void diagonalKernel(int n, int nnz, const int* __restrict__ start, const int* __restrict__ positions, const W* __restrict__ values,
                                                       W* __restrict__ out, int* missing) {
	__shared__ int blockMissing;
	if (threadIdx.x == 0) blockMissing = 0;
	__syncthreads();
	const long long i = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (i < n) {
		int lo = min(max(start[i], 0), nnz);
		int hi = min(max(start[i + 1], lo), nnz);
		const int end = hi;
		while (lo < hi) {
			const int mid = lo + ((hi - lo) >> 1);
			if (positions[mid] < i) lo = mid + 1;
			else hi = mid;
		}
		const bool found = lo < end && positions[lo] == i;
		out[i] = found ? values[lo] : W(0);
		if (!found && missing) atomicAdd(&blockMissing, 1);
	}
	__syncthreads();
	if (threadIdx.x == 0 && missing && blockMissing) atomicAdd(missing, blockMissing);
}

template <typename T>
__global__ __launch_bounds__(CTPB) void scaleKernel(int nnz, int rows, int cols, const int* __restrict__ start, const int* __restrict__ positions,
                                                    const T* __restrict__ r, const T* __restrict__ c, T* __restrict__ values) {
	const long long e = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	if (e >= nnz) return;
	T v = values[e];
	if (r) v = r[rowOfEntry(rows, start, static_cast<int>(e))] * v;
	if (c) {
		const int col = positions[e];
		if (col < 0 || col >= cols) return;  // (no such element of c: the entry stays)
		v = v * c[col];
	}
	values[e] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int lanesLogFor(long long rows, long long nnz, int cap) {
	const long long mean = rows > 0 ? nnz / rows : 0;
	int lg = 0;
	while (lg < cap && (4LL << lg) < mean) ++lg;
	return lg;
}

template <typename T>
unsigned long long wordOf(T v) {
	typename Word<T>::type w;
	memcpy(&w, &v, sizeof(T));
	return w;
}

// The table of a p x q block matrix from the handles as they are now: shapes derived and compared, the slots' descriptors, the fill
// launch's workgroups.  *totalNnz in 64 bits.  Every block is ready and has passed the operand check.
template <typename T>
int buildBlockTable(const char* what, int p, int q, const smm_hip_csr* const* blocks, const T* coef, const int* rowSizes, const int* colSizes, hipStream_t s,
                    BlockTable* tab, long long* totalRows, long long* totalCols, long long* totalNnz, long long* groups, std::vector<int>* sizes = nullptr) {
	std::vector<int> h(p, -1), w(q, -1);
	for (int I = 0; I < p; ++I) {
		for (int J = 0; J < q; ++J) {
			const smm_hip_csr* m = blocks[I * q + J];
			if (!m) continue;
			if (m->dtype != dtypeOf<T>()) {
				setError("%s: block (%d, %d) holds the other element type", what, I, J);
				return SMM_HIP_ERR_INVALID;
			}
			SMM_TRY(ensureCsrReady(m, s, true));
			if ((h[I] >= 0 && h[I] != m->rows) || (w[J] >= 0 && w[J] != m->cols)) {
				setError("%s: block (%d, %d) is %d x %d, block row %d is %d high and block column %d is %d wide", what, I, J, m->rows, m->cols, I, h[I] >= 0 ? h[I] : m->rows,
				         J, w[J] >= 0 ? w[J] : m->cols);
				return SMM_HIP_ERR_INVALID;
			}
			h[I] = m->rows;
			w[J] = m->cols;
		}
	}
	for (int I = 0; I < p; ++I) {
		if (rowSizes && rowSizes[I] >= 0 && h[I] >= 0 && rowSizes[I] != h[I]) {
			setError("%s: row_sizes[%d] = %d, the blocks of that block row are %d high", what, I, rowSizes[I], h[I]);
			return SMM_HIP_ERR_INVALID;
		}
		if (h[I] < 0) h[I] = rowSizes ? rowSizes[I] : -1;
		if (h[I] < 0) {
			setError("%s: block row %d holds no block and row_sizes gives no height for it", what, I);
			return SMM_HIP_ERR_INVALID;
		}
	}
	for (int J = 0; J < q; ++J) {
		if (colSizes && colSizes[J] >= 0 && w[J] >= 0 && colSizes[J] != w[J]) {
			setError("%s: col_sizes[%d] = %d, the blocks of that block column are %d wide", what, J, colSizes[J], w[J]);
			return SMM_HIP_ERR_INVALID;
		}
		if (w[J] < 0) w[J] = colSizes ? colSizes[J] : -1;
		if (w[J] < 0) {
			setError("%s: block column %d holds no block and col_sizes gives no width for it", what, J);
			return SMM_HIP_ERR_INVALID;
		}
	}
	long long rows = 0, cols = 0, nnz = 0;
	std::vector<long long> colOff(q);
	for (int J = 0; J < q; ++J) {
		colOff[J] = cols;
		cols += w[J];
	}
	for (int I = 0; I < p; ++I) rows += h[I];
	for (int k = 0; k < p * q; ++k) nnz += blocks[k] ? blocks[k]->nnz : 0;
	if (rows > INT_MAX || cols > INT_MAX || nnz > INT_MAX) {
		setError("%s: the block matrix would be %lld x %lld with %lld entries, beyond 2^31 - 1", what, rows, cols, nnz);
		return SMM_HIP_ERR_INVALID;
	}
	memset(tab, 0, sizeof(*tab));
	tab->p = p;
	tab->q = q;
	int r = 0;
	for (int I = 0; I < p; ++I) {
		tab->rowOff[I] = r;
		r += h[I];
	}
	tab->rowOff[p] = r;
	long long g = 0;
	for (int k = 0; k < p * q; ++k) {
		const smm_hip_csr* m = blocks[k];
		Slot& sl = tab->slot[k];
		sl.firstGroup = g;
		if (!m || m->rows == 0 || m->nnz == 0) continue;  // (start stays null: nothing to copy)
		SMM_TRY(csrCheckSorted(what, "a block", m, s));
		const T cf = coef ? coef[k] : T(1);
		sl.start = m->d_start;
		sl.positions = m->d_positions;
		sl.values = m->d_values;
		sl.coef = wordOf<T>(cf);
		sl.one = cf == T(1) ? 1 : 0;
		sl.colOff = static_cast<int>(colOff[k % q]);
		sl.lanesLog = lanesLogFor(m->rows, m->nnz, MAX_LANES_LOG);
		g += (static_cast<long long>(m->rows) << sl.lanesLog) / CTPB + 1;
	}
	if (g > INT_MAX) {
		setError("%s: the fill would take %lld workgroups", what, g);
		return SMM_HIP_ERR_INVALID;
	}
	if (sizes) {
		*sizes = h;
		sizes->insert(sizes->end(), w.begin(), w.end());
	}
	*totalRows = rows;
	*totalCols = cols;
	*totalNnz = nnz;
	*groups = g;
	return SMM_HIP_OK;
}

int checkTableArgs(const char* what, int p, int q, const void* blocks) {
	if (p < 1 || q < 1 || static_cast<long long>(p) * q > MAX_SLOTS || !blocks) {
		setError("%s: p and q must be at least 1 with p q <= %d, and blocks not null", what, MAX_SLOTS);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
int blockCreate(int p, int q, const smm_hip_csr* const* blocks, const T* coef, const int* rowSizes, const int* colSizes, smm_hip_stream stream, smm_hip_csr** out) {
	using W = typename Word<T>::type;
	const char* what = "csr_block_create";
	if (!out) {
		setError("%s: out is null", what);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(checkTableArgs(what, p, q, blocks));
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	SetupTrace trace("block matrix: create");
	std::unique_ptr<BlockTable> tab(new BlockTable);
	long long rows = 0, cols = 0, nnz = 0, groups = 0;
	std::vector<int> sizes;
	SMM_TRY(buildBlockTable<T>(what, p, q, blocks, coef, rowSizes, colSizes, s, tab.get(), &rows, &cols, &nnz, &groups, &sizes));
	OwnedCsr c;
	SMM_TRY(newOwnedCsr(static_cast<int>(rows), static_cast<int>(cols), dtypeOf<T>(), &c));
	SMM_TRY(allocCsrEntries(c.get(), nnz, false));
	DevBuf<BlockTable> d_tab;
	SMM_TRY(d_tab.alloc(1));
	SMM_TRY(hostToDev(d_tab.p, tab.get(), sizeof(BlockTable), s));
	blockCountKernel<<<gridOf(rows + 1), CTPB, 0, s>>>(d_tab.p, c->rows, c->d_start);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(scanExclusive(c->d_start, c->d_start, static_cast<size_t>(rows) + 1, s));
	if (groups > 0) blockFillKernel<T><<<static_cast<int>(groups), CTPB, 0, s>>>(d_tab.p, c->d_start, c->d_positions, static_cast<W*>(c->d_values));
	SMM_HIP_TRY(hipGetLastError());
	c->blockSlots.assign({p, q});
	c->blockSlots.insert(c->blockSlots.end(), sizes.begin(), sizes.end());  // the p heights, the q widths
	for (int k = 0; k < p * q; ++k) {
		const smm_hip_csr* m = blocks[k];
		c->blockSlots.insert(c->blockSlots.end(), {m ? m->rows : -1, m ? m->cols : -1, m ? m->nnz : -1});
	}
	SMM_TRY(ensureCsrReady(c.get(), s, true));  // nnz, the first active row, the typical row and the kernel choice as for caller-owned device arrays
	c->sorted_ok.store(1, std::memory_order_release);  // (by construction)
	*out = c.release();
	return SMM_HIP_OK;
}

template <typename T>
int blockRefresh(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const T* coef, smm_hip_stream stream) {
	using W = typename Word<T>::type;
	const char* what = "csr_block_refresh";
	if (!c) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(checkTableArgs(what, p, q, blocks));
	if (c->dtype != dtypeOf<T>()) {
		setError("%s: the matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (c->blockSlots.size() != 2 + static_cast<size_t>(p) + q + 3 * static_cast<size_t>(p) * q || c->blockSlots[0] != p || c->blockSlots[1] != q) {
		setError("%s: the handle was not made by smm_hip_csr_block_create from a %d x %d table", what, p, q);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	const int* h = &c->blockSlots[2];  // the heights and widths at create: also those of the block rows and columns that hold no block
	const int* w = h + p;
	for (int k = 0; k < p * q; ++k) {
		const smm_hip_csr* m = blocks[k];
		const int* rec = &c->blockSlots[2 + p + q + 3 * k];
		if (m == c) {
			setError("%s: block (%d, %d) is the matrix itself", what, k / q, k % q);
			return SMM_HIP_ERR_INVALID;
		}
		if (m) SMM_TRY(ensureCsrReady(m, s, true));
		if ((m == nullptr) != (rec[0] < 0) || (m && (m->rows != rec[0] || m->cols != rec[1] || m->nnz != rec[2]))) {
			setError("%s: block (%d, %d) has not the shape and the entry count of the block at create", what, k / q, k % q);
			return SMM_HIP_ERR_INVALID;
		}
	}
	SMM_TRY(ensureCsrReady(c, s, true));
	std::unique_ptr<BlockTable> tab(new BlockTable);
	long long rows = 0, cols = 0, nnz = 0, groups = 0;
	SMM_TRY(buildBlockTable<T>(what, p, q, blocks, coef, h, w, s, tab.get(), &rows, &cols, &nnz, &groups));
	if (rows != c->rows || cols != c->cols || nnz != c->nnz) {
		setError("%s: the table gives a %lld x %lld matrix with %lld entries, the handle is %d x %d with %d", what, rows, cols, nnz, c->rows, c->cols, c->nnz);
		return SMM_HIP_ERR_INVALID;
	}
	if (groups > 0) {
		DevBuf<BlockTable> d_tab;
		SMM_TRY(d_tab.alloc(1));
		SMM_TRY(hostToDev(d_tab.p, tab.get(), sizeof(BlockTable), s));
		blockFillKernel<T><<<static_cast<int>(groups), CTPB, 0, s>>>(d_tab.p, c->d_start, nullptr, static_cast<W*>(c->d_values));
		SMM_HIP_TRY(hipGetLastError());
	}
	return csrValuesEdited(c, s);
}

// ---- submatrix ---------------------------------------------------------------------------------------------------------------------------
// rows: d_rows (nr indices, device) or the range [r0, r0 + nr); columns: d_cols (nc strictly ascending indices, device) or the range [c0, c1)
int submatrixOnDevice(const char* what, const smm_hip_csr* a, const int* d_rows, int r0, int nr, const int* d_cols, int c0, int c1, int nc, hipStream_t s,
                      smm_hip_csr** out) {
	SetupTrace trace("submatrix: create");
	SMM_TRY(csrCheckSorted(what, "a", a, s));
	if (d_rows || d_cols) {
		DevBuf<int> d_words;
		SMM_TRY(d_words.alloc(2));
		wordsInitKernel<<<1, 64, 0, s>>>(d_words.p);
		if (d_rows && nr > 0) indexCheckKernel<<<gridOf(nr), CTPB, 0, s>>>(d_rows, nr, a->rows, 0, d_words.p);
		if (d_cols && nc > 0) indexCheckKernel<<<gridOf(nc), CTPB, 0, s>>>(d_cols, nc, a->cols, 1, d_words.p + 1);
		SMM_HIP_TRY(hipGetLastError());
		int words[2];
		SMM_HIP_TRY(hipMemcpyAsync(words, d_words.p, sizeof(words), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (words[0] != NO_POS) {
			setError("%s: rows_idx[%d] lies outside [0, %d)", what, words[0], a->rows);
			return SMM_HIP_ERR_INVALID;
		}
		if (words[1] != NO_POS) {
			setError("%s: cols_idx[%d] lies outside [0, %d) or is not above cols_idx[%d]: the columns must ascend strictly", what, words[1], a->cols, words[1] - 1);
			return SMM_HIP_ERR_INVALID;
		}
	}
	const int width = d_cols ? nc : c1 - c0;
	OwnedCsr c;
	SMM_TRY(newOwnedCsr(nr, width, a->dtype, &c));
	DevBuf<int> colMap, counts;
	if (d_cols) {
		SMM_TRY(colMap.alloc(static_cast<size_t>(a->cols)));
		if (a->cols > 0) SMM_HIP_TRY(hipMemsetAsync(colMap.p, 0xFF, static_cast<size_t>(a->cols) * sizeof(int), s));
		if (nc > 0) colMapKernel<<<gridOf(nc), CTPB, 0, s>>>(d_cols, nc, colMap.p);
	}
	const int* map = d_cols ? colMap.p : nullptr;
	const int lanesLog = lanesLogFor(a->rows, a->nnz, 6);
	const int grid = gridOf(static_cast<long long>(std::max(nr, 1)) << lanesLog);
	SMM_TRY(counts.alloc(static_cast<size_t>(nr) + 1));
	const bool f32 = a->dtype == SMM_DTYPE_F32;
	// (the count reads no values: one instantiation serves both element types)
	subKernel<unsigned, false><<<grid, CTPB, 0, s>>>(nr, d_rows, r0, map, c0, c1, lanesLog, a->d_start, a->d_positions, nullptr, counts.p, nullptr, nullptr, nullptr, nullptr);
	SMM_HIP_TRY(hipGetLastError());
	long long nnz = 0;
	SMM_TRY(startsFromCounts(what, "submatrix", counts.p, nr, c.get(), &nnz, s));
	SMM_TRY(allocCsrEntries(c.get(), nnz, true));
	if (nnz > 0) {
		if (f32) {
			subKernel<unsigned, true><<<grid, CTPB, 0, s>>>(nr, d_rows, r0, map, c0, c1, lanesLog, a->d_start, a->d_positions, static_cast<const unsigned*>(a->d_values), nullptr,
			                                                c->d_start, c->d_positions, static_cast<unsigned*>(c->d_values), c->d_tperm);
		} else {
			subKernel<unsigned long long, true><<<grid, CTPB, 0, s>>>(nr, d_rows, r0, map, c0, c1, lanesLog, a->d_start, a->d_positions,
			                                                          static_cast<const unsigned long long*>(a->d_values), nullptr, c->d_start, c->d_positions,
			                                                          static_cast<unsigned long long*>(c->d_values), c->d_tperm);
		}
	}
	SMM_HIP_TRY(hipGetLastError());
	c->subSrcRows = a->rows;
	c->subSrcCols = a->cols;
	c->subSrcNnz = a->nnz;
	SMM_TRY(ensureCsrReady(c.get(), s, true));
	c->sorted_ok.store(1, std::memory_order_release);  // (by construction: a's rows ascend and cols_idx does)
	*out = c.release();
	return SMM_HIP_OK;
}

int submatrixChecked(const char* what, const smm_hip_csr* a, smm_hip_csr** out, long long nr, long long nc, hipStream_t s) {
	if (!out) {
		setError("%s: out is null", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (!a) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (nr < 0 || nc < 0 || nr > INT_MAX || nc > INT_MAX) {
		setError("%s: an index count is negative or beyond 2^31 - 1", what);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	return ensureCsrReady(a, s, true);
}

int submatrixCreate(const smm_hip_csr* a, const int* rowsIdx, size_t nr, const int* colsIdx, size_t nc, bool onDevice, smm_hip_stream stream, smm_hip_csr** out) {
	const char* what = "csr_submatrix_create";
	hipStream_t s = pickStream(stream);
	SMM_TRY(submatrixChecked(what, a, out, rowsIdx ? static_cast<long long>(nr) : 0, colsIdx ? static_cast<long long>(nc) : 0, s));
	DevBuf<int> dr, dc;
	const int* d_rows = rowsIdx;
	const int* d_cols = colsIdx;
	if (!onDevice) {
		if (rowsIdx) {
			SMM_TRY(dr.alloc(nr));
			SMM_TRY(hostToDev(dr.p, rowsIdx, nr * sizeof(int), s));
			d_rows = dr.p;
		}
		if (colsIdx) {
			SMM_TRY(dc.alloc(nc));
			SMM_TRY(hostToDev(dc.p, colsIdx, nc * sizeof(int), s));
			d_cols = dc.p;
		}
	}
	return submatrixOnDevice(what, a, d_rows, 0, rowsIdx ? static_cast<int>(nr) : a->rows, d_cols, 0, a->cols, colsIdx ? static_cast<int>(nc) : a->cols, s, out);
}

template <typename T>
int submatrixRefresh(smm_hip_csr* sub, const smm_hip_csr* a, smm_hip_stream stream) {
	using W = typename Word<T>::type;
	const char* what = "csr_submatrix_refresh";
	if (!sub || !a) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (sub->dtype != dtypeOf<T>() || a->dtype != dtypeOf<T>()) {
		setError("%s: a matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (sub->subSrcNnz < 0 || !sub->d_tperm) {
		setError("%s: the handle was not made by smm_hip_csr_submatrix_create", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (sub == a) {
		setError("%s: the source is the submatrix itself", what);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(sub, s, true));
	if (a->rows != sub->subSrcRows || a->cols != sub->subSrcCols || a->nnz != sub->subSrcNnz) {
		setError("%s: the matrix has not the shape or the entry count of the submatrix's source", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (sub->nnz > 0) {
		gatherKernel<W><<<gridOf(sub->nnz), CTPB, 0, s>>>(sub->nnz, sub->d_tperm, static_cast<const W*>(a->d_values), static_cast<W*>(sub->d_values));
		SMM_HIP_TRY(hipGetLastError());
	}
	return csrValuesEdited(sub, s);
}

// ---- diagonal and scaling ----------------------------------------------------------------------------------------------------------------
int checkHandle(const smm_hip_csr* m, int dtype, const char* what) {
	if (!m) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (m->dtype != dtype) {
		setError("%s: the matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

template <typename T>
int diagonalOnDevice(const smm_hip_csr* a, T* d_out, int* d_missing, hipStream_t s) {
	using W = typename Word<T>::type;
	const int n = std::min(a->rows, a->cols);
	if (d_missing) SMM_HIP_TRY(hipMemsetAsync(d_missing, 0, sizeof(int), s));
	if (n > 0) {
		diagonalKernel<W><<<gridOf(n), CTPB, 0, s>>>(n, a->nnz, a->d_start, a->d_positions, static_cast<const W*>(a->d_values), reinterpret_cast<W*>(d_out), d_missing);
		SMM_HIP_TRY(hipGetLastError());
	}
	return SMM_HIP_OK;
}

template <typename T>
int diagonalDev(const smm_hip_csr* a, T* d_out, int* d_missing, smm_hip_stream stream) {
	const char* what = "csr_diagonal_dev";
	SMM_TRY(checkHandle(a, dtypeOf<T>(), what));
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(a, s, true));
	if (!d_out && std::min(a->rows, a->cols) > 0) {
		setError("%s: null output", what);
		return SMM_HIP_ERR_INVALID;
	}
	return diagonalOnDevice<T>(a, d_out, d_missing, s);
}

template <typename T>
int diagonalHost(const smm_hip_csr* a, T* out, int* missing) {
	const char* what = "csr_diagonal";
	SMM_TRY(checkHandle(a, dtypeOf<T>(), what));
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	const int n = std::min(a->rows, a->cols);
	if (!out && n > 0) {
		setError("%s: null output", what);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_HIP_TRY(hipDeviceSynchronize());  // (no stream: the arrays may still be being written on any of the caller's streams)
	hipStream_t s = libStream();
	DevBuf<T> d_out;
	DevBuf<int> d_missing;
	SMM_TRY(d_out.alloc(static_cast<size_t>(n)));
	SMM_TRY(d_missing.alloc(1));
	SMM_TRY(diagonalOnDevice<T>(a, d_out.p, d_missing.p, s));
	int count = 0;
	if (n > 0) SMM_TRY(devToHost(out, d_out.p, static_cast<size_t>(n) * sizeof(T), s));
	SMM_TRY(devToHost(&count, d_missing.p, sizeof(int), s));
	if (missing) *missing = count;
	return SMM_HIP_OK;
}

template <typename T>
int scaleOnDevice(smm_hip_csr* m, const T* d_r, const T* d_c, hipStream_t s) {
	if (!d_r && !d_c) return SMM_HIP_OK;  // (nothing is written: the bits and everything derived from them stay)
	if (m->nnz > 0 && m->rows > 0) {
		scaleKernel<T><<<gridOf(m->nnz), CTPB, 0, s>>>(m->nnz, m->rows, m->cols, m->d_start, m->d_positions, d_r, d_c, static_cast<T*>(m->d_values));
		SMM_HIP_TRY(hipGetLastError());
	}
	return csrValuesEdited(m, s);
}

template <typename T>
int scaleRowsCols(smm_hip_csr* m, const T* d_r, const T* d_c, smm_hip_stream stream) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_scale_rows_cols_dev"));
	hipStream_t s = pickStream(stream);
	SMM_TRY(ensureCsrReady(m, s, true));
	return scaleOnDevice<T>(m, d_r, d_c, s);
}

template <typename T>
int scaleRowsColsHost(smm_hip_csr* m, const T* r, const T* c) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_scale_rows_cols"));
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	SMM_HIP_TRY(hipDeviceSynchronize());  // (no stream: the values may still be being written on any of the caller's streams)
	hipStream_t s = libStream();
	DevBuf<T> dr, dc;
	if (r) {
		SMM_TRY(dr.alloc(static_cast<size_t>(m->rows)));
		SMM_TRY(hostToDev(dr.p, r, static_cast<size_t>(m->rows) * sizeof(T), s));
	}
	if (c) {
		SMM_TRY(dc.alloc(static_cast<size_t>(m->cols)));
		SMM_TRY(hostToDev(dc.p, c, static_cast<size_t>(m->cols) * sizeof(T), s));
	}
	SMM_TRY(scaleOnDevice<T>(m, r ? dr.p : nullptr, c ? dc.p : nullptr, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

}  // namespace
}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_block_create_f32(int p, int q, const smm_hip_csr* const* blocks, const float* coef, const int* row_sizes, const int* col_sizes, smm_hip_stream stream,
                                 smm_hip_csr** out) {
	return blockCreate<float>(p, q, blocks, coef, row_sizes, col_sizes, stream, out);
}
int smm_hip_csr_block_create_f64(int p, int q, const smm_hip_csr* const* blocks, const double* coef, const int* row_sizes, const int* col_sizes, smm_hip_stream stream,
                                 smm_hip_csr** out) {
	return blockCreate<double>(p, q, blocks, coef, row_sizes, col_sizes, stream, out);
}
int smm_hip_csr_block_refresh_f32(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const float* coef, smm_hip_stream stream) {
	return blockRefresh<float>(c, p, q, blocks, coef, stream);
}
int smm_hip_csr_block_refresh_f64(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const double* coef, smm_hip_stream stream) {
	return blockRefresh<double>(c, p, q, blocks, coef, stream);
}

int smm_hip_csr_submatrix_create(const smm_hip_csr* a, const int* rows_idx, size_t nr, const int* cols_idx, size_t nc, smm_hip_stream stream, smm_hip_csr** out) {
	return submatrixCreate(a, rows_idx, nr, cols_idx, nc, false, stream, out);
}
int smm_hip_csr_submatrix_create_dev(const smm_hip_csr* a, const int* d_rows_idx, size_t nr, const int* d_cols_idx, size_t nc, smm_hip_stream stream, smm_hip_csr** out) {
	return submatrixCreate(a, d_rows_idx, nr, d_cols_idx, nc, true, stream, out);
}
int smm_hip_csr_submatrix_range_create(const smm_hip_csr* a, int r0, int r1, int c0, int c1, smm_hip_stream stream, smm_hip_csr** out) {
	const char* what = "csr_submatrix_range_create";
	hipStream_t s = pickStream(stream);
	SMM_TRY(submatrixChecked(what, a, out, 0, 0, s));
	if (r0 < 0 || r0 > r1 || r1 > a->rows || c0 < 0 || c0 > c1 || c1 > a->cols) {
		setError("%s: rows [%d, %d) and columns [%d, %d) must lie inside the %d x %d matrix", what, r0, r1, c0, c1, a->rows, a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	return submatrixOnDevice(what, a, nullptr, r0, r1 - r0, nullptr, c0, c1, c1 - c0, s, out);
}
int smm_hip_csr_submatrix_refresh_f32(smm_hip_csr* sub, const smm_hip_csr* a, smm_hip_stream stream) { return submatrixRefresh<float>(sub, a, stream); }
int smm_hip_csr_submatrix_refresh_f64(smm_hip_csr* sub, const smm_hip_csr* a, smm_hip_stream stream) { return submatrixRefresh<double>(sub, a, stream); }

int smm_hip_csr_diagonal_f32(const smm_hip_csr* a, float* out, int* missing) { return diagonalHost<float>(a, out, missing); }
int smm_hip_csr_diagonal_f64(const smm_hip_csr* a, double* out, int* missing) { return diagonalHost<double>(a, out, missing); }
int smm_hip_csr_diagonal_dev_f32(const smm_hip_csr* a, float* d_out, int* d_missing, smm_hip_stream stream) { return diagonalDev<float>(a, d_out, d_missing, stream); }
int smm_hip_csr_diagonal_dev_f64(const smm_hip_csr* a, double* d_out, int* d_missing, smm_hip_stream stream) { return diagonalDev<double>(a, d_out, d_missing, stream); }

int smm_hip_csr_scale_rows_cols_dev_f32(smm_hip_csr* m, const float* d_r, const float* d_c, smm_hip_stream stream) { return scaleRowsCols<float>(m, d_r, d_c, stream); }
int smm_hip_csr_scale_rows_cols_dev_f64(smm_hip_csr* m, const double* d_r, const double* d_c, smm_hip_stream stream) { return scaleRowsCols<double>(m, d_r, d_c, stream); }
int smm_hip_csr_scale_rows_cols_f32(smm_hip_csr* m, const float* r, const float* c) { return scaleRowsColsHost<float>(m, r, c); }
int smm_hip_csr_scale_rows_cols_f64(smm_hip_csr* m, const double* r, const double* c) { return scaleRowsColsHost<double>(m, r, c); }

}  // extern "C"
