// smm_multiblock.h -- the block x block tall-skinny kernels (smm_solvers_lobpcg.hip): G = V^T W for two blocks of at most MB_MAX columns, and
// W = W - V H with H in device memory.  smm_multivec.h pairs a block with ONE vector; built from it a 24-column basis would be read 24 times
// per Gram matrix.  Column conventions as there: column i at V + i * ld, ld >= n, nothing between n and ld is read or written, element
// alignment is legal, 16-byte accesses when the alignment and ld allow.  Each unit that includes this instantiates its own copies.
#pragma once
#include <algorithm>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_multivec.h"

namespace smm {

constexpr int MB_MAX = SMM_LOBPCG_MAX_BASIS;
static_assert(MB_MAX == 24, "two 16-column MFMA tiles a side, three 8-column register groups");
constexpr int MG_NPART = 1024;  // workgroups of a multiGram launch at most: one slot of per-workgroup partial sums each
constexpr int MG_U = 4;         // chunks of rows a wavefront has in flight

// ---------------------------------------------------------------------------------------------------------
// multiGram: G = V^T W on the matrix cores, v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: an fmaf chain).
// One instruction is a 16 x 16 tile of G from 4 rows of the blocks: lane (c = lane & 15, q = lane >> 4) supplies A[c][q] = V[row q][column c]
// and B[q][c] = W[row q][column c], ONE element each.  So a lane loads the elements it feeds straight from memory into the operand
// registers: no LDS stage, no element loaded twice, and with V == W the same register is both operands.  Up to 2 x 2 tiles cover the
// 24 x 24 result (columns >= m, l contribute zeros and are not loaded): TI + TJ loads feed TI * TJ instructions.
// The sum over the rows has no order to keep, so the 4 k-slots of an instruction need not be 4 CONSECUTIVE rows: a lane takes a run of
// R consecutive rows of its column (R = 1, or one 16-byte pack), the four q's take consecutive runs, and step r of a chunk uses element r
// of every lane's run -- A and B see the same row in the same slot, which is all the product needs.  A wavefront's load of one column
// is then 4 R consecutive elements, and MG_U chunks are in flight: 4 R MG_U consecutive elements of each of 16 columns.
// Accumulators: 4 per lane and tile (D[row (lane >> 4) + 4 reg][column lane & 15] in fp64, D[row 4 (lane >> 4) + reg][...] in fp32).
// A wavefront's sums have a fixed order; the four of a workgroup are added left to right through LDS; workgroup b stores its m l sums
// to partials[(i + j m) MG_NPART + b]; multiGramFinish adds the workgroups' in the project's fixed order.  No atomics.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
struct Mfma16;
template <>
struct Mfma16<double> {
	typedef double Acc __attribute__((ext_vector_type(4)));
	static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
	static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <>
struct Mfma16<float> {
	typedef float Acc __attribute__((ext_vector_type(4)));
	static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
	static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

// the run of R rows starting at `row` of column `col` of a block; a lane without a column or a row loads the block's first run and
// takes zeros (the instruction wants every lane)
template <typename T, int R>
__device__ __forceinline__ void gramLoad(const T* B, long long ld, int cols, int col, long long row, bool rowLive, T (&out)[R]) {
	using P = typename Pack16<T>::V;
	const bool live = rowLive && col < cols;
	const T* p = B + (live ? static_cast<long long>(col) * ld + row : 0);
	if constexpr (R == 1) {
		const T v = *p;
		out[0] = live ? v : T(0);
	} else {
		const P v = *reinterpret_cast<const P*>(p);
#pragma unroll
		for (int e = 0; e < R; ++e) out[e] = live ? v[e] : T(0);
	}
}

// SYM: W is V and l is m -- V is loaded once and feeds both operands.  R > 1 needs both blocks 16-byte aligned and both leading
// dimensions multiples of R (the launcher checks); the last n % R rows take one lane each.  n >= 1.
template <typename T, int TI, int TJ, bool SYM, int R>
__global__ __launch_bounds__(MV_TPB) void multiGramKernel(long long n, int m, int l, const T* __restrict__ V, long long ldV, const T* __restrict__ W, long long ldW,
                                                          T* __restrict__ partials) {
	using M = Mfma16<T>;
	using Acc = typename M::Acc;
	static_assert(!SYM || TI == TJ, "the symmetric case is square");
	__shared__ T sums[4][TI * TJ * 4 * 64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int c = lane & 15, q = lane >> 4;
	Acc acc[TI][TJ];
#pragma unroll
	for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
		for (int tj = 0; tj < TJ; ++tj) acc[ti][tj] = Acc{T(0), T(0), T(0), T(0)};
	}
	const long long nmain = n / R * R;
	const long long chunk = 4 * R;  // rows of a wavefront's step
	const long long stride = static_cast<long long>(gridDim.x) * 4 * MG_U * chunk;
	for (long long base = (static_cast<long long>(blockIdx.x) * 4 + wave) * MG_U * chunk; base < nmain; base += stride) {  // (uniform over the wavefront)
		T a[TI][MG_U][R], b[SYM ? 1 : TJ][SYM ? 1 : MG_U][R];
#pragma unroll
		for (int u = 0; u < MG_U; ++u) {
			const long long row = base + u * chunk + q * R;
			const bool live = row < nmain;
#pragma unroll
			for (int ti = 0; ti < TI; ++ti) gramLoad<T, R>(V, ldV, m, ti * 16 + c, row, live, a[ti][u]);
			if constexpr (!SYM) {
#pragma unroll
				for (int tj = 0; tj < TJ; ++tj) gramLoad<T, R>(W, ldW, l, tj * 16 + c, row, live, b[tj][u]);
			}
		}
#pragma unroll
		for (int u = 0; u < MG_U; ++u) {
#pragma unroll
			for (int r = 0; r < R; ++r) {
#pragma unroll
				for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
					for (int tj = 0; tj < TJ; ++tj) {
						if constexpr (SYM) acc[ti][tj] = M::mma(a[ti][u][r], a[tj][u][r], acc[ti][tj]);
						else acc[ti][tj] = M::mma(a[ti][u][r], b[tj][u][r], acc[ti][tj]);
					}
				}
			}
		}
	}
	if (R > 1 && blockIdx.x == 0 && wave == 0 && nmain < n) {  // (uniform over the wavefront) the last n % R rows: one step, a row per q
		const long long row = nmain + q;
		const bool live = row < n;
		T a[TI][1], b[TJ][1];
#pragma unroll
		for (int ti = 0; ti < TI; ++ti) gramLoad<T, 1>(V, ldV, m, ti * 16 + c, row, live, a[ti]);
#pragma unroll
		for (int tj = 0; tj < TJ; ++tj) gramLoad<T, 1>(SYM ? V : W, SYM ? ldV : ldW, l, tj * 16 + c, row, live, b[tj]);
#pragma unroll
		for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
			for (int tj = 0; tj < TJ; ++tj) acc[ti][tj] = M::mma(a[ti][0], b[tj][0], acc[ti][tj]);
		}
	}
#pragma unroll
	for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
		for (int tj = 0; tj < TJ; ++tj) {
#pragma unroll
			for (int reg = 0; reg < 4; ++reg) sums[wave][((ti * TJ + tj) * 4 + reg) * 64 + lane] = acc[ti][tj][reg];
		}
	}
	__syncthreads();
	for (int e = threadIdx.x; e < TI * TJ * 4 * 64; e += MV_TPB) {
		const int tile = e >> 8, reg = (e >> 6) & 3, ln = e & 63;
		const int i = (tile / TJ) * 16 + M::row(ln, reg), j = (tile % TJ) * 16 + (ln & 15);
		if (i < m && j < l) partials[static_cast<long long>(i + j * m) * MG_NPART + blockIdx.x] = ((sums[0][e] + sums[1][e]) + sums[2][e]) + sums[3][e];
	}
}

// workgroup e = i + j m adds the nb partials of G[i][j] in the project's fixed order (t, t + 256, ...; then blockSum256)
template <typename T>
__global__ __launch_bounds__(MV_TPB) void multiGramFinish(const T* __restrict__ partials, int nb, int m, T* __restrict__ G, long long ldG) {
	__shared__ T red[4];
	const T* p = partials + static_cast<long long>(blockIdx.x) * MG_NPART;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += MV_TPB) acc += p[i];
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) G[blockIdx.x % m + static_cast<long long>(blockIdx.x / m) * ldG] = s;
}

template <typename T, int TI, int TJ, bool SYM>
inline void multiGramLaunchT(long long n, int m, int l, const T* V, long long ldV, const T* W, long long ldW, T* partials, T* G, long long ldG, hipStream_t s) {
	constexpr int N = Pack16<T>::N;
	const bool vec = ((reinterpret_cast<unsigned long long>(V) | reinterpret_cast<unsigned long long>(W)) & 15ull) == 0 && ldV % N == 0 && ldW % N == 0;
	const long long rowsPerGroup = 4ll * MG_U * 4 * (vec ? N : 1);
	const int g = static_cast<int>(std::max<long long>(1, std::min<long long>((n + rowsPerGroup - 1) / rowsPerGroup, MG_NPART)));
	if (vec) multiGramKernel<T, TI, TJ, SYM, N><<<g, MV_TPB, 0, s>>>(n, m, l, V, ldV, W, ldW, partials);
	else multiGramKernel<T, TI, TJ, SYM, 1><<<g, MV_TPB, 0, s>>>(n, m, l, V, ldV, W, ldW, partials);
	multiGramFinish<T><<<m * l, MV_TPB, 0, s>>>(partials, g, m, G, ldG);
}

// G (m x l, column-major, ldG >= m, device memory) = V^T W.  partials: MB_MAX * MB_MAX * MG_NPART elements.  1 <= m, l <= MB_MAX, n >= 1
// (the caller checks).
template <typename T>
inline void multiGramLaunch(long long n, int m, int l, const T* V, long long ldV, const T* W, long long ldW, T* partials, T* G, long long ldG, hipStream_t s) {
	const bool sym = V == W && m == l && ldV == ldW;
	const int ti = m > 16 ? 2 : 1, tj = l > 16 ? 2 : 1;
	if (sym && ti == 1) multiGramLaunchT<T, 1, 1, true>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
	else if (sym) multiGramLaunchT<T, 2, 2, true>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
	else if (ti == 1 && tj == 1) multiGramLaunchT<T, 1, 1, false>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
	else if (ti == 1) multiGramLaunchT<T, 1, 2, false>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
	else if (tj == 1) multiGramLaunchT<T, 2, 1, false>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
	else multiGramLaunchT<T, 2, 2, false>(n, m, l, V, ldV, W, ldW, partials, G, ldG, s);
}

// ---------------------------------------------------------------------------------------------------------
// multiBlockAxpy: W[:, c] = W[:, c] - sum_j H[j][c] V[:, j] for all c < l, j ascending, each term smmFma(-H[j][c], V_j, W_c).  Rows are
// independent: a lane loads the m values of its R rows of V once (as multiRotateKernel does) and then reads, updates and writes its
// rows of one column of W after the other.  n m elements of V read, n l of W read and written, none twice.  H (m x l, column-major,
// leading dimension ldH, DEVICE memory -- a Gram result feeds it with no host read in between) is staged in LDS once per workgroup and
// read from there at wave-uniform addresses.  The row lives in registers under static indices: MP is m rounded up to 8 / 16 / 24.
// ---------------------------------------------------------------------------------------------------------
template <typename T, int MP, int R>
__device__ __forceinline__ void multiBlockAxpyRows(const T* vrow, long long ldV, T* wrow, long long ldW, int m, int l, const T* Hs) {
	using P = typename Pack16<T>::V;
	static_assert(R == 1 || R == Pack16<T>::N, "one row per lane, or one 16-byte pack of rows");
	T v[MP][R];
#pragma unroll
	for (int j = 0; j < MP; ++j) {
		if (j < m) {  // (uniform)
			if constexpr (R == 1) {
				v[j][0] = vrow[j * ldV];
			} else {
				const P p = *reinterpret_cast<const P*>(vrow + j * ldV);
#pragma unroll
				for (int e = 0; e < R; ++e) v[j][e] = p[e];
			}
		} else {
#pragma unroll
			for (int e = 0; e < R; ++e) v[j][e] = T(0);
		}
	}
	for (int c = 0; c < l; ++c) {
		const T* h = Hs + c * MP;
		T acc[R];
		if constexpr (R == 1) {
			acc[0] = wrow[c * ldW];
		} else {
			const P p = *reinterpret_cast<const P*>(wrow + c * ldW);
#pragma unroll
			for (int e = 0; e < R; ++e) acc[e] = p[e];
		}
#pragma unroll
		for (int j = 0; j < MP; ++j) {
			if (j < m) {  // (uniform)
				const T hj = -h[j];
#pragma unroll
				for (int e = 0; e < R; ++e) acc[e] = smmFma(hj, v[j][e], acc[e]);
			}
		}
		if constexpr (R == 1) {
			wrow[c * ldW] = acc[0];
		} else {
			P p;
#pragma unroll
			for (int e = 0; e < R; ++e) p[e] = acc[e];
			*reinterpret_cast<P*>(wrow + c * ldW) = p;
		}
	}
}

// The rows of one workgroup.  R > 1 needs V and W 16-byte aligned and both leading dimensions multiples of R; the last n % R rows take one lane each.
template <typename T, int MP, int R>
__device__ __forceinline__ void multiBlockAxpyBody(long long n, int m, int l, const T* V, long long ldV, T* W, long long ldW, const T* Hs) {
	const long long packs = n / R;
	for (long long i = static_cast<long long>(blockIdx.x) * MV_TPB + threadIdx.x; i < packs; i += static_cast<long long>(gridDim.x) * MV_TPB) {
		multiBlockAxpyRows<T, MP, R>(V + i * R, ldV, W + i * R, ldW, m, l, Hs);
	}
	if (R > 1 && blockIdx.x == 0) {
		const long long i = packs * R + threadIdx.x;
		if (i < n) multiBlockAxpyRows<T, MP, 1>(V + i, ldV, W + i, ldW, m, l, Hs);
	}
}

template <typename T, int MP>
__device__ __forceinline__ void multiBlockAxpyStage(int m, int l, const T* __restrict__ H, long long ldH, T* Hs) {
	for (int i = threadIdx.x; i < MP * l; i += MV_TPB) {
		const int j = i % MP, c = i / MP;
		Hs[i] = j < m ? H[j + c * ldH] : T(0);
	}
	__syncthreads();
}

// R as multiBlockAxpyBody's: the launcher checks.
template <typename T, int MP, int R>
__global__ __launch_bounds__(MV_TPB) void multiBlockAxpyKernel(long long n, int m, int l, const T* __restrict__ V, long long ldV, const T* __restrict__ H, long long ldH,
                                                               T* __restrict__ W, long long ldW) {
	__shared__ T Hs[MP * MB_MAX];
	multiBlockAxpyStage<T, MP>(m, l, H, ldH, Hs);
	multiBlockAxpyBody<T, MP, R>(n, m, l, V, ldV, W, ldW, Hs);
}

// The same update of up to MV_MAX_BASES pairs (V_b, W_b) with ONE H in one launch: blockIdx.y is the pair, the pointers travel by value in
// the kernel arguments.  Every pair takes the 16-byte path or the element path by its OWN alignment (uniform over the workgroup), so each
// gets the bits of multiBlockAxpyKernel on it alone.
template <typename T, int MP>
__global__ __launch_bounds__(MV_TPB) void multiBlockAxpyBasesKernel(long long n, int m, int l, BasePtrs<const T> Vs, long long ldV, const T* __restrict__ H, long long ldH,
                                                                    BasePtrs<T> Ws, long long ldW) {
	constexpr int N = Pack16<T>::N;
	__shared__ T Hs[MP * MB_MAX];
	multiBlockAxpyStage<T, MP>(m, l, H, ldH, Hs);
	const T* V = Vs.at(blockIdx.y);
	T* W = Ws.at(blockIdx.y);
	if (aligned16(V) && aligned16(W) && ldV % N == 0 && ldW % N == 0) multiBlockAxpyBody<T, MP, N>(n, m, l, V, ldV, W, ldW, Hs);
	else multiBlockAxpyBody<T, MP, 1>(n, m, l, V, ldV, W, ldW, Hs);
}

template <typename T, int MP>
inline void multiBlockAxpyLaunchMP(long long n, int m, int l, const T* V, long long ldV, const T* H, long long ldH, T* W, long long ldW, hipStream_t s) {
	constexpr int N = Pack16<T>::N;
	const bool vec = ((reinterpret_cast<unsigned long long>(V) | reinterpret_cast<unsigned long long>(W)) & 15ull) == 0 && ldV % N == 0 && ldW % N == 0;
	const int g = rowLanesGrid<T>(n, vec);
	if (vec) multiBlockAxpyKernel<T, MP, N><<<g, MV_TPB, 0, s>>>(n, m, l, V, ldV, H, ldH, W, ldW);
	else multiBlockAxpyKernel<T, MP, 1><<<g, MV_TPB, 0, s>>>(n, m, l, V, ldV, H, ldH, W, ldW);
}

template <typename T, int MP>
inline void multiBlockAxpyBasesLaunchMP(long long n, int m, int l, int nb, const T* const* V, long long ldV, const T* H, long long ldH, T* const* W, long long ldW,
                                        hipStream_t s) {
	constexpr int N = Pack16<T>::N;
	BasePtrs<const T> vs;
	BasePtrs<T> ws;
	int g = 1;  // the widest any pair needs: the rows are walked by a grid-stride loop
	for (int b = 0; b < MV_MAX_BASES; ++b) {
		vs.p[b] = V[b < nb ? b : 0];
		ws.p[b] = W[b < nb ? b : 0];
		const bool vec = ((reinterpret_cast<unsigned long long>(vs.p[b]) | reinterpret_cast<unsigned long long>(ws.p[b])) & 15ull) == 0 && ldV % N == 0 && ldW % N == 0;
		g = std::max(g, rowLanesGrid<T>(n, vec));
	}
	multiBlockAxpyBasesKernel<T, MP><<<dim3(g, nb), MV_TPB, 0, s>>>(n, m, l, vs, ldV, H, ldH, ws, ldW);
}

// 1 <= m, l <= MB_MAX, n >= 1, V and W do not overlap (the caller checks).
template <typename T>
inline void multiBlockAxpyLaunch(long long n, int m, int l, const T* V, long long ldV, const T* H, long long ldH, T* W, long long ldW, hipStream_t s) {
	if (m <= 8) multiBlockAxpyLaunchMP<T, 8>(n, m, l, V, ldV, H, ldH, W, ldW, s);
	else if (m <= 16) multiBlockAxpyLaunchMP<T, 16>(n, m, l, V, ldV, H, ldH, W, ldW, s);
	else multiBlockAxpyLaunchMP<T, 24>(n, m, l, V, ldV, H, ldH, W, ldW, s);
}

// W_b -= V_b H for the pairs b < nb in ONE launch.  1 <= nb <= MV_MAX_BASES, otherwise as multiBlockAxpyLaunch; no V_b overlaps any W_c (the
// caller checks).
template <typename T>
inline void multiBlockAxpyBasesLaunch(long long n, int m, int l, int nb, const T* const* V, long long ldV, const T* H, long long ldH, T* const* W, long long ldW,
                                      hipStream_t s) {
	if (m <= 8) multiBlockAxpyBasesLaunchMP<T, 8>(n, m, l, nb, V, ldV, H, ldH, W, ldW, s);
	else if (m <= 16) multiBlockAxpyBasesLaunchMP<T, 16>(n, m, l, nb, V, ldV, H, ldH, W, ldW, s);
	else multiBlockAxpyBasesLaunchMP<T, 24>(n, m, l, nb, V, ldV, H, ldH, W, ldW, s);
}

}  // namespace smm
