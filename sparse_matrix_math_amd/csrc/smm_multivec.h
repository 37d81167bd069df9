// smm_multivec.h -- what the five drivers that keep a block of columns on the device share (smm_solvers_gmres.hip: the Krylov basis;
// smm_solvers_idrs.hip: G, U and the shadow space; smm_solvers_eigsh.hip and smm_solvers_svds.hip: the Lanczos bases; smm_solvers_lobpcg.hip:
// the start block).  The tall-skinny kernels: all products of the columns with one vector from one pass (multiDot), one vector plus a
// combination of the columns (multiAxpy), the columns times a small matrix in place (multiRotate).  And what every such basis is built
// with: the hash column, classical Gram-Schmidt applied twice, the division by the norm and by a device scalar, the staging of
// multiRotate's operand.  Each unit that includes this instantiates its own copies.
#pragma once
#include <algorithm>
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"

namespace smm {

constexpr int MV_TPB = 256;
// multiDot: columns whose accumulators a lane holds at a time, and 16-byte packs of w it holds across them (fp64 keeps
// MD_C * MV_U packs of V in flight in 64 VGPRs and stays under 128 VGPRs, the limit for four waves per SIMD)
constexpr int MD_C = 8;
constexpr int MV_U = 2;
// multiAxpy: columns loaded before the first of them is consumed
constexpr int MA_C = 4;

template <typename T>
__device__ __forceinline__ bool aligned16(const T* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// partials[i * NPART + block] = this workgroup's share of v_i . w, i < k; w's elements stay in registers across the MD_C columns of a chunk.
// A V or w that is only element-aligned (or a leading dimension that breaks the columns' alignment) takes one element per lane.
template <typename T>
__global__ __launch_bounds__(MV_TPB) void multiDotKernel(long long n, int k, const T* __restrict__ V, long long ld, const T* __restrict__ w, T* __restrict__ partials,
                                                         const int* __restrict__ flag) {
	using P = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	__shared__ T red[4];
	if (flag && *flag) return;
	const bool vec = aligned16(V) && aligned16(w) && ld % N == 0;
	const long long nvec = vec ? n / N : 0;
	const long long tile = static_cast<long long>(MV_U) * MV_TPB;
	for (int c0 = 0; c0 < k; c0 += MD_C) {
		T acc[MD_C];
		const T* colp[MD_C];
#pragma unroll
		for (int c = 0; c < MD_C; ++c) {
			acc[c] = T(0);
			colp[c] = V + static_cast<long long>(min(c0 + c, k - 1)) * ld;  // (a short last chunk re-reads the last column; those sums are dropped)
		}
		for (long long base = static_cast<long long>(blockIdx.x) * tile; base < nvec; base += static_cast<long long>(gridDim.x) * tile) {
			P wv[MV_U];
			P vv[MD_C][MV_U];
			bool live[MV_U];
#pragma unroll
			for (int u = 0; u < MV_U; ++u) {
				const long long i = base + u * MV_TPB + threadIdx.x;
				live[u] = i < nvec;
				const long long li = live[u] ? i : nvec - 1;
				wv[u] = reinterpret_cast<const P*>(w)[li];
#pragma unroll
				for (int c = 0; c < MD_C; ++c) vv[c][u] = reinterpret_cast<const P*>(colp[c])[li];
			}
#pragma unroll
			for (int u = 0; u < MV_U; ++u) {
				if (live[u]) {
#pragma unroll
					for (int c = 0; c < MD_C; ++c) {
#pragma unroll
						for (int e = 0; e < N; ++e) acc[c] += wv[u][e] * vv[c][u][e];
					}
				}
			}
		}
		for (long long i = nvec * N + static_cast<long long>(blockIdx.x) * MV_TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * MV_TPB) {
			const T wi = w[i];
#pragma unroll
			for (int c = 0; c < MD_C; ++c) acc[c] += wi * colp[c][i];
		}
#pragma unroll
		for (int c = 0; c < MD_C; ++c) {
			if (c0 + c < k) {  // (uniform over the workgroup)
				const T s = blockSum256(acc[c], red);
				if (threadIdx.x == 0) partials[static_cast<long long>(c0 + c) * NPART + blockIdx.x] = s;
			}
		}
	}
}

// workgroup i adds the nb partials of column i in the project's fixed order (i = t, t + 256, ...; then blockSum256)
template <typename T>
__global__ __launch_bounds__(MV_TPB) void multiDotFinish(const T* __restrict__ partials, int nb, T* __restrict__ out, T* __restrict__ negOut, const int* __restrict__ flag) {
	__shared__ T red[4];
	if (flag && *flag) return;
	const T* p = partials + static_cast<long long>(blockIdx.x) * NPART;
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += MV_TPB) acc += p[i];
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) {
		out[blockIdx.x] = s;
		if (negOut) negOut[blockIdx.x] = -s;
	}
}

// out = w + sum_i coef_i v_i, i ascending, smmFma nesting; w == nullptr: out = coef_0 v_0 + ..., starting from the plain product.  out may
// alias w.  kDev (may be null): the column count in device memory; no column and no w: nothing is written.  WW: the partial sums of
// out . out go to wwParts[block].
template <typename T, bool WW>
__global__ __launch_bounds__(MV_TPB) void multiAxpyKernel(long long n, int k, const int* __restrict__ kDev, const T* V, long long ld, const T* __restrict__ coef, const T* w,
                                                       T* out, T* __restrict__ wwParts, const int* __restrict__ flag) {
	using P = typename Pack16<T>::V;
	constexpr int N = Pack16<T>::N;
	__shared__ T red[4];
	if (flag && *flag) return;
	if (kDev) k = *kDev;
	if (k <= 0 && !w) return;
	const bool vec = aligned16(V) && (!w || aligned16(w)) && aligned16(out) && ld % N == 0;
	const long long nvec = vec ? n / N : 0;
	const long long tile = static_cast<long long>(MV_U) * MV_TPB;
	const int first = w ? 0 : 1;
	T ww = T(0);
	for (long long base = static_cast<long long>(blockIdx.x) * tile; base < nvec; base += static_cast<long long>(gridDim.x) * tile) {
		P acc[MV_U];
		long long li[MV_U];
		bool live[MV_U];
#pragma unroll
		for (int u = 0; u < MV_U; ++u) {
			const long long i = base + u * MV_TPB + threadIdx.x;
			live[u] = i < nvec;
			li[u] = live[u] ? i : nvec - 1;
			if (w) {
				acc[u] = reinterpret_cast<const P*>(w)[li[u]];
			} else {
				const P v0 = reinterpret_cast<const P*>(V)[li[u]];
				const T c0 = coef[0];
#pragma unroll
				for (int e = 0; e < N; ++e) acc[u][e] = c0 * v0[e];
			}
		}
		for (int c0 = first; c0 < k; c0 += MA_C) {
			P vv[MA_C][MV_U];
			T cf[MA_C];
#pragma unroll
			for (int c = 0; c < MA_C; ++c) {
				const int col = min(c0 + c, k - 1);
				cf[c] = coef[col];
#pragma unroll
				for (int u = 0; u < MV_U; ++u) vv[c][u] = reinterpret_cast<const P*>(V + static_cast<long long>(col) * ld)[li[u]];
			}
#pragma unroll
			for (int c = 0; c < MA_C; ++c) {
				if (c0 + c < k) {
#pragma unroll
					for (int u = 0; u < MV_U; ++u) {
#pragma unroll
						for (int e = 0; e < N; ++e) acc[u][e] = smmFma(cf[c], vv[c][u][e], acc[u][e]);
					}
				}
			}
		}
#pragma unroll
		for (int u = 0; u < MV_U; ++u) {
			if (live[u]) {
				reinterpret_cast<P*>(out)[li[u]] = acc[u];
				if (WW) {
#pragma unroll
					for (int e = 0; e < N; ++e) ww += acc[u][e] * acc[u][e];
				}
			}
		}
	}
	for (long long i = nvec * N + static_cast<long long>(blockIdx.x) * MV_TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * MV_TPB) {
		T acc = w ? w[i] : coef[0] * V[i];
		for (int c = first; c < k; ++c) acc = smmFma(coef[c], V[static_cast<long long>(c) * ld + i], acc);
		out[i] = acc;
		if (WW) ww += acc * acc;
	}
	if (WW) {
		const T s = blockSum256(ww, red);
		if (threadIdx.x == 0) wwParts[blockIdx.x] = s;
	}
}

inline int gridMV(long long n, size_t elemBytes) {
	const long long tile = static_cast<long long>(MV_TPB) * MV_U * (16 / static_cast<long long>(elemBytes));
	return static_cast<int>(std::max<long long>(1, std::min<long long>((n + tile - 1) / tile, NPART)));
}

// w (n elements, a column of Q or a vector of its own) against the first c columns of Q, classical Gram-Schmidt applied twice, with the
// partial sums of w . w left in parts1 (gmv of them).  Six launches: multiDot + finish + multiAxpy, twice; the products of the two passes
// go to h1 and h2 (which may be one array), their negatives to coef.  c == 0: the last launch alone, which copies nothing and leaves w . w.
// parts: c * NPART elements.  `flag` (may be null) guards every launch.
template <typename T>
inline void orthogonaliseTwice(const T* Q, long long ld, int n, int gmv, int c, T* w, T* parts, T* parts1, T* h1, T* h2, T* coef, const int* flag, hipStream_t s) {
	if (c > 0) {
		multiDotKernel<T><<<gmv, MV_TPB, 0, s>>>(n, c, Q, ld, w, parts, flag);
		multiDotFinish<T><<<c, MV_TPB, 0, s>>>(parts, gmv, h1, coef, flag);
		multiAxpyKernel<T, false><<<gmv, MV_TPB, 0, s>>>(n, c, nullptr, Q, ld, coef, w, w, nullptr, flag);
		multiDotKernel<T><<<gmv, MV_TPB, 0, s>>>(n, c, Q, ld, w, parts, flag);
		multiDotFinish<T><<<c, MV_TPB, 0, s>>>(parts, gmv, h2, coef, flag);
	}
	multiAxpyKernel<T, true><<<gmv, MV_TPB, 0, s>>>(n, c, nullptr, Q, ld, coef, w, w, parts1, flag);
}

__host__ __device__ inline unsigned long long splitmix64(unsigned long long z) {
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// The hash columns (IDR(s)'s shadow space, the start vectors of eigsh, svds and lobpcg): column blockIdx.y of the launch, at
// X + blockIdx.y * ld, is column col = firstCol + blockIdx.y of the hash.  Its element `row` is ((h >> 40) + 0.5) 2^-23 - 1 with
// h = splitmix64(splitmix64(splitmix64(seed) ^ col) ^ row): an odd multiple of 2^-24 inside (-1, 1), formed from the integer so that it
// is exact in fp32 too.
template <typename T>
__global__ __launch_bounds__(MV_TPB) void hashFillKernel(long long n, unsigned long long seed, unsigned long long firstCol, T* X, long long ld) {
	const unsigned long long hc = splitmix64(splitmix64(seed) ^ (firstCol + blockIdx.y));
	T* col = X + static_cast<long long>(blockIdx.y) * ld;
	for (long long i = static_cast<long long>(blockIdx.x) * MV_TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * MV_TPB) {
		const unsigned long long h = splitmix64(hc ^ static_cast<unsigned long long>(i));
		const int m = 2 * static_cast<int>(h >> 40) + 1 - (1 << 24);
		col[i] = static_cast<T>(m) * T(1.0 / 16777216.0);
	}
}

// v = v / sqrt(v . v), the nb partial sums of v . v added by every workgroup in the project's fixed order.  `bad` and `done` (each may
// be null): a norm that is zero or not finite raises those given and divides nothing -- every workgroup comes to the same verdict.  With
// neither there is no verdict: the division happens whatever the norm is.
template <typename T>
__global__ __launch_bounds__(MV_TPB) void normaliseKernel(long long n, T* v, const T* __restrict__ wwParts, int nb, int* bad, int* done) {
	__shared__ T red[5];
	T acc = T(0);
	for (int i = threadIdx.x; i < nb; i += MV_TPB) acc += wwParts[i];
	const T ww = blockSum256(acc, red);
	if (threadIdx.x == 0) red[4] = sqrt(ww);
	__syncthreads();
	const T d = red[4];
	if ((bad || done) && (!(d > T(0)) || !isfinite(d))) {
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			if (bad) *bad = 1;
			if (done) *done = 1;
		}
		return;
	}
	const T* const in[1] = {v};
	T* const out[1] = {v};
	streamMap<T, false, 1, 1>(n, in, out, [&](const T(&e)[1], T(&o)[1]) { o[0] = e[0] / d; });
}

// out = in / *divisor unless *flag (v_0 = r / beta, v_{j+1} = w / beta_j): a division, as the definitions say
template <typename T>
__global__ __launch_bounds__(MV_TPB) void scaleKernel(int n, const T* __restrict__ divisor, const T* in, T* out, const int* __restrict__ flag) {
	if (*flag) return;
	const T d = *divisor;
	const T* const i1[1] = {in};
	T* const o1[1] = {out};
	streamMap<T, false, 1, 1>(n, i1, o1, [&](const T(&v)[1], T(&o)[1]) { o[0] = v[0] / d; });
}

// multiRotate: V[:, 0..l-1] = V[:, 0..m-1] Y in place (smm_solvers_eigsh.hip: a Lanczos basis compressed onto its Ritz vectors).  Rows are
// independent: a lane loads the m values of its R rows (R consecutive rows: one load of R elements per column), forms the l outputs one
// after the other -- j ascending, smmFma nesting, from the plain product of column 0 -- and stores each as it is formed: the lane holds its
// whole row by then, so writing column c over a column that was read is safe.  n m elements read, n l written, none twice.
// The row lives in registers under static indices: MP is m rounded up to 16 / 32 / 64, the columns m .. MP-1 are not loaded (zeros stand
// in for them) and Y's rows m .. MP-1 are zero.  Y (MP x l, column-major, leading dimension MP) is staged in LDS once per workgroup and
// read from there at wave-uniform addresses.  MR_MAX_HELD: the row values a lane may hold, in 32-bit registers -- 128 of the 512 a SIMD
// lane has, so that with the accumulators and addresses three waves per SIMD stay resident.
constexpr int MR_MAX = 64;
constexpr int MR_MAX_HELD = 128;

template <typename T, int MP, int R>
__device__ __forceinline__ void multiRotateRows(T* row, long long ld, int m, int l, const T* Ys) {
	using P = typename Pack16<T>::V;
	static_assert(R == 1 || R == Pack16<T>::N, "one row per lane, or one 16-byte pack of rows");
	T v[MP][R];
#pragma unroll
	for (int j = 0; j < MP; ++j) {
		if (j < m) {  // (uniform)
			if constexpr (R == 1) {
				v[j][0] = row[j * ld];
			} else {
				const P p = *reinterpret_cast<const P*>(row + j * ld);
#pragma unroll
				for (int e = 0; e < R; ++e) v[j][e] = p[e];
			}
		} else {
#pragma unroll
			for (int e = 0; e < R; ++e) v[j][e] = T(0);
		}
	}
	for (int c = 0; c < l; ++c) {
		const T* y = Ys + c * MP;
		T acc[R];
#pragma unroll
		for (int e = 0; e < R; ++e) acc[e] = y[0] * v[0][e];
#pragma unroll
		for (int j = 1; j < MP; ++j) {
			const T yj = y[j];
#pragma unroll
			for (int e = 0; e < R; ++e) acc[e] = smmFma(yj, v[j][e], acc[e]);
		}
		if constexpr (R == 1) {
			row[c * ld] = acc[0];
		} else {
			P p;
#pragma unroll
			for (int e = 0; e < R; ++e) p[e] = acc[e];
			*reinterpret_cast<P*>(row + c * ld) = p;
		}
	}
}

// The rows of one workgroup.  R > 1 needs V 16-byte aligned and ld a multiple of R; the last n % R rows take one lane each.
template <typename T, int MP, int R>
__device__ __forceinline__ void multiRotateBody(long long n, int m, int l, T* V, long long ld, const T* Ys) {
	const long long packs = n / R;
	for (long long i = static_cast<long long>(blockIdx.x) * MV_TPB + threadIdx.x; i < packs; i += static_cast<long long>(gridDim.x) * MV_TPB) {
		multiRotateRows<T, MP, R>(V + i * R, ld, m, l, Ys);
	}
	if (R > 1 && blockIdx.x == 0) {
		const long long i = packs * R + threadIdx.x;
		if (i < n) multiRotateRows<T, MP, 1>(V + i, ld, m, l, Ys);
	}
}

// R as multiRotateBody's: the launcher checks.
template <typename T, int MP, int R>
__global__ __launch_bounds__(MV_TPB) void multiRotateKernel(long long n, int m, int l, T* V, long long ld, const T* __restrict__ Y) {
	__shared__ T Ys[MP * MP];
	for (int i = threadIdx.x; i < MP * l; i += MV_TPB) Ys[i] = Y[i];
	__syncthreads();
	multiRotateBody<T, MP, R>(n, m, l, V, ld, Ys);
}

// Up to MV_MAX_BASES bases that one launch of a row-per-lane kernel works on (smm_solvers_lobpcg.hip: S, AS and BS take the same small
// matrix).  The pointers travel BY VALUE in the kernel arguments; blockIdx.y picks one by comparisons, so the array is never indexed by
// a run-time value and stays in scalar registers.
constexpr int MV_MAX_BASES = SMM_LOBPCG_MAX_BASES;
static_assert(MV_MAX_BASES == 3, "BasePtrs::at picks among three");
template <typename T>
struct BasePtrs {
	T* p[MV_MAX_BASES];
	__device__ __forceinline__ T* at(unsigned b) const { return b == 0 ? p[0] : b == 1 ? p[1] : p[2]; }
};

// a pack of rows per lane only where its values fit the budget
template <typename T, int MP>
constexpr bool multiRotateFits = MP * Pack16<T>::N * static_cast<int>(sizeof(T) / 4) <= MR_MAX_HELD;

// multiRotateKernel on the bases b < gridDim.y with ONE Y in one launch.  Every basis takes the 16-byte path or the element path by its
// OWN alignment (uniform over the workgroup), so each gets the bits of multiRotateKernel on it alone.
template <typename T, int MP>
__global__ __launch_bounds__(MV_TPB) void multiRotateBasesKernel(long long n, int m, int l, BasePtrs<T> Vs, long long ld, const T* __restrict__ Y) {
	constexpr int N = Pack16<T>::N;
	__shared__ T Ys[MP * MP];
	for (int i = threadIdx.x; i < MP * l; i += MV_TPB) Ys[i] = Y[i];
	__syncthreads();
	T* V = Vs.at(blockIdx.y);
	if constexpr (multiRotateFits<T, MP>) {
		if (aligned16(V) && ld % N == 0) {
			multiRotateBody<T, MP, N>(n, m, l, V, ld, Ys);
			return;
		}
	}
	multiRotateBody<T, MP, 1>(n, m, l, V, ld, Ys);
}

// workgroups of a row-per-lane launch over n rows: a lane owns one row, or one 16-byte pack of rows
template <typename T>
inline int rowLanesGrid(long long n, bool vec) {
	constexpr int N = Pack16<T>::N;
	const long long lanes = vec ? (n / N > 0 ? n / N : 1) : n;
	return static_cast<int>(std::max<long long>(1, std::min<long long>((lanes + MV_TPB - 1) / MV_TPB, 4 * NPART)));
}

template <typename T, int MP>
inline void multiRotateLaunchMP(long long n, int m, int l, T* V, long long ld, const T* dY, hipStream_t s) {
	constexpr int N = Pack16<T>::N;
	constexpr bool fits = multiRotateFits<T, MP>;
	const bool vec = fits && (reinterpret_cast<unsigned long long>(V) & 15ull) == 0 && ld % N == 0;
	const int g = rowLanesGrid<T>(n, vec);
	if constexpr (fits) {
		if (vec) {
			multiRotateKernel<T, MP, N><<<g, MV_TPB, 0, s>>>(n, m, l, V, ld, dY);
			return;
		}
	}
	multiRotateKernel<T, MP, 1><<<g, MV_TPB, 0, s>>>(n, m, l, V, ld, dY);
}

template <typename T, int MP>
inline void multiRotateBasesLaunchMP(long long n, int m, int l, int nb, T* const* V, long long ld, const T* dY, hipStream_t s) {
	constexpr int N = Pack16<T>::N;
	BasePtrs<T> vs;
	int g = 1;  // the widest any basis needs: the rows are walked by a grid-stride loop
	for (int b = 0; b < MV_MAX_BASES; ++b) {
		vs.p[b] = V[b < nb ? b : 0];
		const bool vec = multiRotateFits<T, MP> && (reinterpret_cast<unsigned long long>(vs.p[b]) & 15ull) == 0 && ld % N == 0;
		g = std::max(g, rowLanesGrid<T>(n, vec));
	}
	multiRotateBasesKernel<T, MP><<<dim3(g, nb), MV_TPB, 0, s>>>(n, m, l, vs, ld, dY);
}

inline int multiRotatePad(int m) { return m <= 16 ? 16 : m <= 32 ? 32 : MR_MAX; }

// `count` columns of the host's mat (m rows, row-major with `stride` columns; column pick[c] goes to position c, column c itself with no
// pick) as multiRotate's operand at d: multiRotatePad(m) x count, column-major, zero rows below row m, in T.  `h` is the caller's staging
// array: it lives until the stream is next synchronised.
template <typename T>
inline int stageRotation(int m, int stride, int count, const std::vector<double>& mat, const int* pick, std::vector<T>& h, T* d, hipStream_t s) {
	const int MP = multiRotatePad(m);
	h.assign(static_cast<size_t>(MP) * count, T(0));
	for (int c = 0; c < count; ++c) {
		for (int r = 0; r < m; ++r) h[static_cast<size_t>(c) * MP + r] = static_cast<T>(mat[r * stride + (pick ? pick[c] : c)]);
	}
	return hostToDev(d, h.data(), sizeof(T) * h.size(), s);
}

// dY: multiRotatePad(m) x l, column-major, zero rows below row m.  1 <= l <= m <= MR_MAX, n > 0 (the caller checks).
template <typename T>
inline void multiRotateLaunch(long long n, int m, int l, T* V, long long ld, const T* dY, hipStream_t s) {
	switch (multiRotatePad(m)) {
		case 16: multiRotateLaunchMP<T, 16>(n, m, l, V, ld, dY, s); break;
		case 32: multiRotateLaunchMP<T, 32>(n, m, l, V, ld, dY, s); break;
		default: multiRotateLaunchMP<T, 64>(n, m, l, V, ld, dY, s); break;
	}
}

// V_b[:, 0..l-1] = V_b[:, 0..m-1] Y for the bases b < nb in ONE launch.  1 <= nb <= MV_MAX_BASES, otherwise as multiRotateLaunch.
template <typename T>
inline void multiRotateBasesLaunch(long long n, int m, int l, int nb, T* const* V, long long ld, const T* dY, hipStream_t s) {
	switch (multiRotatePad(m)) {
		case 16: multiRotateBasesLaunchMP<T, 16>(n, m, l, nb, V, ld, dY, s); break;
		case 32: multiRotateBasesLaunchMP<T, 32>(n, m, l, nb, V, ld, dY, s); break;
		default: multiRotateBasesLaunchMP<T, 64>(n, m, l, nb, V, ld, dY, s); break;
	}
}

}  // namespace smm
