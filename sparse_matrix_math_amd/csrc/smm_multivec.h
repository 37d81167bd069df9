// smm_multivec.h -- the tall-skinny kernels shared by the drivers that keep a block of columns on the device (smm_solvers_gmres.hip: the
// Krylov basis; smm_solvers_idrs.hip: G, U and the shadow space): all products of the columns with one vector from one pass, and one
// vector plus a combination of the columns.  Each unit that includes this instantiates its own copies.
#pragma once
#include <algorithm>

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

}  // namespace smm
