// smm_solver_scal.h -- the recurrence scalars of the device-resident Krylov loops and the fixed-order sums of their partials: shared by the
// steps of the CG and BiCGStab loops (smm_krylov_steps.h; their kernels are in smm_solvers.hip and smm_dist.hip), the other solver units and
// the SpMV kernel that forms CG's next direction in its own load phase (smm_spmv_march.hip).
#pragma once
#include "smm_device.h"
#include "smm_internal.h"

namespace smm {

constexpr int SCAL_TPB = 256;
// ConjugateGradient with the deferred x update (smm_krylov_steps.h cgLazyStep): directions kept before x is brought up to date
constexpr int LAZY_M = 8;

template <typename T>
struct Scal {
	T rr;       // CG: residualNormSquared / rz for PCG ; BiCGStab: rr0
	T denom;    // p.Ap / ap.r0
	T alpha;
	T beta;
	T omega;
	T res;      // CG: last ||r||^2 ; BiCGStab: last ||r||
	T rrPing[2];  // fused loops: rr (CG) / rr0 (BiCGStab) double-buffered by iteration parity
	T alphaRing[LAZY_M];  // CG with the deferred x update: alpha of the last LAZY_M iterations
	int done;
	int iters;
	int status;
	int pad;
	int flushIter;  // CG, deferred x update: the iteration whose SpMV launch found its predecessor converged (-1: none): that iteration's flush launch completes x
	int pad2;
};

template <typename T>
__device__ __forceinline__ T sumParts(const T* __restrict__ partials, T* red) {
	T acc = T(0);
	for (int i = threadIdx.x; i < NPART; i += SCAL_TPB) acc += partials[i];
	return blockSum256(acc, red);
}

template <typename T>
__device__ __forceinline__ T sumPartsAll(const T* __restrict__ partials, T* red5) {
	const T s = sumParts(partials, red5);
	if (threadIdx.x == 0) red5[4] = s;
	__syncthreads();
	const T v = red5[4];
	__syncthreads();
	return v;
}

// the correctly rounded square root of the residual norm (ref:2268)
template <typename T>
__device__ __forceinline__ T sqrtRn(T v) {
	return sizeof(T) == 4 ? static_cast<T>(__fsqrt_rn(static_cast<float>(v))) : static_cast<T>(__dsqrt_rn(static_cast<double>(v)));
}

// the start of BiCGStab (ref:2231) and of ConjugateGradientSquared (ref:2128): rr0 = r.r0 ; iterations = 0 (one workgroup)
template <typename T>
__global__ __launch_bounds__(SCAL_TPB) void rr0InitScal(const T* __restrict__ partials, Scal<T>* sc) {
	__shared__ T red[4];
	const T rr0 = sumParts(partials, red);
	if (threadIdx.x == 0) {
		sc->rr = rr0;
		sc->rrPing[0] = rr0;
		sc->res = T(0);
		sc->iters = 0;
		sc->done = 0;
		sc->status = SMM_SOLVER_SUCCESS;
	}
}

// launches an update kernel templated on <T, NT> with the cache policy updateNT chose (T and TPB are those of the unit that expands it)
#define SMM_LAUNCH_UPDATE(KERNEL, NTFLAG, GRID, STREAM, ...)                    \
	do {                                                                       \
		if (NTFLAG) KERNEL<T, true><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); \
		else KERNEL<T, false><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__);       \
	} while (0)

}  // namespace smm
