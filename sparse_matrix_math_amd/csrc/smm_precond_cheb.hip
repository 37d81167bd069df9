// smm_precond_cheb.hip -- Chebyshev polynomial preconditioner in D^-1 A on gfx950 (an addition, no counterpart in the reference).
//
// z = M^-1 r is the degree-d Chebyshev iteration for A z = r from z = 0, preconditioned by the stored diagonal D, on the interval
// [lmin, lmax] that is to hold the spectrum of D^-1 A (the definition, line by line, is tests/chebyshev_restatement.py):
//   theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma
//   rho_k = 1 / (2 sigma - rho_{k-1}), c1_k = rho_k rho_{k-1}, c2_k = 2 rho_k / delta              (double, on the host, cast to T once)
//   d = (r / diag) * T(1 / theta);  z = d
//   k = 1 .. degree:  q = r - A z  (the library's SpMV);  t = q / diag;  u = c2_k * t;  d = _smm_fma(c1_k, d, u);  z = z + d
// An apply is `degree` SpMVs and degree + 1 element-wise passes: no dependency chain between rows, no inner product, no host round
// trip.  The residual polynomial is T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma); M^-1 is symmetric positive definite when A is
// and the interval is right of 0, so ConjugateGradient may use it.
//
// The element-wise passes go through streamMap (smm_device.h: 16-byte accesses, a one-element tail) with the update kernels'
// non-temporal policy (updateNT).  Passes over a vector per step: the SpMV's 3 (r, z read, q written) and the step's 6 (q, diag, d, z
// read; d, z written; the last step of an apply does not write d: 5).  Forming the step inside the SpMV's epilogue would leave 6;
// DESIGN.md section 3.13.
#include <algorithm>
#include <cmath>
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

// scratch and scalars of one Chebyshev handle, behind the public handle
struct smm_precond_cheb {
	int degree = 0;
	int boundMode = SMM_CHEB_BOUND_GERSHGORIN;
	double lmin = 0, lmax = 0;
	double invTheta = 0;
	std::vector<double> c1, c2;  // [1 .. degree]
	// q = r - A z and the correction d of an apply in flight: ONE set per handle, so a handle serves one stream at a time
	void* q = nullptr;
	void* d = nullptr;
};

namespace smm {

constexpr int TPB = 256;

// Per row, one lane: the diagonal copied out (the first stored entry with column == row), the row's sum of |a_ij| in DOUBLE,
// sequentially, in stored order, divided by |a_ii| in double; the largest quotient over all rows lands in *lmaxBits (the bit pattern of
// a non-negative double orders like the unsigned integer, so the maximum needs no floating-point atomic and does not depend on how the
// rows are dealt to the lanes).  err |= 1: an empty row, a missing diagonal or |d| < 1e-5 (the Jacobi rule).
template <typename T>
__global__ __launch_bounds__(TPB) void chebGershgorinKernel(int rows, const int* __restrict__ start, const int* __restrict__ positions,
                                                            const T* __restrict__ vals, T* __restrict__ diag, unsigned long long* lmaxBits,
                                                            int* __restrict__ err) {
	unsigned long long top = 0ull;
	bool bad = false;
	for (long long row = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; row < rows; row += static_cast<long long>(gridDim.x) * TPB) {
		const int b = start[row], e = start[row + 1];
		bool found = false;
		T d = T(0);
		double sum = 0.0;
		for (int k = b; k < e; ++k) {
			const T v = vals[k];
			if (!found && positions[k] == row) {
				d = v;
				found = true;
			}
			sum += fabs(static_cast<double>(v));
		}
		diag[row] = d;
		if (e <= b || !found || (d < T(0) ? -d : d) < T(1e-5)) {
			bad = true;
		} else {
			const double ratio = sum / fabs(static_cast<double>(d));
			const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(ratio));
			top = bits > top ? bits : top;  // (a NaN or an Inf among the values wins the maximum: the host refuses the bound)
		}
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) {
		const unsigned long long other = __shfl_xor(top, o, WAVE);
		top = other > top ? other : top;
	}
	if ((threadIdx.x & (WAVE - 1)) == 0 && top != 0ull) atomicMax(lmaxBits, top);
	if (bad) atomicOr(err, 1);
}

// d = (r / diag) * invTheta ; z = d.  WRITE_D false (degree 0, a scaled Jacobi): z only.
template <typename T, bool NT, bool WRITE_D>
__device__ __forceinline__ void chebFirstBody(int n, T invTheta, const T* r, const T* diag, T* d, T* z) {
	const T* const in[2] = {r, diag};
	T* const out[2] = {z, d};
	streamMap<T, NT, 2, WRITE_D ? 2 : 1>(n, in, out, [&](const T(&v)[2], T(&o)[WRITE_D ? 2 : 1]) {
		const T t = v[0] / v[1];
		const T d0 = t * invTheta;
		o[0] = d0;
		if (WRITE_D) o[1] = d0;
	});
}
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void chebFirstKernel(int n, T invTheta, int writeD, const T* r, const T* diag, T* d, T* z,
                                                       const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	if (writeD) chebFirstBody<T, NT, true>(n, invTheta, r, diag, d, z);
	else chebFirstBody<T, NT, false>(n, invTheta, r, diag, d, z);
}

// t = q / diag ; u = c2 * t ; d = _smm_fma(c1, d, u) ; z = z + d.  The last step of an apply (writeD == 0) does not write d.
template <typename T, bool NT, bool WRITE_D>
__device__ __forceinline__ void chebStepBody(int n, T c1, T c2, const T* q, const T* diag, T* d, T* z) {
	const T* const in[4] = {q, diag, d, z};
	T* const out[2] = {z, d};
	streamMap<T, NT, 4, WRITE_D ? 2 : 1>(n, in, out, [&](const T(&v)[4], T(&o)[WRITE_D ? 2 : 1]) {
		const T t = v[0] / v[1];
		const T u = c2 * t;
		const T dk = smmFma(c1, v[2], u);
		o[0] = v[3] + dk;
		if (WRITE_D) o[1] = dk;
	});
}
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void chebStepKernel(int n, T c1, T c2, int writeD, const T* q, const T* diag, T* d, T* z,
                                                      const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	if (writeD) chebStepBody<T, NT, true>(n, c1, c2, q, diag, d, z);
	else chebStepBody<T, NT, false>(n, c1, c2, q, diag, d, z);
}

// the power method's vectors: v[i] = 1 + (i mod 7) / 8 (exact in both dtypes) ; v = w * scale
template <typename T>
__global__ __launch_bounds__(TPB) void chebPowerStartKernel(int n, T* __restrict__ v) {
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		v[i] = T(1) + static_cast<T>(i % 7) / T(8);
	}
}
template <typename T>
__global__ __launch_bounds__(TPB) void chebScaleKernel(int n, T scale, const T* w, T* v) {
	const T* const in[1] = {w};
	T* const out[1] = {v};
	streamMap<T, false, 1, 1>(n, in, out, [&](const T(&a)[1], T(&o)[1]) { o[0] = a[0] * scale; });
}

template <typename T>
int chebApplyDev(const smm_hip_precond* M, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_precond_cheb* C = M->cheb;
	if (!C) {
		setError("precond_apply: the Chebyshev preconditioner has no plan");
		return SMM_HIP_ERR_INVALID;
	}
	const int n = M->a->rows;
	const int g = solverGrid(n);
	const T* diag = static_cast<const T*>(M->d_values);
	T* q = static_cast<T*>(C->q);
	T* d = static_cast<T*>(C->d);
	const int degree = C->degree;
	std::lock_guard<std::mutex> whole(M->enqueueMutex);  // q and d are the handle's: one apply's launches stay together
	SMM_LAUNCH_UPDATE(chebFirstKernel, updateNT(n, sizeof(T), degree > 0 ? 4 : 3), g, s, n, static_cast<T>(C->invTheta), degree > 0 ? 1 : 0, rhs, diag, d, x, doneFlag);
	for (int k = 1; k <= degree; ++k) {
		SMM_TRY(launchSpmv<T>(M->a, SMM_OP_SUB, rhs, x, q, 0, nullptr, nullptr, doneFlag, s));  // q = r - A z
		const int writeD = k < degree ? 1 : 0;
		SMM_LAUNCH_UPDATE(chebStepKernel, updateNT(n, sizeof(T), writeD ? 6 : 5), g, s, n, static_cast<T>(C->c1[k]), static_cast<T>(C->c2[k]), writeD, q, diag, d, x,
		                  doneFlag);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template int chebApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int chebApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void chebDestroy(smm_precond_cheb* C) {
	if (!C) return;
	devFree(C->q);
	devFree(C->d);
	delete C;
}

// one device scalar a.b on the host (the dot kernels of the solvers; synchronises `s`)
template <typename T>
static int dotToHost(int n, const T* a, const T* b, T* parts, T* result, double* out, hipStream_t s) {
	SMM_TRY(launchDotPartials<T>(n, a, b, parts, nullptr, s));
	SMM_TRY(launchSumPartials<T>(parts, result, s));
	T h = T(0);
	SMM_HIP_TRY(hipMemcpyAsync(&h, result, sizeof(T), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	*out = static_cast<double>(h);
	return SMM_HIP_OK;
}

// `steps` steps of the power method on D^-1 A from the fixed start: w = (A v) / diag ; rq = (v.w) / (v.v) ; v = w * T(1 / sqrt(w.w)).
// *rq = the last Rayleigh quotient (the dot products in T, the quotient and the square root in double).
template <typename T>
static int powerRayleigh(const smm_hip_csr* a, const T* diag, int steps, double* rq, hipStream_t s) {
	const int n = a->rows;
	DevBuf<T> v, w, parts, result;
	SMM_TRY(v.alloc(n));
	SMM_TRY(w.alloc(n));
	SMM_TRY(parts.alloc(NPART));
	SMM_TRY(result.alloc(1));
	const int g = solverGrid(n);
	chebPowerStartKernel<T><<<g, TPB, 0, s>>>(n, v);
	*rq = 0.0;
	for (int k = 0; k < steps; ++k) {
		SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, diag, v, w, 0, nullptr, nullptr, nullptr, s, SPMV_DIV_LHS));
		double vw = 0, vv = 0, ww = 0;
		SMM_TRY(dotToHost<T>(n, v, w, parts, result, &vw, s));
		SMM_TRY(dotToHost<T>(n, v, v, parts, result, &vv, s));
		SMM_TRY(dotToHost<T>(n, w, w, parts, result, &ww, s));
		*rq = vw / vv;
		chebScaleKernel<T><<<g, TPB, 0, s>>>(n, static_cast<T>(1.0 / std::sqrt(ww)), w, v);
	}
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));  // the scratch vectors go back to the allocator when this scope ends
	return SMM_HIP_OK;
}

template <typename T>
int chebCreateTyped(const smm_hip_csr* a, int degree, int boundMode, double eigRatio, int powerSteps, double lmin, double lmax, smm_hip_precond* M) {
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());  // the matrix may still be being written on a caller's stream
	const int n = a->rows;
	auto* C = new smm_precond_cheb();
	M->cheb = C;  // (smm_hip_precond_destroy releases it together with whatever the steps below have allocated so far)
	C->degree = degree;
	C->boundMode = boundMode;
	const size_t len = static_cast<size_t>(std::max(1, n));
	SMM_TRY(devAlloc(&M->d_values, len * sizeof(T)));
	M->n_values = static_cast<size_t>(n);
	SMM_TRY(devAlloc(&C->q, len * sizeof(T)));
	SMM_TRY(devAlloc(&C->d, len * sizeof(T)));
	double gersh = 1.0;  // (no rows: the spectrum is empty and every interval holds it)
	if (n) {
		if (a->firstActiveStart != 0) {
			setError("chebyshev: matrix has leading empty rows");
			return SMM_HIP_ERR_PRECOND;
		}
		DevBuf<unsigned long long> top;
		DevBuf<int> err;
		SMM_TRY(top.alloc(1));
		SMM_TRY(err.alloc(1));
		SMM_HIP_TRY(hipMemsetAsync(top, 0, sizeof(unsigned long long), s));
		SMM_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int), s));
		const int grid = static_cast<int>(std::min<long long>((n + TPB - 1LL) / TPB, numCUs() * 8LL));
		chebGershgorinKernel<T><<<grid, TPB, 0, s>>>(n, a->d_start, a->d_positions, static_cast<const T*>(a->d_values), static_cast<T*>(M->d_values), top, err);
		SMM_HIP_TRY(hipGetLastError());
		int herr = 0;
		SMM_HIP_TRY(hipMemcpyAsync(&gersh, top, sizeof(double), hipMemcpyDeviceToHost, s));  // the one 8-byte read-back (the bits are the double's)
		SMM_HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (herr) {
			setError("chebyshev: empty row, missing diagonal or |d|<1e-5");
			return SMM_HIP_ERR_PRECOND;
		}
	}
	if (boundMode != SMM_CHEB_BOUND_USER) {
		lmax = gersh;
		if (boundMode == SMM_CHEB_BOUND_POWER && n) {
			double rq = 0.0;
			SMM_TRY(powerRayleigh<T>(a, static_cast<const T*>(M->d_values), powerSteps, &rq, s));
			if (!std::isfinite(rq)) {
				setError("chebyshev: the power method's Rayleigh quotient is not finite");
				return SMM_HIP_ERR_PRECOND;
			}
			lmax = std::min(gersh, 1.1 * rq);
		}
		lmin = lmax / eigRatio;
	}
	if (!std::isfinite(lmin) || !std::isfinite(lmax) || !(lmin > 0.0) || !(lmin < lmax)) {
		setError("chebyshev: the bounds must be finite with 0 < lambda_min < lambda_max (got %g, %g)", lmin, lmax);
		return SMM_HIP_ERR_PRECOND;
	}
	C->lmin = lmin;
	C->lmax = lmax;
	const double theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta;
	C->invTheta = 1.0 / theta;
	C->c1.assign(static_cast<size_t>(degree) + 1, 0.0);
	C->c2.assign(static_cast<size_t>(degree) + 1, 0.0);
	double rho = 1.0 / sigma;
	for (int k = 1; k <= degree; ++k) {
		const double next = 1.0 / (2.0 * sigma - rho);
		C->c1[k] = next * rho;
		C->c2[k] = 2.0 * next / delta;
		rho = next;
	}
	return SMM_HIP_OK;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_precond_create_chebyshev(const smm_hip_csr* a, int degree, int bound_mode, double eig_ratio, int power_steps, double lambda_min, double lambda_max,
                                     smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_chebyshev: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (degree < 0 || degree > SMM_CHEB_MAX_DEGREE) {
		setError("precond_create_chebyshev: degree must be 0 .. %d", SMM_CHEB_MAX_DEGREE);
		return SMM_HIP_ERR_INVALID;
	}
	if (bound_mode < SMM_CHEB_BOUND_GERSHGORIN || bound_mode > SMM_CHEB_BOUND_USER) {
		setError("precond_create_chebyshev: bound_mode must be SMM_CHEB_BOUND_GERSHGORIN, _POWER or _USER");
		return SMM_HIP_ERR_INVALID;
	}
	if (bound_mode == SMM_CHEB_BOUND_POWER && (power_steps < 1 || power_steps > 1000)) {
		setError("precond_create_chebyshev: power_steps must be 1 .. 1000");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("preconditioner needs a square matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (bound_mode != SMM_CHEB_BOUND_USER && !(eig_ratio > 1.0 && std::isfinite(eig_ratio))) {
		setError("precond_create_chebyshev: eig_ratio must be finite and > 1");
		return SMM_HIP_ERR_PRECOND;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));  // a set-up call without a stream: drains the device once
	auto* M = new smm_hip_precond();
	M->kind = SMM_PRECOND_CHEBYSHEV;
	M->dtype = a->dtype;
	M->a = a;
	const int st = a->dtype == SMM_DTYPE_F32 ? chebCreateTyped<float>(a, degree, bound_mode, eig_ratio, power_steps, lambda_min, lambda_max, M)
	                                         : chebCreateTyped<double>(a, degree, bound_mode, eig_ratio, power_steps, lambda_min, lambda_max, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

int smm_hip_precond_chebyshev_info(const smm_hip_precond* M, int* degree, int* bound_mode, double* lambda_min, double* lambda_max) {
	if (!M || M->kind != SMM_PRECOND_CHEBYSHEV || !M->cheb) {
		setError("precond_chebyshev_info: not a Chebyshev preconditioner");
		return SMM_HIP_ERR_INVALID;
	}
	if (degree) *degree = M->cheb->degree;
	if (bound_mode) *bound_mode = M->cheb->boundMode;
	if (lambda_min) *lambda_min = M->cheb->lmin;
	if (lambda_max) *lambda_max = M->cheb->lmax;
	return SMM_HIP_OK;
}

}  // extern "C"
