// smm_solvers_refine.hip -- mixed-precision iterative refinement: an fp64 answer from fp32 solves (include/smm_hip.h states the loop;
// tests/refine_restatement.py is its definition).  The outer loop is fp64 and runs on the host frame of the Krylov drivers
// (smm_solver_host.h); the inner solve is one of the library's fp32 drivers, called as any caller would call it.
//
// An outer step is
//   1. refineDemote:    r32 = (float)(r 2^-e), d32 = 0           8 n read, 8 n written
//   2. the inner solve  A32 d32 = r32                            (smm_hip_cg_dev_f32 / bicgstab / gmres: it synchronises the stream)
//   3. refineCandidate: xc = fma(2^e, (double)d32, x)            12 n read, 8 n written
//   4. r = b - A xc (the fp64 handle's SpMV), r.r (partials, sum), the sum to the host through the watch's mailbox
//   5. accepted: x = xc                                          8 n read, 8 n written
// r is dead once it has been demoted, so the candidate's residual is formed in r itself: two fp64 vectors (r, xc) and two fp32 ones
// (r32, d32).  2^-e and 2^e are powers of two that travel by value: both products are exact, each line rounds once, and fma or a*x+b
// give the candidate the same bits (the SMM_WITH_STD_FMA flavour changes nothing here).
// x is written in step 5 only: a rejected candidate, an error of the inner driver or a failed launch leaves it bit for bit.
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"

namespace smm {
namespace {

constexpr int RTPB = 256;
constexpr int RPACK = 4;  // elements per lane and step: one 16-byte access per fp32 vector, two per fp64 vector

typedef float ref_f32x4 __attribute__((ext_vector_type(4)));
typedef double ref_f64x2 __attribute__((ext_vector_type(2)));

// r32[i] = (float)(r[i] * scale), d32[i] = 0.  The three vectors are the driver's own (16-byte aligned); n % 4 elements one per lane.
__global__ __launch_bounds__(RTPB) void refineDemoteKernel(int n, double scale, const double* __restrict__ r, float* __restrict__ r32, float* __restrict__ d32) {
	const long long stride = static_cast<long long>(gridDim.x) * RTPB;
	const long long lane = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	const long long packs = n / RPACK;
	const ref_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
	for (long long p = lane; p < packs; p += stride) {
		const ref_f64x2 a = reinterpret_cast<const ref_f64x2*>(r)[2 * p];
		const ref_f64x2 b = reinterpret_cast<const ref_f64x2*>(r)[2 * p + 1];
		const ref_f32x4 o = {static_cast<float>(a[0] * scale), static_cast<float>(a[1] * scale), static_cast<float>(b[0] * scale), static_cast<float>(b[1] * scale)};
		reinterpret_cast<ref_f32x4*>(r32)[p] = o;
		reinterpret_cast<ref_f32x4*>(d32)[p] = zero;
	}
	for (long long i = packs * RPACK + lane; i < n; i += stride) {
		r32[i] = static_cast<float>(r[i] * scale);
		d32[i] = 0.f;
	}
}

// xc[i] = fma(scale, (double)d32[i], x[i]).  d32 and xc are the driver's own; x is the caller's and may be element-aligned: VEC false
// reads it one element per lane.
template <bool VEC>
__global__ __launch_bounds__(RTPB) void refineCandidateKernel(int n, double scale, const float* __restrict__ d32, const double* __restrict__ x,
                                                              double* __restrict__ xc) {
	const long long stride = static_cast<long long>(gridDim.x) * RTPB;
	const long long lane = static_cast<long long>(blockIdx.x) * RTPB + threadIdx.x;
	long long done = 0;
	if constexpr (VEC) {
		const long long packs = n / RPACK;
		for (long long p = lane; p < packs; p += stride) {
			const ref_f32x4 d = reinterpret_cast<const ref_f32x4*>(d32)[p];
			const ref_f64x2 a = reinterpret_cast<const ref_f64x2*>(x)[2 * p];
			const ref_f64x2 b = reinterpret_cast<const ref_f64x2*>(x)[2 * p + 1];
			const ref_f64x2 oa = {__builtin_fma(scale, static_cast<double>(d[0]), a[0]), __builtin_fma(scale, static_cast<double>(d[1]), a[1])};
			const ref_f64x2 ob = {__builtin_fma(scale, static_cast<double>(d[2]), b[0]), __builtin_fma(scale, static_cast<double>(d[3]), b[1])};
			reinterpret_cast<ref_f64x2*>(xc)[2 * p] = oa;
			reinterpret_cast<ref_f64x2*>(xc)[2 * p + 1] = ob;
		}
		done = packs * RPACK;
	}
	for (long long i = done + lane; i < n; i += stride) xc[i] = __builtin_fma(scale, static_cast<double>(d32[i]), x[i]);
}

int gridFor(long long work) { return static_cast<int>(std::max<long long>(1, std::min<long long>((work + RTPB - 1) / RTPB, numCUs() * 8LL))); }

struct CsrOwner {  // the fp32 matrix a solve converted for itself
	smm_hip_csr* m = nullptr;
	~CsrOwner() { smm_hip_csr_destroy(m); }
};

int innerSolve(int inner, const smm_hip_csr* a32, const float* r32, float* d32, int maxInner, float innerEps, int restart, const smm_hip_precond* M32,
               hipStream_t s, int* iterations) {
	int st = 0;
	float res = 0.f;
	smm_hip_stream stream = static_cast<smm_hip_stream>(s);
	if (inner == SMM_REFINE_INNER_CG) return smm_hip_cg_dev_f32(a32, r32, d32, d32, maxInner, innerEps, M32, stream, &st, iterations, &res);
	if (inner == SMM_REFINE_INNER_BICGSTAB) return smm_hip_bicgstab_dev_f32(a32, r32, d32, maxInner, innerEps, M32, stream, &st, iterations, &res);
	return smm_hip_gmres_dev_f32(a32, r32, d32, maxInner, innerEps, restart, M32, stream, &st, iterations, &res);
}

// the checks that need no device: shared by the device-pointer driver and the host-pointer wrapper
int refineCheck(const smm_hip_csr* a, const smm_hip_csr* a32, const double* b, const double* x, int inner, int maxOuter, const smm_hip_precond* M32) {
	SMM_TRY(solverCheck<double>("refine", a, b, x));
	if (a32 && a32->dtype != SMM_DTYPE_F32) {
		setError("refine: a32 must be an fp32 matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (a32 && (a32->rows != a->rows || a32->cols != a->cols)) {
		setError("refine: a32 is %d x %d, a is %d x %d", a32->rows, a32->cols, a->rows, a->cols);
		return SMM_HIP_ERR_INVALID;
	}
	if (!a32 && M32) {
		setError("refine: a preconditioner needs the a32 it was created for");
		return SMM_HIP_ERR_INVALID;
	}
	if (maxOuter < 0) {
		setError("refine: maxOuter is negative");
		return SMM_HIP_ERR_INVALID;
	}
	if (inner != SMM_REFINE_INNER_CG && inner != SMM_REFINE_INNER_BICGSTAB && inner != SMM_REFINE_INNER_GMRES) {
		setError("refine: unknown inner solver %d", inner);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

int refineDev(const smm_hip_csr* a, const smm_hip_csr* a32, const double* b, double* x, int inner, int maxOuter, int maxInner, double eps, float innerEps,
              int restart, const smm_hip_precond* M32, hipStream_t s, int* status, int* outerIterations, int* innerIterations, double* resnorm2) {
	SMM_TRY(refineCheck(a, a32, b, x, inner, maxOuter, M32));
	const int n = a->rows;
	// (in this order: an error return synchronises, then releases the vectors, then destroys the converted matrix -- never under queued kernels)
	CsrOwner built;
	DevBuf<double> r, xc, parts, d_rr;
	DevBuf<float> r32, d32;
	SyncOnExit drain{s};
	SMM_TRY(ensureCsrReady(a, s, true));
	if (a32) SMM_TRY(ensureCsrReady(a32, s, true));
	if (a32 && a32->nnz != a->nnz) {
		setError("refine: a32 stores %d entries, a %d", a32->nnz, a->nnz);
		return SMM_HIP_ERR_INVALID;
	}
	int outer = 0, innerTotal = 0;
	double rr = 0.0;
	bool rejected = false;
	if (n > 0) {
		if (!a32) {
			SMM_TRY(csrConvertCreate(a, SMM_DTYPE_F32, s, &built.m));
			a32 = built.m;
		}
		SMM_TRY(r.alloc(n));
		SMM_TRY(xc.alloc(n));
		SMM_TRY(r32.alloc(n));
		SMM_TRY(d32.alloc(n));
		SMM_TRY(parts.alloc(NPART));
		SMM_TRY(d_rr.alloc(1));
		LoopWatch watch;
		SMM_TRY(watch.begin(s, nullptr, 0));
		// r = b - A v and r.r on the host: the loop test and the exponent need it
		auto residual = [&](const double* v, double* sum) -> int {
			SMM_TRY(launchSpmv<double>(a, SMM_OP_SUB, b, v, r, 0, nullptr, nullptr, nullptr, s));
			SMM_TRY(launchDotPartials<double>(n, r, r, parts, nullptr, s));
			SMM_TRY(launchSumPartials<double>(parts, d_rr, s));
			return watch.fetch(d_rr.p, sum);
		};
		SMM_TRY(residual(x, &rr));
		const bool xAligned = reinterpret_cast<uintptr_t>(x) % 16 == 0;
		while (rr > eps * eps && outer < maxOuter) {
			int e = 0;
			const double nrm = std::sqrt(rr);
			if (std::isfinite(nrm)) (void)std::frexp(nrm, &e);  // (an infinite rr: e = 0, and the candidate cannot pass)
			refineDemoteKernel<<<gridFor(n / RPACK + 1), RTPB, 0, s>>>(n, std::ldexp(1.0, -e), r, r32, d32);
			SMM_HIP_TRY(hipGetLastError());
			int it = 0;
			SMM_TRY(innerSolve(inner, a32, r32, d32, maxInner, innerEps, restart, M32, s, &it));
			innerTotal += it;
			if (xAligned) refineCandidateKernel<true><<<gridFor(n / RPACK + 1), RTPB, 0, s>>>(n, std::ldexp(1.0, e), d32, x, xc);
			else refineCandidateKernel<false><<<gridFor(n), RTPB, 0, s>>>(n, std::ldexp(1.0, e), d32, x, xc);
			SMM_HIP_TRY(hipGetLastError());
			double rrc = 0.0;
			SMM_TRY(residual(xc, &rrc));
			if (!(rrc < rr)) {
				rejected = true;
				break;
			}
			SMM_TRY(launchCopy2<double>(n, xc, x, nullptr, s));
			rr = rrc;
			++outer;
		}
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	int st = SMM_SOLVER_MAX_ITERATIONS_REACHED;
	if (rejected || !std::isfinite(rr)) st = SMM_SOLVER_DIVERGED;
	else if (!(rr > eps * eps)) st = SMM_SOLVER_SUCCESS;
	if (status) *status = st;
	if (outerIterations) *outerIterations = outer;
	if (innerIterations) *innerIterations = innerTotal;
	if (resnorm2) *resnorm2 = rr;
	return SMM_HIP_OK;
}

}  // namespace
}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_refine_f64(const smm_hip_csr* a, const smm_hip_csr* a32, double* b, double* x, int inner, int maxOuter, int maxInner, double eps, float innerEps,
                       int restart, const smm_hip_precond* M32, int* solver_status, int* outer_iterations, int* inner_iterations, double* resnorm2) {
	SMM_TRY(refineCheck(a, a32, b, x, inner, maxOuter, M32));
	int outer = 0;  // x comes back only when a step was accepted
	const int rc = solveFromHost<double>(
	    a->rows, b, nullptr, x,
	    [&](const double* db, const double*, double* dx, hipStream_t s) {
		    return refineDev(a, a32, db, dx, inner, maxOuter, maxInner, eps, innerEps, restart, M32, s, solver_status, &outer, inner_iterations, resnorm2);
	    },
	    &outer);
	if (rc == SMM_HIP_OK && outer_iterations) *outer_iterations = outer;
	return rc;
}

int smm_hip_refine_dev_f64(const smm_hip_csr* a, const smm_hip_csr* a32, const double* d_b, double* d_x, int inner, int maxOuter, int maxInner, double eps,
                           float innerEps, int restart, const smm_hip_precond* M32, smm_hip_stream stream, int* solver_status, int* outer_iterations,
                           int* inner_iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return refineDev(a, a32, d_b, d_x, inner, maxOuter, maxInner, eps, innerEps, restart, M32, pickStream(stream), solver_status, outer_iterations,
	                 inner_iterations, resnorm2);
}

}  // extern "C"
