// smm_precond_jsweep.hip -- JSWEEP_SGS / JSWEEP_ILU0 / JSWEEP_IC0: the exact kind's factor in the natural numbering, each of its two
// triangular solves replaced by a FIXED number of Jacobi steps (a truncated Neumann series of the triangular factor).
//
// A Jacobi step of a sweep is the exact sweep's row walk (sweepStart / sweepTerm / sweepFinish of smm_trisweep.h, the row's triangular part
// in the stored order, one lane per row) for ALL rows at once, every y[col] read from the PREVIOUS iterate.  Iterate 0 is the walk with no
// terms: sweepFinish(sweepStart(own), own, diag).  The lower phase does sweeps_lower steps on own = rhs; the upper phase takes the finished
// lower result as own and does sweeps_upper steps.  Two consequences (include/smm_hip.h states them, tests/test_gpu_jsweep.py holds them):
//   exactness  after k steps every row of dependency level <= k (levels counted from 0) holds the exact sweep's bits, and keeps them: with
//              sweeps >= levels - 1 the apply IS the exact kind's, bit for bit;
//   symmetry   with sweeps_lower == sweeps_upper the IC0 form is P^T P and the SGS form is symmetric for symmetric A: a fixed, linear,
//              symmetric operator -- ConjugateGradient takes it.
// No ticket counter, no poll, no in-kernel wait: a step is shaped like an SpMV over one triangle and nothing in it can stall a grid.
//
// A step reads ITS triangle only: create splits the factor (SGS: A) into a strict lower triangle, a strict upper triangle (each row's
// entries in the order the exact upper sweep walks them: from the row's end backwards) and the diagonal.  The entries of 64 consecutive rows
// are then one contiguous range: a wavefront stages it through LDS with coalesced loads (all loads issued before the first LDS store) and
// each lane walks its own row out of LDS; a range of more than JS_CAP entries is walked from global memory in the same order.  Bytes per
// step: nnz_tri (4 + sizeof T) + 4 rows of row pointers + the vectors (own, diag, the gathered previous iterate, the result).
// Launches per apply: sweeps_lower + sweeps_upper, plus one element-wise pass for SGS / IC0 whose lower iterate 0 is rhs / d (ILU0's is rhs
// itself: its first step reads rhs as the previous iterate); the last lower step also writes the upper phase's iterate 0 (SGS: that is the
// lower result itself).  Iterates ping-pong between two scratch vectors kept per stream and x.
// The batched BiCGStab applies the kinds column by column (smm_solvers_batch.hip).
// The set-up is the exact kind's (smm_precond.hip: checks, level analysis, factor; of its plan the level counts and, for the refresh of an
// ILU0 / IC0 factor, the lower schedule are kept); the handle is a SNAPSHOT, JSWEEP_SGS included.
#include <algorithm>
#include <map>

#include "smm_trisweep.h"

struct smm_precond_jsweep {
	int base = SMM_PRECOND_SGS;  // the exact kind whose factor is iterated on
	int sweepsLo = 3, sweepsUp = 3;  // (read and written under the handle's enqueueMutex)
	int* d_startL = nullptr;  // strict lower triangle: rows + 1 row pointers, columns, values
	int* d_colL = nullptr;
	void* d_valL = nullptr;
	int* d_startU = nullptr;  // strict upper triangle, each row from its end backwards
	int* d_colU = nullptr;
	void* d_valU = nullptr;
	void* d_diag = nullptr;   // the entry the exact walk stops at: the divisor of sweepFinish
	int nnzL = 0, nnzU = 0;
	// the two vectors the iterates ping-pong between, one pair per stream the handle is applied on (the exact kinds' rule)
	struct Scratch {
		void* s0 = nullptr;
		void* s1 = nullptr;
	};
	std::mutex scratchMutex;
	std::map<hipStream_t, Scratch> scratch;
};

namespace smm {
namespace {

constexpr int JS_TPB = 256;
constexpr int JS_CAP = 512;  // entries of a wavefront's 64 rows staged through LDS (8 per row; more: the rows are walked from global memory)
constexpr int JS_TRIPS = JS_CAP / WAVE;

// ---- the split at create time.  The walks are sweepRow's: the lower one from the row's start while col < row, the upper one from the
// row's end backwards while col > row.
__global__ __launch_bounds__(JS_TPB) void jsCountKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, int* __restrict__ cntL,
                                                        int* __restrict__ cntU) {
	const long long i = static_cast<long long>(blockIdx.x) * JS_TPB + threadIdx.x;
	if (i >= n) return;
	const int b = start[i], e = start[i + 1];
	int k = b;
	while (k < e && positions[k] < i) ++k;
	cntL[i] = k - b;
	int q = e - 1;
	while (q >= b && positions[q] > i) --q;
	cntU[i] = e - 1 - q;
}

template <typename T>
__global__ __launch_bounds__(JS_TPB) void jsFillKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals,
                                                       const int* __restrict__ startL, const int* __restrict__ startU, int* __restrict__ colL, T* __restrict__ valL,
                                                       int* __restrict__ colU, T* __restrict__ valU, T* __restrict__ diag) {
	const long long i = static_cast<long long>(blockIdx.x) * JS_TPB + threadIdx.x;
	if (i >= n) return;
	const int b = start[i], e = start[i + 1];
	const int nl = startL[i + 1] - startL[i], nu = startU[i + 1] - startU[i];
	int o = startL[i];
	for (int k = 0; k < nl; ++k) {
		colL[o + k] = positions[b + k];
		valL[o + k] = vals[b + k];
	}
	diag[i] = b + nl < e ? vals[b + nl] : T(0);  // (the create-time check made sure of a diagonal)
	o = startU[i];
	for (int k = 0; k < nu; ++k) {
		colU[o + k] = positions[e - 1 - k];
		valU[o + k] = vals[e - 1 - k];
	}
}

// ---- a step
// the terms of one row, in the stored order; four gathers of the previous iterate in flight at a time
template <typename T, int MODE, typename PC, typename PV>
__device__ __forceinline__ T jsWalk(PC pc, PV pv, int len, const T* __restrict__ prev, T acc) {
	int k = 0;
	for (; k + 4 <= len; k += 4) {
		const int c0 = pc[k], c1 = pc[k + 1], c2 = pc[k + 2], c3 = pc[k + 3];
		const T x0 = prev[c0], x1 = prev[c1], x2 = prev[c2], x3 = prev[c3];
		acc = sweepTerm<T, MODE>(acc, pv[k], x0);
		acc = sweepTerm<T, MODE>(acc, pv[k + 1], x1);
		acc = sweepTerm<T, MODE>(acc, pv[k + 2], x2);
		acc = sweepTerm<T, MODE>(acc, pv[k + 3], x3);
	}
	for (; k < len; ++k) acc = sweepTerm<T, MODE>(acc, pv[k], prev[pc[k]]);
	return acc;
}

// out[row] = the row walk of MODE over (start, cols, vals) with y[] = prev; DUAL >= 0: out0[row] = iterate 0 of the sweep DUAL whose input
// is out[row].  Writes every row exactly once.  out / out0 are distinct from every vector read.
template <typename T, int MODE, int DUAL>
__global__ __launch_bounds__(JS_TPB) void jsStepKernel(int n, const int* __restrict__ start, const int* __restrict__ cols, const T* __restrict__ vals,
                                                       const T* __restrict__ diag, const T* own, const T* prev, T* __restrict__ out, T* __restrict__ out0,
                                                       const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	__shared__ int sCol[JS_TPB / WAVE][JS_CAP];
	__shared__ T sVal[JS_TPB / WAVE][JS_CAP];
	const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	const long long r0 = static_cast<long long>(blockIdx.x) * JS_TPB + wave * WAVE;  // the wavefront's first row
	const long long rowL = r0 + lane;
	const bool live = rowL < n;
	const int row = live ? static_cast<int>(rowL) : 0;
	int b = 0, e = 0;
	if (live) {
		b = start[row];
		e = start[row + 1];
	}
	// the wavefront's rows hold the contiguous range [base, base + cnt)
	int base = 0, cnt = 0;
	if (r0 < n) {
		base = start[r0];
		cnt = start[std::min<long long>(r0 + WAVE, n)] - base;
	}
	const bool staged = cnt <= JS_CAP;
	if (staged) {
		int rc[JS_TRIPS];
		T rv[JS_TRIPS];
#pragma unroll
		for (int u = 0; u < JS_TRIPS; ++u) {
			const int k = u * WAVE + lane;
			rc[u] = 0;
			rv[u] = T(0);
			if (k < cnt) {
				rc[u] = cols[base + k];
				rv[u] = vals[base + k];
			}
		}
#pragma unroll
		for (int u = 0; u < JS_TRIPS; ++u) {
			const int k = u * WAVE + lane;
			if (k < cnt) {
				sCol[wave][k] = rc[u];
				sVal[wave][k] = rv[u];
			}
		}
	}
	__syncthreads();
	if (!live) return;
	const T mine = own[row];
	T acc = sweepStart<T, MODE>(mine);
	if (staged) acc = jsWalk<T, MODE>(&sCol[wave][b - base], &sVal[wave][b - base], e - b, prev, acc);
	else acc = jsWalk<T, MODE>(cols + b, vals + b, e - b, prev, acc);
	const T d = diag[row];
	const T r = sweepFinish<T, MODE>(acc, mine, d);
	out[row] = r;
	if (DUAL >= 0) {
		constexpr int UP = DUAL >= 0 ? DUAL : MODE;
		out0[row] = sweepFinish<T, UP>(sweepStart<T, UP>(r), r, d);
	}
}

// iterate 0 where it is not one of the caller's vectors: the walk with no terms
template <typename T, int MODE>
__global__ __launch_bounds__(JS_TPB) void jsStartKernel(int n, const T* __restrict__ diag, const T* __restrict__ own, T* __restrict__ out,
                                                        const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	const long long i = static_cast<long long>(blockIdx.x) * JS_TPB + threadIdx.x;
	if (i >= n) return;
	const T mine = own[i];
	out[i] = sweepFinish<T, MODE>(sweepStart<T, MODE>(mine), mine, diag[i]);
}

void freeScratch(smm_precond_jsweep* J) {
	for (auto& kv : J->scratch) {
		devFree(kv.second.s0);
		devFree(kv.second.s1);
	}
	J->scratch.clear();
}

// the exact kinds' ownership rule: one set per stream, at most 8 kept (the ninth drains the device and frees them all)
int scratchFor(const smm_hip_precond* M, size_t elemBytes, hipStream_t s, smm_precond_jsweep::Scratch* out) {
	smm_precond_jsweep* J = M->jsw;
	std::lock_guard<std::mutex> lock(J->scratchMutex);
	auto it = J->scratch.find(s);
	if (it == J->scratch.end()) {
		if (J->scratch.size() >= 8) {
			SMM_HIP_TRY(hipDeviceSynchronize());
			freeScratch(J);
		}
		smm_precond_jsweep::Scratch sc;
		const size_t bytes = static_cast<size_t>(std::max(1, M->a->rows)) * elemBytes;
		SMM_TRY(devAlloc(&sc.s0, bytes));
		if (devAlloc(&sc.s1, bytes) != SMM_HIP_OK) {
			devFree(sc.s0);
			return SMM_HIP_ERR_HIP;
		}
		it = J->scratch.emplace(s, sc).first;
	}
	*out = it->second;
	return SMM_HIP_OK;
}

// the values the sweeps walk: A's for SGS, the factor for ILU0 / IC0
template <typename T>
const T* sweptValues(const smm_hip_precond* M) {
	return static_cast<const T*>(M->jsw->base == SMM_PRECOND_SGS ? M->a->d_values : M->d_values);
}

template <typename T>
void fillSplit(const smm_hip_precond* M, hipStream_t s) {
	const smm_precond_jsweep* J = M->jsw;
	const smm_hip_csr* a = M->a;
	if (a->rows == 0) return;
	jsFillKernel<T><<<gridOf(a->rows), JS_TPB, 0, s>>>(a->rows, a->d_start, a->d_positions, sweptValues<T>(M), J->d_startL, J->d_startU, J->d_colL,
	                                                    static_cast<T*>(J->d_valL), J->d_colU, static_cast<T*>(J->d_valU), static_cast<T*>(J->d_diag));
}

// the split copies of a handle whose exact set-up (M->plan, M->d_values) is done
template <typename T>
int buildSplit(smm_hip_precond* M, hipStream_t s) {
	smm_precond_jsweep* J = M->jsw;
	const smm_hip_csr* a = M->a;
	const int n = a->rows;
	const size_t n1 = static_cast<size_t>(n) + 1;
	DevBuf<int> cntL, cntU;
	SMM_TRY(cntL.alloc(n1));
	SMM_TRY(cntU.alloc(n1));
	SMM_HIP_TRY(hipMemsetAsync(cntL, 0, n1 * sizeof(int), s));
	SMM_HIP_TRY(hipMemsetAsync(cntU, 0, n1 * sizeof(int), s));
	if (n) jsCountKernel<<<gridOf(n), JS_TPB, 0, s>>>(n, a->d_start, a->d_positions, cntL, cntU);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&J->d_startL), n1 * sizeof(int)));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&J->d_startU), n1 * sizeof(int)));
	SMM_TRY(scanExclusive(cntL.p, J->d_startL, n1, s));
	SMM_TRY(scanExclusive(cntU.p, J->d_startU, n1, s));
	SMM_HIP_TRY(hipMemcpyAsync(&J->nnzL, J->d_startL + n, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(&J->nnzU, J->d_startU + n, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&J->d_colL), std::max<size_t>(1, J->nnzL) * sizeof(int)));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&J->d_colU), std::max<size_t>(1, J->nnzU) * sizeof(int)));
	SMM_TRY(devAlloc(&J->d_valL, std::max<size_t>(1, J->nnzL) * sizeof(T)));
	SMM_TRY(devAlloc(&J->d_valU, std::max<size_t>(1, J->nnzU) * sizeof(T)));
	SMM_TRY(devAlloc(&J->d_diag, static_cast<size_t>(std::max(1, n)) * sizeof(T)));
	fillSplit<T>(M, s);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template <typename T>
int jsCreateTyped(const smm_hip_csr* a, smm_hip_precond* M) {
	SMM_TRY(exactCreateTyped<T>(a, M->jsw->base, M));
	exactDropSchedules(M, M->jsw->base != SMM_PRECOND_SGS);  // what stays of the plan: the level counts, and the lower schedule refresh factorises over
	return buildSplit<T>(M, libStream());
}

const smm_precond_jsweep* jsOf(const smm_hip_precond* M, const char* who) {
	if (!M || !isJsweepKind(M->kind) || !M->jsw) {
		setError("%s: not an iterated-sweep (JSWEEP_) preconditioner", who);
		return nullptr;
	}
	return M->jsw;
}

bool sweepsInRange(int v) { return v >= 1 && v <= SMM_JSWEEP_MAX_SWEEPS; }

}  // namespace

template <typename T>
int jsweepApplyDev(const smm_hip_precond* M, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_precond_jsweep* J = M->jsw;
	if (!J || !J->d_diag) {
		setError("precond_apply: the iterated-sweep preconditioner was not set up");
		return SMM_HIP_ERR_INVALID;
	}
	const int n = M->a->rows;
	// the launches of an apply stay together on the stream; the counts are read under the lock, and so is the scratch taken: a thread that
	// brings a ninth stream drains the device and frees the sets only between whole applies
	std::lock_guard<std::mutex> whole(M->enqueueMutex);
	smm_precond_jsweep::Scratch sc;
	SMM_TRY(scratchFor(M, sizeof(T), s, &sc));
	T* const P = static_cast<T*>(sc.s0);  // where the finished lower result stays during the upper phase
	T* const Q = static_cast<T*>(sc.s1);
	const T* valL = static_cast<const T*>(J->d_valL);
	const T* valU = static_cast<const T*>(J->d_valU);
	const T* diag = static_cast<const T*>(J->d_diag);
	const int grid = gridOf(n);
	const int sL = J->sweepsLo, sU = J->sweepsUp;
	return withSweepModes(J->base, [&](auto lo, auto up) -> int {
		constexpr int LO = decltype(lo)::value, UP = decltype(up)::value;
		constexpr bool LO0_FREE = LO == ILU_LO;  // the lower phase's iterate 0 is rhs itself
		constexpr bool UP0_FREE = UP == SGS_UP;  // the upper phase's iterate 0 is the lower result itself
		// upper iterate j lives in x when sU - j is even, else in Q: the last one is x.  The lower iterates alternate between P (the last
		// one) and R, the one of x / Q that the upper phase's iterate 0 does not take.
		auto upLoc = [&](int j) { return (sU - j) % 2 == 0 ? x : Q; };
		T* const R = upLoc(0) == x ? Q : x;
		auto loLoc = [&](int j) { return (sL - j) % 2 == 0 ? P : R; };
		const T* prev = rhs;
		if (!LO0_FREE) {
			jsStartKernel<T, LO><<<grid, JS_TPB, 0, s>>>(n, diag, rhs, loLoc(0), doneFlag);
			prev = loLoc(0);
		}
		for (int j = 1; j <= sL; ++j) {
			T* out = loLoc(j);
			if (j == sL && !UP0_FREE) jsStepKernel<T, LO, UP><<<grid, JS_TPB, 0, s>>>(n, J->d_startL, J->d_colL, valL, diag, rhs, prev, out, upLoc(0), doneFlag);
			else jsStepKernel<T, LO, -1><<<grid, JS_TPB, 0, s>>>(n, J->d_startL, J->d_colL, valL, diag, rhs, prev, out, nullptr, doneFlag);
			prev = out;
		}
		prev = UP0_FREE ? P : upLoc(0);
		for (int j = 1; j <= sU; ++j) {
			T* out = upLoc(j);
			jsStepKernel<T, UP, -1><<<grid, JS_TPB, 0, s>>>(n, J->d_startU, J->d_colU, valU, diag, P, prev, out, nullptr, doneFlag);
			prev = out;
		}
		SMM_HIP_TRY(hipGetLastError());
		return SMM_HIP_OK;
	});
}
template int jsweepApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int jsweepApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void jsweepDestroy(smm_precond_jsweep* J) {
	if (!J) return;
	devFree(J->d_startL);
	devFree(J->d_colL);
	devFree(J->d_valL);
	devFree(J->d_startU);
	devFree(J->d_colU);
	devFree(J->d_valU);
	devFree(J->d_diag);
	freeScratch(J);
	delete J;
}

bool jsweepSymmetric(const smm_hip_precond* M) {
	std::lock_guard<std::mutex> lock(M->enqueueMutex);
	return M->jsw && M->jsw->sweepsLo == M->jsw->sweepsUp;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_precond_create_jsweep(const smm_hip_csr* a, int base_kind, int sweeps_lower, int sweeps_upper, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_jsweep: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (base_kind != SMM_PRECOND_SGS && base_kind != SMM_PRECOND_ILU0 && base_kind != SMM_PRECOND_IC0) {
		setError("precond_create_jsweep: base_kind must be SMM_PRECOND_SGS, _ILU0 or _IC0");
		return SMM_HIP_ERR_INVALID;
	}
	if (sweeps_lower == 0) sweeps_lower = SMM_JSWEEP_DEFAULT_SWEEPS;
	if (sweeps_upper == 0) sweeps_upper = SMM_JSWEEP_DEFAULT_SWEEPS;
	if (!sweepsInRange(sweeps_lower) || !sweepsInRange(sweeps_upper)) {
		setError("precond_create_jsweep: sweeps must be 0 (default %d) or 1 .. %d", SMM_JSWEEP_DEFAULT_SWEEPS, SMM_JSWEEP_MAX_SWEEPS);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	auto* M = new smm_hip_precond();
	M->kind = base_kind == SMM_PRECOND_SGS ? SMM_PRECOND_JSWEEP_SGS : base_kind == SMM_PRECOND_ILU0 ? SMM_PRECOND_JSWEEP_ILU0 : SMM_PRECOND_JSWEEP_IC0;
	M->dtype = a->dtype;
	M->a = a;
	M->jsw = new smm_precond_jsweep();
	M->jsw->base = base_kind;
	M->jsw->sweepsLo = sweeps_lower;
	M->jsw->sweepsUp = sweeps_upper;
	const int st = a->dtype == SMM_DTYPE_F32 ? jsCreateTyped<float>(a, M) : jsCreateTyped<double>(a, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

int smm_hip_precond_jsweep_info(const smm_hip_precond* M, int* base_kind, int* sweeps_lower, int* sweeps_upper, int* levels_lower, int* levels_upper) {
	const smm_precond_jsweep* J = jsOf(M, "precond_jsweep_info");
	if (!J) return SMM_HIP_ERR_INVALID;
	if (base_kind) *base_kind = J->base;
	{
		std::lock_guard<std::mutex> lock(M->enqueueMutex);
		if (sweeps_lower) *sweeps_lower = J->sweepsLo;
		if (sweeps_upper) *sweeps_upper = J->sweepsUp;
	}
	return smm_hip_precond_info(M, nullptr, levels_lower, levels_upper);
}

int smm_hip_precond_jsweep_set_sweeps(smm_hip_precond* M, int sweeps_lower, int sweeps_upper) {
	if (!jsOf(M, "precond_jsweep_set_sweeps")) return SMM_HIP_ERR_INVALID;
	if (sweeps_lower == 0) sweeps_lower = SMM_JSWEEP_DEFAULT_SWEEPS;
	if (sweeps_upper == 0) sweeps_upper = SMM_JSWEEP_DEFAULT_SWEEPS;
	if (!sweepsInRange(sweeps_lower) || !sweepsInRange(sweeps_upper)) {
		setError("precond_jsweep_set_sweeps: sweeps must be 0 (default %d) or 1 .. %d", SMM_JSWEEP_DEFAULT_SWEEPS, SMM_JSWEEP_MAX_SWEEPS);
		return SMM_HIP_ERR_INVALID;
	}
	std::lock_guard<std::mutex> lock(M->enqueueMutex);
	M->jsw->sweepsLo = sweeps_lower;
	M->jsw->sweepsUp = sweeps_upper;
	return SMM_HIP_OK;
}

int smm_hip_precond_jsweep_refresh(smm_hip_precond* M) {
	if (!jsOf(M, "precond_jsweep_refresh")) return SMM_HIP_ERR_INVALID;
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(M->a, nullptr, false));  // as create does
	SMM_HIP_TRY(hipDeviceSynchronize());
	hipStream_t s = libStream();
	if (M->dtype == SMM_DTYPE_F32) {
		SMM_TRY(exactRefactor<float>(M, M->jsw->base, s));
		fillSplit<float>(M, s);
	} else {
		SMM_TRY(exactRefactor<double>(M, M->jsw->base, s));
		fillSplit<double>(M, s);
	}
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

}  // extern "C"
