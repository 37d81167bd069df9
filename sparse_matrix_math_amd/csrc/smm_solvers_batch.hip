// smm_solvers_batch.hip -- BiCGStab (ref:2191-2303) and ConjugateGradient (ref:2316-2398) for k right-hand sides at once.
//
// Additions with no counterpart in the reference: its solvers take one b.  Every vector is an interleaved n x k block (element (i, j)
// at i * k + j, 1 <= k <= SMM_HIP_MAX_RHS) and the matrix is streamed once per SpMM for all k columns (smm_spmm.hip) instead of k times.
//
// These are the plain loops of bicgstabLoop and of cgDev's non-lazy path (smm_solvers.hip) with every scalar per column:
//   * one Scal<T> per column; the dot products of a column are its own NPART partial sums, added in the fixed order of sumParts;
//   * the same launches per iteration as the single loops: BiCGStab 2 SpMM with fused dots + 3 update kernels, CG 1 SpMM + 2 updates;
//     alpha / omega / beta are formed per column inside the update kernels that consume them;
//   * column j runs the reference's loop for ITS b: do { } while (res_j > eps && it_j < maxIterations) with the reference's clamp of
//     maxIterations, status rule and NaN behaviour (ref:2200-2283, 2330-2398).  A column that has left its loop is FROZEN: its x, r, res,
//     iterations and status are never written again (its elements are left out of the stores), and since no scalar is shared its NaNs
//     or zeros cannot reach another column;
//   * the host stops enqueueing when ALL columns are done: the device raises one all-done word that the DonePoller watches and that the
//     SpMM launches test.
//   * BiCGStab takes JACOBI (folded into the SpMM's rows) and the iterated sweeps JSWEEP_SGS / _ILU0, which work on one vector: the SpMM
//     writes a temporary, each column is gathered, applied and scattered, and batchDot forms the sums the epilogue would have.
// No resident, lazy-x, PATTERN-adoption or autotune path is entered from here.
#include <algorithm>
#include <cmath>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

namespace {

constexpr int TPB = 256;
constexpr int COLPARTS = 2 * NPART;  // partial-sum slots of one column (launchSpmm's layout)

// the KC elements of one row of an interleaved block: loaded and stored as one access (element alignment: any k)
template <typename T, int KC>
struct Row {
	T v[KC];
};

// Element-wise map over the rows of interleaved n x KC blocks, one lane per row: out[q](i, j) = f(j, in[0](i, j), in[1](i, j), ...).
// A lane loads all its inputs, computes, then stores, so an output may be one of the inputs.  frozen[q]: bit j set = column j of out[q]
// is not written (whole-row stores when no bit is set, the unfrozen elements one by one otherwise); out may be null when NOUT == 0.
template <typename T, int KC, int NIN, int NOUT, typename F>
__device__ __forceinline__ void rowMap(int n, const T* const* in, T* const* out, const unsigned* frozen, F&& f) {
	using R = Row<T, KC>;
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		R a[NIN];
#pragma unroll
		for (int q = 0; q < NIN; ++q) a[q] = reinterpret_cast<const R*>(in[q])[i];
		R o[NOUT > 0 ? NOUT : 1];
#pragma unroll
		for (int j = 0; j < KC; ++j) {
			T iv[NIN], ov[NOUT > 0 ? NOUT : 1];
#pragma unroll
			for (int q = 0; q < NIN; ++q) iv[q] = a[q].v[j];
			f(j, iv, ov);
#pragma unroll
			for (int q = 0; q < NOUT; ++q) o[q].v[j] = ov[q];
		}
#pragma unroll
		for (int q = 0; q < NOUT; ++q) {
			if (frozen[q] == 0u) {
				reinterpret_cast<R*>(out[q])[i] = o[q];
			} else {
#pragma unroll
				for (int j = 0; j < KC; ++j) {
					if (!((frozen[q] >> j) & 1u)) out[q][i * KC + j] = o[q].v[j];
				}
			}
		}
	}
}

// one word per column read ONCE per workgroup (bit j = word of column j is non-zero): every lane of the workgroup then sees the same
// mask, also while workgroup 0 of the same launch is raising `done` words
template <typename T, int KC>
__device__ __forceinline__ unsigned columnMask(const Scal<T>* sc, int Scal<T>::*word) {
	__shared__ unsigned sMask;
	if (threadIdx.x == 0) {
		unsigned m = 0;
#pragma unroll
		for (int j = 0; j < KC; ++j) m |= (sc[j].*word) ? (1u << j) : 0u;
		sMask = m;
	}
	__syncthreads();
	const unsigned m = sMask;
	__syncthreads();
	return m;
}

// parts[j][0 .. NPART) = per-workgroup sums of a(:, j) . b(:, j)
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void batchDot(int n, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ parts) {
	__shared__ T red[4];
	T acc[KC];
#pragma unroll
	for (int j = 0; j < KC; ++j) acc[j] = T(0);
	const T* const in[2] = {a, b};
	const unsigned none = 0;
	rowMap<T, KC, 2, 0>(n, in, nullptr, &none, [&](int j, const T(&v)[2], T(&)[1]) { acc[j] += v[0] * v[1]; });
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T s = blockSum256(acc[j], red);
		if (threadIdx.x == 0) parts[static_cast<size_t>(j) * COLPARTS + blockIdx.x] = s;
	}
}

// column j of an interleaved n x k block and a contiguous vector: gather (block -> vec) or scatter (vec -> block)
template <typename T>
__global__ __launch_bounds__(TPB) void batchColumnCopy(int n, int k, int j, T* block, int gather, T* vec, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	for (long long i = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * TPB) {
		if (gather) vec[i] = block[i * k + j];
		else block[i * k + j] = vec[i];
	}
}

// ---- BiCGStab ---------------------------------------------------------------------------------------------------------------------
// rr0_j = r_j . r0_j (ref:2231)
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void bicgBatchInit(const T* __restrict__ parts, Scal<T>* sc, int* allDone) {
	__shared__ T red[4];
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T rr0 = sumParts(parts + static_cast<size_t>(j) * COLPARTS, red);
		if (threadIdx.x == 0) {
			sc[j].rr = rr0;
			sc[j].rrPing[0] = rr0;
			sc[j].res = T(0);
			sc[j].iters = 0;
			sc[j].done = 0;
			sc[j].pad = 0;
			sc[j].status = SMM_SOLVER_SUCCESS;
		}
	}
	if (threadIdx.x == 0) *allDone = 0;
}

// alpha_j = rr0_j / (ap_j . r0_j) ; s = -alpha ap + r   (ref:2243-2247)
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void bicgBatchS(int n, Scal<T>* sc, int par, const T* __restrict__ partsA, const T* ap, const T* r, T* sv) {
	__shared__ T red[5];
	const unsigned frozen = columnMask<T, KC>(sc, &Scal<T>::done);
	if (frozen == (1u << KC) - 1u) return;
	T alpha[KC];
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		alpha[j] = sc[j].rrPing[par] / sumPartsAll(partsA + static_cast<size_t>(j) * COLPARTS, red);
		if (blockIdx.x == 0 && threadIdx.x == 0 && !((frozen >> j) & 1u)) sc[j].alpha = alpha[j];
	}
	const T* const in[2] = {ap, r};
	T* const out[1] = {sv};
	rowMap<T, KC, 2, 1>(n, in, out, &frozen, [&](int j, const T(&v)[2], T(&o)[1]) { o[0] = smmFma(-alpha[j], v[0], v[1]); });
}

// omega_j = (as.s)/(as.as) ; x, r update ; partial ||r||^2 and r.r0   (ref:2259-2269); per column partsB = [as.as | as.s], partsC = [r.r | r.r0]
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void bicgBatchXR(int n, Scal<T>* sc, const T* __restrict__ partsB, const T* p, const T* sv, const T* as, const T* r0, T* x,
                                                   T* r, T* __restrict__ partsC) {
	__shared__ T red[5];
	const unsigned frozen = columnMask<T, KC>(sc, &Scal<T>::done);
	if (frozen == (1u << KC) - 1u) return;
	T alpha[KC], omega[KC], acc0[KC], acc1[KC];
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T asas = sumPartsAll(partsB + static_cast<size_t>(j) * COLPARTS, red);
		const T ass = sumPartsAll(partsB + static_cast<size_t>(j) * COLPARTS + NPART, red);
		omega[j] = ass / asas;
		alpha[j] = sc[j].alpha;
		acc0[j] = acc1[j] = T(0);
		if (blockIdx.x == 0 && threadIdx.x == 0 && !((frozen >> j) & 1u)) sc[j].omega = omega[j];
	}
	const T* const in[5] = {sv, x, p, as, r0};
	T* const out[2] = {x, r};
	const unsigned fz[2] = {frozen, frozen};
	rowMap<T, KC, 5, 2>(n, in, out, fz, [&](int j, const T(&v)[5], T(&o)[2]) {
		const T si = v[0];
		o[0] = smmFma(alpha[j], v[2], smmFma(omega[j], si, v[1]));
		const T ri = smmFma(-omega[j], v[3], si);
		o[1] = ri;
		acc0[j] += ri * ri;
		acc1[j] += ri * v[4];
	});
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T s0 = blockSum256(acc0[j], red);
		const T s1 = blockSum256(acc1[j], red);
		if (threadIdx.x == 0) {
			partsC[static_cast<size_t>(j) * COLPARTS + blockIdx.x] = s0;
			partsC[static_cast<size_t>(j) * COLPARTS + NPART + blockIdx.x] = s1;
		}
	}
}

// per column: resL2Norm, loop test, beta, p = beta (-omega ap + p) + r   (ref:2268-2277); the all-done word
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void bicgBatchP(int n, Scal<T>* sc, int* allDone, int par, const T* __restrict__ partsC, T eps, const T* ap, const T* r, T* p) {
	__shared__ T red[5];
	const unsigned frozen = columnMask<T, KC>(sc, &Scal<T>::done);
	if (frozen == (1u << KC) - 1u) return;
	T omega[KC], beta[KC];
	unsigned leaving = 0;
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T rr = sumPartsAll(partsC + static_cast<size_t>(j) * COLPARTS, red);
		const T newRR0 = sumPartsAll(partsC + static_cast<size_t>(j) * COLPARTS + NPART, red);
		const T res = sqrtRn(rr);
		const T alpha = sc[j].alpha;
		omega[j] = sc[j].omega;
		const T rr0 = sc[j].rrPing[par];
		const bool leave = !(res > eps);  // while (resL2Norm > eps ...): NaN leaves the loop too
		if (leave) leaving |= 1u << j;
		beta[j] = (newRR0 * alpha) / (rr0 * omega[j]);  // ref:2271
		if (blockIdx.x == 0 && threadIdx.x == 0 && !((frozen >> j) & 1u)) {
			sc[j].res = res;
			sc[j].rrPing[par ^ 1] = newRR0;
			sc[j].iters += 1;
			if (leave) sc[j].done = 1;
		}
	}
	const unsigned skip = frozen | leaving;
	if (blockIdx.x == 0 && threadIdx.x == 0 && skip == (1u << KC) - 1u) *allDone = 1;
	if (skip == (1u << KC) - 1u) return;
	const T* const in[3] = {ap, p, r};
	T* const out[1] = {p};
	rowMap<T, KC, 3, 1>(n, in, out, &skip, [&](int j, const T(&v)[3], T(&o)[1]) { o[0] = smmFma(beta[j], smmFma(-omega[j], v[0], v[1]), v[2]); });
}

// ---- ConjugateGradient ------------------------------------------------------------------------------------------------------------
// rr_j = r_j . r_j ; eps^2 > rr_j: column j is done before its loop, SUCCESS, x(:, j) untouched (ref:2341-2344)
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void cgBatchInit(const T* __restrict__ parts, Scal<T>* sc, int* allDone, T eps) {
	__shared__ T red[4];
	int all = 1;
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T rr = sumParts(parts + static_cast<size_t>(j) * COLPARTS, red);
		if (threadIdx.x == 0) {
			const bool converged = eps * eps > rr;
			sc[j].rr = rr;
			sc[j].rrPing[0] = rr;
			sc[j].res = rr;
			sc[j].iters = 0;
			sc[j].status = converged ? SMM_SOLVER_SUCCESS : SMM_SOLVER_MAX_ITERATIONS_REACHED;
			sc[j].done = converged ? 1 : 0;
			sc[j].pad = 0;
			sc[j].flushIter = -1;
			if (!converged) all = 0;
		}
	}
	if (threadIdx.x == 0) *allDone = all;
}

// alpha_j = rr_j / (Ap_j . p_j) ; r = -alpha Ap + r ; partial ||r||^2 (ref:2354-2375).  sc[j].pad = the done word as this iteration found
// it: the second kernel decides by it (its own workgroup 0 raises `done` while other workgroups of that launch may not have started)
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void cgBatchR(int n, Scal<T>* sc, int par, const T* __restrict__ partsA, const T* Ap, T* r, T* __restrict__ partsC) {
	__shared__ T red[5];
	const unsigned frozen = columnMask<T, KC>(sc, &Scal<T>::done);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
		for (int j = 0; j < KC; ++j) sc[j].pad = (frozen >> j) & 1u;
	}
	if (frozen == (1u << KC) - 1u) return;
	T alpha[KC], acc[KC];
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		alpha[j] = sc[j].rrPing[par] / sumPartsAll(partsA + static_cast<size_t>(j) * COLPARTS, red);
		acc[j] = T(0);
		if (blockIdx.x == 0 && threadIdx.x == 0 && !((frozen >> j) & 1u)) sc[j].alpha = alpha[j];
	}
	const T* const in[2] = {Ap, r};
	T* const out[1] = {r};
	rowMap<T, KC, 2, 1>(n, in, out, &frozen, [&](int j, const T(&v)[2], T(&o)[1]) {
		const T ri = smmFma(-alpha[j], v[0], v[1]);
		o[0] = ri;
		acc[j] += ri * ri;
	});
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T s = blockSum256(acc[j], red);
		if (threadIdx.x == 0) partsC[static_cast<size_t>(j) * COLPARTS + blockIdx.x] = s;
	}
}

// per column: x = alpha p + xcur ; convergence test ; beta ; p = beta p + r   (ref:2362-2394: x is updated before the test, p only when the
// loop goes on); the all-done word
template <typename T, int KC>
__global__ __launch_bounds__(TPB) void cgBatchXP(int n, Scal<T>* sc, int* allDone, int par, const T* __restrict__ partsC, T eps, T* p, const T* r, const T* xcur,
                                                 T* x) {
	__shared__ T red[5];
	const unsigned frozen = columnMask<T, KC>(sc, &Scal<T>::pad);
	if (frozen == (1u << KC) - 1u) return;
	T alpha[KC], beta[KC];
	unsigned converged = 0;
#pragma unroll
	for (int j = 0; j < KC; ++j) {
		const T rrNew = sumPartsAll(partsC + static_cast<size_t>(j) * COLPARTS, red);
		const T rrOld = sc[j].rrPing[par];
		alpha[j] = sc[j].alpha;
		const bool conv = eps * eps > rrNew;
		if (conv) converged |= 1u << j;
		beta[j] = rrNew / rrOld;
		if (blockIdx.x == 0 && threadIdx.x == 0 && !((frozen >> j) & 1u)) {
			sc[j].iters += 1;
			sc[j].res = rrNew;
			if (conv) {
				sc[j].done = 1;
				sc[j].status = SMM_SOLVER_SUCCESS;
			} else {
				sc[j].rrPing[par ^ 1] = rrNew;
			}
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0 && (frozen | converged) == (1u << KC) - 1u) *allDone = 1;
	const T* const in[3] = {p, xcur, r};
	T* const out[2] = {x, p};
	const unsigned fz[2] = {frozen, frozen | converged};
	rowMap<T, KC, 3, 2>(n, in, out, fz, [&](int j, const T(&v)[3], T(&o)[2]) {
		o[0] = smmFma(alpha[j], v[0], v[1]);
		o[1] = smmFma(beta[j], v[0], v[2]);
	});
}

// KERNEL<T, k> for the run-time k (one instantiation per number of columns: the row of a block is a compile-time struct)
#define SMM_BATCH_LAUNCH(KERNEL, K, GRID, STREAM, ...)                         \
	do {                                                                       \
		switch (K) {                                                           \
		case 1: KERNEL<T, 1><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 2: KERNEL<T, 2><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 3: KERNEL<T, 3><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 4: KERNEL<T, 4><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 5: KERNEL<T, 5><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 6: KERNEL<T, 6><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		case 7: KERNEL<T, 7><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		default: KERNEL<T, 8><<<(GRID), TPB, 0, (STREAM)>>>(__VA_ARGS__); break; \
		}                                                                      \
	} while (0)

// solverCheck on the n x k blocks, and k in range
template <typename T, typename... V>
int batchCheck(const char* who, const smm_hip_csr* a, int k, const V*... blocks) {
	SMM_TRY(solverCheck<T>(who, a, blocks...));
	if (k < 1 || k > SMM_HIP_MAX_RHS) {
		setError("%s: k = %d, must be 1 .. %d", who, k, SMM_HIP_MAX_RHS);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
int bicgstabBatchDev(const smm_hip_csr* a, int k, const T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, hipStream_t s, int* status,
                     int* iterations, T* resnorm) {
	SMM_TRY(batchCheck<T>("bicgstab_batch", a, k, b, x));
	const int n = a->rows;
	const bool precondition = M != nullptr && M->kind != SMM_PRECOND_NONE;  // ref:2209
	SMM_TRY(precondAdmissible("bicgstab_batch", M, a, SOLVER_BATCHED));  // (the sweeps of the other kinds exist for one right-hand side only)
	if (precondition && M->dtype != dtypeOf<T>()) {
		setError("bicgstab_batch: the preconditioner holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureCsrReady(a, s, true));
	// the Jacobi apply x = rhs / diag is folded into the rows of the SpMM that precedes it, exactly as the single loop folds it into its SpMV
	const bool sweeps = precondition && isJsweepKind(M->kind);
	const T* diag = precondition && !sweeps ? static_cast<const T*>(M->d_values) : nullptr;
	// The iterated sweeps (JSWEEP_SGS / _ILU0) work on one vector: the SpMM leaves A v in t, every column of t goes through the apply by
	// way of two contiguous vectors, and the dot products the SpMM would have fused are formed by batchDot afterwards.  A frozen column's
	// apply writes a temporary only (ap / as), which no update reads for that column.
	DevBuf<T> t, cin, cout;
	if (sweeps) {
		SMM_TRY(t.alloc(static_cast<size_t>(n) * k));
		SMM_TRY(cin.alloc(n));
		SMM_TRY(cout.alloc(n));
	}
	auto sweepColumns = [&](T* dst, const int* flag) -> int {
		for (int j = 0; j < k && n > 0; ++j) {
			batchColumnCopy<T><<<solverGrid(n), TPB, 0, s>>>(n, k, j, t.p, 1, cin.p, flag);
			SMM_TRY(precondApplyDev<T>(M, cin.p, cout.p, flag, s));
			batchColumnCopy<T><<<solverGrid(n), TPB, 0, s>>>(n, k, j, dst, 0, cout.p, flag);
		}
		SMM_HIP_TRY(hipGetLastError());
		return SMM_HIP_OK;
	};
	maxIterations = std::min(maxIterations, n);  // ref:2200
	if (maxIterations == -1) maxIterations = n;  // ref:2201-2203
	const size_t nk = static_cast<size_t>(n) * k;
	DevBuf<T> r, r0, p, ap, sv, as, parts, parts2;
	DevBuf<Scal<T>> sc;
	DevBuf<int> allDone;
	SMM_TRY(r.alloc(nk));
	SMM_TRY(r0.alloc(nk));
	SMM_TRY(p.alloc(nk));
	SMM_TRY(ap.alloc(nk));
	SMM_TRY(sv.alloc(nk));
	SMM_TRY(as.alloc(nk));
	SMM_TRY(parts.alloc(static_cast<size_t>(k) * COLPARTS));   // per column [ap.r0] then [as.as | as.s]
	SMM_TRY(parts2.alloc(static_cast<size_t>(k) * COLPARTS));  // per column [r.r | r.r0]
	SMM_TRY(sc.alloc(k));
	SMM_TRY(allDone.alloc(1));

	// r = M^-1 (b - A x), ref:2215-2224
	if (sweeps) {
		SMM_TRY(launchSpmm<T>(a, SMM_OP_SUB, k, b, x, t.p, 0, nullptr, nullptr, nullptr, s));
		SMM_TRY(sweepColumns(r, nullptr));
	} else {
		SMM_TRY(launchSpmm<T>(a, diag ? SPMM_OP_SUB_DIV : SMM_OP_SUB, k, b, x, r, 0, nullptr, nullptr, nullptr, s, diag));
	}
	if (nk) {
		SMM_HIP_TRY(hipMemcpyAsync(r0, r, sizeof(T) * nk, hipMemcpyDeviceToDevice, s));  // ref:2225-2226
		SMM_HIP_TRY(hipMemcpyAsync(p, r, sizeof(T) * nk, hipMemcpyDeviceToDevice, s));
	}
	SMM_BATCH_LAUNCH(batchDot, k, NPART, s, n, r, r0, parts);  // ref:2231
	SMM_BATCH_LAUNCH(bicgBatchInit, k, 1, s, parts, sc, allDone);

	const int* doneFlag = allDone;
	const int planned = std::max(1, maxIterations);  // do { } while: the body always runs once (ref:2232, 2277)
	const int spmmOp = diag ? SPMV_OP_DIV : SMM_OP_ASSIGN;
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 1));
	for (int i = 0; i < planned && !watch.leave(i); ++i) {
		if (sweeps) {
			SMM_TRY(launchSpmm<T>(a, SMM_OP_ASSIGN, k, nullptr, p, t.p, 0, nullptr, nullptr, doneFlag, s));
			SMM_TRY(sweepColumns(ap, doneFlag));
			SMM_BATCH_LAUNCH(batchDot, k, NPART, s, n, ap, r0, parts);  // ap.r0
		} else {
			SMM_TRY(launchSpmm<T>(a, spmmOp, k, nullptr, p, ap, 1, r0, parts, doneFlag, s, diag));  // ref:2234-2235 + 2243 fused
		}
		SMM_BATCH_LAUNCH(bicgBatchS, k, solverGrid(n), s, n, sc, i & 1, parts, ap, r, sv);
		if (sweeps) {
			SMM_TRY(launchSpmm<T>(a, SMM_OP_ASSIGN, k, nullptr, sv, t.p, 0, nullptr, nullptr, doneFlag, s));
			SMM_TRY(sweepColumns(as, doneFlag));
			SMM_BATCH_LAUNCH(batchDot, k, NPART, s, n, as, as, parts);           // [as.as | as.s]
			SMM_BATCH_LAUNCH(batchDot, k, NPART, s, n, as, sv, parts.p + NPART);
		} else {
			SMM_TRY(launchSpmm<T>(a, spmmOp, k, nullptr, sv, as, 2, sv, parts, doneFlag, s, diag));  // ref:2250-2251 + 2256-2261 fused
		}
		SMM_BATCH_LAUNCH(bicgBatchXR, k, NPART, s, n, sc, parts, p, sv, as, r0, x, r, parts2);
		SMM_BATCH_LAUNCH(bicgBatchP, k, solverGrid(n), s, n, sc, allDone, i & 1, parts2, eps, ap, r, p);
	}
	Scal<T> h[SMM_HIP_MAX_RHS];
	SMM_TRY(loopFinish(watch, h, sc.p, sizeof(Scal<T>) * k, s));
	for (int j = 0; j < k; ++j) {
		if (status) status[j] = h[j].iters > maxIterations ? SMM_SOLVER_MAX_ITERATIONS_REACHED : SMM_SOLVER_SUCCESS;  // ref:2279-2282
		if (iterations) iterations[j] = h[j].iters;
		if (resnorm) resnorm[j] = h[j].res;
	}
	return SMM_HIP_OK;
}

template <typename T>
int cgBatchDev(const smm_hip_csr* a, int k, const T* b, const T* x0, T* x, int maxIterations, T eps, hipStream_t s, int* status, int* iterations,
               T* resnorm2) {
	SMM_TRY(batchCheck<T>("cg_batch", a, k, b, x0, x));
	const int n = a->rows;
	SMM_TRY(ensureCsrReady(a, s, true));
	const size_t nk = static_cast<size_t>(n) * k;
	DevBuf<T> r, p, Ap, parts, parts2;
	DevBuf<Scal<T>> sc;
	DevBuf<int> allDone;
	SMM_TRY(r.alloc(nk));
	SMM_TRY(p.alloc(nk));
	SMM_TRY(Ap.alloc(nk));
	SMM_TRY(parts.alloc(static_cast<size_t>(k) * COLPARTS));
	SMM_TRY(parts2.alloc(static_cast<size_t>(k) * COLPARTS));
	SMM_TRY(sc.alloc(k));
	SMM_TRY(allDone.alloc(1));

	SMM_TRY(launchSpmm<T>(a, SMM_OP_SUB, k, b, x0, r, 0, nullptr, nullptr, nullptr, s));  // r = b - A x0, ref:2337
	if (nk) SMM_HIP_TRY(hipMemcpyAsync(p, r, sizeof(T) * nk, hipMemcpyDeviceToDevice, s));  // p = r, ref:2340
	SMM_BATCH_LAUNCH(batchDot, k, NPART, s, n, r, r, parts);                              // ref:2341
	SMM_BATCH_LAUNCH(cgBatchInit, k, 1, s, parts, sc, allDone, eps);
	if (maxIterations == -1) maxIterations = n;  // ref:2345-2347 (no clamp otherwise)

	const int* doneFlag = allDone;
	LoopWatch watch;
	SMM_TRY(watch.begin(s, doneFlag, 0));
	for (int i = 0; i < maxIterations && !watch.leave(i); ++i) {
		SMM_TRY(launchSpmm<T>(a, SMM_OP_ASSIGN, k, nullptr, p, Ap, 1, p, parts, doneFlag, s));  // Ap = A p with p.Ap fused (ref:2353-2354)
		const T* xcur = i == 0 ? x0 : x;  // ref:2351, 2395
		SMM_BATCH_LAUNCH(cgBatchR, k, NPART, s, n, sc, i & 1, parts, Ap, r, parts2);
		SMM_BATCH_LAUNCH(cgBatchXP, k, solverGrid(n), s, n, sc, allDone, i & 1, parts2, eps, p, r, xcur, x);
	}
	Scal<T> h[SMM_HIP_MAX_RHS];
	SMM_TRY(loopFinish(watch, h, sc.p, sizeof(Scal<T>) * k, s));
	for (int j = 0; j < k; ++j) {
		if (status) status[j] = h[j].status;
		if (iterations) iterations[j] = h[j].iters;
		if (resnorm2) resnorm2[j] = h[j].res;
	}
	return SMM_HIP_OK;
}

// ---- host-pointer wrappers: blocks in caller-owned host memory, as the single forms take their vectors ---------------------------
template <typename T>
int bicgstabBatchHost(const smm_hip_csr* a, int k, T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, int* status, int* iterations, T* resnorm) {
	SMM_TRY(batchCheck<T>("bicgstab_batch", a, k, b, x));
	return solveFromHost<T>(static_cast<size_t>(a->rows) * k, b, nullptr, x, [&](const T* db, const T*, T* dx, hipStream_t s) {
		return bicgstabBatchDev<T>(a, k, db, dx, maxIterations, eps, M, s, status, iterations, resnorm);
	});
}

// a column whose first residual already passes is never written (ref:2342-2344): the device block starts as the caller's x and comes back
// whole, so such a column returns bit for bit
template <typename T>
int cgBatchHost(const smm_hip_csr* a, int k, const T* b, const T* x0, T* x, int maxIterations, T eps, int* status, int* iterations, T* resnorm2) {
	SMM_TRY(batchCheck<T>("cg_batch", a, k, b, x0, x));
	return solveFromHost<T>(static_cast<size_t>(a->rows) * k, b, x0, x, [&](const T* db, const T* dx0, T* dx, hipStream_t s) {
		return cgBatchDev<T>(a, k, db, dx0, dx, maxIterations, eps, s, status, iterations, resnorm2);
	});
}

}  // namespace

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_bicgstab_batch_f32(const smm_hip_csr* a, int k, float* b, float* x, int maxIterations, float eps, const smm_hip_precond* M, int* solver_status,
                               int* iterations, float* resnorm) {
	return bicgstabBatchHost<float>(a, k, b, x, maxIterations, eps, M, solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_batch_f64(const smm_hip_csr* a, int k, double* b, double* x, int maxIterations, double eps, const smm_hip_precond* M, int* solver_status,
                               int* iterations, double* resnorm) {
	return bicgstabBatchHost<double>(a, k, b, x, maxIterations, eps, M, solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_batch_dev_f32(const smm_hip_csr* a, int k, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M,
                                   smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm) {
	SMM_TRY(ensureInit());
	return bicgstabBatchDev<float>(a, k, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm);
}
int smm_hip_bicgstab_batch_dev_f64(const smm_hip_csr* a, int k, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M,
                                   smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm) {
	SMM_TRY(ensureInit());
	return bicgstabBatchDev<double>(a, k, d_b, d_x, maxIterations, eps, M, pickStream(stream), solver_status, iterations, resnorm);
}

int smm_hip_cg_batch_f32(const smm_hip_csr* a, int k, const float* b, const float* x0, float* x, int maxIterations, float eps, int* solver_status,
                         int* iterations, float* resnorm2) {
	return cgBatchHost<float>(a, k, b, x0, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_cg_batch_f64(const smm_hip_csr* a, int k, const double* b, const double* x0, double* x, int maxIterations, double eps, int* solver_status,
                         int* iterations, double* resnorm2) {
	return cgBatchHost<double>(a, k, b, x0, x, maxIterations, eps, solver_status, iterations, resnorm2);
}
int smm_hip_cg_batch_dev_f32(const smm_hip_csr* a, int k, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps, smm_hip_stream stream,
                             int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(ensureInit());
	return cgBatchDev<float>(a, k, d_b, d_x0, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}
int smm_hip_cg_batch_dev_f64(const smm_hip_csr* a, int k, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                             smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(ensureInit());
	return cgBatchDev<double>(a, k, d_b, d_x0, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2);
}

}  // extern "C"
