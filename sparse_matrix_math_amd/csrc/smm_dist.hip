// smm_dist.hip -- the SpMV + Krylov loop row-partitioned over the GPUs of one node, behind the C ABI.
//
// One process per GPU.  Rank g owns a contiguous range of rows of A (values / positions / start exactly as in the reference's
// CSRMatrix, ref:1243-1259, with GLOBAL column numbers) and the matching slices of every vector.  The reference has no
// counterpart (single process, shared memory: SURVEY.md section 2.1); what is kept is the arithmetic of ref:2191-2283 (BiCGStab)
// and ref:2316-2398 (ConjugateGradient): the same update expressions in the same order, with the dot products completed across
// ranks.
//
//   * halo: a rank needs x only on the column range its rows touch.  The parts owned by other ranks are received point to point
//     (RCCL ncclSend / ncclRecv over xGMI) straight into a halo-extended vector [left halo | owned | right halo].
//   * the local rows are split ON THE DEVICE into A_loc (owned columns) and A_rem (halo columns): A_loc x runs on the caller's
//     stream while the exchange is in flight on the communicator's side stream; A_rem x is added in place when it has landed,
//     with the dot products of the freshly computed vector fused into that launch and completed by its last workgroup
//     (lastBlockSums, smm_device.h); the sums an update kernel leaves behind are added by a one-workgroup launch (distFinishSums).
//   * the 1-2 scalars of each reduction point are all-reduced in place (ncclAllReduce) on the side stream; every workgroup of
//     the next update kernel reads the all-reduced totals and forms alpha / omega / beta itself, so there are no scalar launches:
//     8 kernels per BiCGStab iteration (4 SpMV launches, s, r, x, p updates) + 1 finishing launch, 6 + 1 per CG iteration.  The x update does not depend
//     on the last all-reduce of an iteration (||r||^2, r.r0) and runs beside it.
//   * nothing in the loop synchronises with the host; the `done` flag is polled through a pinned mailbox (DonePoller).
//   * r05 / r06: between processes the halo and the scalars travel PEER TO PEER by default (smm_p2p.h: pushes into IPC-mapped landing areas with
//     relay ranks, slot reductions -- no collective inside the loop), and a rank's SpMV runs as ONE launch over A_loc and A_rem
//     (smm_spmv_split.hip: local half, a bounded wait for the word the land kernel raises, remote half).  The collectives above are the
//     fall-back (SMM_HIP_P2P=0, a failed self-test, ranks that are threads of one process).
//
// Communicators: RCCL (librccl resolved with dlopen at run time, so single-GPU users need no RCCL), or host callbacks (the
// caller moves the bytes: used by the tests to run several ranks on one GPU, where RCCL cannot, and by the gloo rehearsal of
// bench.py), or none (world size 1).
//
// The units of the path (what they share: smm_dist.h):
//   smm_dist_comm.hip    the communicator: RCCL through dlopen, host callbacks, bounded waits and abort; smm_hip_comm_*
//   smm_dist_create.hip  A_loc / A_rem, the thin block's rows, the halo in pieces, the workspace; smm_hip_dist_csr_* (create, destroy, queries)
//   smm_dist_p2p.hip     the peer-to-peer plan, set-up and self-test, the push / land / slot launches; smm_hip_dist_p2p_plan
//   smm_dist_matvec.hip  the exchange and the SpMV in two halves, the all-reduce of its dot products; smm_hip_dist_spmv_dev_*
//   smm_dist.hip         (this file) the update kernels and the BiCGStab / CG loops; smm_hip_dist_bicgstab_dev_*, smm_hip_dist_cg_dev_*
#include <algorithm>

#include "smm_dist.h"

namespace smm {

// ---------------------------------------------------------------------------------------------------------
// kernels of the loops: each reads the all-reduced totals itself (no scalar launches)
// ---------------------------------------------------------------------------------------------------------
// totals[0] = a.b, totals[1] = a.c (nsets 2); NPART workgroups, finished by the last one
// The totals of a reduction whose partials an UPDATE kernel left behind (distDots, distBicgR, distCgR): one workgroup adds the NPART
// partials of each quantity in the order the fused hand-off uses (lastBlockSums, smm_device.h: i = t, t + 256, ...; then blockSum256) --
// the same bits -- and leaves them where the all-reduce expects them.  r01-r04 had the LAST workgroup of the update kernel do this: every
// workgroup then ends with two dependent trips to memory (publish the partial, take a ticket), which for a 5 us kernel over a rank's
// 1.25 M rows was most of its time (distBicgR 28.6 us; this launch: 4.7-6.3 us, started without a gap; profiles/r05/rank_loop_gaps.txt).
// The SpMV kernels keep the fused hand-off (SPMV_FINISH): there it costs what this launch would.
template <typename T>
__global__ __launch_bounds__(TPB) void distFinishSums(const T* __restrict__ parts, int nsets, T* totals, const int* __restrict__ doneFlag) {
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	for (int k = 0; k < nsets; ++k) {
		T acc = T(0);
		for (int i = threadIdx.x; i < NPART; i += TPB) acc += parts[k * NPART + i];
		const T s = blockSum256(acc, red);
		if (threadIdx.x == 0) totals[k] = s;
	}
}

template <typename T>
__global__ __launch_bounds__(TPB) void distDots(int n, const T* a, const T* b, const T* cvec, int nsets, T* parts, const int* __restrict__ doneFlag) {
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	T acc0 = T(0), acc1 = T(0);
	if (nsets == 2) {
		const T* const in[3] = {a, b, cvec};
		streamMap<T, false, 3, 0>(n, in, nullptr, [&](const T(&v)[3], T(&)[1]) {
			acc0 += v[0] * v[1];
			acc1 += v[0] * v[2];
		});
	} else {
		const T* const in[2] = {a, b};
		streamMap<T, false, 2, 0>(n, in, nullptr, [&](const T(&v)[2], T(&)[1]) { acc0 += v[0] * v[1]; });
	}
	const T s0 = blockSum256(acc0, red);
	if (threadIdx.x == 0) parts[blockIdx.x] = s0;
	if (nsets == 2) {
		const T s1 = blockSum256(acc1, red);
		if (threadIdx.x == 0) parts[NPART + blockIdx.x] = s1;
	}
}

template <typename T>
__global__ void distBicgInit(const T* __restrict__ totals, Scal<T>* sc) {
	sc->rrPing[0] = totals[0];  // rr0 = r.r0, ref:2231
	sc->res = T(0);
	sc->iters = 0;
	sc->done = 0;
	sc->status = SMM_SOLVER_SUCCESS;
}

// The steps are those of the single-GPU loop (smm_krylov_steps.h): the kernels here hand them the all-reduced totals and the rows of their
// launch.  book: this launch records the scalars (the other launch of a pair -- boundary rows first, then the bulk -- forms the same
// scalars from the same operands and only uses them).
// alpha = rr0 / (ap.r0) ; s = -alpha ap + r   (ref:2243-2247)
template <typename T>
__global__ __launch_bounds__(TPB) void distBicgS(RowRanges rg, int book, Scal<T>* sc, int par, const T* __restrict__ totalsA, const T* ap, const T* r, T* sv) {
	if (sc->done) return;
	bicgStepS<T, false>(rg, book, sc, sc->rrPing[par], totalsA[0], ap, r, sv);
}

// omega = (as.s) / (as.as) ; r = -omega as + s ; local ||r||^2 and r.r0   (ref:2259-2261, 2265)
template <typename T>
__global__ __launch_bounds__(TPB) void distBicgR(int n, Scal<T>* sc, const T* __restrict__ totalsB, const T* sv, const T* as, const T* r0, T* r,
                                                 T* partsC) {
	__shared__ T red[4];
	if (sc->done) return;
	bicgStepXR<T, false, false>(n, sc, totalsB[0], totalsB[1], red, nullptr, sv, as, r0, nullptr, r, partsC);
}

// The same with x = alpha p + (omega s + x) (ref:2264) folded in: s is read once for both, one launch instead of two.  Taken when the scalars
// go through the per-rank slots (the reduction behind this kernel is then a single-workgroup launch on the solver's own stream: there is no
// side-stream collective for a separate x update to run beside).
template <typename T>
__global__ __launch_bounds__(TPB) void distBicgRX(int n, Scal<T>* sc, const T* __restrict__ totalsB, const T* sv, const T* as, const T* r0, const T* p, T* r,
                                                  T* x, T* partsC) {
	__shared__ T red[4];
	if (sc->done) return;
	bicgStepXR<T, false, true>(n, sc, totalsB[0], totalsB[1], red, p, sv, as, r0, x, r, partsC);
}

// x = alpha p + (omega s + x)   (ref:2264) -- independent of the all-reduce of ||r||^2, r.r0 and runs beside it
template <typename T>
__global__ __launch_bounds__(TPB) void distBicgX(int n, const Scal<T>* __restrict__ sc, const T* p, const T* sv, T* x) {
	if (sc->done) return;
	const T alpha = sc->alpha, omega = sc->omega;
	const T* const in[3] = {sv, x, p};
	T* const out[1] = {x};
	streamMap<T, false, 3, 1>(n, in, out, [&](const T(&v)[3], T(&o)[1]) { o[0] = smmFma(alpha, v[2], smmFma(omega, v[0], v[1])); });
}

// resL2Norm, loop test, beta, p = beta (-omega ap + p) + r   (ref:2268-2277)
template <typename T>
__global__ __launch_bounds__(TPB) void distBicgP(RowRanges rg, int book, Scal<T>* sc, int par, const T* __restrict__ totalsC, T eps, const T* ap, const T* r, T* p) {
	if (sc->done) return;
	bicgStepP<T, false>(rg, book, sc, par, totalsC[0], totalsC[1], eps, ap, r, p);
}

template <typename T>
__global__ void distCgInit(const T* __restrict__ totals, Scal<T>* sc, T eps) {
	const T rr = totals[0];  // ref:2341
	sc->rrPing[0] = rr;
	sc->res = rr;
	sc->iters = 0;
	sc->done = 0;
	sc->status = SMM_SOLVER_MAX_ITERATIONS_REACHED;
	sc->flushIter = -1;
	if (eps * eps > rr) {  // ref:2342-2344: x stays untouched
		sc->done = 1;
		sc->status = SMM_SOLVER_SUCCESS;
	}
	sc->pad = sc->done;
}

// alpha = rr / (Ap.p) ; r = -alpha Ap + r ; local ||r||^2   (ref:2354-2375)
// (NT in the CG kernels: non-temporal loads / stores when the vectors cannot stay in the Infinity Cache anyway -- updateNT, as in smm_solvers.hip)
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void distCgR(int n, Scal<T>* sc, int par, const T* __restrict__ totalsA, const T* Ap, T* r, T* partsC, int alphaSlot) {
	__shared__ T red[4];
	if (cgSnapshotDone(sc)) return;
	cgStepR<T, NT>(n, sc, sc->rrPing[par], totalsA[0], red, Ap, r, partsC, alphaSlot);
}

// x = alpha p + xcur   (ref:2372)
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void distCgX(int n, const Scal<T>* __restrict__ sc, const T* p, const T* xcur, T* x) {
	if (sc->done) return;
	const T alpha = sc->alpha;
	const T* const in[2] = {p, xcur};
	T* const out[1] = {x};
	streamMap<T, NT, 2, 1>(n, in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(alpha, v[0], v[1]); });
}

// convergence test, beta, p = beta p + r   (ref:2377-2394).  book: as in distBicgP
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void distCgP(RowRanges rg, int book, Scal<T>* sc, int par, const T* __restrict__ totalsC, T eps, T* p, const T* r) {
	if (sc->done) return;
	const T rrNew = totalsC[0];
	const T rrOld = sc->rrPing[par];
	const bool converged = eps * eps > rrNew;
	if (book && blockIdx.x == 0 && threadIdx.x == 0) {
		sc->iters += 1;
		sc->res = rrNew;
		if (converged) {
			sc->done = 1;
			sc->status = SMM_SOLVER_SUCCESS;
		} else {
			sc->rrPing[par ^ 1] = rrNew;
		}
	}
	if (converged) return;
	const T beta = rrNew / rrOld;
	const T* const in[2] = {p, r};
	T* const out[1] = {p};
	rg.map<T, 2, 1, NT>(in, out, [&](const T(&v)[2], T(&o)[1]) { o[0] = smmFma(beta, v[0], v[1]); });
}

// The deferred x update of the single-GPU loop (cgLazyStep, smm_krylov_steps.h) in the row-partitioned one: the ring's vectors are
// halo-extended, 11 vector passes per iteration become 9.125.  Range-aware like distCgP (boundary rows first, then the bulk: each launch
// flushes its own rows).
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void distCgLazyP(RowRanges rg, int book, Scal<T>* sc, int par, const T* __restrict__ totalsC, T eps, LazyRing<T> ring, int cur,
                                                   int pending, int flush, int alphaSlot, const T* r, const T* xcur, T* x) {
	if (sc->pad) return;
	cgLazyStep<T, NT>(rg, book, sc, par, totalsC[0], eps, ring, cur, pending, flush, alphaSlot, r, xcur, x);
}

// what is left of distCgLazyP once the direction is formed in the SpMV
template <typename T, bool NT>
__global__ __launch_bounds__(TPB) void distCgFlushOnly(RowRanges rg, const Scal<T>* __restrict__ sc, LazyRing<T> ring, int cur, int pending, int scheduled, int iter,
                                                       int alphaSlot, const T* xcur, T* x) {
	cgFlushOnlyStep<T, NT>(rg, sc, ring, cur, pending, scheduled, iter, alphaSlot, xcur, x);
}

// Leaving the loop early must be the SAME decision on every rank (a rank that stops issuing iterations while another goes on leaves the
// other one alone in its next collective).  The `done` flag is formed from all-reduced -- hence identical -- numbers at the same
// iteration on every rank, so a BLOCKING read of it at fixed iteration numbers is consistent; the asynchronous mailbox of the single-GPU
// loops (whose answer depends on how far the host has run ahead) is not.  One pipeline drain every CHECK_EVERY iterations.
static int readDone(smm_hip_dist_csr* D, const int* d_done, hipStream_t s, int* done) {
	unsigned long long err = 0;
	SMM_HIP_TRY(hipMemcpyAsync(done, d_done, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_TRY(p2pPostErrRead(D, &err, s));
	SMM_TRY(boundedSync(D->comm, s));
	return p2pFailIf(D, err);
}

// A vector update whose result feeds the next SpMV, halo first: the boundary rows some peer receives in a small launch, the exchange posted
// right behind it, the bulk in a second launch -- the same expressions on the same operands, the same bits as one launch.
// LAUNCH(ranges, book) enqueues the update kernel on `s` for those rows; `book`: that launch does the kernel's scalar bookkeeping.
template <typename T, typename Launch>
static int updateThenExchange(smm_hip_dist_csr* D, T* ext, int kind, hipStream_t s, Launch&& launch) {
	if (D->haloFirst) {
		launch(D->boundary, 0);
		SMM_TRY(distExchangeBegin<T>(D, ext, kind, s));
		launch(D->bulk, 1);
	} else {
		launch(wholeRange(D->nLocal), 1);
		SMM_TRY(distExchangeBegin<T>(D, ext, kind, s));
	}
	return SMM_HIP_OK;
}

// many SpMVs ahead: both local blocks may take the index-free family (each rank decides for its own blocks; no collective involved)
// (the blocks' own configuration first: a block nobody has multiplied with yet still carries the handle's initial word, and the adoption
// below only moves a block that is on the STREAM family -- r05: the FIRST solve of a distributed matrix ran on the CSR kernels)
static int distBlocksReady(smm_hip_dist_csr* D, int maxIterations, hipStream_t s) {
	if (D->aLoc) SMM_TRY(ensureCsrReady(D->aLoc, s, true));
	if (D->aRem) SMM_TRY(ensureCsrReady(D->aRem, s, true));
	if (D->aLoc) SMM_TRY(adoptPatternForSolver(D->aLoc, maxIterations, s));
	if (D->aRem) SMM_TRY(adoptPatternForSolver(D->aRem, maxIterations, s));
	for (smm_hip_csr* piece : D->aRemK) SMM_TRY(adoptPatternForSolver(piece, maxIterations, s));
	return SMM_HIP_OK;
}

// the end of a loop: the scalars to the host with the error word of the bounded device-side waits, behind everything enqueued on `s`
template <typename T>
static int distLoopFinish(smm_hip_dist_csr* D, const Scal<T>* sc, Scal<T>* h, hipStream_t s) {
	unsigned long long p2pErr = 0;
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(h, sc, sizeof(*h), hipMemcpyDeviceToHost, s));
	SMM_TRY(p2pPostErrRead(D, &p2pErr, s));
	SMM_TRY(boundedSync(D->comm, s));
	return p2pFailIf(D, p2pErr);
}

// one more halo-extended vector of the CG loop, zeroed when first allocated (halo slots outside every recv segment are never read by A_rem;
// zero keeps them finite).  *there: whether the loop has it -- a failed allocation leaves the pointer null and is no error
template <typename T>
static int extVector(smm_hip_dist_csr* D, void** vec, hipStream_t s, bool* there) {
	*there = true;
	if (*vec) return SMM_HIP_OK;
	const size_t eb = static_cast<size_t>(std::max(1, D->extLen)) * sizeof(T);
	if (devAlloc(vec, eb) != SMM_HIP_OK) {
		(void)hipGetLastError();
		*vec = nullptr;
		*there = false;
		return SMM_HIP_OK;
	}
	SMM_HIP_TRY(hipMemsetAsync(*vec, 0, eb, s));
	return SMM_HIP_OK;
}

template <typename T>
static int distBicgstab(smm_hip_dist_csr* D, const T* b, T* x, int maxIterations, T eps, const smm_hip_precond* M, hipStream_t s, int* status,
                        int* iterations, T* resnorm) {
	SMM_TRY(checkDist<T>(D, "dist_bicgstab"));
	SMM_TRY(ensureInit());
	const int n = D->nLocal;
	if (n > 0 && (!b || !x)) {
		setError("dist_bicgstab: null vector");
		return SMM_HIP_ERR_INVALID;
	}
	// block-Jacobi by rank: M is this rank's preconditioner of its diagonal block A_loc, applied without
	// communication; with one rank it is the single-GPU preconditioner, with more a weaker one (iteration counts differ)
	const bool pre = M != nullptr && M->kind != SMM_PRECOND_NONE;
	SMM_TRY(precondAdmissible("dist_bicgstab", M, D->aLoc, SOLVER_DIST_LOCAL));
	D->reducedInKernel = false;  // (a call that failed between an SpMV and its reduction point must not leave the mark behind)
	D->totalsFinal = false;
	maxIterations = std::min(maxIterations, D->nGlobal);  // ref:2200
	if (maxIterations == -1) maxIterations = D->nGlobal;  // ref:2201-2203
	SMM_TRY(distBlocksReady(D, maxIterations, s));
	T *r = static_cast<T*>(D->r), *r0 = static_cast<T*>(D->r0), *ap = static_cast<T*>(D->ap), *as = static_cast<T*>(D->as);
	T *pExt = static_cast<T*>(D->pExt), *sExt = static_cast<T*>(D->sExt), *xExt = static_cast<T*>(D->xExt);
	T *p = pExt + D->ownOffset, *sv = sExt + D->ownOffset;
	T *partsA = static_cast<T*>(D->partsA), *partsB = static_cast<T*>(D->partsB), *partsC = static_cast<T*>(D->partsC);
	auto* sc = static_cast<Scal<T>*>(D->sc);
	if (pre && !D->scratch) SMM_TRY(devAlloc(&D->scratch, static_cast<size_t>(std::max(1, n)) * sizeof(T)));
	T* scratch = static_cast<T*>(D->scratch);
	hipEvent_t ev = nullptr;
	// Jacobi: x = rhs / diag is folded into the rows of the SpMV (smm_solvers.hip does the same on one GPU): no apply launch, no dot
	// launch -- 8 kernels per iteration like the unpreconditioned loop
	const T* jacobiDiag = pre && M->kind == SMM_PRECOND_JACOBI ? static_cast<const T*>(M->d_values) : nullptr;

	// r = b - A x (ref:2215) [; r = M^-1 r, ref:2217-2224]
	if (n > 0) SMM_HIP_TRY(hipMemcpyAsync(xExt + D->ownOffset, x, sizeof(T) * n, hipMemcpyDeviceToDevice, s));
	if (pre) {
		SMM_TRY(distMatvec<T>(D, xExt, 2, SMM_OP_SUB, b, scratch, 0, nullptr, nullptr, nullptr, s));
		SMM_TRY(precondApplyDev<T>(M, scratch, r, nullptr, s));
	} else {
		SMM_TRY(distMatvec<T>(D, xExt, 2, SMM_OP_SUB, b, r, 0, nullptr, nullptr, nullptr, s));
	}
	SMM_TRY(launchCopy2<T>(n, r, r0, p, s));                              // r0 = p = r, ref:2225-2226
	SMM_TRY(distExchangeBegin<T>(D, pExt, 0, s));                         // the halo of p travels while r.r0 is reduced
	distDots<T><<<NPART, TPB, 0, s>>>(n, r, r, nullptr, 1, partsC, nullptr);  // r.r0 with r0 == r, ref:2231
	if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsC, 1, partsC + PARTS_TOTALS, nullptr);
	SMM_TRY(allreduceTotals<T>(D, partsC, 1, s, &ev, 2));
	SMM_TRY(join(s, ev));
	distBicgInit<T><<<1, 1, 0, s>>>(partsC + PARTS_TOTALS, sc);

	const int* doneFlag = &sc->done;
	const int planned = std::max(1, maxIterations);  // do { } while: the body always runs once (ref:2232, 2277)
	for (int i = 0; i < planned; ++i) {
		if (i > 0 && i % CHECK_EVERY == 0) {
			int seen = 0;
			SMM_TRY(readDone(D, doneFlag, s, &seen));
			if (seen) break;
		}
		const int par = i & 1;
		// ap = [M^-1] A p ; ap.r0 (ref:2233-2243) -- the exchange of p was posted behind its update
		if (jacobiDiag) {
			SMM_TRY(distMatvecCompute<T>(D, pExt, SMM_OP_ASSIGN, nullptr, ap, 1, r0, partsA, doneFlag, s, jacobiDiag, 0));
		} else if (pre) {
			SMM_TRY(distMatvecCompute<T>(D, pExt, SMM_OP_ASSIGN, nullptr, scratch, 0, nullptr, nullptr, doneFlag, s));
			SMM_TRY(precondApplyDev<T>(M, scratch, ap, doneFlag, s));
			distDots<T><<<NPART, TPB, 0, s>>>(n, ap, r0, nullptr, 1, partsA, doneFlag);
			if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsA, 1, partsA + PARTS_TOTALS, doneFlag);
		} else {
			SMM_TRY(distMatvecCompute<T>(D, pExt, SMM_OP_ASSIGN, nullptr, ap, 1, r0, partsA, doneFlag, s, nullptr, 0));
		}
		SMM_TRY(allreduceTotals<T>(D, partsA, 1, s, &ev, 0, doneFlag));
		SMM_TRY(join(s, ev));
		SMM_TRY((updateThenExchange<T>(D, sExt, 1, s, [&](const RowRanges& rg, int book) {
			distBicgS<T><<<solverGrid(rg.rows()), TPB, 0, s>>>(rg, book, sc, par, partsA + PARTS_TOTALS, ap, r, sv);
		})));
		// as = [M^-1] A s ; as.as, as.s (ref:2249-2261)
		if (jacobiDiag) {
			SMM_TRY(distMatvecCompute<T>(D, sExt, SMM_OP_ASSIGN, nullptr, as, 2, sv, partsB, doneFlag, s, jacobiDiag, 1));
		} else if (pre) {
			SMM_TRY(distMatvecCompute<T>(D, sExt, SMM_OP_ASSIGN, nullptr, scratch, 0, nullptr, nullptr, doneFlag, s));
			SMM_TRY(precondApplyDev<T>(M, scratch, as, doneFlag, s));
			distDots<T><<<NPART, TPB, 0, s>>>(n, as, as, sv, 2, partsB, doneFlag);
			if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsB, 2, partsB + PARTS_TOTALS, doneFlag);
		} else {
			SMM_TRY(distMatvecCompute<T>(D, sExt, SMM_OP_ASSIGN, nullptr, as, 2, sv, partsB, doneFlag, s, nullptr, 1));
		}
		SMM_TRY(allreduceTotals<T>(D, partsB, 2, s, &ev, 1, doneFlag));
		SMM_TRY(join(s, ev));
		if (D->p2p) {
			distBicgRX<T><<<NPART, TPB, 0, s>>>(n, sc, partsB + PARTS_TOTALS, sv, as, r0, p, r, x, partsC);  // (r and x in one pass over s)
			SMM_TRY(allreduceTotals<T>(D, partsC, 2, s, &ev, 2, doneFlag));
		} else {
			distBicgR<T><<<NPART, TPB, 0, s>>>(n, sc, partsB + PARTS_TOTALS, sv, as, r0, r, partsC);
			distFinishSums<T><<<1, TPB, 0, s>>>(partsC, 2, partsC + PARTS_TOTALS, doneFlag);
			SMM_TRY(allreduceTotals<T>(D, partsC, 2, s, &ev, 2, doneFlag));  // (the communicator's collectives: on the side stream ...
			distBicgX<T><<<solverGrid(n), TPB, 0, s>>>(n, sc, p, sv, x);         // ... while x is updated)
		}
		SMM_TRY(join(s, ev));
		if (i + 1 < planned) {
			SMM_TRY((updateThenExchange<T>(D, pExt, 0, s, [&](const RowRanges& rg, int book) {
				distBicgP<T><<<solverGrid(rg.rows()), TPB, 0, s>>>(rg, book, sc, par, partsC + PARTS_TOTALS, eps, ap, r, p);
			})));
		} else {
			distBicgP<T><<<solverGrid(n), TPB, 0, s>>>(wholeRange(n), 1, sc, par, partsC + PARTS_TOTALS, eps, ap, r, p);  // the last pass: no SpMV follows
		}
	}
	SMM_TRY(distExchangeDrain<T>(D, pExt, s));  // (left early: the exchange posted for the pass that never ran)
	Scal<T> h;
	SMM_TRY(distLoopFinish(D, sc, &h, s));
	if (status) *status = h.iters > maxIterations ? SMM_SOLVER_MAX_ITERATIONS_REACHED : SMM_SOLVER_SUCCESS;  // ref:2279-2282
	if (iterations) *iterations = h.iters;
	if (resnorm) *resnorm = h.res;
	return pre ? precondTakeError(M, s) : SMM_HIP_OK;
}

template <typename T>
static int distCg(smm_hip_dist_csr* D, const T* b, const T* x0, T* x, int maxIterations, T eps, hipStream_t s, int* status, int* iterations,
                  T* resnorm2) {
	SMM_TRY(checkDist<T>(D, "dist_cg"));
	SMM_TRY(ensureInit());
	const int n = D->nLocal;
	if (n > 0 && (!b || !x0 || !x)) {
		setError("dist_cg: null vector");
		return SMM_HIP_ERR_INVALID;
	}
	D->reducedInKernel = false;
	D->totalsFinal = false;
	if (maxIterations == -1) maxIterations = D->nGlobal;  // ref:2345-2347 (no clamp otherwise)
	SMM_TRY(distBlocksReady(D, maxIterations, s));
	T *r = static_cast<T*>(D->r), *ap = static_cast<T*>(D->ap);
	T *pExt = static_cast<T*>(D->pExt), *xExt = static_cast<T*>(D->xExt);
	T* p = pExt + D->ownOffset;
	T *partsA = static_cast<T*>(D->partsA), *partsC = static_cast<T*>(D->partsC);
	auto* sc = static_cast<Scal<T>*>(D->sc);
	hipEvent_t ev = nullptr;
	// vectors beyond the caches: x deferred through a ring of LAZY_M more direction vectors (distCgLazyP); when they cannot be had, the eager loop
	bool lazy = n > 0 && static_cast<long long>(n) * static_cast<long long>(sizeof(T)) >= cgLazyMinBytes();
	T* ringExt[LAZY_M + 1] = {pExt};
	LazyRing<T> ring{};
	ring.p[0] = p;
	if (lazy) {
		for (int k = 0; k < LAZY_M && lazy; ++k) {
			SMM_TRY(extVector<T>(D, &D->lazyExt[k], s, &lazy));
			if (!lazy) break;
			ringExt[k + 1] = static_cast<T*>(D->lazyExt[k]);
			ring.p[k + 1] = ringExt[k + 1] + D->ownOffset;
		}
	}
	// ... and the next direction formed inside the local block's SpMV where that block is served by the 2.5-D constant-diagonal kernel and the
	// remote one is empty or thin (the slabs of a grid): the halo of r travels instead of p's, in a halo-extended r.  What travels differs from
	// the other loop forms, so the ranks must AGREE: decided once per solve by a vote (one small all-reduce; nothing is in flight yet)
	bool fuse = false;
	if (lazy && D->aLoc && constMarchFusable(D->aLoc, sizeof(T)) && D->recvs.size() <= static_cast<size_t>(P2P_MAX_WORLD) && D->chunks == 1) {
		bool thin = false;
		if (!D->remEmpty) SMM_TRY(thinUsable(D, s, &thin));
		fuse = D->remEmpty || thin;
	}
	if (fuse) SMM_TRY(extVector<T>(D, &D->rExt, s, &fuse));
	if (env::isSet(env::DIST_DEBUG)) {
		const smm_hip_csr* m = D->aLoc;
		fprintf(stderr, "libsmm_hip: dist_cg rank %d: lazy %d, local block fusable %d (family %d lanes %d state %d encoding %d const %d const_off %d clusters %d), remote empty %d thin rows %d, candidate %d\n",
		        D->comm->rank, lazy ? 1 : 0, m && constMarchFusable(m, sizeof(T)) ? 1 : 0, m ? m->family() : -1, m ? m->lanes() : -1, m ? static_cast<int>(m->pat_state.load()) : -1,
		        m ? m->pat_encoding : -1, m ? static_cast<int>(m->pat_const) : -1, m ? static_cast<int>(m->pat_const_off) : -1, m ? static_cast<int>(m->march_clusters) : -1,
		        D->remEmpty ? 1 : 0, D->nThin, fuse ? 1 : 0);
	}
	if (D->comm->world > 1) {
		long long votes = fuse ? 1 : 0;
		SMM_TRY(commAllreduceI64(D->comm, &votes, 1));
		fuse = votes == D->comm->world;
	}
	T* rExt = nullptr;
	if (fuse) {
		rExt = static_cast<T*>(D->rExt);
		r = rExt + D->ownOffset;
	}
	if (n > 0) SMM_HIP_TRY(hipMemcpyAsync(xExt + D->ownOffset, x0, sizeof(T) * n, hipMemcpyDeviceToDevice, s));
	SMM_TRY(distMatvec<T>(D, xExt, 2, SMM_OP_SUB, b, r, 0, nullptr, nullptr, nullptr, s));  // r = b - A x0, ref:2337
	SMM_TRY(launchCopy2<T>(n, r, p, nullptr, s));                                           // p = r, ref:2340
	distDots<T><<<NPART, TPB, 0, s>>>(n, r, r, nullptr, 1, partsC, nullptr);
	if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsC, 1, partsC + PARTS_TOTALS, nullptr);
	SMM_TRY(allreduceTotals<T>(D, partsC, 1, s, &ev, 2));
	SMM_TRY(join(s, ev));
	distCgInit<T><<<1, 1, 0, s>>>(partsC + PARTS_TOTALS, sc, eps);
	const int* doneFlag = &sc->done;
	T* lastExt = pExt;  // the vector the last posted exchange fills
	const bool nt3 = updateNT(n, sizeof(T), 3);
	HaloSegs segs{};
	for (const Seg& g : D->recvs) {
		if (segs.n < P2P_MAX_WORLD) {
			segs.off[segs.n] = g.offset;
			segs.cnt[segs.n++] = g.count;
		}
	}
	const RowRanges allRows = wholeRange(n);
	for (int i = 0; i < maxIterations; ++i) {
		if (i % CHECK_EVERY == 0) {  // i == 0: the early exit of ref:2342-2344 costs nothing more than this read
			int seen = 0;
			SMM_TRY(readDone(D, doneFlag, s, &seen));
			if (seen) break;
		}
		const int par = i & 1;
		const int cur = lazy ? i % (LAZY_M + 1) : 0, next = lazy ? (cur + 1) % (LAZY_M + 1) : 0;
		T* const curExt = ringExt[cur];
		T* const pc = ring.p[cur];
		if (fuse) {
			// the loop of smm_solvers.hip's cgDev with the direction formed INSIDE the SpMV: SpMV' (iteration i - 1's bookkeeping, p_i, A_loc p_i, the local
			// share of p.Ap) while r's halo is in flight, the thin remote block -- which forms the halo of p_i -- behind it, the flush of x (scheduled every LAZY_M-th
			// iteration, or because SpMV' found iteration i - 1 converged), the r update -- and r's halo on its way while ||r||^2 is reduced
			if (i == 0) {
				SMM_TRY(distExchangeBegin<T>(D, curExt, 0, s));
				SMM_TRY(distMatvecCompute<T>(D, curExt, SMM_OP_ASSIGN, nullptr, ap, 1, pc, partsA, doneFlag, s, nullptr, 0, SPMV_HALF_TILES));
			} else {
				const int prev = (i - 1) % (LAZY_M + 1);
				auto& pend = D->pending;
				const bool exchange = pend.active;
				pend.active = false;
				const CgFuseBook<T> bk{&sc->pad, sc->rrPing, &sc->res, &sc->iters, &sc->done, &sc->status, &sc->flushIter};
				CgFuseArgs<T> f{r, pc, bk, nullptr, eps, (i - 1) & 1, i};
				f.totalsC = partsC + PARTS_TOTALS;
				f.extraFlags = SPMV_FINISH | (exchange && pend.async ? SPMV_LEAVE_ROOM : 0);
				if (!launchConstMarchFusedP<T>(D->aLoc, ring.p[prev], ap, partsA, doneFlag, f, s)) {
					setError("dist_cg: the fused SpMV could not be launched");
					return SMM_HIP_ERR_HIP;
				}
				++D->cgFused;
				if (exchange && pend.landed[0]) {  // (also a rank that only sends: r's boundary rows must not be rewritten before they have left)
					profWaitWaiting(pend.waitSlot[0], s);
					SMM_HIP_TRY(hipStreamWaitEvent(s, pend.landed[0], 0));
				}
				D->totalsFinal = true;
				if (!D->remEmpty) {  // the thin remote block, forming the halo of p_i as it goes (and storing it for iteration i + 1)
					ThinForm<T> fm;
					fm.pOldExt = ringExt[prev];
					fm.rExt = rExt;
					fm.pNewExt = curExt;
					fm.sc = sc;
					fm.totalsC = partsC + PARTS_TOTALS;
					fm.par = (i - 1) & 1;
					fm.segs = segs;
					SMM_TRY(launchThinRemote<T>(D, curExt, false, ap, 1, pc, partsA, doneFlag, s, &fm));
				}
				SMM_LAUNCH_UPDATE(distCgFlushOnly, updateNT(n, sizeof(T), 5), solverGrid(n), s, allRows, sc, ring, prev, (i - 1) % LAZY_M + 1, i % LAZY_M == 0 ? 1 : 0, i,
				                (i - 1) % LAZY_M, i <= LAZY_M ? x0 : x, x);
			}
			SMM_TRY(allreduceTotals<T>(D, partsA, 1, s, &ev, 0, doneFlag));
			SMM_TRY(join(s, ev));
			SMM_LAUNCH_UPDATE(distCgR, nt3, NPART, s, n, sc, par, partsA + PARTS_TOTALS, ap, r, partsC, i % LAZY_M);
			if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsC, 1, partsC + PARTS_TOTALS, doneFlag);
			SMM_TRY(allreduceTotals<T>(D, partsC, 1, s, &ev, 2, doneFlag));
			const bool lastPass = i + 1 >= maxIterations;
			if (!lastPass) {
				SMM_TRY(distExchangeBegin<T>(D, rExt, 1, s));  // r's halo travels behind the reduction of ||r||^2 and beside the next SpMV'
				lastExt = rExt;
			}
			SMM_TRY(join(s, ev));
			if (lastPass) {  // the last planned iteration has no SpMV' behind it: its bookkeeping and the rest of x
				SMM_LAUNCH_UPDATE(distCgLazyP, nt3, solverGrid(n), s, allRows, 1, sc, par, partsC + PARTS_TOTALS, eps, ring, cur, i % LAZY_M + 1, 1, i % LAZY_M, r,
				                i < LAZY_M ? x0 : x, x);
			}
			continue;
		}
		if (i == 0) SMM_TRY(distExchangeBegin<T>(D, curExt, 0, s));  // (later passes: posted behind the update of p)
		SMM_TRY(distMatvecCompute<T>(D, curExt, SMM_OP_ASSIGN, nullptr, ap, 1, pc, partsA, doneFlag, s, nullptr, 0, SPMV_HALF_TILES));  // Ap = A p ; p.Ap, ref:2353-2354
		SMM_TRY(allreduceTotals<T>(D, partsA, 1, s, &ev, 0, doneFlag));
		SMM_TRY(join(s, ev));
		SMM_LAUNCH_UPDATE(distCgR, nt3, NPART, s, n, sc, par, partsA + PARTS_TOTALS, ap, r, partsC, i % LAZY_M);
		if (!D->p2p) distFinishSums<T><<<1, TPB, 0, s>>>(partsC, 1, partsC + PARTS_TOTALS, doneFlag);
		SMM_TRY(allreduceTotals<T>(D, partsC, 1, s, &ev, 2, doneFlag));           // (the communicator's collectives: on the side stream ...
		if (!lazy) SMM_LAUNCH_UPDATE(distCgX, nt3, solverGrid(n), s, n, sc, pc, i == 0 ? x0 : x, x);  // ... while x is updated; ref:2351, 2395)
		SMM_TRY(join(s, ev));
		const bool last = i + 1 >= maxIterations;
		if (lazy) {
			const int pending = i % LAZY_M + 1;
			const int flush = (pending == LAZY_M || last) ? 1 : 0;
			const T* xc = i < LAZY_M ? x0 : x;  // (until the first scheduled flush x has not been written: ref:2351, 2395)
			auto launch = [&](const RowRanges& rg, int book) {
				SMM_LAUNCH_UPDATE(distCgLazyP, nt3, solverGrid(rg.rows()), s, rg, book, sc, par, partsC + PARTS_TOTALS, eps, ring, cur, pending, flush, i % LAZY_M, r, xc, x);
			};
			if (!last) {
				SMM_TRY((updateThenExchange<T>(D, ringExt[next], 0, s, launch)));
				lastExt = ringExt[next];
			} else {
				launch(allRows, 1);
			}
		} else if (!last) {
			SMM_TRY((updateThenExchange<T>(D, pExt, 0, s, [&](const RowRanges& rg, int book) {
				SMM_LAUNCH_UPDATE(distCgP, nt3, solverGrid(rg.rows()), s, rg, book, sc, par, partsC + PARTS_TOTALS, eps, p, r);
			})));
		} else {
			SMM_LAUNCH_UPDATE(distCgP, nt3, solverGrid(n), s, allRows, 1, sc, par, partsC + PARTS_TOTALS, eps, p, r);
		}
	}
	SMM_TRY(distExchangeDrain<T>(D, lastExt, s));
	Scal<T> h;
	SMM_TRY(distLoopFinish(D, sc, &h, s));
	if (status) *status = h.status;
	if (iterations) *iterations = h.iters;
	if (resnorm2) *resnorm2 = h.res;
	return SMM_HIP_OK;
}

void preloadDistLoopsUnit() { preloadUnitOf(reinterpret_cast<const void*>(distFinishSums<double>)); }

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_dist_bicgstab_dev_f32(smm_hip_dist_csr* D, const float* d_b, float* d_x, int maxIterations, float eps, const smm_hip_precond* M_loc,
                                  smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distBicgstab<float>(D, d_b, d_x, maxIterations, eps, M_loc, pickStream(stream), solver_status, iterations, resnorm));
}
int smm_hip_dist_bicgstab_dev_f64(smm_hip_dist_csr* D, const double* d_b, double* d_x, int maxIterations, double eps, const smm_hip_precond* M_loc,
                                  smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distBicgstab<double>(D, d_b, d_x, maxIterations, eps, M_loc, pickStream(stream), solver_status, iterations, resnorm));
}

int smm_hip_dist_cg_dev_f32(smm_hip_dist_csr* D, const float* d_b, const float* d_x0, float* d_x, int maxIterations, float eps,
                            smm_hip_stream stream, int* solver_status, int* iterations, float* resnorm2) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distCg<float>(D, d_b, d_x0, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2));
}
int smm_hip_dist_cg_dev_f64(smm_hip_dist_csr* D, const double* d_b, const double* d_x0, double* d_x, int maxIterations, double eps,
                            smm_hip_stream stream, int* solver_status, int* iterations, double* resnorm2) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distCg<double>(D, d_b, d_x0, d_x, maxIterations, eps, pickStream(stream), solver_status, iterations, resnorm2));
}

}  // extern "C"
