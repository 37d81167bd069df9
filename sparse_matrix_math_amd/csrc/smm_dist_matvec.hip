// smm_dist_matvec.hip -- one row-partitioned SpMV in two halves (overview: smm_dist.hip): posting the halo exchange, the local block while
// it is in flight, the remote block -- in the same launch, as a launch over a thin block's rows, or as the general second launch -- and the
// all-reduce of the dot products that rode along; smm_hip_dist_spmv_dev_*.
#include <algorithm>

#include "smm_dist.h"

namespace smm {

// ---- one row-partitioned SpMV in two halves ---------------------------------------------------------------------------------------
// distExchangeBegin: the boundary slices of `ext`'s owned part are final on `s` -- post the halo exchange (side stream; peer-to-peer
// pushes or the communicator's grouped send / receive, in one piece or in `chunks`).  Called right behind the small "boundary" launch
// of a vector update (halo first), so that the transfer starts before the bulk of the update has run.
// distMatvecCompute: out = op(lhs, A ext) on the owned rows: the local block while the halo is in flight, then -- once it has landed --
// the remote block(s), with the dot products of the freshly computed vector (dotMode / w1 / parts as in launchSpmv; parts a finishing
// buffer) and the Jacobi division in the epilogue of the launch that completes a row.
static bool p2pHaloOn(const smm_hip_dist_csr* D) { return D->p2p && D->p2p->haloOn; }

// the device word the one-launch SpMV polls, and where an expired wait of it is recorded
static unsigned long long* splitErrWord(smm_hip_dist_csr* D) {
	if (D->p2p) return &D->p2p->hdr()->err;
	return D->splitSync ? D->splitSync + P2P_KINDS : nullptr;
}
// The one-launch SpMV is taken behind the peer-to-peer halo (the kernels it waits for are this library's own few workgroups, for which its grid
// leaves room) and wherever the exchange has completed before the launch is enqueued (the host-callback communicator: same stream).  Behind an
// RCCL exchange (the collectives, the hybrid) the two launches stay: a grid that waits inside the kernel must not depend on a library kernel
// whose resource needs are not ours to know finding room beside it.
static bool splitWordWanted(const smm_hip_dist_csr* D) {
	if (!D->splitAllowed || !D->splitSync || D->remEmpty || D->chunks != 1) return false;
	if (D->p2p && D->p2p->haloOn) return !D->sharedGpu || D->splitForced;  // (ranks that share a card: the two launches, see p2pSetup)
	return D->labWindow != 0 || D->comm->kind != SMM_COMM_RCCL;
}

template <typename T>
int distExchangeBegin(smm_hip_dist_csr* D, T* ext, int kind, hipStream_t s) {
	smm_hip_comm* c = D->comm;
	auto& pend = D->pending;
	pend = smm_hip_dist_csr::Pending{};
	const bool exchange = !D->sends.empty() || !D->recvs.empty();
	if (D->labWindow != 0 && !D->remEmpty) {
		// one rank, "remote" entries by distance (measurements): nothing travels, but the word is raised from the communicator's stream behind
		// the update -- the one-launch SpMV takes exactly the path it takes behind a real exchange
		hipStream_t cs = c->stream;
		noteStream(cs);
		pend.active = true;
		pend.kind = kind;
		pend.async = true;
		SMM_TRY(orderAfter(c, s, cs));
		if (splitWordWanted(D)) {
			pend.landSeq = ++D->landSeq[kind];
			launchSplitSignal(D->splitSync + kind, pend.landSeq, cs);
		}
		pend.landed[0] = takeEvent(c);
		SMM_HIP_TRY(hipEventRecord(pend.landed[0], cs));
		pend.waitSlot[0] = profWaitAwaited(cs);
		return SMM_HIP_OK;
	}
	if (p2pHaloOn(D) && !exchange) {
		// A rank that neither sends nor receives may still RELAY (planRelays picks by ring distance alone: a decoupled diagonal block in a
		// world >= 3): its forwards must run, and its sequence numbers must advance, with every exchange of the peers -- r05 returned here
		// before looking at nFwd, and every solve of such a world expired.  Nothing of `ext` is read or written: no ordering
		// against `s`, no event for `s` to wait for, nothing pending.
		hipStream_t cs = c->stream;
		noteStream(cs);
		return p2pHaloLaunch<T>(D, ext, kind, cs);
	}
	if (!exchange) return SMM_HIP_OK;
	pend.active = true;
	pend.kind = kind;
	if (p2pHaloOn(D)) {
		hipStream_t cs = c->stream;
		noteStream(cs);
		SMM_TRY(orderAfter(c, s, cs));
		SMM_TRY(p2pHaloLaunch<T>(D, ext, kind, cs));
		pend.seq = D->p2p->haloSeq[kind];
		// the land kernel (waits for every part of every segment, then landing area -> halo of `ext`) runs on the side stream as well, beside
		// the local block: the solver's stream only waits for its event, as it waits for a collective exchange
		// (r06: the land kernel raises the word the one-launch SpMV polls itself -- write-through stores, drained, then the word: no launch behind it)
		if (splitWordWanted(D)) pend.landSeq = ++D->landSeq[kind];
		SMM_TRY(p2pLandLaunch<T>(D, ext, kind, pend.seq, cs, pend.landSeq ? D->splitSync + kind : nullptr, pend.landSeq));
		pend.landed[0] = takeEvent(c);
		SMM_HIP_TRY(hipEventRecord(pend.landed[0], cs));
		pend.waitSlot[0] = profWaitAwaited(cs);
		pend.async = true;
		return SMM_HIP_OK;
	}
	hipStream_t cs = c->kind == SMM_COMM_RCCL ? c->stream : s;  // the callback kind blocks anyway
	noteStream(cs);
	SMM_TRY(orderAfter(c, s, cs));
	pend.async = cs != s;
	if (D->chunks > 1) {
		// (`chunks` is agreed by all ranks at create time and decides ALONE which form of the exchange runs: a rank whose own A_rem is empty --
		// one-sided / upwind stencils, any structurally non-symmetric matrix: it sends but receives nothing -- must still post the K piece-sized
		// sends its peers' K receives are waiting for; r04 tested `!remEmpty` as well and such a rank fell through to ONE full-count exchange:
		// mismatched RCCL call sequences, a hang or a corrupt halo.  ADVICE r04.)
		// The halo in pieces: every piece is an exchange of its own on the communicator's stream (all of them enqueued at once, so the links
		// never idle between them)
		for (int k = 0; k < D->chunks; ++k) {
			SMM_TRY(commExchange<T>(c, ext, D->sendsK[static_cast<size_t>(k)], D->recvsK[static_cast<size_t>(k)], cs));
			if (cs != s) {
				pend.landed[k] = takeEvent(c);
				SMM_HIP_TRY(hipEventRecord(pend.landed[k], cs));
				pend.waitSlot[k] = profWaitAwaited(cs);
			}
		}
		return SMM_HIP_OK;
	}
	SMM_TRY(commExchange<T>(c, ext, D->sends, D->recvs, cs));
	if (splitWordWanted(D)) {  // (behind the grouped receive / the staged copies, on the stream they ran on)
		pend.landSeq = ++D->landSeq[kind];
		launchSplitSignal(D->splitSync + kind, pend.landSeq, cs);
	}
	if (cs != s) {
		pend.landed[0] = takeEvent(c);
		SMM_HIP_TRY(hipEventRecord(pend.landed[0], cs));
		pend.waitSlot[0] = profWaitAwaited(cs);
	}
	return SMM_HIP_OK;
}

// The second half of a row-partitioned SpMV whose remote block is THIN (smm_hip_dist_csr::thinRows): out[row] (+|-)= A_rem[row] . ext for the
// listed rows only -- one lane per row, the row's entries in order: the sum the one-lane kernels form -- where the general form passes over
// every row of out[] to add nothing to most of them and to read them for the dot products.  The dot products were taken by the LOCAL
// launch over the half-finished vector (its totals are in `totals`); this launch adds what its rows change: with o = a + d,
//   o . w = a . w + d . w          o . o = a . a + d (a + o)
// (the same numbers up to the order of the additions: the partial sums of a rank are not the reference's in any form).  The workgroups'
// shares go through a buffer of their own; thinFinishKernel adds them to `totals` in a fixed order.
constexpr int THIN_MAX_GRID = NPART;
template <typename T, bool FORM>
__global__ __launch_bounds__(TPB) void thinRemoteKernel(int nThin, const int* __restrict__ rowsList, const int* __restrict__ start, const int* __restrict__ positions,
                                                        const T* __restrict__ values, const T* __restrict__ ext, int subtract, T* out, int dotMode,
                                                        const T* __restrict__ w1, T* __restrict__ partsThin, const int* __restrict__ doneFlag, ThinForm<T> fm) {
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	T beta = T(0);
	if constexpr (FORM) {
		beta = fm.totalsC[0] / fm.sc->rrPing[fm.par];
		for (int g = 0; g < fm.segs.n; ++g) {
			const int base = fm.segs.off[g];
			for (int i = blockIdx.x * TPB + threadIdx.x; i < fm.segs.cnt[g]; i += gridDim.x * TPB) {
				fm.pNewExt[base + i] = smmFma(beta, fm.pOldExt[base + i], fm.rExt[base + i]);
			}
		}
	}
	T acc0 = T(0), acc1 = T(0);
	for (int k = blockIdx.x * TPB + threadIdx.x; k < nThin; k += gridDim.x * TPB) {
		const int row = rowsList[k];
		const int e = start[row + 1];
		T sum = T(0);
		for (int j = start[row]; j < e; ++j) {
			const int c = positions[j];
			T xv;
			if constexpr (FORM) xv = smmFma(beta, fm.pOldExt[c], fm.rExt[c]);
			else xv = ext[c];
			sum = smmFma(values[j], xv, sum);
		}
		const T a = out[row];
		const T o = subtract ? a - sum : a + sum;
		out[row] = o;
		if (dotMode) {
			const T dlt = subtract ? -sum : sum;
			if (dotMode == 2) acc0 += dlt * (a + o);
			acc1 += dlt * w1[row];
		}
	}
	if (!dotMode) return;
	if (dotMode == 2) {
		const T s0 = blockSum256(acc0, red);
		if (threadIdx.x == 0) partsThin[blockIdx.x] = s0;
	}
	const T s1 = blockSum256(acc1, red);
	if (threadIdx.x == 0) partsThin[(dotMode == 2 ? NPART : 0) + blockIdx.x] = s1;
}
// (a launch of its own, started without a gap, instead of a ticket taken by every workgroup of a kernel that lasts microseconds: as distFinishSums)
template <typename T>
__global__ __launch_bounds__(TPB) void thinFinishKernel(const T* __restrict__ partsThin, int groups, int nsets, T* totals, const int* __restrict__ doneFlag) {
	__shared__ T red[4];
	if (doneFlag && *doneFlag) return;
	for (int k = 0; k < nsets; ++k) {
		T acc = T(0);
		for (int i = threadIdx.x; i < groups; i += TPB) acc += partsThin[(nsets == 2 ? k * NPART : 0) + i];
		const T s = blockSum256(acc, red);
		if (threadIdx.x == 0) totals[k] += s;
	}
}

// whether the thin form serves this matrix now (the remote block's kernel configuration is settled first: it decides the lanes per row)
int thinUsable(smm_hip_dist_csr* D, hipStream_t s, bool* usable) {
	*usable = false;
	if (D->nThin <= 0 || D->chunks != 1) return SMM_HIP_OK;
	SMM_TRY(ensureCsrReady(D->aRem, s, true));
	*usable = D->aRem->lanes() == 1;
	return SMM_HIP_OK;
}
// out[listed rows] (+|-)= A_rem . ext, the launch's share of the dot products added to the totals the local launch left in `parts`; form: the
// halo of `ext` is formed here (fused ConjugateGradient), not read
template <typename T>
int launchThinRemote(smm_hip_dist_csr* D, const T* ext, bool subtract, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
                     const ThinForm<T>* form) {
	const int g = std::max(1, std::min(THIN_MAX_GRID, (D->nThin + TPB - 1) / TPB));
	const int* startRem = static_cast<const int*>(D->arrays[0]) + D->nLocal + 1;
	if (form) {
		thinRemoteKernel<T, true><<<g, TPB, 0, s>>>(D->nThin, D->thinRows, startRem, static_cast<const int*>(D->arrays[4]), static_cast<const T*>(D->arrays[5]), ext,
		                                           subtract ? 1 : 0, out, dotMode, w1, static_cast<T*>(D->partsThin), doneFlag, *form);
	} else {
		thinRemoteKernel<T, false><<<g, TPB, 0, s>>>(D->nThin, D->thinRows, startRem, static_cast<const int*>(D->arrays[4]), static_cast<const T*>(D->arrays[5]), ext,
		                                            subtract ? 1 : 0, out, dotMode, w1, static_cast<T*>(D->partsThin), doneFlag, ThinForm<T>{});
	}
	if (dotMode) thinFinishKernel<T><<<1, TPB, 0, s>>>(static_cast<const T*>(D->partsThin), g, dotMode == 2 ? 2 : 1, parts + PARTS_TOTALS, doneFlag);
	SMM_HIP_TRY(hipGetLastError());
	D->totalsFinal = dotMode != 0;
	++D->matvecsThin;
	return SMM_HIP_OK;
}

// locFlags: flags of the LOCAL block's launch beyond those formed here (SPMV_HALF_TILES: ConjugateGradient's launches, smm_internal.h)
template <typename T>
int distMatvecCompute(smm_hip_dist_csr* D, T* ext, int op, const T* lhs, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
                      const T* jacobiDiag, int slotPoint, int locFlags) {
	const T* own = ext + D->ownOffset;
	auto& pend = D->pending;
	const bool exchange = pend.active;
	pend.active = false;
	const int finish = dotMode && !D->p2p ? SPMV_FINISH : 0;  // (peer to peer: the slot kernel adds the partials itself)
	// jacobiDiag (op must be SMM_OP_ASSIGN): out = (A x) / diag with the division folded into the launch that completes a row -- the
	// local block's when nothing is remote, else the remote block's epilogue ("add, then divide"): the loop then has the kernel count
	// of the unpreconditioned one, and the dot products of the divided vector ride in the same epilogue
	if (D->remEmpty && !exchange) {
		if (jacobiDiag) return launchSpmv<T>(D->aLoc, op, jacobiDiag, own, out, dotMode, w1, parts, doneFlag, s, finish | SPMV_DIV_LHS | locFlags);
		return launchSpmv<T>(D->aLoc, op, lhs, own, out, dotMode, w1, parts, doneFlag, s, finish | locFlags);
	}
	// ONE launch for both halves where the blocks allow it (smm_spmv_split.hip; r06): the local half of the workgroup's rows, a bounded wait for the
	// word this exchange raises, the remote half -- the arithmetic of the two launches below, bit for bit, without the second ramp and tail, the
	// second pass over out[] and the kernel boundary behind the exchange
	if (exchange && pend.landSeq != 0 && !D->remEmpty) {
		SMM_TRY(ensureCsrReady(D->aLoc, s, true));
		SMM_TRY(ensureCsrReady(D->aRem, s, true));
		// peer-to-peer scalars: the launch finishes its dot products and runs their reduction point in its last workgroup (slotPoint: which one)
		P2PSlotArgs slots{};
		const bool fuseSlots = D->p2p && dotMode && slotPoint >= 0;
		if (fuseSlots) {
			P2PState* P = D->p2p;
			slots.peers = P->peers;
			slots.world = P->world;
			slots.me = P->rank;
			slots.point = slotPoint;
			slots.count = dotMode == 2 ? 2 : 1;
			slots.seq = P->redSeq[slotPoint] + 1;
			slots.ticks = P->ticks;
		}
		const int st = launchSpmvSplit<T>(D->aLoc, D->aRem, op, lhs, jacobiDiag, own, ext, out, dotMode, w1, parts, doneFlag,
		                                  (fuseSlots ? SPMV_FINISH : finish) | (jacobiDiag ? SPMV_ADD_DIV : 0), D->splitSync + pend.kind, pend.landSeq, splitErrWord(D),
		                                  p2pTicks(), s, fuseSlots ? &slots : nullptr, D->splitSumsLdsMax, D->splitSync + P2P_KINDS + 1);
		if (st == SMM_HIP_OK) {
			if (fuseSlots) {
				++D->p2p->redSeq[slotPoint];
				D->reducedInKernel = true;
			}
			++D->matvecsSplit;
			return SMM_HIP_OK;  // (the kernel itself waited for the halo: `s` needs no event of the communicator's stream)
		}
		if (st < 0) return st;
	}
	// a THIN remote block (at most an eighth of the rows hold a remote entry; one lane per row; no Jacobi division in the epilogue): the local
	// launch takes the dot products and finishes them, the remote half is a launch over the listed rows that adds its share to the totals
	bool thin = false;
	if (!jacobiDiag) SMM_TRY(thinUsable(D, s, &thin));
	if (thin) {
		SMM_TRY(launchSpmv<T>(D->aLoc, op, lhs, own, out, dotMode, w1, parts, doneFlag, s,
		                      (dotMode ? SPMV_FINISH : 0) | (exchange && pend.async ? SPMV_LEAVE_ROOM : 0) | locFlags));
		if (exchange && pend.landed[0]) {
			profWaitWaiting(pend.waitSlot[0], s);
			SMM_HIP_TRY(hipStreamWaitEvent(s, pend.landed[0], 0));
		}
		return launchThinRemote<T>(D, ext, op == SMM_OP_SUB, out, dotMode, w1, parts, doneFlag, s);
	}
	if (exchange && !D->remEmpty) ++D->matvecsTwo;
	// the local block runs while the halo is in flight; the exchange is itself a kernel (a few workgroups per peer), and the persistent
	// SpMV grid would otherwise take every workgroup slot of the chip until it ends: it leaves one CU per XCD's worth free
	SMM_TRY(launchSpmv<T>(D->aLoc, op, lhs, own, out, 0, nullptr, nullptr, doneFlag, s, (exchange && pend.async ? SPMV_LEAVE_ROOM : 0) | locFlags));
	const int remOp = op == SMM_OP_SUB ? SMM_OP_SUB : SMM_OP_ADD;
	if (exchange && D->chunks > 1 && !D->p2p) {
		// part k of A_rem reads only piece k and starts as soon as THAT piece has landed: out = ((A_loc x + A_rem,0 x) + A_rem,1 x) + ... -- each
		// part a row sum of its own, added in piece order (deterministic; differs from the one-piece form only in where the row sum is cut)
		const int K = D->chunks;
		for (int k = 0; k < K; ++k) {
			if (pend.landed[k]) {
				profWaitWaiting(pend.waitSlot[k], s);
				SMM_HIP_TRY(hipStreamWaitEvent(s, pend.landed[k], 0));
			}
			const bool last = k == K - 1;
			if (!last) {
				if (D->nnzRemK[static_cast<size_t>(k)] == 0) continue;  // nothing of A_rem reads this piece (the last part always runs: it carries the epilogue)
				SMM_TRY(launchSpmv<T>(D->aRemK[static_cast<size_t>(k)], remOp, out, ext, out, 0, nullptr, nullptr, doneFlag, s, 0));
			} else if (jacobiDiag) {
				return launchSpmv<T>(D->aRemK[static_cast<size_t>(k)], SMM_OP_ADD, out, ext, out, dotMode, w1, parts, doneFlag, s, finish | SPMV_ADD_DIV, jacobiDiag);
			} else {
				return launchSpmv<T>(D->aRemK[static_cast<size_t>(k)], remOp, out, ext, out, dotMode, w1, parts, doneFlag, s, finish);
			}
		}
	} else if (exchange && pend.landed[0]) {
		profWaitWaiting(pend.waitSlot[0], s);  // (profiling on: how long A_rem waits for the halo after A_loc has ended -- the exposed part of the exchange)
		SMM_HIP_TRY(hipStreamWaitEvent(s, pend.landed[0], 0));
	}
	if (jacobiDiag) return launchSpmv<T>(D->aRem, SMM_OP_ADD, out, ext, out, dotMode, w1, parts, doneFlag, s, finish | SPMV_ADD_DIV, jacobiDiag);
	return launchSpmv<T>(D->aRem, remOp, out, ext, out, dotMode, w1, parts, doneFlag, s, finish);
}

// both halves back to back (the set-up SpMVs, the stand-alone distributed SpMV)
template <typename T>
int distMatvec(smm_hip_dist_csr* D, T* ext, int kind, int op, const T* lhs, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
               const T* jacobiDiag) {
	SMM_TRY(distExchangeBegin<T>(D, ext, kind, s));
	return distMatvecCompute<T>(D, ext, op, lhs, out, dotMode, w1, parts, doneFlag, s, jacobiDiag);
}

// all-reduce of the totals of a finishing buffer on the side stream; *joined = event the caller's stream must wait for (null when
// nothing is pending)
template <typename T>
int allreduceTotals(smm_hip_dist_csr* D, T* parts, int count, hipStream_t s, hipEvent_t* joined, int point, const int* doneFlag) {
	smm_hip_comm* c = D->comm;
	*joined = nullptr;
	const bool finished = D->totalsFinal;  // (the thin form: the rank's totals are in place)
	D->totalsFinal = false;
	if (D->reducedInKernel) {  // (the one-launch SpMV in front ran this point in its last workgroup)
		D->reducedInKernel = false;
		return SMM_HIP_OK;
	}
	if (c->kind == SMM_COMM_SELF && !D->p2p) return SMM_HIP_OK;  // (one rank with the slots: the lab's SMM_HIP_LAB_SELF_P2P)
	T* totals = parts + PARTS_TOTALS;
	// peer to peer: ONE single-workgroup kernel on the solver's own stream writes this rank's totals into every rank's slot, waits for all
	// slots of this sequence number and adds them in rank order (smm_p2p.h) -- no collective launch, no cross-stream events
	if (D->p2p) return p2pAllreduceLaunch<T>(D, point, totals, count, doneFlag, s, finished ? nullptr : parts);  // (else it adds the rank's partials itself: nobody finished them)
	if (c->kind == SMM_COMM_HOST) return commAllreduce<T>(c, totals, count, s);
	noteStream(c->stream);
	SMM_TRY(orderAfter(c, s, c->stream));
	SMM_TRY(commAllreduce<T>(c, totals, count, c->stream));
	*joined = takeEvent(c);
	SMM_HIP_TRY(hipEventRecord(*joined, c->stream));
	return SMM_HIP_OK;
}

int join(hipStream_t s, hipEvent_t e) {
	if (e) SMM_HIP_TRY(hipStreamWaitEvent(s, e, 0));
	return SMM_HIP_OK;
}

// an exchange that was posted but whose SpMV never runs (the loop was left): complete in itself on the side stream (the peer-to-peer land
// kernel empties the landing area and acknowledges there); the solver's stream only has to stay behind it
template <typename T>
int distExchangeDrain(smm_hip_dist_csr* D, T* ext, hipStream_t s) {
	auto& pend = D->pending;
	if (!pend.active) return SMM_HIP_OK;
	pend.active = false;
	(void)ext;
	for (hipEvent_t e : pend.landed) {
		if (e) SMM_HIP_TRY(hipStreamWaitEvent(s, e, 0));  // (the next use of `ext` on `s` must not overtake the receive)
	}
	return SMM_HIP_OK;
}

template <typename T>
int checkDist(const smm_hip_dist_csr* D, const char* who) {
	if (!D || D->dtype != dtypeOf<T>()) {
		setError("%s: null distributed matrix or dtype mismatch", who);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int distSpmv(smm_hip_dist_csr* D, int op, const T* lhs, const T* xOwn, T* out, hipStream_t s) {
	SMM_TRY(checkDist<T>(D, "dist_spmv"));
	SMM_TRY(ensureInit());
	if (op < SMM_OP_ASSIGN || op > SMM_OP_SUB || (D->nLocal > 0 && (!xOwn || !out || (op != SMM_OP_ASSIGN && !lhs)))) {
		setError("dist_spmv: bad op or null vector");
		return SMM_HIP_ERR_INVALID;
	}
	T* xExt = static_cast<T*>(D->xExt);
	if (D->nLocal > 0) SMM_HIP_TRY(hipMemcpyAsync(xExt + D->ownOffset, xOwn, sizeof(T) * D->nLocal, hipMemcpyDeviceToDevice, s));
	return distMatvec<T>(D, xExt, 2, op, lhs, out, 0, nullptr, nullptr, nullptr, s);
}

template int distExchangeBegin<float>(smm_hip_dist_csr*, float*, int, hipStream_t);
template int launchThinRemote<float>(smm_hip_dist_csr*, const float*, bool, float*, int, const float*, float*, const int*, hipStream_t, const ThinForm<float>*);
template int distMatvecCompute<float>(smm_hip_dist_csr*, float*, int, const float*, float*, int, const float*, float*, const int*, hipStream_t, const float*, int, int);
template int distMatvec<float>(smm_hip_dist_csr*, float*, int, int, const float*, float*, int, const float*, float*, const int*, hipStream_t, const float*);
template int allreduceTotals<float>(smm_hip_dist_csr*, float*, int, hipStream_t, hipEvent_t*, int, const int*);
template int distExchangeDrain<float>(smm_hip_dist_csr*, float*, hipStream_t);
template int checkDist<float>(const smm_hip_dist_csr*, const char*);
template int distExchangeBegin<double>(smm_hip_dist_csr*, double*, int, hipStream_t);
template int launchThinRemote<double>(smm_hip_dist_csr*, const double*, bool, double*, int, const double*, double*, const int*, hipStream_t, const ThinForm<double>*);
template int distMatvecCompute<double>(smm_hip_dist_csr*, double*, int, const double*, double*, int, const double*, double*, const int*, hipStream_t, const double*, int, int);
template int distMatvec<double>(smm_hip_dist_csr*, double*, int, int, const double*, double*, int, const double*, double*, const int*, hipStream_t, const double*);
template int allreduceTotals<double>(smm_hip_dist_csr*, double*, int, hipStream_t, hipEvent_t*, int, const int*);
template int distExchangeDrain<double>(smm_hip_dist_csr*, double*, hipStream_t);
template int checkDist<double>(const smm_hip_dist_csr*, const char*);

void preloadDistMatvecUnit() { preloadUnitOf(reinterpret_cast<const void*>(thinFinishKernel<double>)); }

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_dist_spmv_dev_f32(smm_hip_dist_csr* D, int op, const float* d_lhs, const float* d_x, float* d_out, smm_hip_stream stream) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distSpmv<float>(D, op, d_lhs, d_x, d_out, pickStream(stream)));
}
int smm_hip_dist_spmv_dev_f64(smm_hip_dist_csr* D, int op, const double* d_lhs, const double* d_x, double* d_out, smm_hip_stream stream) {
	SMM_TRY(commUsable(D ? D->comm : nullptr));
	return guardComm(D ? D->comm : nullptr, distSpmv<double>(D, op, d_lhs, d_x, d_out, pickStream(stream)));
}

}  // extern "C"
