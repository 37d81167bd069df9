// smm_dist.h -- what the units of the row-partitioned path share (internal): the handles behind smm_hip_comm / smm_hip_dist_csr, the
// peer-to-peer plan and state, and the functions that cross a unit boundary.  The overview and the map of the units are at the head of
// smm_dist.hip.  A template declared here is defined in the unit named above it and instantiated there for float and double.
// RCCL's header, rocprim and dlfcn.h stay out of here: smm_dist_comm.hip alone sees RCCL, smm_dist_create.hip alone rocprim.
#pragma once
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_solver_host.h"
#include "smm_p2p.h"
#include "smm_krylov_steps.h"

struct ncclComm;  // RCCL's communicator (ncclComm_t is a pointer to it)

namespace smm {

constexpr int TPB = 256;
constexpr int CHECK_EVERY = 16;     // iterations between two blocking reads of `done` (readDone, smm_dist.hip)
constexpr int MAX_HALO_CHUNKS = 4;  // pieces of the halo (chunkOfColumn, smm_dist_create.hip)

struct Seg {  // a contiguous piece of a halo-extended vector exchanged with one peer
	int peer, offset, count;
};

}  // namespace smm

struct smm_hip_comm {
	int rank = 0, world = 1, kind = SMM_COMM_SELF;
	ncclComm* nccl = nullptr;
	smm_hip_host_allreduce_fn hostAllreduce = nullptr;
	smm_hip_host_sendrecv_fn hostSendrecv = nullptr;
	void* user = nullptr;
	hipStream_t stream = nullptr;  // side stream of the collectives (high priority: a pending exchange must get its few workgroups
	                               // before the persistent SpMV grid of the caller's stream fills every CU)
	std::vector<hipEvent_t> events;
	size_t nextEvent = 0;
	char* pinned = nullptr;  // host staging of the callback kind
	size_t pinnedBytes = 0;
	long long* d_i64 = nullptr;  // set-up reductions
	size_t i64Count = 0;
	bool broken = false;  // aborted after a failure or a time-out: every further call fails at once
};

namespace smm {

struct P2PState {
	int world = 1, rank = 0;
	bool haloOn = true;      // false: the halo stays with the communicator's grouped send / receive, only the scalars go through the slots (the hybrid)
	int relays = 0;          // relay ranks per segment (0: the direct path only)
	double directShare = 1;  // share of a segment that takes the direct path
	void* block = nullptr;   // this rank's symmetric block (fine-grained device memory)
	size_t bytes = 0;
	std::vector<char*> peer;   // every rank's block as mapped here (peer[rank] == block)
	std::vector<bool> opened;  // mapped with hipIpcOpenMemHandle (to be closed)
	size_t landOff[P2P_KINDS] = {}, stageOff[P2P_KINDS] = {};  // byte offsets inside MY block
	long long landElems = 0, stageElems = 0;
	P2PJob* d_push = nullptr;
	int nPush = 0;
	P2PJob* d_fwd = nullptr;
	int nFwd = 0;
	P2PLandSeg* d_land = nullptr;
	int nLand = 0;
	unsigned* d_counters = nullptr;
	P2PPeers peers{};
	unsigned long long haloSeq[P2P_KINDS] = {}, redSeq[P2P_RED_POINTS] = {};
	long long ticks = 0;
	P2PHeader* hdr() const { return reinterpret_cast<P2PHeader*>(block); }
};

}  // namespace smm

struct smm_hip_dist_csr {
	smm_hip_comm* comm = nullptr;
	int dtype = 0;
	int nGlobal = 0, rowBegin = 0, rowEnd = 0, nLocal = 0;
	int cmin = 0, cmaxExcl = 0, extLen = 1, ownOffset = 0;
	long long nnzLoc = 0, nnzRem = 0;
	int haloElements = 0;
	smm_hip_csr* aLoc = nullptr;
	smm_hip_csr* aRem = nullptr;
	void* arrays[6] = {};  // startLoc, posLoc, valLoc, startRem, posRem, valRem (owned)
	std::vector<smm::Seg> sends, recvs;
	bool remEmpty = true;
	// the halo in `chunks` pieces (SMM_HIP_HALO_CHUNKS, default 1 = one exchange, one remote block): piece k of every segment travels in
	// exchange k, and A_rem is cut by columns into aRemK[k] = its entries in piece k of any received segment -- the part of A_rem that
	// needs only piece k runs while the later pieces are still in flight
	int chunks = 1;
	std::vector<std::vector<smm::Seg>> sendsK, recvsK;
	std::vector<smm_hip_csr*> aRemK;
	std::vector<long long> nnzRemK;  // entries of each piece (a piece without entries is not launched unless it carries the epilogue)
	std::vector<void*> chunkArrays;  // start / positions / values of the pieces (owned)
	// workspace of the solvers, kept across solves
	void *r = nullptr, *r0 = nullptr, *ap = nullptr, *as = nullptr, *scratch = nullptr;
	void *pExt = nullptr, *sExt = nullptr, *xExt = nullptr;
	void* lazyExt[smm::LAZY_M] = {};  // CG with the deferred x update: LAZY_M more halo-extended direction vectors (allocated by the first such solve)
	void* rExt = nullptr;  // CG with the direction formed inside the SpMV: the residual, halo-extended (its halo travels instead of the direction's)
	long long cgFused = 0;  // SpMVs of ConjugateGradient that formed the direction themselves (smm_hip_dist_csr_cg_fused)
	void *partsA = nullptr, *partsB = nullptr, *partsC = nullptr;  // finishing buffers (PARTS_LEN): totals are all-reduced in place
	void* sc = nullptr;
	// every rank's column range [cmin, cmaxExcl) and the row bounds (global knowledge: any rank can derive any rank's halo plan)
	std::vector<long long> needs;
	std::vector<int> bounds;
	// halo first (r05): the rows of an updated vector that some peer receives -- merged, clipped, aligned ranges in owned-local numbering --
	// are produced by a small launch of their own, the exchange is posted right behind it, and the bulk launch takes the complement
	smm::RowRanges boundary, bulk;
	bool haloFirst = false;
	// the exchange begun by distExchangeBegin and not yet consumed by distMatvecCompute
	struct Pending {
		bool active = false;
		int kind = 0;
		unsigned long long seq = 0;
		unsigned long long landSeq = 0;  // what splitSync[kind] will read once this exchange has landed (0: no word is raised for it)
		hipEvent_t landed[smm::MAX_HALO_CHUNKS] = {};
		int waitSlot[smm::MAX_HALO_CHUNKS] = {-1, -1, -1, -1};
		bool async = false;
	} pending;
	smm::P2PState* p2p = nullptr;  // peer-to-peer data movement (smm_p2p.h); null: collectives of the communicator
	// the SpMV in ONE launch (smm_spmv_split.hip): splitSync[kind] is raised -- on the stream the exchange ran on, behind it -- to the sequence
	// number of the exchange whose halo has landed in the vector of that kind; splitSync[P2P_KINDS] is the error word of an expired wait
	// (with the peer-to-peer transport the block's own error word is used instead: one word for the host to read); splitSync[P2P_KINDS + 1]
	// accumulates the ticks workgroup 0 of every one-launch SpMV waited for its word (smm_hip_dist_csr_split_wait)
	unsigned long long* splitSync = nullptr;
	unsigned long long landSeq[smm::P2P_KINDS] = {};
	long long matvecsSplit = 0, matvecsTwo = 0;  // how many SpMVs with a halo ran in one launch / in two (smm_hip_dist_csr_matvec_forms)
	int splitSumsLdsMax = 16384;  // SMM_HIP_SPLIT_SUMS_LDS at create time: bytes of LDS the one-launch SpMV's row sums may take (0: always through out[]; tests)
	bool splitForced = false;
	bool sharedGpu = false;  // two ranks of the communicator run on one card (seen in the peer-to-peer set-up's table)
	bool splitAllowed = true;  // SMM_HIP_SPLIT_SPMV=0 at create time: this matrix keeps the two launches (A/B measurements, the bit-equality tests)
	bool reducedInKernel = false;  // the SpMV just launched ran its reduction point itself (the one-launch form with the slots): allreduceTotals has nothing to do
	int labWindow = 0;  // measurements on ONE GPU (SMM_HIP_LAB_SELF_SPLIT, single-rank communicator only): entries |column - row| >= window count as "remote"
	// a THIN remote block (r06): at most an eighth of the rows hold a remote entry (the slabs of a 3-D grid: two planes) -- thinRows lists them, and
	// the second half of the SpMV is a launch over those rows only (thinRemoteKernel) instead of a pass over every row of `out`
	int* thinRows = nullptr;
	int nThin = 0;
	void* partsThin = nullptr;  // finishing buffer of that launch's share of the dot products
	bool totalsFinal = false;   // the SpMV just launched left the rank's TOTALS in the finishing buffer (the thin form): the slot kernel must not add partials again
	long long matvecsThin = 0;
};

namespace smm {

struct PlanSeg {  // a segment rank dst receives from rank src (planRecvs, smm_dist_p2p.hip)
	int src, dst;
	long long extOff;   // element offset in dst's halo-extended vector
	long long landOff;  // element offset in dst's landing area
	int count;
};

// Every part of every segment of every rank, and what each relay stages where: the SAME table on every rank, from global knowledge only.
struct P2PRoute {
	PlanSeg seg;
	int part, relay, a, b;  // elements [a, b) of the segment; relay < 0: the direct part
	int job;                // index among the relay's jobs
	long long stagePos;     // element offset in the relay's staging area
};
struct P2PPlan {
	std::vector<P2PRoute> routes;
	std::vector<long long> stageTotal;  // elements of staging area per rank
	std::vector<int> jobCount;          // relay jobs per rank
};

// FORM of thinRemoteKernel, smm_dist_matvec.hip (ConjugateGradient with the direction formed inside the SpMV, smm_spmv_march.hip MarchFuse): the local block's
// launch reads the previous direction and r and forms p = beta p_old + r for every element it touches; what it cannot form is the HALO of
// the new direction -- so the halo of r travels instead of p's (posted right behind distCgR, while ||r||^2 is reduced) and THIS launch forms
// the halo of p from it, twice: the entries it gathers are formed on the fly, and the halo is stored for the next iteration (no lane reads
// what another stores) -- fma(beta, p_old, r), the owner's expression on the owner's operands, beta from the same all-reduced total and the
// same rrPing on every rank: the owner's bits.  Runs behind the fused launch (whose workgroup 0 did iteration i - 1's bookkeeping: rrPing[par]
// is untouched, `done` is final).
struct HaloSegs {
	int n = 0;
	int off[P2P_MAX_WORLD] = {}, cnt[P2P_MAX_WORLD] = {};
};
template <typename T>
struct ThinForm {
	const T* pOldExt = nullptr;
	const T* rExt = nullptr;
	T* pNewExt = nullptr;
	const Scal<T>* sc = nullptr;
	const T* totalsC = nullptr;
	int par = 0;
	HaloSegs segs{};
};

// What follows crosses the units of this path only: hidden, so that the library exports what it exported as one unit.
#pragma GCC visibility push(hidden)

// ---- smm_dist_comm.hip: the communicator, its failure containment, its collectives
hipEvent_t takeEvent(smm_hip_comm* c);
int boundedSync(smm_hip_comm* c, hipStream_t s);
int guardComm(smm_hip_comm* c, int rc);
int commUsable(const smm_hip_comm* c);
int orderAfter(smm_hip_comm* c, hipStream_t from, hipStream_t to);
template <typename T>
int commAllreduce(smm_hip_comm* c, T* d_buf, int count, hipStream_t s);
int commAllreduceI64(smm_hip_comm* c, long long* h, int count);
template <typename T>
int commExchange(smm_hip_comm* c, T* ext, const std::vector<Seg>& sends, const std::vector<Seg>& recvs, hipStream_t s);

// ---- smm_dist_p2p.hip: the peer-to-peer transport (the only unit that instantiates the kernels of smm_p2p.h)
template <typename T>
int p2pSetup(smm_hip_dist_csr* D);
void p2pTeardown(smm_hip_dist_csr* D);
long long p2pTicks();
template <typename T>
int p2pHaloLaunch(smm_hip_dist_csr* D, T* ext, int kind, hipStream_t cs);
template <typename T>
int p2pLandLaunch(smm_hip_dist_csr* D, T* ext, int kind, unsigned long long seq, hipStream_t s, unsigned long long* word = nullptr, unsigned long long wordSeq = 0);
template <typename T>
int p2pAllreduceLaunch(smm_hip_dist_csr* D, int point, T* totals, int count, const int* doneFlag, hipStream_t s, const T* parts = nullptr);
int p2pPostErrRead(smm_hip_dist_csr* D, unsigned long long* err, hipStream_t s);
int p2pFailIf(smm_hip_dist_csr* D, unsigned long long err);

// ---- smm_dist_matvec.hip: the SpMV in two halves
template <typename T>
int distExchangeBegin(smm_hip_dist_csr* D, T* ext, int kind, hipStream_t s);
int thinUsable(smm_hip_dist_csr* D, hipStream_t s, bool* usable);
template <typename T>
int launchThinRemote(smm_hip_dist_csr* D, const T* ext, bool subtract, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
                     const ThinForm<T>* form = nullptr);
template <typename T>
int distMatvecCompute(smm_hip_dist_csr* D, T* ext, int op, const T* lhs, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
                      const T* jacobiDiag = nullptr, int slotPoint = -1, int locFlags = 0);
template <typename T>
int distMatvec(smm_hip_dist_csr* D, T* ext, int kind, int op, const T* lhs, T* out, int dotMode, const T* w1, T* parts, const int* doneFlag, hipStream_t s,
               const T* jacobiDiag = nullptr);
template <typename T>
int allreduceTotals(smm_hip_dist_csr* D, T* parts, int count, hipStream_t s, hipEvent_t* joined, int point = 0, const int* doneFlag = nullptr);
int join(hipStream_t s, hipEvent_t e);
template <typename T>
int distExchangeDrain(smm_hip_dist_csr* D, T* ext, hipStream_t s);
template <typename T>
int checkDist(const smm_hip_dist_csr* D, const char* who);

// ---- when a unit's code object is built.  distWorkspace (create time) calls these next to preloadSplitUnit so that the first launch of a
// kernel of smm_dist_matvec.hip / smm_dist.hip inside the first solve does not pay for it.  This rests on the runtime building code objects
// per unit on first use, which nobody has measured here; the query is harmless if it does not.
inline void preloadUnitOf(const void* kernel) {
	hipFuncAttributes attr;
	(void)hipFuncGetAttributes(&attr, kernel);
	(void)hipGetLastError();
}
void preloadDistMatvecUnit();
void preloadDistLoopsUnit();

#pragma GCC visibility pop

}  // namespace smm
