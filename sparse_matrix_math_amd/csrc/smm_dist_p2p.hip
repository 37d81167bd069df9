// smm_dist_p2p.hip -- the peer-to-peer transport of the row-partitioned path (overview: smm_dist.hip; the kernels and the memory layout:
// smm_p2p.h): the plan every rank derives alike, the mapping of the blocks, the voted self-test, the push / land / slot launches, the
// error word; smm_hip_dist_p2p_plan.  The only unit that instantiates the kernels of smm_p2p.h.
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "smm_dist.h"

namespace smm {

// ---------------------------------------------------------------------------------------------------------
// peer-to-peer set-up (smm_p2p.h)
// ---------------------------------------------------------------------------------------------------------
// The halo plan of ANY rank from what every rank knows (the column ranges and the row bounds): the segments rank q receives, in
// ascending source order, with their positions in q's landing area.
static std::vector<PlanSeg> planRecvs(int world, const long long* needs, const int* bounds, int q) {
	std::vector<PlanSeg> out;
	long long at = 0;
	for (int p = 0; p < world; ++p) {
		if (p == q) continue;
		const long long lo = std::max<long long>(needs[2 * static_cast<size_t>(q)], bounds[static_cast<size_t>(p)]);
		const long long hi = std::min<long long>(needs[2 * static_cast<size_t>(q) + 1], bounds[static_cast<size_t>(p) + 1]);
		if (lo < hi) {
			out.push_back({p, q, lo - needs[2 * static_cast<size_t>(q)], at, static_cast<int>(hi - lo)});
			at += hi - lo;
		}
	}
	return out;
}

// relay ranks of the segment p -> q: the ranks farthest (on the ring of ranks) from both ends first -- halo partners are near neighbours in
// a row partition, so those are the ranks whose links to p and to q carry nothing else
static std::vector<int> planRelays(int world, int p, int q, int want) {
	std::vector<int> cand;
	for (int r = 0; r < world; ++r) {
		if (r != p && r != q) cand.push_back(r);
	}
	auto ring = [world](int a, int b) {
		const int d = std::abs(a - b);
		return std::min(d, world - d);
	};
	std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return std::min(ring(a, p), ring(a, q)) > std::min(ring(b, p), ring(b, q)); });
	if (static_cast<int>(cand.size()) > want) cand.resize(static_cast<size_t>(std::max(0, want)));
	return cand;
}

// the parts of a segment of `count` elements: part 0 is the direct one, part k >= 1 goes through relay k - 1; cuts at multiples of 4
// elements.  bounds has parts + 1 entries.
static std::vector<int> planParts(int count, int relays, double directShare) {
	std::vector<int> cut(static_cast<size_t>(relays) + 2, 0);
	cut[static_cast<size_t>(relays) + 1] = count;
	if (count < 64 * (relays + 1)) {  // a short segment travels whole on the direct path (no empty part in front of a non-empty one, ever)
		for (int k = 1; k <= relays; ++k) cut[static_cast<size_t>(k)] = count;
		return cut;
	}
	const double rest = relays > 0 ? (1.0 - directShare) / relays : 0.0;
	double cum = directShare;
	for (int k = 1; k <= relays; ++k) {
		int c = static_cast<int>(count * cum) & ~3;
		c = std::max(cut[static_cast<size_t>(k) - 1], std::min(count, c));
		cut[static_cast<size_t>(k)] = c;
		cum += rest;
	}
	return cut;
}

static P2PPlan p2pMakePlan(int world, const long long* needs, const int* bounds, int relays, double directShare, bool* tooMany) {
	P2PPlan plan;
	plan.stageTotal.assign(static_cast<size_t>(world), 0);
	plan.jobCount.assign(static_cast<size_t>(world), 0);
	*tooMany = false;
	for (int q = 0; q < world; ++q) {
		for (const PlanSeg& g : planRecvs(world, needs, bounds, q)) {
			const std::vector<int> via = planRelays(world, g.src, q, relays);
			const std::vector<int> cut = planParts(g.count, static_cast<int>(via.size()), directShare);
			for (size_t k = 0; k + 1 < cut.size(); ++k) {
				P2PRoute rt{g, static_cast<int>(k), k == 0 ? -1 : via[k - 1], cut[k], cut[k + 1], -1, 0};
				if (rt.relay >= 0) {
					rt.job = plan.jobCount[static_cast<size_t>(rt.relay)]++;
					rt.stagePos = plan.stageTotal[static_cast<size_t>(rt.relay)];
					plan.stageTotal[static_cast<size_t>(rt.relay)] += (rt.b - rt.a + 3) & ~3;
					if (rt.job >= P2P_MAX_JOBS) *tooMany = true;
				}
				plan.routes.push_back(rt);
			}
		}
	}
	return plan;
}

// Collective (every rank tears its matrix down in the same order as it built it): a rank's block must outlive every remote write into it
// -- a peer's land kernel acknowledges into the SOURCE's block after the source may have returned from its solve --, so every rank first
// drains its own device (its remote writes are done), the ranks meet, the mappings are closed, the ranks meet again, and only then is the
// block freed.  A communicator that was aborted cannot meet: the mappings are closed and the block freed at once (the process is expected
// to exit).
void p2pTeardown(smm_hip_dist_csr* D) {
	P2PState* P = D->p2p;
	if (!P) return;
	smm_hip_comm* c = D->comm;
	auto meet = [c]() {
		if (!c || c->broken || c->kind == SMM_COMM_SELF) return;
		long long one = 1;
		if (commAllreduceI64(c, &one, 1) != SMM_HIP_OK) c->broken = true;
	};
	(void)hipDeviceSynchronize();
	meet();
	for (size_t q = 0; q < P->peer.size(); ++q) {
		if (P->opened[q] && P->peer[q]) (void)hipIpcCloseMemHandle(P->peer[q]);
	}
	meet();
	for (void* p : {static_cast<void*>(P->d_push), static_cast<void*>(P->d_fwd), static_cast<void*>(P->d_land), static_cast<void*>(P->d_counters)}) devFree(p);
	if (P->block) (void)hipFree(P->block);
	(void)hipGetLastError();
	delete P;
	D->p2p = nullptr;
}

long long p2pTicks() {
	const double sec = env::doubleOr(env::P2P_TIMEOUT_S, 20.0);
	return static_cast<long long>((sec > 0 ? sec : 20.0) * 1.0e8);  // wall_clock64 counts at 100 MHz on gfx9
}

// sum of one 0 / 1 vote per rank == world?
static int p2pAllAgree(smm_hip_comm* c, bool mine, bool* all) {
	std::vector<long long> v(1, mine ? 1 : 0);
	SMM_TRY(commAllreduceI64(c, v.data(), 1));
	*all = v[0] == c->world;
	return SMM_HIP_OK;
}

// Collective.  Leaves D->p2p null (the communicator's collectives are used) unless EVERY rank asked for the peer-to-peer path, could
// allocate and export its block, map every peer's and pass the self-test through every path.
template <typename T>
int p2pSetup(smm_hip_dist_csr* D) {
	smm_hip_comm* c = D->comm;
	const int world = c->world, rank = c->rank;
	// (SMM_HIP_LAB_SELF_P2P=1, single-rank communicator: the slots with ONE rank -- what a rank of a many-GPU run launches per iteration in this
	// transport, measured on one GPU; tools/lab/rank_loop_streams.py)
	const bool labSelf = world == 1 && c->kind == SMM_COMM_SELF && env::flagOr(env::LAB_SELF_P2P, false);
	if ((world < 2 && !labSelf) || world > P2P_MAX_WORLD) return SMM_HIP_OK;
	// r06: ON unless a rank says SMM_HIP_P2P=0 -- the transport is taken whenever EVERY rank can allocate, export and map the blocks and passes
	// the self-test below; anything less leaves all ranks with the communicator's collectives (read at every create, like SMM_HIP_HALO_CHUNKS)
	bool all = false;
	SMM_TRY(p2pAllAgree(c, env::flagOr(env::P2P, true) && D->chunks == 1, &all));
	if (!all) return SMM_HIP_OK;
	std::unique_ptr<P2PState> owner(new P2PState());
	P2PState* P = owner.get();
	P->world = world;
	P->rank = rank;
	P->ticks = p2pTicks();
	{
		P->relays = env::intOr(env::P2P_RELAYS, std::max(0, world - 4));  // 8 ranks: 4 relays per segment -- half of it direct, an eighth through each relay
		P->relays = std::max(0, std::min(std::min(P->relays, world - 2), P2P_MAX_PATHS - 1));
		// the direct link carries its share once; a relay's links carry up to two shares in each of the two stages: d = 4 rho, d + R rho = 1
		P->directShare = 4.0 / (P->relays + 4.0);
		if (env::isSet(env::P2P_DIRECT_SHARE)) P->directShare = std::min(1.0, std::max(0.05, env::doubleOr(env::P2P_DIRECT_SHARE, 1.0)));
		if (P->relays == 0) P->directShare = 1.0;
	}
	// ---- the plan, from global knowledge: what I receive, what I send (directly / staged at a relay), what I forward
	const std::vector<PlanSeg> mine = planRecvs(world, D->needs.data(), D->bounds.data(), rank);
	bool tooMany = false;
	const P2PPlan plan = p2pMakePlan(world, D->needs.data(), D->bounds.data(), P->relays, P->directShare, &tooMany);
	const std::vector<P2PRoute>& routes = plan.routes;
	const std::vector<long long>& stageTotal = plan.stageTotal;
	using Route = P2PRoute;
	// ---- my block: header | landing x 3 | staging x 3, element-aligned to 256 bytes
	long long landElems = 0;
	for (const PlanSeg& g : mine) landElems += g.count;
	P->landElems = landElems;
	P->stageElems = stageTotal[static_cast<size_t>(rank)];
	auto up = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
	size_t at = up(sizeof(P2PHeader));
	for (int k = 0; k < P2P_KINDS; ++k) {
		P->landOff[k] = at;
		at += up(static_cast<size_t>(std::max<long long>(1, landElems)) * sizeof(T) + 64);
	}
	for (int k = 0; k < P2P_KINDS; ++k) {
		P->stageOff[k] = at;
		at += up(static_cast<size_t>(std::max<long long>(1, P->stageElems)) * sizeof(T) + 64);
	}
	P->bytes = at;
	bool ok = !tooMany;
	if (ok) {
		hipError_t e = hipExtMallocWithFlags(&P->block, P->bytes, hipDeviceMallocFinegrained);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			P->block = nullptr;
			e = hipExtMallocWithFlags(&P->block, P->bytes, hipDeviceMallocUncached);
		}
		if (e != hipSuccess) {
			(void)hipGetLastError();
			P->block = nullptr;
			ok = false;
		} else {
			ok = hipMemset(P->block, 0, P->bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
		}
	}
	// ---- every rank learns every rank's handle, process, address and layout
	constexpr int WORDS = 8 + 2 + 2 * P2P_KINDS + 2;  // handle | pid, address | landing, staging offsets | ok | which GPU (a hash of its PCI bus id)
	long long myGpu = 0;
	{
		int dev = 0;
		char bus[64] = {};
		if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetPCIBusId(bus, sizeof(bus), dev) == hipSuccess) {
			unsigned long long hsh = 1469598103934665603ull;  // FNV-1a
			for (const char* ch = bus; *ch; ++ch) hsh = (hsh ^ static_cast<unsigned char>(*ch)) * 1099511628211ull;
			myGpu = static_cast<long long>(hsh >> 1) | 1;
		} else {
			(void)hipGetLastError();
		}
	}
	std::vector<long long> table(static_cast<size_t>(world) * WORDS, 0);
	long long* me = table.data() + static_cast<size_t>(rank) * WORDS;
	hipIpcMemHandle_t handle{};
	static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
	if (ok && hipIpcGetMemHandle(&handle, P->block) != hipSuccess) {
		(void)hipGetLastError();
		ok = false;
	}
	memcpy(me, &handle, 64);
	me[8] = static_cast<long long>(getpid());
	me[9] = static_cast<long long>(reinterpret_cast<uintptr_t>(P->block));
	for (int k = 0; k < P2P_KINDS; ++k) {
		me[10 + k] = static_cast<long long>(P->landOff[k]);
		me[10 + P2P_KINDS + k] = static_cast<long long>(P->stageOff[k]);
	}
	me[10 + 2 * P2P_KINDS] = ok ? 1 : 0;
	me[WORDS - 1] = myGpu;
	SMM_TRY(commAllreduceI64(c, table.data(), world * WORDS));
	for (int q = 0; q < world; ++q) ok = ok && table[static_cast<size_t>(q) * WORDS + 10 + 2 * P2P_KINDS] == 1;
	// Ranks that SHARE a GPU (a rehearsal of several ranks on one card) keep the two-launch SpMV: the one-launch form waits inside a grid that fills
	// the chip but for one CU per XCD's worth of slots, and on a shared card a peer's grid takes exactly those slots -- the land and push kernels
	// the grids are waiting for then find no room until the bounded wait expires (seen with 2 x 2.5 M rows on one MI355X, r06).  One rank per
	// GPU -- the deployment -- leaves the room to the rank's own copy kernels.  Every rank sees the same table: every rank decides alike.
	for (int q = 0; q < world; ++q) {
		for (int r2 = q + 1; r2 < world; ++r2) {
			const long long a = table[static_cast<size_t>(q) * WORDS + WORDS - 1], b = table[static_cast<size_t>(r2) * WORDS + WORDS - 1];
			if (a == 0 || b == 0 || a == b) D->sharedGpu = true;
		}
	}
	P->peer.assign(static_cast<size_t>(world), nullptr);
	P->opened.assign(static_cast<size_t>(world), false);
	if (ok) {
		for (int q = 0; q < world && ok; ++q) {
			const long long* row = table.data() + static_cast<size_t>(q) * WORDS;
			if (q == rank) {
				P->peer[static_cast<size_t>(q)] = static_cast<char*>(P->block);
			} else if (row[8] == static_cast<long long>(getpid())) {
				// A rank of this very process (ranks as threads: the tests).  REFUSED since r06: this transport makes kernels of one rank wait for
				// kernels of another, and inside ONE process HIP gives no control over which hardware queue a stream's dispatches take -- a kernel
				// trace of the thread-rank test under GPU_MAX_HW_QUEUES=32 shows 15 of 59 streams dispatched on more than one queue and the side
				// streams of two live ranks on the same one (profiles/r06/p2p_thread_rank_queues.txt): a waiting kernel then sits in front of the
				// kernel it waits for until its bound expires (the intermittent time-outs of r05 / r06).  Ranks in separate processes -- one per
				// GPU, the deployment -- have queues of their own.  Every rank sees the same table, so every rank votes alike: the collectives.
				ok = false;
			} else {
				hipIpcMemHandle_t h{};
				memcpy(&h, row, 64);
				void* ptr = nullptr;
				if (hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
					(void)hipGetLastError();
					ok = false;
				} else {
					P->peer[static_cast<size_t>(q)] = static_cast<char*>(ptr);
					P->opened[static_cast<size_t>(q)] = true;
				}
			}
		}
	}
	// ---- device tables
	std::vector<P2PJob> push, fwd;
	std::vector<P2PLandSeg> land;
	if (ok) {
		auto hdrOf = [&](int q) { return reinterpret_cast<P2PHeader*>(P->peer[static_cast<size_t>(q)]); };
		auto rowOf = [&](int q) { return table.data() + static_cast<size_t>(q) * WORDS; };
		for (const Route& rt : routes) {
			const int n = rt.b - rt.a;
			if (n <= 0) continue;
			const int q = rt.seg.dst;
			if (rt.seg.src == rank) {  // I push this part: straight into q's landing area, or into the relay's staging area
				P2PJob j{};
				j.srcOff = (static_cast<long long>(D->bounds[static_cast<size_t>(rank)]) - D->cmin) +
				           (D->needs[2 * static_cast<size_t>(q)] + rt.seg.extOff - D->bounds[static_cast<size_t>(rank)]) + rt.a;
				j.count = n;
				j.waitJob = -1;
				j.ackFrom = q;
				for (int k = 0; k < P2P_KINDS; ++k) {
					if (rt.relay < 0) {
						j.dst[k] = P->peer[static_cast<size_t>(q)] + rowOf(q)[10 + k] + (rt.seg.landOff + rt.a) * static_cast<long long>(sizeof(T));
						j.flag[k] = &hdrOf(q)->haloFlag[k][rank][0];
					} else {
						j.dst[k] = P->peer[static_cast<size_t>(rt.relay)] + rowOf(rt.relay)[10 + P2P_KINDS + k] + rt.stagePos * static_cast<long long>(sizeof(T));
						j.flag[k] = &hdrOf(rt.relay)->stageFlag[k][rt.job];
					}
				}
				push.push_back(j);
			}
			if (rt.relay == rank) {  // I forward this part from my staging area into q's landing area
				P2PJob j{};
				j.srcOff = rt.stagePos;
				j.count = n;
				j.waitJob = rt.job;
				j.ackFrom = q;
				for (int k = 0; k < P2P_KINDS; ++k) {
					j.dst[k] = P->peer[static_cast<size_t>(q)] + rowOf(q)[10 + k] + (rt.seg.landOff + rt.a) * static_cast<long long>(sizeof(T));
					j.flag[k] = &hdrOf(q)->haloFlag[k][rt.seg.src][rt.part];
				}
				fwd.push_back(j);
			}
		}
		for (const PlanSeg& g : mine) {
			int paths = 0;
			for (const Route& rt : routes) {
				if (rt.seg.dst == rank && rt.seg.src == g.src && rt.b > rt.a) paths = std::max(paths, rt.part + 1);
			}
			// (a part without elements is never signalled: the land kernel waits for the parts that exist -- they are the first `paths` ones only when
			// no part in between is empty, which planParts guarantees except for tiny segments, where every part but the direct one may be empty)
			bool gaps = false;
			for (const Route& rt : routes) {
				if (rt.seg.dst == rank && rt.seg.src == g.src && rt.b <= rt.a && rt.part < paths) gaps = true;
			}
			if (gaps) ok = false;
			P2PLandSeg ls{g.landOff, g.extOff, g.count, g.src, paths, {}};
			for (int k = 0; k < P2P_KINDS; ++k) ls.ack[k] = &hdrOf(g.src)->ackFlag[k][rank];
			land.push_back(ls);
		}
		P->nPush = static_cast<int>(push.size());
		P->nFwd = static_cast<int>(fwd.size());
		P->nLand = static_cast<int>(land.size());
		for (int q = 0; q < world; ++q) P->peers.hdr[q] = hdrOf(q);
		auto upload = [&](auto& vec, auto** d) -> int {
			using E = typename std::remove_reference<decltype(vec)>::type::value_type;
			void* p = nullptr;
			SMM_TRY(devAlloc(&p, std::max<size_t>(1, vec.size()) * sizeof(E)));
			*d = static_cast<E*>(p);
			if (!vec.empty()) SMM_HIP_TRY(hipMemcpy(p, vec.data(), vec.size() * sizeof(E), hipMemcpyHostToDevice));
			return SMM_HIP_OK;
		};
		// (a failure here must not return: the other ranks are about to vote, and a rank that left would leave them alone in the collective)
		void* cnt = nullptr;
		const size_t nCounters = static_cast<size_t>(P->nPush + P->nFwd + P->nLand + 1);  // (+ 1: finished segments of a land launch)
		if (upload(push, &P->d_push) != SMM_HIP_OK || upload(fwd, &P->d_fwd) != SMM_HIP_OK || upload(land, &P->d_land) != SMM_HIP_OK ||
		    devAlloc(&cnt, nCounters * sizeof(unsigned)) != SMM_HIP_OK || hipMemset(cnt, 0, nCounters * sizeof(unsigned)) != hipSuccess) {
			(void)hipGetLastError();
			ok = false;
		}
		P->d_counters = static_cast<unsigned*>(cnt);
	}
	SMM_TRY(p2pAllAgree(c, ok, &all));
	D->p2p = owner.release();  // (torn down below unless everything checks out; the peers' mappings must be closed either way)
	if (!all) {
		p2pTeardown(D);
		return SMM_HIP_OK;
	}
	// ---- self-test, in two parts with a vote each (no early return between votes -- ADVICE r05: a rank that left would tear its block down in
	// p2pTeardown, whose "meet" all-reduces would pair with the peers' votes; every failure is a `pass = false`).
	// (on the communicator's own stream: kernels of this rank WAIT for kernels of its peers)
	hipStream_t s = c->stream;
	noteStream(s);
	// Part 1, the scalars: every reduction point once -- rank + 1 and 2 (rank + 1) through the slots must give world (world + 1) / 2 and twice that
	// on every rank.  A failure here leaves every rank with the collectives for everything.
	bool pass = true;
	{
		DevBuf<T> tot;
		T mineTot[2 * P2P_RED_POINTS], got[2 * P2P_RED_POINTS] = {};
		for (int k = 0; k < P2P_RED_POINTS; ++k) {
			mineTot[2 * k] = static_cast<T>(rank + 1 + k);
			mineTot[2 * k + 1] = static_cast<T>(2 * (rank + 1 + k));
		}
		unsigned long long err = 0;
		bool okHost = tot.alloc(2 * P2P_RED_POINTS) == SMM_HIP_OK;
		if (okHost) okHost = hipMemcpyAsync(tot, mineTot, sizeof(mineTot), hipMemcpyHostToDevice, s) == hipSuccess;
		int rc = SMM_HIP_OK;
		for (int k = 0; k < P2P_RED_POINTS && okHost && rc == SMM_HIP_OK; ++k) rc = p2pAllreduceLaunch<T>(D, k, tot.p + 2 * k, 2, nullptr, s);
		if (okHost) okHost = hipMemcpyAsync(got, tot, sizeof(got), hipMemcpyDeviceToHost, s) == hipSuccess;
		okHost = hipMemcpyAsync(&err, &P->hdr()->err, sizeof(err), hipMemcpyDeviceToHost, s) == hipSuccess && okHost;
		okHost = hipStreamSynchronize(s) == hipSuccess && okHost;
		if (!okHost) (void)hipGetLastError();
		pass = okHost && rc == SMM_HIP_OK && err == 0;
		for (int k = 0; k < P2P_RED_POINTS && pass; ++k) {
			const T want = static_cast<T>(0.5 * world * (world + 1) + static_cast<double>(k) * world);
			pass = got[2 * k] == want && got[2 * k + 1] == 2 * want;
		}
	}
	SMM_TRY(p2pAllAgree(c, pass, &all));
	if (!all) {
		if (!pass) fprintf(stderr, "libsmm_hip: rank %d: the peer-to-peer self-test (scalars) failed; every rank stays with the communicator's collectives\n", rank);
		p2pTeardown(D);
		return SMM_HIP_OK;
	}
	// Part 2, the halo: the halo-extended vector carries (global column + 7 round) mod 8191 in every owned element; after an exchange every halo
	// element of every rank must hold ITS column's number -- once through the areas of each vector kind, then twice more back to back through
	// the last kind's (a push then waits for the acknowledgement of the exchange before).  A failure here leaves the HALO with the
	// communicator's grouped send / receive and keeps the scalars in the slots (the hybrid: a reduction point costs ~3 us instead of ~23).
	const bool haloWanted = env::flagOr(env::P2P_HALO, true);  // 0: do not try (tests of the hybrid)
	pass = haloWanted;
	{
		T* xExt = static_cast<T*>(D->xExt);
		std::vector<T> host(static_cast<size_t>(D->extLen), T(-1));
		unsigned long long err = 0;
		const int kinds[5] = {0, 1, 2, 2, 2};
		for (int round = 0; round < 5 && pass; ++round) {
			std::fill(host.begin(), host.end(), T(-1));
			for (int i = 0; i < D->nLocal; ++i) host[static_cast<size_t>(D->ownOffset + i)] = static_cast<T>((D->rowBegin + i + 7LL * round) % 8191);
			bool okHost = hipMemcpyAsync(xExt, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, s) == hipSuccess;
			// (whatever fails on the host, the launches go out if they can at all: the peers' kernels are waiting for this rank's parts)
			int rc = p2pHaloLaunch<T>(D, xExt, kinds[round], s);
			if (rc == SMM_HIP_OK) rc = p2pLandLaunch<T>(D, xExt, kinds[round], P->haloSeq[kinds[round]], s);
			okHost = hipMemcpyAsync(host.data(), xExt, host.size() * sizeof(T), hipMemcpyDeviceToHost, s) == hipSuccess && okHost;
			okHost = hipMemcpyAsync(&err, &P->hdr()->err, sizeof(err), hipMemcpyDeviceToHost, s) == hipSuccess && okHost;
			okHost = hipStreamSynchronize(s) == hipSuccess && okHost;
			if (!okHost) (void)hipGetLastError();
			pass = okHost && rc == SMM_HIP_OK && err == 0;
			for (const PlanSeg& g : mine) {
				for (int i = 0; i < g.count && pass; ++i) {
					const long long col = D->cmin + g.extOff + i;
					pass = host[static_cast<size_t>(g.extOff + i)] == static_cast<T>((col + 7LL * round) % 8191);
				}
			}
		}
		if (hipMemsetAsync(xExt, 0, host.size() * sizeof(T), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
	}
	SMM_TRY(p2pAllAgree(c, pass, &all));
	if (!all) {
		if (!pass && haloWanted) {
			fprintf(stderr, "libsmm_hip: rank %d: the peer-to-peer self-test (halo) failed; the halo stays with the communicator's send / receive on every rank\n", rank);
		}
		// every rank is past its own waits (each synchronised its stream above, and the vote was a collective): the error words of the halo part
		// are history, the slots go on
		P->haloOn = false;
		P->relays = 0;
		P->directShare = 1.0;
		if (hipMemset(&P->hdr()->err, 0, sizeof(unsigned long long)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
		bool cleared = false;
		SMM_TRY(p2pAllAgree(c, true, &cleared));  // (nobody enters a reduction before every rank has cleared its word)
	}
	return SMM_HIP_OK;
}

// the exchange of `ext`'s boundary slices: push kernel (direct parts + the shares staged at relays), then this rank's forwards
template <typename T>
int p2pHaloLaunch(smm_hip_dist_csr* D, T* ext, int kind, hipStream_t cs) {
	P2PState* P = D->p2p;
	const unsigned long long seq = ++P->haloSeq[kind];
	if (P->nPush > 0) {
		p2pCopyKernel<T, false><<<dim3(P2P_BLOCKS_PER_JOB, static_cast<unsigned>(P->nPush)), P2P_TPB, 0, cs>>>(P->d_push, P->d_counters, ext, kind, seq, P->hdr(), P->ticks);
	}
	if (P->nFwd > 0) {
		const T* staging = reinterpret_cast<const T*>(static_cast<char*>(P->block) + P->stageOff[kind]);
		p2pCopyKernel<T, true><<<dim3(P2P_BLOCKS_PER_JOB, static_cast<unsigned>(P->nFwd)), P2P_TPB, 0, cs>>>(P->d_fwd, P->d_counters + P->nPush, staging, kind, seq, P->hdr(),
		                                                                                              P->ticks);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template <typename T>
int p2pLandLaunch(smm_hip_dist_csr* D, T* ext, int kind, unsigned long long seq, hipStream_t s, unsigned long long* word, unsigned long long wordSeq) {
	P2PState* P = D->p2p;
	if (P->nLand == 0) {
		if (word) launchSplitSignal(word, wordSeq, s);  // (nothing lands here, yet a launch is waiting for the word)
		return SMM_HIP_OK;
	}
	const T* landing = reinterpret_cast<const T*>(static_cast<char*>(P->block) + P->landOff[kind]);
	p2pLandKernel<T><<<dim3(16, static_cast<unsigned>(P->nLand)), P2P_TPB, 0, s>>>(P->d_land, P->d_counters + P->nPush + P->nFwd, landing, ext, kind, seq, P->hdr(), P->ticks,
	                                                                               word, wordSeq, P->d_counters + P->nPush + P->nFwd + P->nLand);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template <typename T>
int p2pAllreduceLaunch(smm_hip_dist_csr* D, int point, T* totals, int count, const int* doneFlag, hipStream_t s, const T* parts) {
	P2PState* P = D->p2p;
	const unsigned long long seq = ++P->redSeq[point];
	p2pAllreduceKernel<T><<<1, P2P_TPB, 0, s>>>(P->peers, P->world, P->rank, point, seq, count, totals, parts, NPART, P->ticks, doneFlag);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// the error word of the peer-to-peer path, read wherever the host reads `done` (stream `s` is synchronised by the caller afterwards)
int p2pPostErrRead(smm_hip_dist_csr* D, unsigned long long* err, hipStream_t s) {
	*err = 0;
	// (without the peer-to-peer transport the one-launch SpMV's own word -- smm_hip_dist_csr::splitSync -- is the only bounded device-side wait)
	const unsigned long long* word = D->p2p ? &D->p2p->hdr()->err : D->splitSync ? D->splitSync + P2P_KINDS : nullptr;
	if (!word) return SMM_HIP_OK;
	SMM_HIP_TRY(hipMemcpyAsync(err, word, sizeof(*err), hipMemcpyDeviceToHost, s));
	return SMM_HIP_OK;
}
int p2pFailIf(smm_hip_dist_csr* D, unsigned long long err) {
	if (!err) return SMM_HIP_OK;
	const unsigned what = static_cast<unsigned>(err >> 32);
	static const char* const names[] = {"?", "a push for the destination's acknowledgement of the previous exchange (vector, destination rank)",
	                                    "a forward for its staged share (vector, relay job)", "the land kernel for a part (vector, source rank, path)",
	                                    "a reduction for a rank's slot (reduction point, rank)", "the one-launch SpMV for the halo of its exchange"};
	setError("dist: rank %d waited longer than SMM_HIP_P2P_TIMEOUT_S for a peer (%s): %s = (%u, %u, %u), sequence number %llu; the communicator "
	         "is unusable", D->comm->rank, D->p2p ? "peer-to-peer path" : "collectives", names[std::min(5u, what >> 12)], (what >> 8) & 0xFu, (what >> 4) & 0xFu, what & 0xFu,
	         err & 0xFFFFFFFFull);
	fprintf(stderr, "libsmm_hip: %s\n", smm_hip_last_error());
	D->comm->broken = true;
	return SMM_HIP_ERR_COMM;
}

template int p2pSetup<float>(smm_hip_dist_csr*);
template int p2pHaloLaunch<float>(smm_hip_dist_csr*, float*, int, hipStream_t);
template int p2pLandLaunch<float>(smm_hip_dist_csr*, float*, int, unsigned long long, hipStream_t, unsigned long long*, unsigned long long);
template int p2pAllreduceLaunch<float>(smm_hip_dist_csr*, int, float*, int, const int*, hipStream_t, const float*);
template int p2pSetup<double>(smm_hip_dist_csr*);
template int p2pHaloLaunch<double>(smm_hip_dist_csr*, double*, int, hipStream_t);
template int p2pLandLaunch<double>(smm_hip_dist_csr*, double*, int, unsigned long long, hipStream_t, unsigned long long*, unsigned long long);
template int p2pAllreduceLaunch<double>(smm_hip_dist_csr*, int, double*, int, const int*, hipStream_t, const double*);

}  // namespace smm

using namespace smm;

extern "C" {

// The peer-to-peer plan of one rank as plain numbers (host arithmetic only: no device, no communicator) -- what the set-up derives from
// the globally known column ranges and row bounds.  The CPU tests replay it for every rank of a world of 8 and check that every halo
// element arrives exactly once.  Records of 8 values:
//   {0, dst, relay (-1: direct), first global column, position (dst's landing area / the relay's staging area), count, path, relay job (-1)}   push
//   {1, src, dst, position in my staging area, position in dst's landing area, count, path, relay job}                                           forward
//   {2, src, offset in my halo-extended vector, position in my landing area, count, paths, 0, 0}                                                 land
int smm_hip_dist_p2p_plan(int world, int rank, const long long* needs, const int* bounds, int relays, double direct_share, long long* out, int out_capacity,
                          int* out_count) {
	if (world < 1 || world > P2P_MAX_WORLD || rank < 0 || rank >= world || !needs || !bounds || !out_count || relays < 0 || relays > P2P_MAX_PATHS - 1) {
		setError("dist_p2p_plan: bad arguments");
		return SMM_HIP_ERR_INVALID;
	}
	relays = std::min(relays, std::max(0, world - 2));
	if (relays == 0) direct_share = 1.0;
	bool tooMany = false;
	const P2PPlan plan = p2pMakePlan(world, needs, bounds, relays, direct_share, &tooMany);
	if (tooMany) {
		setError("dist_p2p_plan: more relay jobs per rank than the header holds");
		return SMM_HIP_ERR_INVALID;
	}
	std::vector<long long> rec;
	for (const P2PRoute& rt : plan.routes) {
		const long long n = rt.b - rt.a;
		if (n <= 0) continue;
		const int q = rt.seg.dst;
		if (rt.seg.src == rank) {
			const long long col = needs[2 * static_cast<size_t>(q)] + rt.seg.extOff + rt.a;
			rec.insert(rec.end(), {0LL, q, rt.relay, col, rt.relay < 0 ? rt.seg.landOff + rt.a : rt.stagePos, n, rt.part, rt.relay < 0 ? -1LL : rt.job});
		}
		if (rt.relay == rank) rec.insert(rec.end(), {1LL, rt.seg.src, q, rt.stagePos, rt.seg.landOff + rt.a, n, rt.part, rt.job});
	}
	for (const PlanSeg& g : planRecvs(world, needs, bounds, rank)) {
		long long paths = 0;
		for (const P2PRoute& rt : plan.routes) {
			if (rt.seg.dst == rank && rt.seg.src == g.src && rt.b > rt.a) paths = std::max<long long>(paths, rt.part + 1);
		}
		rec.insert(rec.end(), {2LL, g.src, g.extOff, g.landOff, g.count, paths, 0LL, 0LL});
	}
	*out_count = static_cast<int>(rec.size() / 8);
	if (out && static_cast<size_t>(out_capacity) >= rec.size()) memcpy(out, rec.data(), rec.size() * sizeof(long long));
	return SMM_HIP_OK;
}

}  // extern "C"
