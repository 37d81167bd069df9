// smm_dist_comm.hip -- the communicator of the row-partitioned path (overview: smm_dist.hip): RCCL resolved with dlopen, the host-callback
// kind, the single-rank kind; the bounded waits and the abort that contain a failure; the all-reduce and the halo exchange of the
// collectives; smm_hip_comm_* and smm_hip_partition_rows_by_nnz.  The only unit that includes RCCL's header.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <thread>

#include <rccl/rccl.h>  // types and prototypes only: every call goes through dlsym'd pointers

#include "smm_dist.h"

namespace smm {

// ---------------------------------------------------------------------------------------------------------
// RCCL through dlopen
// ---------------------------------------------------------------------------------------------------------
struct RcclApi {
	void* handle = nullptr;
	decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
	decltype(&ncclCommInitRank) CommInitRank = nullptr;
	decltype(&ncclCommDestroy) CommDestroy = nullptr;
	decltype(&ncclAllReduce) AllReduce = nullptr;
	decltype(&ncclSend) Send = nullptr;
	decltype(&ncclRecv) Recv = nullptr;
	decltype(&ncclGroupStart) GroupStart = nullptr;
	decltype(&ncclGroupEnd) GroupEnd = nullptr;
	decltype(&ncclGetErrorString) GetErrorString = nullptr;
	// optional (older libraries): resolved when present
	decltype(&ncclCommAbort) CommAbort = nullptr;
	decltype(&ncclCommCount) CommCount = nullptr;
};

static RcclApi* rccl() {
	static RcclApi api;
	static std::mutex mu;
	std::lock_guard<std::mutex> lock(mu);
	if (api.handle) return &api;
	// the copy PyTorch already mapped (same SONAME) wins, so one RCCL serves both; otherwise the system ROCm one
	const char* candidates[] = {env::raw(env::RCCL_PATH), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
	void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
	for (const char* c : candidates) {
		if (h) break;
		if (c && *c) h = dlopen(c, RTLD_NOW | RTLD_LOCAL);
	}
	if (!h) {
		setError("RCCL not found (dlopen librccl.so.1: %s); set SMM_HIP_RCCL_PATH", dlerror());
		return nullptr;
	}
#define SMM_RCCL_SYM(NAME)                                                        \
	api.NAME = reinterpret_cast<decltype(api.NAME)>(dlsym(h, "nccl" #NAME));      \
	if (!api.NAME) {                                                              \
		setError("RCCL symbol nccl" #NAME " missing");                           \
		return nullptr;                                                           \
	}
	SMM_RCCL_SYM(GetUniqueId)
	SMM_RCCL_SYM(CommInitRank)
	SMM_RCCL_SYM(CommDestroy)
	SMM_RCCL_SYM(AllReduce)
	SMM_RCCL_SYM(Send)
	SMM_RCCL_SYM(Recv)
	SMM_RCCL_SYM(GroupStart)
	SMM_RCCL_SYM(GroupEnd)
	SMM_RCCL_SYM(GetErrorString)
#undef SMM_RCCL_SYM
	api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(dlsym(h, "ncclCommAbort"));
	api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(h, "ncclCommCount"));
	api.handle = h;
	return &api;
}

static int rcclFail(ncclResult_t r, const char* what) {
	RcclApi* api = rccl();
	setError("RCCL error %d (%s) in %s", static_cast<int>(r), api && api->GetErrorString ? api->GetErrorString(r) : "?", what);
	return SMM_HIP_ERR_COMM;
}
#define SMM_RCCL_TRY(expr)                                  \
	do {                                                    \
		ncclResult_t _r = (expr);                           \
		if (_r != ncclSuccess) return rcclFail(_r, #expr);  \
	} while (0)

hipEvent_t takeEvent(smm_hip_comm* c) {
	if (c->events.empty()) {
		// between two drains of the pipeline (every CHECK_EVERY = 16 iterations) a BiCGStab loop records ~10 events per iteration; an event
		// re-recorded while an earlier wait on it is still queued is legal (a wait refers to the record that preceded it), but the pool is
		// sized so that it does not happen
		c->events.resize(256);
		for (auto& e : c->events) {
			if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
		}
	}
	hipEvent_t e = c->events[c->nextEvent];
	c->nextEvent = (c->nextEvent + 1) % c->events.size();
	return e;
}

// ---- failure containment (a collective that a peer never joins would otherwise block this rank for ever) ---------------------
// Every wait of the row-partitioned code on a stream that may carry RCCL work goes through boundedSync: the stream is POLLED, and
// after SMM_HIP_COMM_TIMEOUT_S seconds (default 180) the communicator is aborted (ncclCommAbort: queued collectives of this rank are
// torn down instead of waiting for a peer that is gone) and the call fails with SMM_HIP_ERR_COMM.  Any other failure inside a
// distributed call aborts the communicator too (guardComm), so that the peers run into THEIR bounded wait instead of hanging in the
// next collective.  The process is expected to exit then (bench.py does, with a non-zero status).
static double commTimeoutSeconds() {
	const double v = env::doubleOr(env::COMM_TIMEOUT_S, 180.0);
	return v > 0 ? v : 180.0;
}

static void commAbort(smm_hip_comm* c) {
	if (!c || c->broken) return;
	c->broken = true;
	if (c->kind == SMM_COMM_RCCL && c->nccl) {
		RcclApi* api = rccl();
		if (api && api->CommAbort) api->CommAbort(c->nccl);
		c->nccl = nullptr;  // (without ncclCommAbort the handle is leaked rather than destroyed: ncclCommDestroy would wait for the peers)
	}
}

int boundedSync(smm_hip_comm* c, hipStream_t s) {
	if (!c || c->kind != SMM_COMM_RCCL) {
		SMM_HIP_TRY(hipStreamSynchronize(s));
		return SMM_HIP_OK;
	}
	const auto t0 = std::chrono::steady_clock::now();
	for (unsigned spins = 0;; ++spins) {
		const hipError_t q = hipStreamQuery(s);
		if (q == hipSuccess) return SMM_HIP_OK;
		if (q != hipErrorNotReady) {
			commAbort(c);
			return hipFail(q, "hipStreamQuery", __FILE__, __LINE__);
		}
		if (spins > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));  // (the first polls spin: short waits stay short)
		if ((spins & 1023) == 1023 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > commTimeoutSeconds()) {
			commAbort(c);
			setError("comm: rank %d waited %.0f s for a collective to complete (a peer missing or failed?); communicator aborted", c->rank,
			         commTimeoutSeconds());
			return SMM_HIP_ERR_COMM;
		}
	}
}

// Only failures that can leave the ranks out of step tear the communicator down: a HIP or RCCL failure somewhere inside the call.  A
// caller's mistake that is found before anything was enqueued (SMM_HIP_ERR_INVALID: a wrong dtype, a null vector, a foreign
// preconditioner; SMM_HIP_ERR_PRECOND) is returned as it is and the communicator stays usable -- every rank makes the same call with
// the same kind of arguments, so every rank gets the same refusal.
int guardComm(smm_hip_comm* c, int rc) {
	if ((rc == SMM_HIP_ERR_HIP || rc == SMM_HIP_ERR_COMM || rc == SMM_HIP_ERR_NOMEM) && c && c->kind == SMM_COMM_RCCL) commAbort(c);
	return rc;
}

int commUsable(const smm_hip_comm* c) {
	if (c && c->broken) {
		setError("comm: the communicator was aborted after an earlier failure");
		return SMM_HIP_ERR_COMM;
	}
	return SMM_HIP_OK;
}

// everything enqueued on `from` so far happens before whatever is enqueued on `to` from now on
int orderAfter(smm_hip_comm* c, hipStream_t from, hipStream_t to) {
	if (from == to) return SMM_HIP_OK;
	hipEvent_t e = takeEvent(c);
	if (!e) {
		setError("comm: event pool exhausted");
		return SMM_HIP_ERR_HIP;
	}
	SMM_HIP_TRY(hipEventRecord(e, from));
	SMM_HIP_TRY(hipStreamWaitEvent(to, e, 0));
	return SMM_HIP_OK;
}

static int ensurePinned(smm_hip_comm* c, size_t bytes) {
	if (c->pinnedBytes >= bytes) return SMM_HIP_OK;
	if (c->pinned) hipHostFree(c->pinned);
	c->pinned = nullptr;
	c->pinnedBytes = 0;
	SMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->pinned), bytes, hipHostMallocDefault));
	c->pinnedBytes = bytes;
	return SMM_HIP_OK;
}

template <typename T>
static ncclDataType_t ncclTypeOf() { return sizeof(T) == 4 ? ncclFloat32 : ncclFloat64; }

// in-place sum of d_buf[0..count) over the ranks, enqueued on `s` (the callback kind blocks until `s` has drained)
template <typename T>
int commAllreduce(smm_hip_comm* c, T* d_buf, int count, hipStream_t s) {
	if (c->kind == SMM_COMM_SELF) return SMM_HIP_OK;
	if (c->kind == SMM_COMM_RCCL) {
		SMM_RCCL_TRY(rccl()->AllReduce(d_buf, d_buf, static_cast<size_t>(count), ncclTypeOf<T>(), ncclSum, c->nccl, s));
		return SMM_HIP_OK;
	}
	SMM_TRY(ensurePinned(c, count * sizeof(T)));
	SMM_HIP_TRY(hipMemcpyAsync(c->pinned, d_buf, count * sizeof(T), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (c->hostAllreduce(c->user, c->pinned, count, dtypeOf<T>()) != 0) {
		setError("comm: host all-reduce callback failed");
		return SMM_HIP_ERR_COMM;
	}
	SMM_HIP_TRY(hipMemcpyAsync(d_buf, c->pinned, count * sizeof(T), hipMemcpyHostToDevice, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));  // the staging buffer is reused by the next call
	return SMM_HIP_OK;
}

// blocking sum of host 64-bit integers (set-up only)
int commAllreduceI64(smm_hip_comm* c, long long* h, int count) {
	if (c->kind == SMM_COMM_SELF) return SMM_HIP_OK;
	if (c->kind == SMM_COMM_HOST) {
		if (c->hostAllreduce(c->user, h, count, SMM_DTYPE_I64) != 0) {
			setError("comm: host all-reduce callback failed");
			return SMM_HIP_ERR_COMM;
		}
		return SMM_HIP_OK;
	}
	if (c->i64Count < static_cast<size_t>(count)) {
		if (c->d_i64) hipFree(c->d_i64);
		c->d_i64 = nullptr;
		SMM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_i64), count * sizeof(long long)));
		c->i64Count = count;
	}
	SMM_HIP_TRY(hipMemcpyAsync(c->d_i64, h, count * sizeof(long long), hipMemcpyHostToDevice, c->stream));
	SMM_RCCL_TRY(rccl()->AllReduce(c->d_i64, c->d_i64, static_cast<size_t>(count), ncclInt64, ncclSum, c->nccl, c->stream));
	SMM_HIP_TRY(hipMemcpyAsync(h, c->d_i64, count * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
	SMM_TRY(boundedSync(c, c->stream));
	return SMM_HIP_OK;
}

// halo exchange of the halo-extended vector `ext`, enqueued on `s`
template <typename T>
int commExchange(smm_hip_comm* c, T* ext, const std::vector<Seg>& sends, const std::vector<Seg>& recvs, hipStream_t s) {
	if (sends.empty() && recvs.empty()) return SMM_HIP_OK;
	if (c->kind == SMM_COMM_SELF) {
		setError("comm: a single-rank communicator cannot exchange halos");
		return SMM_HIP_ERR_INVALID;
	}
	if (c->kind == SMM_COMM_RCCL) {
		RcclApi* api = rccl();
		SMM_RCCL_TRY(api->GroupStart());
		for (const Seg& g : recvs) SMM_RCCL_TRY(api->Recv(ext + g.offset, static_cast<size_t>(g.count), ncclTypeOf<T>(), g.peer, c->nccl, s));
		for (const Seg& g : sends) SMM_RCCL_TRY(api->Send(ext + g.offset, static_cast<size_t>(g.count), ncclTypeOf<T>(), g.peer, c->nccl, s));
		SMM_RCCL_TRY(api->GroupEnd());
		return SMM_HIP_OK;
	}
	size_t total = 0;
	for (const Seg& g : sends) total += g.count * sizeof(T);
	for (const Seg& g : recvs) total += g.count * sizeof(T);
	SMM_TRY(ensurePinned(c, total));
	std::vector<int> sp, rp;
	std::vector<void*> sb, rb;
	std::vector<size_t> sn, rn;
	char* at = c->pinned;
	for (const Seg& g : sends) {
		SMM_HIP_TRY(hipMemcpyAsync(at, ext + g.offset, g.count * sizeof(T), hipMemcpyDeviceToHost, s));
		sp.push_back(g.peer);
		sb.push_back(at);
		sn.push_back(g.count * sizeof(T));
		at += g.count * sizeof(T);
	}
	char* recvBase = at;
	for (const Seg& g : recvs) {
		rp.push_back(g.peer);
		rb.push_back(at);
		rn.push_back(g.count * sizeof(T));
		at += g.count * sizeof(T);
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (c->hostSendrecv(c->user, static_cast<int>(sp.size()), sp.data(), sb.data(), sn.data(), static_cast<int>(rp.size()), rp.data(), rb.data(), rn.data()) != 0) {
		setError("comm: host send/recv callback failed");
		return SMM_HIP_ERR_COMM;
	}
	at = recvBase;
	for (const Seg& g : recvs) {
		SMM_HIP_TRY(hipMemcpyAsync(ext + g.offset, at, g.count * sizeof(T), hipMemcpyHostToDevice, s));
		at += g.count * sizeof(T);
	}
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template int commAllreduce<float>(smm_hip_comm*, float*, int, hipStream_t);
template int commAllreduce<double>(smm_hip_comm*, double*, int, hipStream_t);
template int commExchange<float>(smm_hip_comm*, float*, const std::vector<Seg>&, const std::vector<Seg>&, hipStream_t);
template int commExchange<double>(smm_hip_comm*, double*, const std::vector<Seg>&, const std::vector<Seg>&, hipStream_t);

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_comm_unique_id(void* id) {
	if (!id) {
		setError("comm_unique_id: null buffer");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	RcclApi* api = rccl();
	if (!api) return SMM_HIP_ERR_COMM;
	static_assert(sizeof(ncclUniqueId) == SMM_HIP_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
	ncclUniqueId u;
	SMM_RCCL_TRY(api->GetUniqueId(&u));
	memcpy(id, &u, sizeof(u));
	return SMM_HIP_OK;
}

static int commFinish(smm_hip_comm* c, smm_hip_comm** out) {
	int least = 0, greatest = 0;
	hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
	if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest);
	if (e != hipSuccess) {
		smm_hip_comm_destroy(c);
		return hipFail(e, "comm stream", __FILE__, __LINE__);
	}
	*out = c;
	return SMM_HIP_OK;
}

int smm_hip_comm_create_self(smm_hip_comm** out) {
	if (!out) {
		setError("comm_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(ensureInit());
	auto* c = new smm_hip_comm();
	return commFinish(c, out);
}

int smm_hip_comm_create_rccl(int rank, int world, const void* id, smm_hip_comm** out) {
	if (!out || !id || world < 1 || rank < 0 || rank >= world) {
		setError("comm_create_rccl: bad arguments");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(ensureInit());
	RcclApi* api = rccl();
	if (!api) return SMM_HIP_ERR_COMM;
	auto* c = new smm_hip_comm();
	c->rank = rank;
	c->world = world;
	c->kind = SMM_COMM_RCCL;
	ncclUniqueId u;
	memcpy(&u, id, sizeof(u));
	// ncclCommInitRank blocks until every rank has arrived.  It runs on a helper thread so that this rank can give up after
	// SMM_HIP_COMM_TIMEOUT_S seconds (a peer that never starts, a wrong unique id): the helper is then left behind -- it cannot be
	// cancelled -- and the caller is expected to exit; nothing else is shared with it but the state block below.
	struct InitState {
		std::mutex mu;
		std::condition_variable cv;
		bool done = false;
		bool abandoned = false;  // the waiter gave up: a communicator that arrives later belongs to nobody and is aborted by the helper
		ncclResult_t result = ncclSuccess;
		ncclComm_t comm = nullptr;
	};
	auto state = std::make_shared<InitState>();
	int device = 0;
	SMM_HIP_TRY(hipGetDevice(&device));
	std::thread([state, api, world, u, rank, device]() {
		(void)hipSetDevice(device);
		ncclComm_t comm = nullptr;
		const ncclResult_t r = api->CommInitRank(&comm, world, u, rank);
		std::lock_guard<std::mutex> lock(state->mu);
		if (state->abandoned) {  // (a peer that arrived after the time-out: nothing may leak into a process that went on without it)
			if (r == ncclSuccess && comm && api->CommAbort) api->CommAbort(comm);
			return;
		}
		state->result = r;
		state->comm = comm;
		state->done = true;
		state->cv.notify_all();
	}).detach();
	{
		std::unique_lock<std::mutex> lock(state->mu);
		if (!state->cv.wait_for(lock, std::chrono::duration<double>(commTimeoutSeconds()), [&] { return state->done; })) {
			state->abandoned = true;
			delete c;
			setError("comm_create_rccl: rank %d of %d waited %.0f s in ncclCommInitRank (is every rank running, with the same unique id?)", rank, world,
			         commTimeoutSeconds());
			return SMM_HIP_ERR_COMM;
		}
	}
	if (state->result != ncclSuccess) {
		delete c;
		return rcclFail(state->result, "ncclCommInitRank");
	}
	c->nccl = state->comm;
	if (api->CommCount) {  // the size as RCCL itself reports it
		int count = 0;
		if (api->CommCount(c->nccl, &count) != ncclSuccess || count != world) {
			const int st = rcclFail(ncclInternalError, "ncclCommCount (communicator size differs from the requested world)");
			commAbort(c);
			delete c;
			return st;
		}
	}
	return commFinish(c, out);
}

int smm_hip_comm_create_host(int rank, int world, smm_hip_host_allreduce_fn allreduce, smm_hip_host_sendrecv_fn sendrecv, void* user,
                             smm_hip_comm** out) {
	if (!out || !allreduce || !sendrecv || world < 1 || rank < 0 || rank >= world) {
		setError("comm_create_host: bad arguments");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	SMM_TRY(ensureInit());
	auto* c = new smm_hip_comm();
	c->rank = rank;
	c->world = world;
	c->kind = SMM_COMM_HOST;
	c->hostAllreduce = allreduce;
	c->hostSendrecv = sendrecv;
	c->user = user;
	return commFinish(c, out);
}

int smm_hip_comm_destroy(smm_hip_comm* c) {
	if (!c) return SMM_HIP_OK;
	if (c->stream) {
		hipStreamSynchronize(c->stream);
		forgetStream(c->stream);
		hipStreamDestroy(c->stream);
	}
	for (hipEvent_t e : c->events) {
		if (e) hipEventDestroy(e);
	}
	if (c->nccl && rccl()) rccl()->CommDestroy(c->nccl);
	if (c->pinned) hipHostFree(c->pinned);
	if (c->d_i64) hipFree(c->d_i64);
	delete c;
	return SMM_HIP_OK;
}

int smm_hip_comm_info(const smm_hip_comm* c, int* rank, int* world, int* kind) {
	if (!c) {
		setError("comm_info: null communicator");
		return SMM_HIP_ERR_INVALID;
	}
	if (rank) *rank = c->rank;
	if (world) *world = c->world;
	if (kind) *kind = c->kind;
	return SMM_HIP_OK;
}

int smm_hip_comm_rccl_ranks(const smm_hip_comm* c, int* count) {
	if (!c || !count) {
		setError("comm_rccl_ranks: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*count = 0;
	if (c->kind != SMM_COMM_RCCL) return SMM_HIP_OK;  // not an RCCL communicator: 0
	SMM_TRY(commUsable(c));
	RcclApi* api = rccl();
	if (!api || !api->CommCount) {
		setError("comm_rccl_ranks: this librccl has no ncclCommCount");
		return SMM_HIP_ERR_COMM;
	}
	SMM_RCCL_TRY(api->CommCount(c->nccl, count));
	return SMM_HIP_OK;
}

// exercises every collective the loops use on this communicator: an all-reduce of (rank + 1) and a ring exchange (with one rank:
// a send to / receive from itself).  Returns SMM_HIP_ERR_COMM when a result is wrong.
static int commSelftest(smm_hip_comm* c);
int smm_hip_comm_selftest(smm_hip_comm* c) {
	if (!c) {
		setError("comm_selftest: null communicator");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(commUsable(c));
	return guardComm(c, commSelftest(c));
}

static int commSelftest(smm_hip_comm* c) {
	hipStream_t s = c->stream;
	DevBuf<double> buf;
	SMM_TRY(buf.alloc(4));
	double h[4] = {static_cast<double>(c->rank + 1), 2.0 * (c->rank + 1), static_cast<double>(c->rank), -1.0};
	SMM_HIP_TRY(hipMemcpyAsync(buf, h, sizeof(h), hipMemcpyHostToDevice, s));
	if (c->kind != SMM_COMM_SELF) SMM_TRY(commAllreduce<double>(c, buf, 2, s));
	if (c->kind != SMM_COMM_SELF) {
		const int next = (c->rank + 1) % c->world, prev = (c->rank + c->world - 1) % c->world;
		std::vector<Seg> sends{{next, 2, 1}}, recvs{{prev, 3, 1}};
		SMM_TRY(commExchange<double>(c, buf.p, sends, recvs, s));
	}
	double g[4];
	SMM_HIP_TRY(hipMemcpyAsync(g, buf, sizeof(g), hipMemcpyDeviceToHost, s));
	SMM_TRY(boundedSync(c, s));
	if (c->kind != SMM_COMM_SELF) {
		const double want = 0.5 * c->world * (c->world + 1);
		const int prev = (c->rank + c->world - 1) % c->world;
		if (g[0] != want || g[1] != 2 * want || g[3] != static_cast<double>(prev)) {
			setError("comm_selftest: got %g %g %g, expected %g %g %d", g[0], g[1], g[3], want, 2 * want, prev);
			return SMM_HIP_ERR_COMM;
		}
	}
	return SMM_HIP_OK;
}

int smm_hip_partition_rows_by_nnz(const int* start, int rows, int world, int* bounds) {
	if (!start || !bounds || rows < 0 || world < 1) {
		setError("partition_rows_by_nnz: bad arguments");
		return SMM_HIP_ERR_INVALID;
	}
	const long long total = start[rows];
	bounds[0] = 0;
	for (int g = 1; g < world; ++g) {
		const long long target = total * g / world;
		const int* it = std::lower_bound(start + bounds[g - 1], start + rows, target, [](int v, long long t) { return static_cast<long long>(v) < t; });
		bounds[g] = static_cast<int>(it - start);
	}
	bounds[world] = rows;
	return SMM_HIP_OK;
}

}  // extern "C"
