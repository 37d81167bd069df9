// smm_solver_host.h -- the host frame of the device-resident Krylov drivers (smm_solvers*.hip): the argument check, the grid of an update
// kernel, the host's look at the loop's `done` word, the read-back that ends a loop, the report of the thick-restart drivers, and the
// host-pointer form of a driver.  What a driver launches per iteration stays written out in its own file.
#pragma once
#include <algorithm>

#include "smm_internal.h"
#include "smm_solver_scal.h"

namespace smm {

// workgroups of an update kernel of 256 lanes over n elements: at most one per partial-sum slot
inline int solverGrid(long long n) { return static_cast<int>(std::max<long long>(1, std::min<long long>((n + SCAL_TPB - 1) / SCAL_TPB, NPART))); }

// The argument check of a driver and of its host-pointer wrapper: a matrix of T's dtype, square, and no null vector when it has rows.
template <typename T, typename... V>
int solverCheck(const char* who, const smm_hip_csr* a, const V*... vectors) {
	if (!a || a->dtype != dtypeOf<T>()) {
		setError("%s: null matrix or dtype mismatch", who);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("%s: matrix must be square", who);
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows > 0 && !(true && ... && (vectors != nullptr))) {
		setError("%s: null vector", who);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

// The rectangular sibling (LSQR): `a` is rows x cols with any rows and cols, `b` has rows elements and `x` has cols; a vector may be null
// only when it has no element.
template <typename T>
int solverCheckRect(const char* who, const smm_hip_csr* a, const T* b, const T* x) {
	if (!a || a->dtype != dtypeOf<T>()) {
		setError("%s: null matrix or dtype mismatch", who);
		return SMM_HIP_ERR_INVALID;
	}
	if ((a->rows > 0 && a->cols > 0) && (!b || !x)) {
		setError("%s: null vector", who);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

// Synchronises `s` when the scope is left while still armed.  Declared after whatever the queued work touches (staging buffers, a
// transpose built for the solve) and disarmed on the path that has synchronised anyway: no error return releases them under queued work.
struct SyncOnExit {
	hipStream_t s;
	bool armed = true;
	~SyncOnExit() {
		if (armed) (void)hipStreamSynchronize(s);
	}
};

// The host's look at a loop's device `done` word (DonePoller: no stall of the queue).  One poller per host thread, reused by every solve
// of that thread.  The word is first asked for at iteration `first`, then `every` iterations later each time; every == 0: after
// max(4, min(64, i / 4)) iterations -- kernels enqueued past the end of the loop are no-ops, so a late answer costs launches, not results.
// `planned` (every == 0 only): the iterations the loop will enqueue at most.  A look with fewer than MIN_SAVING of them left is not made: it
// could spare a few no-op launches at best, and whether its answer -- or an earlier look's, which is read at the same place -- has arrived
// by then depends on how far the GPU has got, so a short loop (a handful of planned iterations) would enqueue a number of launches that
// varies from run to run.  Without it such a loop enqueues every planned iteration, every time.
struct LoopWatch {
	static constexpr int MIN_SAVING = 4;
	DonePoller* poller = nullptr;
	const int* flag = nullptr;
	int next = 0, every = 0, planned = 0x7fffffff;
	int rc = SMM_HIP_OK;  // what a failed look returned: loopFinish hands it on
	int begin(hipStream_t s, const int* doneFlag, int first, int fixedInterval = 0, int plannedIterations = 0x7fffffff) {
		static thread_local DonePoller threadPoller;
		poller = &threadPoller;
		flag = doneFlag;
		next = first;
		every = fixedInterval;
		planned = plannedIterations;
		return poller->init(s);
	}
	// one device word on the host, through the poller's pinned mailbox; synchronises the stream.  Between begin() and the first leave().
	int fetch(const int* word, int* seen) {
		SMM_HIP_TRY(hipMemcpyAsync(&poller->mailbox[0], word, sizeof(int), hipMemcpyDeviceToHost, poller->s));
		SMM_HIP_TRY(hipStreamSynchronize(poller->s));
		*seen = poller->mailbox[0];
		poller->mailbox[0] = 0;
		return SMM_HIP_OK;
	}
	// ... and one fp64 device word the same way (two of the mailbox's four ints)
	int fetch(const double* word, double* seen) {
		SMM_HIP_TRY(hipMemcpyAsync(&poller->mailbox[0], word, sizeof(double), hipMemcpyDeviceToHost, poller->s));
		SMM_HIP_TRY(hipStreamSynchronize(poller->s));
		memcpy(seen, &poller->mailbox[0], sizeof(double));
		poller->mailbox[0] = poller->mailbox[1] = 0;
		return SMM_HIP_OK;
	}
	// true: enqueue no iteration i -- the loop was seen done, or the look failed (rc)
	bool leave(int i) {
		if (i != next) return false;
		if (every == 0 && planned - i < MIN_SAVING) return false;  // (next stays: no later look either)
		const int seen = poller->post(flag);
		if (seen < 0) rc = seen;
		next = i + (every ? every : std::max(4, std::min(64, i / 4)));
		return seen != 0;
	}
};

// The zero start.  A driver's set-up residual r = b - A x0 from an x0 of zeros is b, bit for bit, when every stored value is finite: each
// product is v * (+-0) = +-0, a row's sum starts at +0 and +0 + (-0) = +0 under round-to-nearest, so it -- and the sum of its pieces --
// stays +0, and b[i] - (+0) = b[i], b[i] = -0 included.  (An Inf or a NaN among the values must still reach r: 0 * Inf = NaN.)  *skip:
// the host knows both, so the driver launches no SpMV for the set-up and copies b instead.  x0 is read once (n elements); values[] is read
// once per version of the values (smm_hip_csr::values_finite), the first time a start is found to be zero.  Each look is one word through
// the watch's mailbox and a stream synchronise, before the set-up is enqueued.  SMM_HIP_ZERO_START=0: never (the SpMV runs).
// `count`: the elements of x0 -- a->cols, which a square matrix's driver may write as a->rows (the form without it).
template <typename T>
int zeroStart(const smm_hip_csr* a, const T* x0, long long count, LoopWatch& watch, hipStream_t s, bool* skip) {
	*skip = false;
	if (count <= 0 || !env::flagOr(env::ZERO_START, true)) return SMM_HIP_OK;
	int finite = a->values_finite.load(std::memory_order_acquire);
	if (finite == 0) return SMM_HIP_OK;
	DevBuf<int> word;
	SMM_TRY(word.alloc(1));
	int zero = 0;
	SMM_TRY(launchScanFlag<T>(count, x0, false, word, s));
	SMM_TRY(watch.fetch(word, &zero));
	if (!zero) return SMM_HIP_OK;
	if (finite < 0) {
		SMM_TRY(launchScanFlag<T>(a->nnz, static_cast<const T*>(a->d_values), true, word, s));
		SMM_TRY(watch.fetch(word, &finite));
		a->values_finite.store(finite ? 1 : 0, std::memory_order_release);
	}
	*skip = finite != 0;
	return SMM_HIP_OK;
}

template <typename T>
int zeroStart(const smm_hip_csr* a, const T* x0, LoopWatch& watch, hipStream_t s, bool* skip) {
	return zeroStart<T>(a, x0, a->rows, watch, s, skip);
}

// The end of every loop: the watch's or a launch's error, else `bytes` of the loop's device scalars on the host; synchronises `s`.
inline int loopFinish(const LoopWatch& watch, void* h, const void* d, size_t bytes, hipStream_t s) {
	SMM_TRY(watch.rc);
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// What a thick-restart driver (eigsh, svds) reports besides its arrays, and the hand-over to the caller's pointers (each may be null).
struct RitzOut {
	int status = SMM_SOLVER_SUCCESS, nconv = 0, restarts = 0, matvecs = 0;
	int wrote = 0;  // eigenpairs or singular triplets written to the outputs
};

inline void ritzReport(const RitzOut& o, int* nconv, int* restarts, int* matvecs, int* status) {
	if (nconv) *nconv = o.nconv;
	if (restarts) *restarts = o.restarts;
	if (matvecs) *matvecs = o.matvecs;
	if (status) *status = o.status;
}

// labels of a traced wrapper's SetupTrace lines (null: not traced)
struct HostTrace {
	const char *all = nullptr, *alloc = nullptr, *in = nullptr, *loop = nullptr, *out = nullptr;
};

// The host-pointer form of a driver, the reference's calling convention: b, x0 (null: the solver has none) and x, `count` elements each in
// caller-owned host memory, are staged onto the device, run(d_b, d_x0, d_x, stream) is the driver on the copies, and x comes back -- when
// `wrote` is given only if *wrote != 0 afterwards.  A failure on the way synchronises the stream before the copies are released.
template <typename T, typename Run>
int solveFromHost(size_t count, const T* b, const T* x0, T* x, Run&& run, const int* wrote = nullptr, const HostTrace& tr = {}) {
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	SetupTrace traceAll(tr.all);
	DevBuf<T> db, dx0, dx;
	SyncOnExit drain{s};
	{
		SetupTrace trace(tr.alloc);
		SMM_TRY(db.alloc(count));
		if (x0) SMM_TRY(dx0.alloc(count));
		SMM_TRY(dx.alloc(count));
	}
	if (count) {
		SetupTrace trace(tr.in);
		SMM_TRY(hostToDev(db, b, sizeof(T) * count, s));
		if (x0) SMM_TRY(hostToDev(dx0, x0, sizeof(T) * count, s));
		SMM_TRY(hostToDev(dx, x, sizeof(T) * count, s));
		if (tr.in && SetupTrace::on()) SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	{
		SetupTrace trace(tr.loop);
		SMM_TRY(run(static_cast<const T*>(db), static_cast<const T*>(dx0), static_cast<T*>(dx), s));
	}
	if (count && (!wrote || *wrote)) {
		SetupTrace trace(tr.out);
		SMM_TRY(devToHost(x, dx, sizeof(T) * count, s));
	}
	drain.armed = false;  // (the driver's read-back and devToHost have synchronised)
	return SMM_HIP_OK;
}

// The host-pointer form of a driver whose two vectors differ in length (LSQR: b has the matrix's rows, x its columns): b (`countB`
// elements) and x (`countX`, in / out) are staged, run(d_b, d_x, stream) is the driver on the copies, and x comes back.
template <typename T, typename Run>
int solveFromHost2(size_t countB, size_t countX, const T* b, T* x, Run&& run) {
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	DevBuf<T> db, dx;
	SyncOnExit drain{s};
	SMM_TRY(db.alloc(countB));
	SMM_TRY(dx.alloc(countX));
	if (countB) SMM_TRY(hostToDev(db, b, sizeof(T) * countB, s));
	if (countX) SMM_TRY(hostToDev(dx, x, sizeof(T) * countX, s));
	SMM_TRY(run(static_cast<const T*>(db), static_cast<T*>(dx), s));
	if (countX) SMM_TRY(devToHost(x, dx, sizeof(T) * countX, s));
	drain.armed = false;  // (the driver's read-back and devToHost have synchronised)
	return SMM_HIP_OK;
}

}  // namespace smm
