// smm_assembly.hip -- a CSRMatrix assembled from triplets ON THE DEVICE: the reference's TripletMatrix::addEntry (ref:606-618: repeated
// (row, col) pairs add up in the order they were given) followed by CSRMatrix::fillArrays (ref:1606-1641), in two passes.
//   symbolic (once per triplet list, smm_hip_assembly_create*): one 64-bit key per triplet, row above column, packed into the bits that
//     rows and cols need; a STABLE radix sort of (key, list index) -- rocprim, as in the other set-up paths --; the heads of the runs of
//     equal keys numbered by a prefix sum; positions[] and run_begin[] written by the heads, start[] by one binary search per row.  Kept:
//     start[rows + 1], positions[nnz], perm[n] (the list index of every sorted contribution, list order inside a run) and
//     run_begin[nnz + 1] -- the latter dropped when no pair repeats (n == nnz).
//   numeric (per csr_create / refill, assembleKernel): one lane per stored entry reads its run of perm[], gathers values[perm[j]] and adds
//     them strictly left to right -- the first contribution taken as it is, one rounding per further one --, one coalesced store.  No
//     atomics, no sort, no search: the result depends on the list alone, never on the launch geometry.
//     Bytes: n (s + 4) + (nnz + 1) 4 read, nnz s written (+ nnz s read for ADD); without repeats n (s + 4) read, n s written.
// A refill writes the matrix's values[] and then takes the path of every other value edit (csrValuesEdited, smm_csr_update.hip).
#include <algorithm>
#include <climits>

#include "smm_csr_build.h"

struct smm_hip_assembly {
	int rows = 0, cols = 0, nnz = 0;
	long long n = 0;
	int longestRun = 0;
	int firstActiveStart = 0;
	int midLen = 0;                // entries of the middle row (what the SpMV heuristic of a created matrix looks at)
	unsigned long long stamp = 0;  // left in every matrix this plan creates (smm_hip_csr::assemblyStamp): refill recognises them by it
	int* d_start = nullptr;
	int* d_positions = nullptr;
	int* d_perm = nullptr;
	int* d_run_begin = nullptr;  // null when n == nnz: entry k is contribution perm[k]
};

namespace smm {
namespace {

constexpr int ATPB = BUILD_TPB;
constexpr unsigned long long NO_BAD = ~0ULL;

// one lane per triplet: key = row above col in colBits + rowBits bits, seq = list index; the smallest list index of an entry outside
// [0, rows) x [0, cols) lands in *firstBad (its key is not used: the caller stops there)
__global__ __launch_bounds__(ATPB) void keyBuildKernel(long long n, int rows, int cols, int colBits, const int* __restrict__ r, const int* __restrict__ c,
                                                       unsigned long long* __restrict__ key, int* __restrict__ seq, unsigned long long* firstBad) {
	const long long i = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (i >= n) return;
	const int row = r[i], col = c[i];
	const bool ok = row >= 0 && row < rows && col >= 0 && col < cols;
	key[i] = ok ? (static_cast<unsigned long long>(row) << colBits) | static_cast<unsigned long long>(col) : 0ULL;
	seq[i] = static_cast<int>(i);
	if (!ok) atomicMin(firstBad, static_cast<unsigned long long>(i));
}

// sorted keys: 1 where a run of equal keys begins
__global__ __launch_bounds__(ATPB) void runHeadKernel(long long n, const unsigned long long* __restrict__ key, int* __restrict__ head) {
	const long long j = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (j >= n) return;
	head[j] = j == 0 || key[j] != key[j - 1] ? 1 : 0;
}

// runIdx = inclusive prefix sum of the heads: the head of run k (runIdx == k + 1) writes the entry's column and where its run begins
__global__ __launch_bounds__(ATPB) void runScatterKernel(long long n, int nnz, int colBits, const unsigned long long* __restrict__ key,
                                                         const int* __restrict__ runIdx, int* __restrict__ positions, int* __restrict__ runBegin) {
	const long long j = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (j >= n) return;
	const int k = runIdx[j] - 1;
	if (j == 0 || runIdx[j - 1] != k + 1) {
		positions[k] = static_cast<int>(key[j] & ((1ULL << colBits) - 1ULL));
		if (runBegin) runBegin[k] = static_cast<int>(j);
	}
	if (j == n - 1 && runBegin) runBegin[nnz] = static_cast<int>(n);
}

// start[r] = number of stored entries in the rows before r: the first sorted contribution whose row is >= r is the head of a run
// (n > 0; r = 0 .. rows)
__global__ __launch_bounds__(ATPB) void rowStartKernel(int rows, long long n, int nnz, int colBits, const unsigned long long* __restrict__ key,
                                                       const int* __restrict__ runIdx, int* __restrict__ start) {
	const long long r = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (r > rows) return;
	const unsigned long long want = static_cast<unsigned long long>(r) << colBits;
	long long lo = 0, hi = n;  // first j in [0, n] with key[j] >= want
	while (lo < hi) {
		const long long mid = lo + ((hi - lo) >> 1);
		if (key[mid] < want) lo = mid + 1;
		else hi = mid;
	}
	start[r] = lo == n ? nnz : runIdx[lo] - 1;
}

// info[0] = the longest run, info[1] = the first row that holds an entry
__global__ __launch_bounds__(ATPB) void planInfoKernel(int nnz, int colBits, const unsigned long long* __restrict__ key, const int* __restrict__ runBegin,
                                                       int* info) {
	__shared__ int sMax;
	const long long k = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (threadIdx.x == 0) sMax = 0;
	__syncthreads();
	if (k == 0) info[1] = static_cast<int>(key[0] >> colBits);
	if (k < nnz) atomicMax(&sMax, runBegin ? runBegin[k + 1] - runBegin[k] : 1);
	__syncthreads();
	if (threadIdx.x == 0) atomicMax(info, sMax);  // (one per workgroup)
}

// THE NUMERIC PASS.  One lane per stored entry k: its contributions are perm[runBegin[k] .. runBegin[k + 1]) in list order (RUNS), or
// perm[k] alone.  v = first; v = v + next; ... (a lone -0.0 stays -0.0); ADD: out[k] = out[k] + v, one more rounding.  Consecutive lanes
// read consecutive runs of perm[] and store consecutive out[k]; only values[perm[j]] is a gather, as local as the caller's list is.
// One workgroup per 256 entries, not a persistent grid: the lanes waiting on their gather are what hides its latency.
template <typename T, bool RUNS, bool ADD>
__global__ __launch_bounds__(ATPB) void assembleKernel(int nnz, const int* __restrict__ perm, const int* __restrict__ runBegin, const T* __restrict__ vals,
                                                       T* out) {
	const long long k = static_cast<long long>(blockIdx.x) * ATPB + threadIdx.x;
	if (k >= nnz) return;
	T v;
	if constexpr (RUNS) {
		const int b = runBegin[k], e = runBegin[k + 1];
		v = vals[perm[b]];
		for (int j = b + 1; j < e; ++j) v = v + vals[perm[j]];
	} else {
		v = vals[perm[k]];
	}
	if constexpr (ADD) out[k] = out[k] + v;
	else out[k] = v;
}

template <typename T>
int launchAssemble(const smm_hip_assembly* p, const T* d_vals, T* d_out, bool add, hipStream_t s) {
	if (p->nnz <= 0) return SMM_HIP_OK;
	const int grid = gridOf(p->nnz);
	if (p->d_run_begin) {
		if (add) assembleKernel<T, true, true><<<grid, ATPB, 0, s>>>(p->nnz, p->d_perm, p->d_run_begin, d_vals, d_out);
		else assembleKernel<T, true, false><<<grid, ATPB, 0, s>>>(p->nnz, p->d_perm, p->d_run_begin, d_vals, d_out);
	} else {
		if (add) assembleKernel<T, false, true><<<grid, ATPB, 0, s>>>(p->nnz, p->d_perm, nullptr, d_vals, d_out);
		else assembleKernel<T, false, false><<<grid, ATPB, 0, s>>>(p->nnz, p->d_perm, nullptr, d_vals, d_out);
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

void planFree(smm_hip_assembly* p) {
	if (!p) return;
	devFree(p->d_start);
	devFree(p->d_positions);
	devFree(p->d_perm);
	devFree(p->d_run_begin);
	delete p;
}
struct PlanDeleter {
	void operator()(smm_hip_assembly* p) const { planFree(p); }
};

// the symbolic pass over index arrays in device memory; synchronises `s` (the range verdict and nnz are needed on the host)
int planOnDevice(int rows, int cols, long long n, const int* d_rows, const int* d_cols, hipStream_t s, smm_hip_assembly** out) {
	SetupTrace trace("assembly: symbolic pass");
	static std::atomic<unsigned long long> nextStamp{1};
	std::unique_ptr<smm_hip_assembly, PlanDeleter> p(new smm_hip_assembly());
	p->rows = rows;
	p->cols = cols;
	p->n = n;
	p->stamp = nextStamp.fetch_add(1, std::memory_order_relaxed);
	p->firstActiveStart = rows;
	SMM_TRY(allocArray(&p->d_start, static_cast<size_t>(rows) + 1));
	if (n == 0) {
		SMM_TRY(allocArray(&p->d_positions, 0));
		SMM_TRY(allocArray(&p->d_perm, 0));
		SMM_HIP_TRY(hipMemsetAsync(p->d_start, 0, (static_cast<size_t>(rows) + 1) * sizeof(int), s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		*out = p.release();
		return SMM_HIP_OK;
	}
	const size_t cnt = static_cast<size_t>(n);
	const int colBits = bitsFor(cols), rowBits = bitsFor(rows);
	DevBuf<unsigned long long> keyIn, keyOut, d_bad;
	DevBuf<int> seqIn, runIdx, d_info;
	SMM_TRY(keyIn.alloc(cnt));
	SMM_TRY(seqIn.alloc(cnt));
	SMM_TRY(d_bad.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), s));
	keyBuildKernel<<<gridOf(n), ATPB, 0, s>>>(n, rows, cols, colBits, d_rows, d_cols, keyIn, seqIn, d_bad);
	SMM_HIP_TRY(hipGetLastError());
	unsigned long long bad = NO_BAD;
	SMM_HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (bad != NO_BAD) {
		setError("assembly_create: entry %llu of the list lies outside the %d x %d matrix", bad, rows, cols);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(keyOut.alloc(cnt));
	SMM_TRY(allocArray(&p->d_perm, cnt));
	SMM_TRY(sortPairs(keyIn.p, keyOut.p, seqIn.p, p->d_perm, cnt, static_cast<unsigned>(std::max(1, colBits + rowBits)), s));
	keyIn.release();  // (stream-ordered: the allocator hands a block out again only behind the work that was using it)
	seqIn.release();
	SMM_TRY(runIdx.alloc(cnt));
	runHeadKernel<<<gridOf(n), ATPB, 0, s>>>(n, keyOut, runIdx);
	SMM_HIP_TRY(hipGetLastError());
	SMM_TRY(scanInclusive(runIdx.p, runIdx.p, cnt, s));
	int nnz = 0;
	SMM_HIP_TRY(hipMemcpyAsync(&nnz, runIdx.p + (cnt - 1), sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	p->nnz = nnz;  // (1 .. n, and n <= 2^31 - 1: the library's 32-bit limit holds by construction)
	SMM_TRY(allocArray(&p->d_positions, static_cast<size_t>(nnz)));
	if (nnz != n) SMM_TRY(allocArray(&p->d_run_begin, static_cast<size_t>(nnz) + 1));
	SMM_TRY(d_info.alloc(2));
	SMM_HIP_TRY(hipMemsetAsync(d_info, 0, 2 * sizeof(int), s));
	runScatterKernel<<<gridOf(n), ATPB, 0, s>>>(n, nnz, colBits, keyOut, runIdx, p->d_positions, p->d_run_begin);
	rowStartKernel<<<gridOf(rows + 1LL), ATPB, 0, s>>>(rows, n, nnz, colBits, keyOut, runIdx, p->d_start);
	planInfoKernel<<<gridOf(nnz), ATPB, 0, s>>>(nnz, colBits, keyOut, p->d_run_begin, d_info);
	SMM_HIP_TRY(hipGetLastError());
	int info[2] = {0, 0}, mid[2] = {0, 0};
	SMM_HIP_TRY(hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(mid, p->d_start + rows / 2, 2 * sizeof(int), hipMemcpyDeviceToHost, s));  // (rows >= 1 here)
	SMM_HIP_TRY(hipStreamSynchronize(s));
	p->longestRun = info[0];
	p->firstActiveStart = info[1];
	p->midLen = mid[1] - mid[0];
	*out = p.release();
	return SMM_HIP_OK;
}

int checkList(int rows, int cols, long long n, const int* r, const int* c, smm_hip_assembly** out) {
	if (!out) {
		setError("assembly_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (n > INT_MAX) {
		setError("assembly_create: %lld triplets exceed the library's 32-bit limit of 2^31 - 1", n);
		return SMM_HIP_ERR_INVALID;
	}
	if (rows < 0 || cols < 0 || n < 0 || (n > 0 && (!r || !c))) {
		setError("assembly_create: negative size or null index array");
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

int planFromHost(int rows, int cols, long long n, const int* r, const int* c, smm_hip_assembly** out) {
	SMM_TRY(checkList(rows, cols, n, r, c, out));
	hipStream_t s = libStream();
	DevBuf<int> dr, dc;
	SMM_TRY(dr.alloc(static_cast<size_t>(n)));
	SMM_TRY(dc.alloc(static_cast<size_t>(n)));
	SMM_TRY(hostToDev(dr, r, sizeof(int) * static_cast<size_t>(n), s));
	SMM_TRY(hostToDev(dc, c, sizeof(int) * static_cast<size_t>(n), s));
	return planOnDevice(rows, cols, n, dr, dc, s, out);
}

// a matrix of its own over copies of the plan's start[] / positions[] and freshly assembled values
template <typename T>
int csrFromPlan(const smm_hip_assembly* p, const T* vals, bool onDevice, hipStream_t s, smm_hip_csr** out) {
	if (!out) {
		setError("assembly_csr_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!p || (p->n > 0 && !vals)) {
		setError("assembly_csr_create: null plan or values");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	if (!onDevice) s = libStream();
	DevBuf<T> staged;
	if (!onDevice && p->n > 0) {
		SMM_TRY(staged.alloc(static_cast<size_t>(p->n)));
		SMM_TRY(hostToDev(staged, vals, sizeof(T) * static_cast<size_t>(p->n), s));
		vals = staged;
	}
	OwnedCsr m;
	SMM_TRY(newOwnedCsr(p->rows, p->cols, dtypeOf<T>(), &m));
	SMM_TRY(allocCsrEntries(m.get(), p->nnz, false));
	const size_t nnz = static_cast<size_t>(p->nnz);
	SMM_HIP_TRY(hipMemcpyAsync(m->d_start, p->d_start, (static_cast<size_t>(p->rows) + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
	if (nnz) SMM_HIP_TRY(hipMemcpyAsync(m->d_positions, p->d_positions, nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
	SMM_TRY(launchAssemble<T>(p, vals, static_cast<T*>(m->d_values), false, s));
	if (!onDevice) SMM_HIP_TRY(hipStreamSynchronize(s));
	m->nnz = p->nnz;
	m->firstActiveStart = p->firstActiveStart;
	m->stream_mid_len = p->midLen;
	m->assemblyStamp = p->stamp;
	chooseSpmvConfig(m.get());
	m->ready = true;
	*out = m.release();
	return SMM_HIP_OK;
}

template <typename T>
int refill(const smm_hip_assembly* p, smm_hip_csr* m, const T* vals, int mode, bool onDevice, hipStream_t s) {
	if (!p || !m || (p->n > 0 && !vals) || (mode != SMM_UPDATE_SET && mode != SMM_UPDATE_ADD)) {
		setError("assembly_refill: null plan, matrix or values, or unknown mode");
		return SMM_HIP_ERR_INVALID;
	}
	if (m->dtype != dtypeOf<T>()) {
		setError("assembly_refill: the matrix holds the other element type");
		return SMM_HIP_ERR_INVALID;
	}
	if (m->assemblyStamp != p->stamp || m->rows != p->rows || m->cols != p->cols) {
		setError("assembly_refill: the matrix was not created by this plan");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	if (!onDevice) s = libStream();
	SMM_TRY(ensureCsrReady(m, s, onDevice));
	DevBuf<T> staged;
	if (!onDevice && p->n > 0) {
		SMM_TRY(staged.alloc(static_cast<size_t>(p->n)));
		SMM_TRY(hostToDev(staged, vals, sizeof(T) * static_cast<size_t>(p->n), s));
		vals = staged;
	}
	SMM_TRY(launchAssemble<T>(p, vals, static_cast<T*>(m->d_values), mode == SMM_UPDATE_ADD, s));
	SMM_TRY(csrValuesEdited(m, s));
	if (!onDevice) SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

}  // namespace
}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_assembly_create(int rows, int cols, long long n, const int* row_idx, const int* col_idx, smm_hip_assembly** out) {
	return planFromHost(rows, cols, n, row_idx, col_idx, out);
}

int smm_hip_assembly_create_dev(int rows, int cols, long long n, const int* d_row_idx, const int* d_col_idx, smm_hip_stream stream, smm_hip_assembly** out) {
	SMM_TRY(checkList(rows, cols, n, d_row_idx, d_col_idx, out));
	return planOnDevice(rows, cols, n, d_row_idx, d_col_idx, pickStream(stream), out);
}

int smm_hip_assembly_info(const smm_hip_assembly* plan, int* rows, int* cols, long long* n, int* nnz, int* longest_run) {
	if (!plan) {
		setError("assembly_info: null plan");
		return SMM_HIP_ERR_INVALID;
	}
	if (rows) *rows = plan->rows;
	if (cols) *cols = plan->cols;
	if (n) *n = plan->n;
	if (nnz) *nnz = plan->nnz;
	if (longest_run) *longest_run = plan->longestRun;
	return SMM_HIP_OK;
}

int smm_hip_assembly_pattern(const smm_hip_assembly* plan, int* start, int* positions) {
	if (!plan) {
		setError("assembly_pattern: null plan");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	if (start) SMM_TRY(devToHost(start, plan->d_start, (static_cast<size_t>(plan->rows) + 1) * sizeof(int), s));
	if (positions && plan->nnz > 0) SMM_TRY(devToHost(positions, plan->d_positions, static_cast<size_t>(plan->nnz) * sizeof(int), s));
	return SMM_HIP_OK;
}

int smm_hip_assembly_destroy(smm_hip_assembly* plan) {
	planFree(plan);
	return SMM_HIP_OK;
}

int smm_hip_assembly_csr_create_f32(const smm_hip_assembly* plan, const float* values, smm_hip_csr** out) { return csrFromPlan<float>(plan, values, false, nullptr, out); }
int smm_hip_assembly_csr_create_f64(const smm_hip_assembly* plan, const double* values, smm_hip_csr** out) { return csrFromPlan<double>(plan, values, false, nullptr, out); }
int smm_hip_assembly_csr_create_dev_f32(const smm_hip_assembly* plan, const float* d_values, smm_hip_stream stream, smm_hip_csr** out) {
	return csrFromPlan<float>(plan, d_values, true, pickStream(stream), out);
}
int smm_hip_assembly_csr_create_dev_f64(const smm_hip_assembly* plan, const double* d_values, smm_hip_stream stream, smm_hip_csr** out) {
	return csrFromPlan<double>(plan, d_values, true, pickStream(stream), out);
}
int smm_hip_assembly_refill_f32(const smm_hip_assembly* plan, smm_hip_csr* m, const float* values, int mode) { return refill<float>(plan, m, values, mode, false, nullptr); }
int smm_hip_assembly_refill_f64(const smm_hip_assembly* plan, smm_hip_csr* m, const double* values, int mode) { return refill<double>(plan, m, values, mode, false, nullptr); }
int smm_hip_assembly_refill_dev_f32(const smm_hip_assembly* plan, smm_hip_csr* m, const float* d_values, int mode, smm_hip_stream stream) {
	return refill<float>(plan, m, d_values, mode, true, pickStream(stream));
}
int smm_hip_assembly_refill_dev_f64(const smm_hip_assembly* plan, smm_hip_csr* m, const double* d_values, int mode, smm_hip_stream stream) {
	return refill<double>(plan, m, d_values, mode, true, pickStream(stream));
}

}  // extern "C"
