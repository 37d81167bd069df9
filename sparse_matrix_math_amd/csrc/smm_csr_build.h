// smm_csr_build.h -- the kit of the device operations that build a new smm_hip_csr or rewrite the values of one they made earlier
// (transpose, permutation, assembly, product, sum, block matrix / submatrix, conversion) and of the set-up code that scans and sorts.
//   device primitives: the rocprim scans and radix sorts, each behind ONE two-phase call (size query, scratch, run) -- no other file of the
//     library names rocprim (smm_dist_create.hip keeps a scan of its own);
//   small host helpers: bitsFor, gridOf, Word<T>, readFlag;
//   handle construction: OwnedCsr, newOwnedCsr, allocCsrEntries (every array holds at least one element);
//   shared tails: startsFromCounts (row counts -> start[] with the 2^31 - 1 refusal), adoptValues (a scratch array becomes the values),
//     refreshVerdict (is this matrix the source of that derived handle?);
//   shared kernels: rowOfEntry, startCheckKernel, intsDifferKernel, narrowKernel.
// Nothing here is on the path of an SpMV, a preconditioner apply or a solver loop.
#pragma once
#include <climits>
#include <memory>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "smm_internal.h"

namespace smm {

constexpr int BUILD_TPB = 256;

// ---- small host helpers ------------------------------------------------------------------------------------------------------------------
inline int bitsFor(long long count) {  // bits that hold 0 .. count - 1, count >= 1 (an int count gives at most 31, as a 31-bit loop would)
	int b = 0;
	while (b < 63 && (count - 1) >> b) ++b;
	return b;
}

inline int gridOf(long long work, int tpb = BUILD_TPB) { return static_cast<int>(std::max<long long>(1, (work + tpb - 1) / tpb)); }

// the unsigned word as wide as T: values that only travel are moved as raw words (no arithmetic: -0.0 and NaN payloads are kept)
template <typename T>
struct Word;
template <>
struct Word<float> {
	using type = unsigned;
};
template <>
struct Word<double> {
	using type = unsigned long long;
};

inline int readFlag(const int* d_flag, hipStream_t s, int* flag) {
	SMM_HIP_TRY(hipMemcpyAsync(flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

// ---- device primitives -------------------------------------------------------------------------------------------------------------------
// The scratch of a primitive.  A call without one allocates its own, which goes back to the allocator stream-ordered (a block is handed out
// again only behind the work that was using it); a loop of calls passes one, which grows and never shrinks.
struct PrimScratch {
	DevBuf<unsigned char> buf;
	int need(size_t bytes) { return bytes <= buf.n && buf.p ? SMM_HIP_OK : buf.alloc(bytes); }
};

// call(temp, bytes) is the rocprim call: with a null temp it only reports the bytes it wants.  Every primitive below is a template, so
// that a unit compiles the device code of those it calls and of no other; input pointers are passed on with the type the caller holds
// them in (K* or const K*), since rocprim instantiates its kernels per iterator type.
template <typename Call>
int primRun(PrimScratch* keep, Call&& call) {
	PrimScratch own;
	PrimScratch& scratch = keep ? *keep : own;
	size_t bytes = 0;
	SMM_HIP_TRY(call(static_cast<void*>(nullptr), bytes));
	SMM_TRY(scratch.need(std::max<size_t>(bytes, 1)));
	SMM_HIP_TRY(call(static_cast<void*>(scratch.buf.p), bytes));
	return SMM_HIP_OK;
}

// out[i] = in[0] + .. + in[i - 1] over ints; in == out scans in place
template <typename In>
int scanExclusive(In in, int* out, size_t n, hipStream_t s) {
	return primRun(nullptr, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, 0, n, rocprim::plus<int>(), s); });
}
template <typename In>
int scanExclusive64(In counts, long long* out, size_t n, hipStream_t s) {
	return primRun(nullptr, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, counts, out, 0LL, n, rocprim::plus<long long>(), s); });
}
// out[i] = in[0] + .. + in[i], summed as Out
template <typename In, typename Out>
int scanInclusive(In in, Out* out, size_t n, hipStream_t s) {
	return primRun(nullptr, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, rocprim::plus<Out>(), s); });
}
// stable radix sorts over the bits [0, endBit) of the key
template <typename KeyIn, typename K, typename ValIn>
int sortPairs(KeyIn keyIn, K* keyOut, ValIn valIn, int* valOut, size_t n, unsigned endBit, hipStream_t s, PrimScratch* keep = nullptr) {
	return primRun(keep, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keyIn, keyOut, valIn, valOut, n, 0u, endBit, s); });
}
template <typename KeyIn, typename K>
int sortKeys(KeyIn keyIn, K* keyOut, size_t n, unsigned endBit, hipStream_t s, PrimScratch* keep = nullptr) {
	return primRun(keep, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, keyIn, keyOut, n, 0u, endBit, s); });
}
// segment k is [begins[k], ends[k]) of the n keys
template <typename KeyIn>
int sortKeysSegmented(KeyIn keyIn, unsigned* keyOut, unsigned n, unsigned segments, int* begins, int* ends, unsigned endBit, hipStream_t s) {
	return primRun(nullptr, [&](void* t, size_t& b) { return rocprim::segmented_radix_sort_keys(t, b, keyIn, keyOut, n, segments, begins, ends, 0u, endBit, s); });
}

// ---- shared kernels ----------------------------------------------------------------------------------------------------------------------
// the row that holds entry e: the last r in [0, rows) with start[r] <= e (rows >= 1); reads start[0 .. rows) only
__device__ __forceinline__ int rowOfEntry(int rows, const int* __restrict__ start, int e) {
	int lo = 0, hi = rows - 1;
	while (lo < hi) {
		const int mid = lo + ((hi - lo + 1) >> 1);
		if (start[mid] <= e) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

// start[0] == 0 and start[] non-decreasing, or *bad is raised: rowOfEntry relies on neither for its own safety (it only ever reads
// start[0 .. rows]), but a matrix that fails here has no transpose and no permutation
static __global__ __launch_bounds__(BUILD_TPB) void startCheckKernel(int rows, const int* __restrict__ start, int* bad) {
	const long long r = static_cast<long long>(blockIdx.x) * BUILD_TPB + threadIdx.x;
	if (r >= rows) return;
	if (start[r] > start[r + 1] || (r == 0 && start[0] != 0)) *bad = 1;  // (every writer writes the same word)
}

static __global__ __launch_bounds__(BUILD_TPB) void intsDifferKernel(long long n, const int* __restrict__ a, const int* __restrict__ b, int* differs) {
	bool d = false;
	for (long long i = static_cast<long long>(blockIdx.x) * BUILD_TPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * BUILD_TPB) d |= a[i] != b[i];
	if (d) *differs = 1;  // (every writer writes the same word)
}

// out[i] = in[i] (the caller has checked that the largest fits 32 bits)
static __global__ __launch_bounds__(BUILD_TPB) void narrowKernel(long long n, const long long* __restrict__ in, int* __restrict__ out) {
	const long long i = static_cast<long long>(blockIdx.x) * BUILD_TPB + threadIdx.x;
	if (i < n) out[i] = static_cast<int>(in[i]);
}

// ---- handle construction -----------------------------------------------------------------------------------------------------------------
struct CsrDeleter {
	void operator()(smm_hip_csr* m) const { smm_hip_csr_destroy(m); }
};
using OwnedCsr = std::unique_ptr<smm_hip_csr, CsrDeleter>;

template <typename T>
int allocArray(T** p, size_t count) { return devAlloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)); }

// a handle that owns its arrays, with start[rows + 1] allocated; an error return of the caller destroys it with whatever it holds by then
inline int newOwnedCsr(int rows, int cols, int dtype, OwnedCsr* c) {
	c->reset(new smm_hip_csr());
	(*c)->rows = rows;
	(*c)->cols = cols;
	(*c)->dtype = dtype;
	(*c)->owns = true;
	return allocArray(&(*c)->d_start, static_cast<size_t>(rows) + 1);
}

// positions[nnz], values[nnz] of the handle's element type and, when asked, tperm[nnz]: each of at least one element
inline int allocCsrEntries(smm_hip_csr* c, long long nnz, bool withTperm) {
	const size_t count = static_cast<size_t>(nnz ? nnz : 1);
	SMM_TRY(allocArray(&c->d_positions, count));
	SMM_TRY(devAlloc(&c->d_values, count * (c->dtype == SMM_DTYPE_F32 ? sizeof(float) : sizeof(double))));
	if (withTperm) SMM_TRY(allocArray(&c->d_tperm, count));
	return SMM_HIP_OK;
}

// ---- shared tails ------------------------------------------------------------------------------------------------------------------------
// c->d_start[0 .. rows] = the exclusive sums of counts[0 .. rows] (counts[rows] is 0), formed in 64 bits; *nnz = their total, refused above
// 2^31 - 1 as "<what>: the <noun> holds ... entries".  Synchronises `s` once, for the total.
template <typename Counts>
int startsFromCounts(const char* what, const char* noun, Counts counts, int rows, smm_hip_csr* c, long long* nnz, hipStream_t s) {
	DevBuf<long long> start64;
	SMM_TRY(start64.alloc(static_cast<size_t>(rows) + 1));
	SMM_TRY(scanExclusive64(counts, start64.p, static_cast<size_t>(rows) + 1, s));
	SMM_HIP_TRY(hipMemcpyAsync(nnz, start64.p + rows, sizeof(long long), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (*nnz > INT_MAX) {
		setError("%s: the %s holds %lld entries, more than 2^31 - 1", what, noun, *nnz);
		return SMM_HIP_ERR_INVALID;
	}
	narrowKernel<<<gridOf(rows + 1LL), BUILD_TPB, 0, s>>>(rows + 1LL, start64.p, c->d_start);
	return SMM_HIP_OK;
}

// The freshly computed values of c (c->nnz of them, in scratch) take the place of the old ones: the scratch becomes the values array and the
// old one goes back to the allocator behind the work queued on it; a borrowed array gets a copy instead.
template <typename T>
int adoptValues(smm_hip_csr* c, DevBuf<T>& scratch, hipStream_t s) {
	if (c->nnz <= 0) return SMM_HIP_OK;
	if (c->owns) {
		void* old = c->d_values;
		c->d_values = scratch.detach();
		devFree(old);
	} else {
		SMM_HIP_TRY(hipMemcpyAsync(c->d_values, scratch.p, static_cast<size_t>(c->nnz) * sizeof(T), hipMemcpyDeviceToDevice, s));
	}
	return SMM_HIP_OK;
}

// Is `a` a matrix with the pattern numbered `uid`, the source of a derived handle (a transpose, a permutation)?  What `a` has on record
// answers; when it has nothing and holds entries, enqueueCheck(d_differs) queues the caller's source check on a zeroed flag, the flag is read
// (synchronising `s`) and the verdict goes on record.
template <typename Check>
int refreshVerdict(const smm_hip_csr* a, unsigned long long uid, hipStream_t s, Check&& enqueueCheck, bool* same) {
	int verdict = csrPatternVerdict(a, uid);
	if (verdict < 0) {
		verdict = 1;
		if (a->nnz > 0) {
			DevBuf<int> d_diff;
			SMM_TRY(d_diff.alloc(1));
			SMM_HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), s));
			enqueueCheck(d_diff.p);
			SMM_HIP_TRY(hipGetLastError());
			int diff = 0;
			SMM_TRY(readFlag(d_diff, s, &diff));
			verdict = diff ? 0 : 1;
		}
		csrPatternRecord(a, uid, verdict == 1);
	}
	*same = verdict == 1;
	return SMM_HIP_OK;
}

}  // namespace smm
