// smm_csr_update.hip -- the VALUES of a device-resident matrix edited in place: the reference's CSRMatrix mutators (operator*=,
// inplaceAdd / inplaceSubtract, updateEntry / addEntry, zeroValues: ref:1525-1604) as device passes, plus bulk replacement of
// values[] from host or device memory.  The pattern (start[], positions[]) never changes, so everything the library derived from it
// alone stays: tile tables, row masks, dictionary codes, the march plan, the kernel choice.  What was derived from the VALUES is kept
// coherent here (valuesEdited):
//   * the constant-diagonal encoding (pat_const, d_pat_cval, pat_cval_host): scale, zero and axpy of two such handles update the k
//     diagonal values exactly and in stream order (cvalUpdateKernel) (every entry of a diagonal holds the same bits, so the per-entry result is the per-diagonal one); any
//     other edit re-verifies every entry (reverifyConst) and drops the handle to the mask encoding with values read when a diagonal
//     is no longer constant.  A handle that was not constant is never promoted (same bits either way: a question of speed only);
//   * the single-launch BiCGStab's slot-major copy of the values (d_res_ell) and the PATTERN slots kernel's wave-sliced copy
//     (d_pat_slots, smm_spmv_slots.hip) are rewritten in place.
//   * what the handle knows about the finiteness of its values (values_finite, the zero start of the Krylov drivers) is forgotten.
// Preconditioners: SGS reads A's values at every apply; ILU0 / IC0 / JACOBI / BLOCK_* hold factors computed at create (snapshots).
#include <algorithm>
#include <cstring>

#include "smm_csr_build.h"

namespace smm {
namespace {

constexpr int UTPB = 256;

typedef float upd_f32x4 __attribute__((ext_vector_type(4)));
typedef double upd_f64x2 __attribute__((ext_vector_type(2)));
template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
	using type = upd_f32x4;
};
template <>
struct Vec16<double> {
	using type = upd_f64x2;
};

constexpr int EDIT_SCALE = 0, EDIT_AXPY = 1, EDIT_ZERO = 2, EDIT_OTHER = 3;

// v = v * alpha (AXPY false) or v = v + alpha * o (two roundings: the library is built with -ffp-contract=off), 16 bytes per lane and step
// when both arrays are 16-byte aligned (VEC), one element otherwise
template <typename T, bool AXPY, bool VEC>
__global__ __launch_bounds__(UTPB) void valuesUpdateKernel(long long n, T alpha, T* v, const T* o) {  // (o may be v: A += A)
	const long long stride = static_cast<long long>(gridDim.x) * UTPB;
	long long done = 0;
	if constexpr (VEC) {
		using V = typename Vec16<T>::type;
		constexpr int W = 16 / sizeof(T);
		const long long nv = n / W;
		V* vv = reinterpret_cast<V*>(v);
		const V* ov = reinterpret_cast<const V*>(o);
		for (long long i = static_cast<long long>(blockIdx.x) * UTPB + threadIdx.x; i < nv; i += stride) {
			V a = vv[i];
			if constexpr (AXPY) {
				const V b = ov[i];
				a = a + alpha * b;
			} else {
				a = a * alpha;
			}
			vv[i] = a;
		}
		done = nv * W;
	}
	for (long long i = done + static_cast<long long>(blockIdx.x) * UTPB + threadIdx.x; i < n; i += stride) {
		if constexpr (AXPY) {
			v[i] = v[i] + alpha * o[i];
		} else {
			v[i] = v[i] * alpha;
		}
	}
}

__global__ __launch_bounds__(UTPB) void patternDiffKernel(long long n, const int* __restrict__ a, const int* __restrict__ b, int* differs) {
	bool d = false;
	for (long long i = static_cast<long long>(blockIdx.x) * UTPB + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * UTPB) d |= a[i] != b[i];
	if (d) *differs = 1;  // (every writer writes the same word)
}

// one lane per entry: its index in values[] by a binary search of its row (ref:1551-1570), `nnz` for an entry that is not stored
// (out-of-range row or column included); key[i] / seq[i] feed the stable sort that puts the entries of one value in batch order
__global__ __launch_bounds__(UTPB) void findEntriesKernel(int n, int rows, int cols, int nnz, const int* __restrict__ start, const int* __restrict__ positions,
                                                          const int* __restrict__ r, const int* __restrict__ c, unsigned* __restrict__ key,
                                                          int* __restrict__ seq, unsigned char* __restrict__ found) {
	for (int i = blockIdx.x * UTPB + threadIdx.x; i < n; i += gridDim.x * UTPB) {
		const int row = r[i], col = c[i];
		int at = -1;
		if (row >= 0 && row < rows && col >= 0 && col < cols) {
			int lo = start[row], hi = start[row + 1] - 1;
			while (lo <= hi) {
				const int mid = lo + ((hi - lo) >> 1);
				const int pc = positions[mid];
				if (col > pc) lo = mid + 1;
				else if (col < pc) hi = mid - 1;
				else {
					at = mid;
					break;
				}
			}
		}
		key[i] = at < 0 ? static_cast<unsigned>(nnz) : static_cast<unsigned>(at);
		seq[i] = i;
		if (found) found[i] = at < 0 ? 0 : 1;
	}
}

// after the stable sort: the first entry of every run of one value walks its run in batch order -- SET keeps the last, ADD sums in order
template <typename T>
__global__ __launch_bounds__(UTPB) void applyEntriesKernel(int n, unsigned nnz, const unsigned* __restrict__ key, const int* __restrict__ seq,
                                                           const T* __restrict__ vals, int add, T* __restrict__ values) {
	for (int p = blockIdx.x * UTPB + threadIdx.x; p < n; p += gridDim.x * UTPB) {
		const unsigned idx = key[p];
		if (idx >= nnz || (p > 0 && key[p - 1] == idx)) continue;
		T v = values[idx];
		for (int q = p; q < n && key[q] == idx; ++q) v = add ? v + vals[seq[q]] : vals[seq[q]];
		values[idx] = v;
	}
}

// ---- the constant-diagonal check again, on the row masks the PATTERN analysis left (nothing pattern-shaped is rebuilt) ----
constexpr int CMAX = 32;  // constant diagonals are looked for in matrices of at most 32 offsets

// The entries of a row and their diagonals straight from the row's mask: the j-th set bit is the row's j-th stored entry.
//   mode 0 (the rows the analysis sampled, row = i (rows - 1) / (samples - 1)): one value per diagonal, plain stores -- any of them will
//          do, since mode 1 compares every entry with it;
//   mode 1 (every row): each entry's bits against its diagonal's value; flags[1] raised on a difference.
// A diagonal that mode 0 left without a value keeps +0 and is kept constant only if every entry on it is +0 -- right either way.
__global__ __launch_bounds__(UTPB) void constCheckKernel(int rows, int samples, int k, const int* __restrict__ start,
                                                         const unsigned long long* __restrict__ masks, const void* __restrict__ values, int elemBytes,
                                                         unsigned long long* cvalBits, int* flags, int mode) {
	__shared__ unsigned long long sCval[CMAX];
	if (mode == 1 && threadIdx.x < k) sCval[threadIdx.x] = cvalBits[threadIdx.x];
	__syncthreads();
	const long long count = mode == 0 ? samples : rows;
	bool varies = false;
	for (long long i = static_cast<long long>(blockIdx.x) * UTPB + threadIdx.x; i < count; i += static_cast<long long>(gridDim.x) * UTPB) {
		const int row = mode == 0 ? static_cast<int>(i * (rows - 1) / max(1, samples - 1)) : static_cast<int>(i);
		unsigned long long msk = masks[row];
		int at = start[row];
		while (msk) {
			const int j = __ffsll(msk) - 1;
			msk &= msk - 1;
			const unsigned long long bits = elemBytes == 4 ? static_cast<unsigned long long>(static_cast<const unsigned*>(values)[at])
			                                               : static_cast<const unsigned long long*>(values)[at];
			++at;
			if (mode == 0) cvalBits[j] = bits;
			else if (bits != sCval[j]) varies = true;
		}
	}
	if (varies) atomicOr(flags + 1, 1);
}

// the exact update of the k diagonal values, on the device and in stream order, with the arithmetic of valuesUpdateKernel:
// SCALE c = c * alpha, ZERO c = +0, AXPY c = c + alpha * other
template <typename T>
__global__ void cvalUpdateKernel(int k, int edit, T alpha, unsigned long long* cval, const unsigned long long* other) {
	const int j = threadIdx.x;
	if (j >= k) return;
	T c = T(0), o = T(0);
	if constexpr (sizeof(T) == 4) {
		c = __uint_as_float(static_cast<unsigned>(cval[j]));
		if (other) o = __uint_as_float(static_cast<unsigned>(other[j]));
	} else {
		c = __longlong_as_double(static_cast<long long>(cval[j]));
		if (other) o = __longlong_as_double(static_cast<long long>(other[j]));
	}
	T r = T(0);
	if (edit == 0) r = c * alpha;
	else if (edit == 1) r = c + alpha * o;
	if constexpr (sizeof(T) == 4) {
		cval[j] = static_cast<unsigned long long>(__float_as_uint(r));
	} else {
		cval[j] = static_cast<unsigned long long>(__double_as_longlong(r));
	}
}

int gridFor(long long work) { return static_cast<int>(std::max<long long>(1, std::min<long long>((work + UTPB - 1) / UTPB, numCUs() * 8LL))); }

template <typename T>
T fromBits(unsigned long long b) {
	T v;
	if constexpr (sizeof(T) == 4) {
		const unsigned lo = static_cast<unsigned>(b);
		memcpy(&v, &lo, 4);
	} else {
		memcpy(&v, &b, 8);
	}
	return v;
}
template <typename T>
unsigned long long toBits(T v) {
	if constexpr (sizeof(T) == 4) {
		unsigned lo;
		memcpy(&lo, &v, 4);
		return lo;
	} else {
		unsigned long long b;
		memcpy(&b, &v, 8);
		return b;
	}
}

unsigned long long uidOf(const smm_hip_csr* cm) {
	static std::atomic<unsigned long long> next{1};
	auto* m = const_cast<smm_hip_csr*>(cm);
	unsigned long long u = m->uid.load(std::memory_order_acquire);
	if (u) return u;
	const unsigned long long mine = next.fetch_add(1, std::memory_order_relaxed);
	return m->uid.compare_exchange_strong(u, mine, std::memory_order_acq_rel) ? mine : u;
}

// rows, cols, nnz, start[] and positions[] equal; the verdict is cached in both handles (patterns never change)
int samePattern(const smm_hip_csr* a, const smm_hip_csr* b, hipStream_t s, bool* same) {
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(ensureCsrReady(b, s, true));
	if (a == b) {
		*same = true;
		return SMM_HIP_OK;
	}
	if (a->rows != b->rows || a->cols != b->cols || a->nnz != b->nnz) {
		*same = false;
		return SMM_HIP_OK;
	}
	const unsigned long long ua = uidOf(a), ub = uidOf(b);
	{
		std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(a)->editMutex);
		for (const auto& e : a->patternSeen) {
			if (e.first == ub) {
				*same = e.second;
				return SMM_HIP_OK;
			}
		}
	}
	bool eq = true;
	const bool shared = a->d_start == b->d_start && (a->nnz == 0 || a->d_positions == b->d_positions);  // (handles over one set of index arrays)
	if (!shared) {
		DevBuf<int> d_diff;
		SMM_TRY(d_diff.alloc(1));
		SMM_HIP_TRY(hipMemsetAsync(d_diff, 0, sizeof(int), s));
		patternDiffKernel<<<gridFor(a->rows + 1LL), UTPB, 0, s>>>(a->rows + 1LL, a->d_start, b->d_start, d_diff);
		if (a->nnz > 0) patternDiffKernel<<<gridFor(a->nnz), UTPB, 0, s>>>(a->nnz, a->d_positions, b->d_positions, d_diff);
		SMM_HIP_TRY(hipGetLastError());
		int diff = 0;
		SMM_HIP_TRY(hipMemcpyAsync(&diff, d_diff, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		eq = diff == 0;
	}
	{
		std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(a)->editMutex);
		const_cast<smm_hip_csr*>(a)->patternSeen.emplace_back(ub, eq);
	}
	{
		std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(b)->editMutex);
		const_cast<smm_hip_csr*>(b)->patternSeen.emplace_back(ua, eq);
	}
	*same = eq;
	return SMM_HIP_OK;
}

// Synchronises `s`: the verdict decides which kernels the next launch takes.  Still constant: the new values go to d_pat_cval IN PLACE
// (the block preconditioners' one-launch form reads that buffer) and to pat_cval_host; not: pat_const drops and the handle reads
// values[] from now on (MASKS); d_pat_cval stays allocated until the handle is destroyed.
int reverifyConst(smm_hip_csr* m, hipStream_t s) {
	SetupTrace trace("edit: constant diagonals re-verified");
	const int k = m->pat_k;
	if (k < 1 || k > CMAX || !m->d_pat_masks || !m->d_pat_off || !m->d_pat_cval) {
		m->pat_const = false;
		return SMM_HIP_OK;
	}
	DevBuf<int> d_flag;
	DevBuf<unsigned long long> d_cval;
	SMM_TRY(d_flag.alloc(2));
	SMM_TRY(d_cval.alloc(CMAX));
	SMM_HIP_TRY(hipMemsetAsync(d_flag, 0, 2 * sizeof(int), s));
	SMM_HIP_TRY(hipMemsetAsync(d_cval, 0, CMAX * sizeof(unsigned long long), s));
	const int elemBytes = m->dtype == SMM_DTYPE_F32 ? 4 : 8;
	const int samples = std::min(m->rows, 16384);  // (the rows the analysis sampled)
	if (samples > 0) {
		const int sgrid = (samples + UTPB - 1) / UTPB;
		constCheckKernel<<<sgrid, UTPB, 0, s>>>(m->rows, samples, k, m->d_start, m->d_pat_masks, m->d_values, elemBytes, d_cval, d_flag, 0);
		constCheckKernel<<<gridFor(m->rows), UTPB, 0, s>>>(m->rows, samples, k, m->d_start, m->d_pat_masks, m->d_values, elemBytes, d_cval, d_flag, 1);
	}
	SMM_HIP_TRY(hipGetLastError());
	int flags[2] = {0, 0};
	std::vector<unsigned long long> cval(static_cast<size_t>(k));
	SMM_HIP_TRY(hipMemcpyAsync(flags, d_flag, sizeof(flags), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipMemcpyAsync(cval.data(), d_cval, static_cast<size_t>(k) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	if (flags[1] != 0) {
		m->pat_const = false;
		return SMM_HIP_OK;
	}
	SMM_HIP_TRY(hipMemcpyAsync(m->d_pat_cval, d_cval, static_cast<size_t>(k) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
	m->pat_cval_host = cval;
	return SMM_HIP_OK;
}

bool isConstForm(const smm_hip_csr* m) {
	return m->pat_state.load(std::memory_order_acquire) == 1 && m->pat_encoding == 0 && m->pat_const && m->d_pat_cval &&
	       static_cast<int>(m->pat_cval_host.size()) == m->pat_k;
}

// the value-dependent state after values[] changed on `s` (see the top of the file)
template <typename T>
int valuesEdited(smm_hip_csr* m, hipStream_t s, int edit, T alpha, const smm_hip_csr* other) {
	m->values_finite.store(-1, std::memory_order_release);  // (every edit, whatever the family: the zero start of the solvers asks again)
	if (m->pat_state.load(std::memory_order_acquire) != 1 || m->pat_encoding != 0) return SMM_HIP_OK;
	std::lock_guard<std::mutex> lock(m->tileMutex);
	if (isConstForm(m)) {
		const int k = m->pat_k;
		std::vector<unsigned long long> bits(m->pat_cval_host);
		bool exact = true;
		if (edit == EDIT_SCALE) {
			for (int j = 0; j < k; ++j) bits[j] = toBits<T>(fromBits<T>(bits[j]) * alpha);
		} else if (edit == EDIT_ZERO) {
			for (int j = 0; j < k; ++j) bits[j] = 0;
		} else if (edit == EDIT_AXPY && other && isConstForm(other) && other->pat_k == k && other->pat_offs_host == m->pat_offs_host) {
			for (int j = 0; j < k; ++j) bits[j] = toBits<T>(fromBits<T>(bits[j]) + alpha * fromBits<T>(other->pat_cval_host[j]));
		} else {
			exact = false;
		}
		if (exact) {
			// asynchronous: the k values are updated in place on `s` (the block preconditioners' one-launch form reads this buffer) with
			// the device's own arithmetic; the host copy (the single-launch BiCGStab's kernel arguments) the same way in IEEE arithmetic
			cvalUpdateKernel<T><<<1, CMAX, 0, s>>>(k, edit == EDIT_SCALE ? 0 : edit == EDIT_AXPY ? 1 : 2, alpha, m->d_pat_cval,
			                                       edit == EDIT_AXPY ? other->d_pat_cval : nullptr);
			SMM_HIP_TRY(hipGetLastError());
			m->pat_cval_host = bits;
		} else {
			SMM_TRY(reverifyConst(m, s));
		}
	}
	SMM_TRY(refreshPatternSlots(m, s));
	return refreshResEll(m, s);
}

int checkHandle(const smm_hip_csr* m, int dtype, const char* what) {
	if (!m) {
		setError("%s: null matrix", what);
		return SMM_HIP_ERR_INVALID;
	}
	if (m->dtype != dtype) {
		setError("%s: the matrix holds the other element type", what);
		return SMM_HIP_ERR_INVALID;
	}
	return ensureInit();
}

template <typename T>
int scaleDev(smm_hip_csr* m, T alpha, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_scale"));
	SMM_TRY(ensureCsrReady(m, s, true));
	if (m->nnz > 0) {
		T* v = static_cast<T*>(m->d_values);
		if (reinterpret_cast<uintptr_t>(v) % 16 == 0) valuesUpdateKernel<T, false, true><<<gridFor(m->nnz / (16 / sizeof(T)) + 1), UTPB, 0, s>>>(m->nnz, alpha, v, nullptr);
		else valuesUpdateKernel<T, false, false><<<gridFor(m->nnz), UTPB, 0, s>>>(m->nnz, alpha, v, nullptr);
		SMM_HIP_TRY(hipGetLastError());
	}
	return valuesEdited<T>(m, s, EDIT_SCALE, alpha, nullptr);
}

template <typename T>
int axpyDev(smm_hip_csr* m, T alpha, const smm_hip_csr* other, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_axpy"));
	SMM_TRY(checkHandle(other, dtypeOf<T>(), "csr_axpy"));
	bool same = false;
	SMM_TRY(samePattern(m, other, s, &same));
	if (!same) {
		setError("csr_axpy: the two matrices have different nonzero patterns");
		return SMM_HIP_ERR_INVALID;
	}
	if (m->nnz > 0) {
		T* v = static_cast<T*>(m->d_values);
		const T* o = static_cast<const T*>(other->d_values);
		if (reinterpret_cast<uintptr_t>(v) % 16 == 0 && reinterpret_cast<uintptr_t>(o) % 16 == 0) {
			valuesUpdateKernel<T, true, true><<<gridFor(m->nnz / (16 / sizeof(T)) + 1), UTPB, 0, s>>>(m->nnz, alpha, v, o);
		} else {
			valuesUpdateKernel<T, true, false><<<gridFor(m->nnz), UTPB, 0, s>>>(m->nnz, alpha, v, o);
		}
		SMM_HIP_TRY(hipGetLastError());
	}
	return valuesEdited<T>(m, s, EDIT_AXPY, alpha, other);
}

template <typename T>
int zeroDev(smm_hip_csr* m, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_zero"));
	SMM_TRY(ensureCsrReady(m, s, true));
	if (m->nnz > 0) SMM_HIP_TRY(hipMemsetAsync(m->d_values, 0, static_cast<size_t>(m->nnz) * sizeof(T), s));
	return valuesEdited<T>(m, s, EDIT_ZERO, T(0), nullptr);
}

// the batch in device memory (d_found may be null)
template <typename T>
int updateEntriesOnDevice(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const T* d_vals, int mode, unsigned char* d_found, hipStream_t s) {
	if (n <= 0) return SMM_HIP_OK;
	DevBuf<unsigned> keyIn, keyOut;
	DevBuf<int> seqIn, seqOut;
	SMM_TRY(keyIn.alloc(n));
	SMM_TRY(keyOut.alloc(n));
	SMM_TRY(seqIn.alloc(n));
	SMM_TRY(seqOut.alloc(n));
	findEntriesKernel<<<gridFor(n), UTPB, 0, s>>>(n, m->rows, m->cols, m->nnz, m->d_start, m->d_positions, d_rows, d_cols, keyIn, seqIn, d_found);
	SMM_HIP_TRY(hipGetLastError());
	unsigned endBit = 1;  // keys run over [0, nnz]: only their low bits are sorted
	while (endBit < 32 && (static_cast<unsigned>(m->nnz) >> endBit) != 0) ++endBit;
	SMM_TRY(sortPairs(keyIn.p, keyOut.p, seqIn.p, seqOut.p, static_cast<size_t>(n), endBit, s));
	applyEntriesKernel<T><<<gridFor(n), UTPB, 0, s>>>(n, static_cast<unsigned>(m->nnz), keyOut, seqOut, d_vals, mode == SMM_UPDATE_ADD ? 1 : 0,
	                                                  static_cast<T*>(m->d_values));
	SMM_HIP_TRY(hipGetLastError());
	return valuesEdited<T>(m, s, EDIT_OTHER, T(0), nullptr);
}

int checkBatch(int n, const void* rows, const void* cols, const void* vals, int mode) {
	if (n < 0 || (n > 0 && (!rows || !cols || !vals)) || (mode != SMM_UPDATE_SET && mode != SMM_UPDATE_ADD)) {
		setError("csr_update_entries: negative count, null array or unknown mode");
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
int updateEntriesDev(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const T* d_vals, int mode, unsigned char* d_found, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_update_entries"));
	SMM_TRY(checkBatch(n, d_rows, d_cols, d_vals, mode));
	SMM_TRY(ensureCsrReady(m, s, true));
	return updateEntriesOnDevice<T>(m, n, d_rows, d_cols, d_vals, mode, d_found, s);
}

template <typename T>
int updateEntriesHost(smm_hip_csr* m, int n, const int* rows, const int* cols, const T* vals, int mode, unsigned char* found) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_update_entries"));
	SMM_TRY(checkBatch(n, rows, cols, vals, mode));
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	if (n == 0) return SMM_HIP_OK;
	hipStream_t s = libStream();
	DevBuf<int> dr, dc;
	DevBuf<T> dv;
	DevBuf<unsigned char> df;
	SMM_TRY(dr.alloc(n));
	SMM_TRY(dc.alloc(n));
	SMM_TRY(dv.alloc(n));
	if (found) SMM_TRY(df.alloc(n));
	SMM_TRY(hostToDev(dr, rows, sizeof(int) * n, s));
	SMM_TRY(hostToDev(dc, cols, sizeof(int) * n, s));
	SMM_TRY(hostToDev(dv, vals, sizeof(T) * n, s));
	SMM_TRY(updateEntriesOnDevice<T>(m, n, dr, dc, dv, mode, found ? df.p : nullptr, s));
	if (found) SMM_TRY(devToHost(found, df, static_cast<size_t>(n), s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template <typename T>
int setValues(smm_hip_csr* m, const T* src, bool srcOnDevice, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_set_values"));
	SMM_TRY(ensureCsrReady(m, s, srcOnDevice));
	if (!srcOnDevice) s = libStream();
	if (m->nnz > 0 && !src) {
		setError("csr_set_values: null values");
		return SMM_HIP_ERR_INVALID;
	}
	const size_t bytes = static_cast<size_t>(m->nnz) * sizeof(T);
	if (srcOnDevice) {
		if (bytes && src != m->d_values) SMM_HIP_TRY(hipMemcpyAsync(m->d_values, src, bytes, hipMemcpyDeviceToDevice, s));
	} else {
		SMM_TRY(hostToDev(m->d_values, src, bytes, s));
	}
	SMM_TRY(valuesEdited<T>(m, s, EDIT_OTHER, T(0), nullptr));
	if (!srcOnDevice) SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

template <typename T>
int getValues(const smm_hip_csr* m, T* dst) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_get_values"));
	SMM_TRY(ensureCsrReady(m, nullptr, false));
	if (m->nnz > 0 && !dst) {
		setError("csr_get_values: null output");
		return SMM_HIP_ERR_INVALID;
	}
	return devToHost(dst, m->d_values, static_cast<size_t>(m->nnz) * sizeof(T), libStream());
}

template <typename T>
int valuesChanged(smm_hip_csr* m, hipStream_t s) {
	SMM_TRY(checkHandle(m, dtypeOf<T>(), "csr_values_changed"));
	SMM_TRY(ensureCsrReady(m, s, true));
	return valuesEdited<T>(m, s, EDIT_OTHER, T(0), nullptr);
}

}  // namespace

unsigned long long csrUid(const smm_hip_csr* m) { return uidOf(m); }

int csrPatternVerdict(const smm_hip_csr* a, unsigned long long uid) {
	if (uidOf(a) == uid) return 1;
	std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(a)->editMutex);
	for (const auto& e : a->patternSeen) {
		if (e.first == uid) return e.second ? 1 : 0;
	}
	return -1;
}

void csrPatternRecord(const smm_hip_csr* a, unsigned long long uid, bool same) {
	std::lock_guard<std::mutex> lock(const_cast<smm_hip_csr*>(a)->editMutex);
	const_cast<smm_hip_csr*>(a)->patternSeen.emplace_back(uid, same);
}

int csrValuesEdited(smm_hip_csr* m, hipStream_t s) {
	return m->dtype == SMM_DTYPE_F32 ? valuesEdited<float>(m, s, EDIT_OTHER, 0.f, nullptr) : valuesEdited<double>(m, s, EDIT_OTHER, 0.0, nullptr);
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_scale_f32(smm_hip_csr* m, float alpha, smm_hip_stream stream) { return scaleDev<float>(m, alpha, pickStream(stream)); }
int smm_hip_csr_scale_f64(smm_hip_csr* m, double alpha, smm_hip_stream stream) { return scaleDev<double>(m, alpha, pickStream(stream)); }
int smm_hip_csr_axpy_f32(smm_hip_csr* m, float alpha, const smm_hip_csr* other, smm_hip_stream stream) { return axpyDev<float>(m, alpha, other, pickStream(stream)); }
int smm_hip_csr_axpy_f64(smm_hip_csr* m, double alpha, const smm_hip_csr* other, smm_hip_stream stream) { return axpyDev<double>(m, alpha, other, pickStream(stream)); }
int smm_hip_csr_zero_f32(smm_hip_csr* m, smm_hip_stream stream) { return zeroDev<float>(m, pickStream(stream)); }
int smm_hip_csr_zero_f64(smm_hip_csr* m, smm_hip_stream stream) { return zeroDev<double>(m, pickStream(stream)); }

int smm_hip_csr_update_entries_f32(smm_hip_csr* m, int n, const int* rows, const int* cols, const float* values, int mode, unsigned char* found) {
	return updateEntriesHost<float>(m, n, rows, cols, values, mode, found);
}
int smm_hip_csr_update_entries_f64(smm_hip_csr* m, int n, const int* rows, const int* cols, const double* values, int mode, unsigned char* found) {
	return updateEntriesHost<double>(m, n, rows, cols, values, mode, found);
}
int smm_hip_csr_update_entries_dev_f32(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const float* d_values, int mode, unsigned char* d_found,
                                       smm_hip_stream stream) {
	return updateEntriesDev<float>(m, n, d_rows, d_cols, d_values, mode, d_found, pickStream(stream));
}
int smm_hip_csr_update_entries_dev_f64(smm_hip_csr* m, int n, const int* d_rows, const int* d_cols, const double* d_values, int mode, unsigned char* d_found,
                                       smm_hip_stream stream) {
	return updateEntriesDev<double>(m, n, d_rows, d_cols, d_values, mode, d_found, pickStream(stream));
}

int smm_hip_csr_set_values_f32(smm_hip_csr* m, const float* values) { return setValues<float>(m, values, false, nullptr); }
int smm_hip_csr_set_values_f64(smm_hip_csr* m, const double* values) { return setValues<double>(m, values, false, nullptr); }
int smm_hip_csr_set_values_dev_f32(smm_hip_csr* m, const float* d_values, smm_hip_stream stream) { return setValues<float>(m, d_values, true, pickStream(stream)); }
int smm_hip_csr_set_values_dev_f64(smm_hip_csr* m, const double* d_values, smm_hip_stream stream) { return setValues<double>(m, d_values, true, pickStream(stream)); }
int smm_hip_csr_get_values_f32(const smm_hip_csr* m, float* values) { return getValues<float>(m, values); }
int smm_hip_csr_get_values_f64(const smm_hip_csr* m, double* values) { return getValues<double>(m, values); }
int smm_hip_csr_values_changed_f32(smm_hip_csr* m, smm_hip_stream stream) { return valuesChanged<float>(m, pickStream(stream)); }
int smm_hip_csr_values_changed_f64(smm_hip_csr* m, smm_hip_stream stream) { return valuesChanged<double>(m, pickStream(stream)); }

int smm_hip_csr_same_pattern(const smm_hip_csr* a, const smm_hip_csr* b, int* same) {
	if (!a || !b || !same) {
		setError("csr_same_pattern: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_HIP_TRY(hipDeviceSynchronize());  // (no stream: the arrays may still be being written on any of the caller's streams)
	bool eq = false;
	SMM_TRY(samePattern(a, b, libStream(), &eq));
	*same = eq ? 1 : 0;
	return SMM_HIP_OK;
}

}  // extern "C"
