// smm_convert.hip -- a matrix in the OTHER PRECISION, made on the device: the handle of smm_hip_csr_convert_create (copies of start[] and
// positions[], values[] converted) and the pass that carries a value edit of the source over to it (smm_hip_csr_convert_refresh).
//   convert: one pass over values[], one lane per pack of PACK elements: f64 -> f32 reads two 16-byte packs and stores one, f32 -> f64 reads
//     one and stores two, a copy moves one each way.  16-byte accesses need both arrays 16-byte aligned at the same element: the host finds
//     the shortest element-wise head after which they are (arrays of the library's allocator: none) and hands it to the kernel; when the two
//     arrays never line up (a caller-owned array at an odd element) the whole array takes one element per lane.  The tail does too.
//     Bytes: nnz (sizeof(S) + sizeof(D)).
//   range: static_cast<float>(v) of a finite double is not finite iff |v| >= 2^128 - 2^103.  A lane that meets such an entry lowers *firstBad
//     to its index (atomicMin from the lane: the smallest index wins whatever the order); the host reads the word before anything is
//     handed out or installed.  NaN -> NaN, Inf -> Inf, -0.0 -> -0.0; underflow to a subnormal or to zero is not an error.
//   refresh: a narrowing conversion goes to scratch, the word is read (the call synchronises), then the scratch becomes dst's values (owned
//     arrays) or is copied into them (caller-owned), as smm_hip_csr_multiply_into_* installs its result; the other conversions cannot fail
//     and write dst's values directly.  Then the path of every value edit (csrValuesEdited).
#include <climits>

#include "smm_csr_build.h"
#include "smm_solver_host.h"

namespace smm {
namespace {

constexpr int CTPB = 256;
constexpr int PACK = 4;  // elements per lane and step of the 16-byte path (two 16-byte accesses on the fp64 side, one on the fp32 side)
constexpr int NO_ENTRY = INT_MAX;

typedef float cvt_f32x4 __attribute__((ext_vector_type(4)));
typedef double cvt_f64x2 __attribute__((ext_vector_type(2)));

// d = (D)v; narrowing: a finite v whose rounding is not finite lowers *firstBad to i
template <typename S, typename D>
__device__ __forceinline__ D convertOne(S v, long long i, int* firstBad) {
	const D d = static_cast<D>(v);
	if constexpr (sizeof(D) < sizeof(S)) {
		if (v - v == S(0) && !(d - d == D(0))) atomicMin(firstBad, static_cast<int>(i));
	}
	return d;
}

__device__ __forceinline__ void loadPack(const float* p, float (&v)[PACK]) {
	const cvt_f32x4 a = *reinterpret_cast<const cvt_f32x4*>(p);
	v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
}
__device__ __forceinline__ void loadPack(const double* p, double (&v)[PACK]) {
	const cvt_f64x2 a = reinterpret_cast<const cvt_f64x2*>(p)[0];
	const cvt_f64x2 b = reinterpret_cast<const cvt_f64x2*>(p)[1];
	v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
}
__device__ __forceinline__ void storePack(float* p, const float (&v)[PACK]) {
	cvt_f32x4 a = {v[0], v[1], v[2], v[3]};
	*reinterpret_cast<cvt_f32x4*>(p) = a;
}
__device__ __forceinline__ void storePack(double* p, const double (&v)[PACK]) {
	cvt_f64x2 a = {v[0], v[1]}, b = {v[2], v[3]};
	reinterpret_cast<cvt_f64x2*>(p)[0] = a;
	reinterpret_cast<cvt_f64x2*>(p)[1] = b;
}

// dst[i] = (D)src[i], i < n.  [0, head) and [head + packs * PACK, n) one element per lane, the packs between 16 bytes per access
// (src + head and dst + head are 16-byte aligned when packs > 0: convertLaunch).  Every index is below n: no access leaves the arrays.
template <typename S, typename D>
__global__ __launch_bounds__(CTPB) void convertKernel(long long n, long long head, long long packs, const S* __restrict__ src, D* __restrict__ dst,
                                                      int* firstBad) {
	const long long stride = static_cast<long long>(gridDim.x) * CTPB;
	const long long lane = static_cast<long long>(blockIdx.x) * CTPB + threadIdx.x;
	for (long long p = lane; p < packs; p += stride) {
		const long long i = head + p * PACK;
		S v[PACK];
		D d[PACK];
		loadPack(src + i, v);
#pragma unroll
		for (int e = 0; e < PACK; ++e) d[e] = convertOne<S, D>(v[e], i + e, firstBad);
		storePack(dst + i, d);
	}
	const long long body = packs * PACK;
	for (long long k = lane; k < n - body; k += stride) {  // the head, then the tail
		const long long i = k < head ? k : k + body;
		dst[i] = convertOne<S, D>(src[i], i, firstBad);
	}
}

int gridFor(long long work) { return static_cast<int>(std::max<long long>(1, std::min<long long>((work + CTPB - 1) / CTPB, numCUs() * 8LL))); }

// the shortest head (in elements) after which both arrays are 16-byte aligned, -1 when there is none
template <typename S, typename D>
long long commonHead(const S* src, const D* dst) {
	for (long long h = 0; h < 4; ++h) {  // (16 / 4: the residues of an fp32 array; an fp64 array has two of them)
		if (reinterpret_cast<uintptr_t>(src + h) % 16 == 0 && reinterpret_cast<uintptr_t>(dst + h) % 16 == 0) return h;
	}
	return -1;
}

// asynchronous on `s`; firstBad (narrowing only; preset to NO_ENTRY by the caller) may be null otherwise
template <typename S, typename D>
int convertLaunch(long long n, const S* src, D* dst, int* firstBad, hipStream_t s) {
	if (n <= 0) return SMM_HIP_OK;
	long long head = commonHead(src, dst), packs = 0;
	if (head < 0 || head > n) head = n;
	else packs = (n - head) / PACK;
	convertKernel<S, D><<<gridFor(std::max(packs, n - packs * PACK)), CTPB, 0, s>>>(n, head, packs, src, dst, firstBad);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

int convertAny(int srcType, int dstType, long long n, const void* src, void* dst, int* firstBad, hipStream_t s) {
	if (srcType == SMM_DTYPE_F64 && dstType == SMM_DTYPE_F32) return convertLaunch(n, static_cast<const double*>(src), static_cast<float*>(dst), firstBad, s);
	if (srcType == SMM_DTYPE_F32 && dstType == SMM_DTYPE_F64) return convertLaunch(n, static_cast<const float*>(src), static_cast<double*>(dst), firstBad, s);
	if (srcType == SMM_DTYPE_F32) return convertLaunch(n, static_cast<const float*>(src), static_cast<float*>(dst), firstBad, s);
	return convertLaunch(n, static_cast<const double*>(src), static_cast<double*>(dst), firstBad, s);
}

bool narrowing(int srcType, int dstType) { return srcType == SMM_DTYPE_F64 && dstType == SMM_DTYPE_F32; }

// the range word of a narrowing conversion: preset before the pass, read (the stream synchronised) after it
struct RangeWord {
	DevBuf<int> d;
	int arm(hipStream_t s) {
		SMM_TRY(d.alloc(1));
		SMM_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.p), NO_ENTRY, 1, s));
		return SMM_HIP_OK;
	}
	int read(hipStream_t s, const char* what) {
		int first = NO_ENTRY;
		SMM_HIP_TRY(hipMemcpyAsync(&first, d.p, sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (first == NO_ENTRY) return SMM_HIP_OK;
		setError("%s: values[%d] is finite in fp64 and outside the range of fp32", what, first);
		return SMM_HIP_ERR_INVALID;
	}
};

int convertCreate(const smm_hip_csr* a, int dtype, hipStream_t s, smm_hip_csr** out) {
	const char* what = "csr_convert_create";
	SetupTrace trace("convert: create");
	SMM_TRY(ensureCsrReady(a, s, true));
	const int rows = a->rows, nnz = a->nnz;
	if (nnz < 0) {
		setError("%s: start[rows] is negative", what);
		return SMM_HIP_ERR_INVALID;
	}
	OwnedCsr c;
	SMM_TRY(newOwnedCsr(rows, a->cols, dtype, &c));
	SMM_TRY(allocCsrEntries(c.get(), nnz, false));
	RangeWord range;
	SyncOnExit drain{s};  // (an error return must not release the new arrays under the copies queued into them)
	SMM_HIP_TRY(hipMemcpyAsync(c->d_start, a->d_start, (static_cast<size_t>(rows) + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
	if (nnz > 0) SMM_HIP_TRY(hipMemcpyAsync(c->d_positions, a->d_positions, static_cast<size_t>(nnz) * sizeof(int), hipMemcpyDeviceToDevice, s));
	const bool narrow = narrowing(a->dtype, dtype);
	if (narrow) SMM_TRY(range.arm(s));
	SMM_TRY(convertAny(a->dtype, dtype, nnz, a->d_values, c->d_values, range.d.p, s));
	if (narrow) SMM_TRY(range.read(s, what));
	SMM_TRY(ensureCsrReady(c.get(), s, true));  // nnz, the first active row, the typical row and the kernel choice as for caller-owned device arrays
	drain.armed = false;                         // (that has synchronised)
	*out = c.release();
	return SMM_HIP_OK;
}

int convertRefresh(smm_hip_csr* dst, const smm_hip_csr* src, hipStream_t s) {
	const char* what = "csr_convert_refresh";
	SMM_TRY(ensureCsrReady(src, s, true));
	SMM_TRY(ensureCsrReady(dst, s, true));
	if (dst->rows != src->rows || dst->cols != src->cols || dst->nnz != src->nnz) {
		setError("%s: dst is %d x %d with %d entries, src %d x %d with %d", what, dst->rows, dst->cols, dst->nnz, src->rows, src->cols, src->nnz);
		return SMM_HIP_ERR_INVALID;
	}
	const int nnz = dst->nnz;
	if (nnz > 0 && narrowing(src->dtype, dst->dtype)) {
		RangeWord range;
		DevBuf<float> scratch;
		SyncOnExit drain{s};
		SMM_TRY(range.arm(s));
		SMM_TRY(scratch.alloc(static_cast<size_t>(nnz)));
		SMM_TRY(convertAny(src->dtype, dst->dtype, nnz, src->d_values, scratch.p, range.d.p, s));
		SMM_TRY(range.read(s, what));
		drain.armed = false;
		SMM_TRY(adoptValues(dst, scratch, s));
	} else if (nnz > 0) {
		SMM_TRY(convertAny(src->dtype, dst->dtype, nnz, src->d_values, dst->d_values, nullptr, s));
	}
	return csrValuesEdited(dst, s);
}

}  // namespace

int csrConvertCreate(const smm_hip_csr* a, int dtype, hipStream_t s, smm_hip_csr** out) { return convertCreate(a, dtype, s, out); }

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_csr_convert_create(const smm_hip_csr* a, int dtype, smm_hip_stream stream, smm_hip_csr** out) {
	if (!out) {
		setError("csr_convert_create: out is null");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (!a) {
		setError("csr_convert_create: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (dtype != SMM_DTYPE_F32 && dtype != SMM_DTYPE_F64) {
		setError("csr_convert_create: dtype must be SMM_DTYPE_F32 or SMM_DTYPE_F64");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	return convertCreate(a, dtype, pickStream(stream), out);
}

int smm_hip_csr_convert_refresh(smm_hip_csr* dst, const smm_hip_csr* src, smm_hip_stream stream) {
	if (!dst || !src) {
		setError("csr_convert_refresh: null matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (dst == src) {
		setError("csr_convert_refresh: dst must not be src");
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	return convertRefresh(dst, src, pickStream(stream));
}

}  // extern "C"
