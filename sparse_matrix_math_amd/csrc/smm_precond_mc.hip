// smm_precond_mc.hip -- the MULTICOLOUR forms of SGS / ILU(0) / IC(0): colour the adjacency graph of A (smm_color.hip), number the rows
// colour by colour (perm[] = a stable sort of the rows by colour), B = P A Pᵀ, and run the exact kind on B:
//     M^-1 r = Pᵀ sweeps_B(P r).
// Rows of one colour do not reference each other, so a colour is a dependency level of BOTH sweeps and the rows of a level are a
// contiguous range of B: a sweep is `ncolors` passes shaped like an SpMV over B's rows, one lane per row, instead of the hundreds of
// levels the natural order has on a grid.  Inside a row the entries are visited exactly as smm_precond.hip's solveRow visits them, so the
// result is bit for bit the sequential sweep on B (tests/multicolor_restatement.py).
// The permutation is folded into the sweeps: the lower sweep reads rhs[perm[row]], the upper sweep's final write also stores
// x[perm[row]] -- no gather or scatter pass over a vector.  In between the sweeps work on y[] (permuted numbering), owned by the handle.
// Launches: one per colour of more than 1024 rows; runs of smaller colours are chained inside one 1024-lane workgroup with a workgroup
// barrier between colours, as the level-scheduled sweeps of smm_precond.hip do.  (A single-launch form with a grid barrier between the
// colours was not built: see DESIGN.md 3.16.)
// The handle is a SNAPSHOT (B is a copy); smm_hip_precond_multicolor_refresh redoes B's values and the factor on the kept colouring.
#include <algorithm>
#include <memory>

#include <rocprim/device/device_radix_sort.hpp>

#include "smm_device.h"
#include "smm_internal.h"

namespace smm {
namespace {

constexpr int MTPB = 256;
constexpr int SMALL_COLOR = 1024;  // colours up to this many rows are chained inside one workgroup

enum McMode { SGS_LO = 0, SGS_UP = 1, ILU_LO = 2, ILU_UP = 3, IC_LO = 4, IC_UP = 5 };

// One row of a sweep on B; the arithmetic is solveRow's (smm_precond.hip), entry for entry.  Lower sweeps read in[perm[row]] (the caller's
// rhs) and write y[row]; upper sweeps read y[] alone and write the row's result to y[row] AND out[perm[row]] (the caller's x).  Every row
// holds its diagonal (checked at create time), which ends the triangular part.
template <typename T, int MODE>
__device__ __forceinline__ void mcRow(int row, const int* __restrict__ start, const int* __restrict__ positions, const T* __restrict__ vals,
                                      const int* __restrict__ perm, const T* __restrict__ in, T* y, T* __restrict__ out) {
	const int b = start[row];
	const int e = start[row + 1];
	if (MODE == SGS_LO) {  // ref:1673-1695
		T lhs = in[perm[row]];
		int k = b;
		for (; k < e && positions[k] < row; ++k) lhs = smmFma(-vals[k], y[positions[k]], lhs);
		y[row] = lhs / vals[k];
	} else if (MODE == SGS_UP) {  // ref:1698-1711
		T lhs = T(0);
		int k = e - 1;
		for (; k >= b && positions[k] > row; --k) lhs = smmFma(vals[k], y[positions[k]], lhs);
		const T r = y[row] - lhs / vals[k];
		y[row] = r;
		out[perm[row]] = r;
	} else if (MODE == ILU_LO) {  // L y = rhs, unit diagonal
		T sum = in[perm[row]];
		for (int k = b; k < e && positions[k] < row; ++k) sum = smmFma(-vals[k], y[positions[k]], sum);
		y[row] = sum;
	} else if (MODE == ILU_UP) {  // U x = y
		T sum = y[row];
		int k = e - 1;
		for (; k >= b && positions[k] > row; --k) sum = smmFma(-vals[k], y[positions[k]], sum);
		const T r = sum / vals[k];
		y[row] = r;
		out[perm[row]] = r;
	} else if (MODE == IC_LO) {  // ref:1806-1819: sum -= l*x (plain multiply and subtract)
		T sum = in[perm[row]];
		int k = b;
		for (; k < e && positions[k] < row; ++k) {
			const T prod = vals[k] * y[positions[k]];
			sum = sum - prod;
		}
		y[row] = sum / vals[k];
	} else {  // IC_UP, ref:1822-1835
		T sum = y[row];
		int k = e - 1;
		for (; k >= b && positions[k] > row; --k) {
			const T prod = vals[k] * y[positions[k]];
			sum = sum - prod;
		}
		const T r = sum / vals[k];
		y[row] = r;
		out[perm[row]] = r;
	}
}

// one large colour: rows [begin, begin + count)
template <typename T, int MODE>
__global__ __launch_bounds__(MTPB) void mcColorKernel(int begin, int count, const int* __restrict__ start, const int* __restrict__ positions,
                                                      const T* __restrict__ vals, const int* __restrict__ perm, const T* __restrict__ in, T* y, T* __restrict__ out,
                                                      const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	const long long i = static_cast<long long>(blockIdx.x) * MTPB + threadIdx.x;
	if (i < count) mcRow<T, MODE>(begin + static_cast<int>(i), start, positions, vals, perm, in, y, out);
}

// a run of small colours inside one workgroup: c0, c0 + step, ... up to (not including) c1; bounds is the device copy of the colour bounds
template <typename T, int MODE>
__global__ __launch_bounds__(SMALL_COLOR) void mcChainKernel(const int* __restrict__ bounds, int c0, int c1, int step, const int* __restrict__ start,
                                                             const int* __restrict__ positions, const T* __restrict__ vals, const int* __restrict__ perm,
                                                             const T* __restrict__ in, T* y, T* __restrict__ out, const int* __restrict__ doneFlag) {
	if (doneFlag && *doneFlag) return;
	for (int c = c0; c != c1; c += step) {
		const int begin = bounds[c];
		const int count = bounds[c + 1] - begin;
		if (static_cast<int>(threadIdx.x) < count) mcRow<T, MODE>(begin + threadIdx.x, start, positions, vals, perm, in, y, out);
		// rows of the next colour read y[] written above by other wavefronts of this workgroup
		__threadfence_block();
		__syncthreads();
	}
}

__global__ __launch_bounds__(MTPB) void mcIotaKernel(int n, int* out) {
	const long long i = static_cast<long long>(blockIdx.x) * MTPB + threadIdx.x;
	if (i < n) out[i] = static_cast<int>(i);
}

// bounds[c] = the first position of the colour-sorted order whose colour is >= c (c = 0 .. ncolors)
__global__ __launch_bounds__(MTPB) void mcBoundsKernel(int n, int ncolors, const int* __restrict__ sortedColor, int* __restrict__ bounds) {
	const long long c = static_cast<long long>(blockIdx.x) * MTPB + threadIdx.x;
	if (c > ncolors) return;
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (sortedColor[mid] < c) lo = mid + 1;
		else hi = mid;
	}
	bounds[c] = lo;
}

// a caller's colouring: every colour in [0, n), no stored off-diagonal entry joins two rows of one colour; info[0] |= 1 otherwise, info[1] = the largest colour
__global__ __launch_bounds__(MTPB) void mcCheckColorsKernel(int n, const int* __restrict__ start, const int* __restrict__ positions, const int* __restrict__ colors,
                                                            int* info) {
	const long long i = static_cast<long long>(blockIdx.x) * MTPB + threadIdx.x;
	if (i >= n) return;
	const int c = colors[i];
	if (c < 0 || c >= n) {
		info[0] = 1;  // (every writer writes the same word)
		return;
	}
	atomicMax(info + 1, c);
	bool bad = false;
	for (int k = start[i]; k < start[i + 1]; ++k) {
		const int j = positions[k];
		if (j < 0 || j >= n) bad = true;  // (not addressed with)
		else if (j != i && colors[j] == c) bad = true;
	}
	if (bad) info[0] = 1;
}

int gridOf(long long work) { return static_cast<int>(std::max<long long>(1, (work + MTPB - 1) / MTPB)); }

}  // namespace
}  // namespace smm

struct smm_precond_mc {
	int base = SMM_PRECOND_SGS;  // the exact kind run on B
	int ncolors = 0;
	smm_hip_csr* B = nullptr;    // P A Pᵀ, owned
	int* d_colors = nullptr;     // colour of every row of A
	int* d_perm = nullptr;       // new row i is A's row d_perm[i]
	int* d_bounds = nullptr;     // ncolors + 1 row bounds of B (device copy of `bounds`)
	void* d_y = nullptr;         // the vector both sweeps work on (permuted numbering)
	std::vector<int> bounds;
	// launch groups of a sweep, in the order of the LOWER sweep (the upper sweep walks them backwards): chains of small colours or single large ones
	struct Group {
		int c0, c1;
		bool chain;
	};
	std::vector<Group> groups;
};

namespace smm {
namespace {

void planColorGroups(smm_precond_mc* C) {
	C->groups.clear();
	const int nc = C->ncolors;
	int c = 0;
	while (c < nc) {
		if (C->bounds[c + 1] - C->bounds[c] > SMALL_COLOR) {
			C->groups.push_back({c, c + 1, false});
			++c;
		} else {
			int e = c + 1;
			while (e < nc && C->bounds[e + 1] - C->bounds[e] <= SMALL_COLOR) ++e;
			C->groups.push_back({c, e, true});
			c = e;
		}
	}
}

template <typename T, int LO, int UP>
int runSweeps(const smm_precond_mc* C, const T* vals, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_hip_csr* B = C->B;
	T* y = static_cast<T*>(C->d_y);
	for (size_t g = 0; g < C->groups.size(); ++g) {
		const auto& G = C->groups[g];
		if (G.chain) {
			mcChainKernel<T, LO><<<1, SMALL_COLOR, 0, s>>>(C->d_bounds, G.c0, G.c1, 1, B->d_start, B->d_positions, vals, C->d_perm, rhs, y, x, doneFlag);
		} else {
			const int begin = C->bounds[G.c0], count = C->bounds[G.c1] - begin;
			mcColorKernel<T, LO><<<gridOf(count), MTPB, 0, s>>>(begin, count, B->d_start, B->d_positions, vals, C->d_perm, rhs, y, x, doneFlag);
		}
	}
	for (size_t g = C->groups.size(); g-- > 0;) {
		const auto& G = C->groups[g];
		if (G.chain) {
			mcChainKernel<T, UP><<<1, SMALL_COLOR, 0, s>>>(C->d_bounds, G.c1 - 1, G.c0 - 1, -1, B->d_start, B->d_positions, vals, C->d_perm, rhs, y, x, doneFlag);
		} else {
			const int begin = C->bounds[G.c0], count = C->bounds[G.c1] - begin;
			mcColorKernel<T, UP><<<gridOf(count), MTPB, 0, s>>>(begin, count, B->d_start, B->d_positions, vals, C->d_perm, rhs, y, x, doneFlag);
		}
	}
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// B's values from A's present values, the structural checks of the exact kind, and the factor
template <typename T>
int mcNumeric(smm_hip_precond* M, bool refreshB, hipStream_t s) {
	smm_precond_mc* C = M->mc;
	int info[2] = {0, 0};
	SMM_TRY(precondRowCheck<T>(M->a, C->base == SMM_PRECOND_SGS, info, s));
	if (info[0]) {
		setError("preconditioner: empty row, missing diagonal or |d|<1e-5");
		return SMM_HIP_ERR_PRECOND;
	}
	if (refreshB) {
		SMM_TRY(csrPermuteRefresh(C->B, M->a, M->dtype, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	if (C->base == SMM_PRECOND_SGS) return SMM_HIP_OK;
	const size_t nnz = static_cast<size_t>(C->B->nnz);
	if (!M->d_values) SMM_TRY(devAlloc(&M->d_values, std::max<size_t>(1, nnz) * sizeof(T)));
	M->n_values = nnz;
	int herr = 0;
	SMM_TRY(factorByRanges<T>(C->B, C->base, C->bounds, static_cast<T*>(M->d_values), &herr, s));
	if (herr && C->base == SMM_PRECOND_ILU0) {
		setError("ilu0: zero / missing pivot (reordering would be needed, ref:1741-1746)");
		return SMM_HIP_ERR_PRECOND;
	}
	if (herr) {
		setError(herr & 1 ? "ic0: matrix is not symmetric positive definite on its pattern (ref:1871-1878)" : "ic0: the pattern of the matrix is not symmetric");
		return SMM_HIP_ERR_PRECOND;
	}
	return SMM_HIP_OK;
}

// colors: the caller's colouring on the HOST, or null for the library's own
template <typename T>
int mcCreateTyped(const smm_hip_csr* a, const int* colors, smm_hip_precond* M) {
	hipStream_t s = libStream();
	SMM_HIP_TRY(hipDeviceSynchronize());  // the matrix may still be being written on a caller's stream
	smm_precond_mc* C = M->mc;
	const int n = a->rows;
	if (a->firstActiveStart != 0 && n > 0) {  // ref:1666-1670, 1737-1739
		setError("preconditioner: matrix has leading empty rows (firstActiveStart != 0)");
		return SMM_HIP_ERR_PRECOND;
	}
	{
		int info[2] = {0, 0};
		SMM_TRY(precondRowCheck<T>(a, C->base == SMM_PRECOND_SGS, info, s));
		if (info[0]) {
			setError("preconditioner: empty row, missing diagonal or |d|<1e-5");
			return SMM_HIP_ERR_PRECOND;
		}
	}
	const size_t n1 = static_cast<size_t>(std::max(1, n));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&C->d_colors), n1 * sizeof(int)));
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&C->d_perm), n1 * sizeof(int)));
	SMM_TRY(devAlloc(&C->d_y, n1 * sizeof(T)));
	if (colors && n > 0) {
		SMM_TRY(hostToDev(C->d_colors, colors, static_cast<size_t>(n) * sizeof(int), s));
		DevBuf<int> dinfo;
		SMM_TRY(dinfo.alloc(2));
		SMM_HIP_TRY(hipMemsetAsync(dinfo, 0, 2 * sizeof(int), s));
		mcCheckColorsKernel<<<gridOf(n), MTPB, 0, s>>>(n, a->d_start, a->d_positions, C->d_colors, dinfo);
		SMM_HIP_TRY(hipGetLastError());
		int info[2] = {0, 0};
		SMM_HIP_TRY(hipMemcpyAsync(info, dinfo, sizeof(info), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
		if (info[0]) {
			setError("precond_create_multicolor: not a colouring (a colour outside [0, rows), or a stored entry joins two rows of one colour)");
			return SMM_HIP_ERR_INVALID;
		}
		C->ncolors = info[1] + 1;
	} else {
		SMM_TRY(csrColor(a, s, C->d_colors, &C->ncolors));
	}
	// perm[] = the rows sorted by colour, stably (the original index ascends inside a colour); the bounds of the colours in that order
	C->bounds.assign(static_cast<size_t>(C->ncolors) + 1, 0);
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&C->d_bounds), C->bounds.size() * sizeof(int)));
	if (n > 0) {
		DevBuf<int> rowsIn, sorted;
		SMM_TRY(rowsIn.alloc(n));
		SMM_TRY(sorted.alloc(n));
		mcIotaKernel<<<gridOf(n), MTPB, 0, s>>>(n, rowsIn);
		int bits = 1;
		while (bits < 31 && (1ll << bits) < C->ncolors) ++bits;
		size_t tempBytes = 0;
		SMM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tempBytes, C->d_colors, sorted.p, rowsIn.p, C->d_perm, static_cast<size_t>(n), 0, bits, s));
		DevBuf<char> temp;
		SMM_TRY(temp.alloc(tempBytes ? tempBytes : 1));
		SMM_HIP_TRY(rocprim::radix_sort_pairs(temp.p, tempBytes, C->d_colors, sorted.p, rowsIn.p, C->d_perm, static_cast<size_t>(n), 0, bits, s));
		mcBoundsKernel<<<gridOf(C->ncolors + 1LL), MTPB, 0, s>>>(n, C->ncolors, sorted, C->d_bounds);
		SMM_HIP_TRY(hipGetLastError());
		SMM_HIP_TRY(hipMemcpyAsync(C->bounds.data(), C->d_bounds, C->bounds.size() * sizeof(int), hipMemcpyDeviceToHost, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
	} else {
		SMM_HIP_TRY(hipMemsetAsync(C->d_bounds, 0, C->bounds.size() * sizeof(int), s));
	}
	planColorGroups(C);
	SMM_TRY(csrPermuteCreate(a, C->d_perm, s, &C->B));
	SMM_TRY(mcNumeric<T>(M, false, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

const smm_precond_mc* mcOf(const smm_hip_precond* M, const char* who) {
	if (!M || !isMulticolorKind(M->kind) || !M->mc || !M->mc->B) {
		setError("%s: not a multicolour preconditioner", who);
		return nullptr;
	}
	return M->mc;
}

}  // namespace

template <typename T>
int mcApplyDev(const smm_hip_precond* M, const T* rhs, T* x, const int* doneFlag, hipStream_t s) {
	const smm_precond_mc* C = M->mc;
	if (!C || !C->B) {
		setError("precond_apply: the multicolour preconditioner was not set up");
		return SMM_HIP_ERR_INVALID;
	}
	const T* bVals = static_cast<const T*>(C->B->d_values);
	const T* fVals = static_cast<const T*>(M->d_values);
	switch (C->base) {
	case SMM_PRECOND_SGS: return runSweeps<T, SGS_LO, SGS_UP>(C, bVals, rhs, x, doneFlag, s);
	case SMM_PRECOND_ILU0: return runSweeps<T, ILU_LO, ILU_UP>(C, fVals, rhs, x, doneFlag, s);
	default: return runSweeps<T, IC_LO, IC_UP>(C, fVals, rhs, x, doneFlag, s);
	}
}
template int mcApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int mcApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void mcDestroy(smm_precond_mc* C) {
	if (!C) return;
	smm_hip_csr_destroy(C->B);
	devFree(C->d_colors);
	devFree(C->d_perm);
	devFree(C->d_bounds);
	devFree(C->d_y);
	delete C;
}

void mcLevels(const smm_precond_mc* C, int* lo, int* up) {
	if (lo) *lo = C->ncolors;
	if (up) *up = C->ncolors;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_precond_create_multicolor(const smm_hip_csr* a, int base_kind, const int* colors, size_t count, smm_hip_precond** out) {
	if (!a || !out) {
		setError("precond_create_multicolor: null argument");
		return SMM_HIP_ERR_INVALID;
	}
	*out = nullptr;
	if (base_kind != SMM_PRECOND_SGS && base_kind != SMM_PRECOND_ILU0 && base_kind != SMM_PRECOND_IC0) {
		setError("precond_create_multicolor: base_kind must be SMM_PRECOND_SGS, _ILU0 or _IC0");
		return SMM_HIP_ERR_INVALID;
	}
	if (a->rows != a->cols) {
		setError("preconditioner needs a square matrix");
		return SMM_HIP_ERR_INVALID;
	}
	if (colors && count != static_cast<size_t>(a->rows)) {
		setError("precond_create_multicolor: %zu colours for %d rows", count, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	SMM_TRY(ensureCsrReady(a, nullptr, false));
	auto* M = new smm_hip_precond();
	M->kind = base_kind == SMM_PRECOND_SGS ? SMM_PRECOND_MULTICOLOR_SGS : base_kind == SMM_PRECOND_ILU0 ? SMM_PRECOND_MULTICOLOR_ILU0 : SMM_PRECOND_MULTICOLOR_IC0;
	M->dtype = a->dtype;
	M->a = a;
	M->mc = new smm_precond_mc();
	M->mc->base = base_kind;
	const int st = a->dtype == SMM_DTYPE_F32 ? mcCreateTyped<float>(a, colors, M) : mcCreateTyped<double>(a, colors, M);
	if (st != SMM_HIP_OK) {
		smm_hip_precond_destroy(M);
		return st;
	}
	*out = M;
	return SMM_HIP_OK;
}

int smm_hip_precond_multicolor_refresh(smm_hip_precond* M) {
	if (!mcOf(M, "precond_multicolor_refresh")) return SMM_HIP_ERR_INVALID;
	SMM_TRY(ensureInit());
	SMM_HIP_TRY(hipDeviceSynchronize());
	hipStream_t s = libStream();
	const int st = M->dtype == SMM_DTYPE_F32 ? mcNumeric<float>(M, true, s) : mcNumeric<double>(M, true, s);
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return st;
}

int smm_hip_precond_multicolor_info(const smm_hip_precond* M, int* ncolors, int* bounds, size_t count) {
	const smm_precond_mc* C = mcOf(M, "precond_multicolor_info");
	if (!C) return SMM_HIP_ERR_INVALID;
	if (ncolors) *ncolors = C->ncolors;
	if (bounds) {
		if (count > C->bounds.size()) {
			setError("precond_multicolor_info: there are %zu bounds", C->bounds.size());
			return SMM_HIP_ERR_INVALID;
		}
		std::copy(C->bounds.begin(), C->bounds.begin() + static_cast<long>(count), bounds);
	}
	return SMM_HIP_OK;
}

int smm_hip_precond_multicolor_perm(const smm_hip_precond* M, int* perm, size_t count) {
	const smm_precond_mc* C = mcOf(M, "precond_multicolor_perm");
	if (!C) return SMM_HIP_ERR_INVALID;
	if (!perm || count > static_cast<size_t>(M->a->rows)) {
		setError("precond_multicolor_perm: null pointer, or more than %d entries asked", M->a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	if (count) SMM_HIP_TRY(hipMemcpyAsync(perm, C->d_perm, count * sizeof(int), hipMemcpyDeviceToHost, s));
	SMM_HIP_TRY(hipStreamSynchronize(s));
	return SMM_HIP_OK;
}

int smm_hip_precond_multicolor_matrix(const smm_hip_precond* M, smm_hip_csr** b) {
	const smm_precond_mc* C = mcOf(M, "precond_multicolor_matrix");
	if (!C) return SMM_HIP_ERR_INVALID;
	if (!b) {
		setError("precond_multicolor_matrix: null pointer");
		return SMM_HIP_ERR_INVALID;
	}
	*b = C->B;
	return SMM_HIP_OK;
}

}  // extern "C"
