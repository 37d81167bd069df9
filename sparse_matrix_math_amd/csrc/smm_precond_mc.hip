// smm_precond_mc.hip -- the MULTICOLOUR forms of SGS / ILU(0) / IC(0): colour the adjacency graph of A (smm_color.hip), number the rows
// colour by colour (perm[] = a stable sort of the rows by colour), B = P A Pᵀ, and run the exact kind on B:
//     M^-1 r = Pᵀ sweeps_B(P r).
// Rows of one colour do not reference each other, so a colour is a dependency level of BOTH sweeps and the rows of a level are a
// contiguous range of B: a sweep is `ncolors` passes shaped like an SpMV over B's rows, one lane per row, instead of the hundreds of
// levels the natural order has on a grid.
// The sweeps are smm_trisweep.h's level sweeps -- the exact kinds' row walker, level / chain kernels and launch plan -- with the rows of a
// level taken as the range itself and the PermutedIO policy: the lower sweep reads rhs[perm[row]], the upper sweep's write also stores
// x[perm[row]], no gather or scatter pass over a vector; in between the sweeps work on y[] (permuted numbering), owned by the handle.  The
// upper sweep walks the lower sweep's launch groups backwards.  So the result is bit for bit the sequential sweep on B
// (tests/multicolor_restatement.py).  (A single-launch form with a grid barrier between the colours was not built: see DESIGN.md 3.16.)
// This unit keeps what is its own: the intake and check of a colouring, B, the refresh, the query entry points.
// The handle is a SNAPSHOT (B is a copy); smm_hip_precond_multicolor_refresh redoes B's values and the factor on the kept colouring.
#include <algorithm>
#include <memory>

#include "smm_trisweep.h"

struct smm_precond_mc {
	int base = SMM_PRECOND_SGS;  // the exact kind run on B
	int ncolors = 0;
	smm_hip_csr* B = nullptr;    // P A Pᵀ, owned
	int* d_colors = nullptr;     // colour of every row of A
	int* d_perm = nullptr;       // new row i is A's row d_perm[i]
	void* d_y = nullptr;         // the vector both sweeps work on (permuted numbering)
	smm::LevelSchedule colours;  // the ncolors + 1 row bounds of B and the launch groups of the LOWER sweep (d_order stays null: a colour's rows are a range)
};

namespace smm {
namespace {

constexpr int MTPB = SWEEP_TPB;

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

// B's values from A's present values, the structural checks of the exact kind, and the factor
template <typename T>
int mcNumeric(smm_hip_precond* M, bool refreshB, hipStream_t s) {
	smm_precond_mc* C = M->mc;
	SMM_TRY(precondRowCheck<T>(M->a, C->base == SMM_PRECOND_SGS, nullptr, s));
	if (refreshB) {
		SMM_TRY(csrPermuteRefresh(C->B, M->a, M->dtype, s));
		SMM_HIP_TRY(hipStreamSynchronize(s));
	}
	if (C->base == SMM_PRECOND_SGS) return SMM_HIP_OK;
	const size_t nnz = static_cast<size_t>(C->B->nnz);
	if (!M->d_values) SMM_TRY(devAlloc(&M->d_values, std::max<size_t>(1, nnz) * sizeof(T)));
	M->n_values = nnz;
	return factorByRanges<T>(C->B, C->base, C->colours, static_cast<T*>(M->d_values), s);
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
	SMM_TRY(precondRowCheck<T>(a, C->base == SMM_PRECOND_SGS, nullptr, s));
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
	SMM_TRY(devAlloc(reinterpret_cast<void**>(&C->colours.d_bounds), (static_cast<size_t>(C->ncolors) + 1) * sizeof(int)));
	SMM_TRY(sortRowsByKey(C->d_colors, n, C->ncolors, s, C->d_perm, C->colours.d_bounds, C->colours.bounds));
	planGroups(C->colours.bounds, C->colours.groups);
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
	const T* vals = static_cast<const T*>(C->base == SMM_PRECOND_SGS ? C->B->d_values : M->d_values);  // SGS sweeps B itself, ILU0 / IC0 their factor
	const PermutedIO<T> io{C->d_perm, rhs, static_cast<T*>(C->d_y), x};
	std::lock_guard<std::mutex> whole(M->enqueueMutex);  // d_y is the handle's: the launches of the two sweeps stay together
	return withSweepModes(C->base, [&](auto lo, auto up) -> int {
		SMM_TRY((runLevelSweep<T, decltype(lo)::value, PermutedIO<T>, false>(C->colours, false, C->B, vals, io, doneFlag, s)));
		return runLevelSweep<T, decltype(up)::value, PermutedIO<T>, false>(C->colours, true, C->B, vals, io, doneFlag, s);
	});
}
template int mcApplyDev<float>(const smm_hip_precond*, const float*, float*, const int*, hipStream_t);
template int mcApplyDev<double>(const smm_hip_precond*, const double*, double*, const int*, hipStream_t);

void mcDestroy(smm_precond_mc* C) {
	if (!C) return;
	smm_hip_csr_destroy(C->B);
	devFree(C->d_colors);
	devFree(C->d_perm);
	C->colours.release();
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
		const std::vector<int>& have = C->colours.bounds;
		if (count > have.size()) {
			setError("precond_multicolor_info: there are %zu bounds", have.size());
			return SMM_HIP_ERR_INVALID;
		}
		std::copy(have.begin(), have.begin() + static_cast<long>(count), bounds);
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
