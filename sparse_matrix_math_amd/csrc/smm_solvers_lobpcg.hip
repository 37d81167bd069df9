// smm_solvers_lobpcg.hip -- LOBPCG (Knyazev 2001), the locally optimal block preconditioned conjugate gradient method: the k algebraically
// largest or smallest eigenpairs of a symmetric matrix from a block of k vectors, with a symmetric positive definite preconditioner.  An
// addition: the reference has no eigensolver.  The definition, line by line, is tests/lobpcg_restatement.py; the contract is in
// include/smm_hip.h.
//
// Two bases, S and AS, are ONE allocation each: column-major, 3k columns, leading dimension rounded up to 64 elements (every column starts
// 16-byte aligned).  Their columns are, in this order,
//   X (k)   the Ritz vectors            AX   their products, carried through every rotation, never recomputed
//   P (np)  the kept directions         AP
//   W (na)  the preconditioned residuals of the na active columns          AW = A W, na SpMVs
// and Z = [P W] is the search block.  The residuals of all k columns are written into the AW columns (free until the SpMVs fill them), the
// preconditioner reads them there and writes W: no vector of the size of a column besides the 6k.
// An iteration, besides the na preconditioner applies and the na SpMVs (column by column: the SpMM of this library is row-interleaved):
//   lobpcgResidual + finish      R_j = AX_j - theta_j X_j and |R_j|^2 for all j: one launch over the block, one to add the partial sums
//   twice:  multiGram            H = X^T Z                                   (H stays on the device)
//           multiBlockAxpy x 2   Z -= X H;  AZ -= AX H
//           multiGram            G = Z^T Z, the symmetric case               -> host
//           multiRotate x 2      Z = Z Y;  AZ = AZ Y                         (SVQB: Y from G's eigenpairs, host)
//   multiGram                    T = S^T AS                                  -> host
//   multiRotate x 2              [X P] = S [C | C_P];  [AX AP] = AS [C | C_P]
// 22 dense launches (every multiGram is two: the tiles and the fixed-order finish) and FOUR host reads: |R|^2, the two G and T.
// The host's part is fp64 for both dtypes: the Rayleigh-Ritz problems by cyclic Jacobi (smm_jacobi.h), at most 24 x 24.
// No floating-point atomics, every sum in a fixed order: two runs of one call give the same bits.
#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "smm_device.h"
#include "smm_internal.h"
#include "smm_jacobi.h"
#include "smm_multiblock.h"
#include "smm_multivec.h"
#include "smm_solver_host.h"
#include "smm_solver_scal.h"

namespace smm {

constexpr int TPB = 256;
constexpr int MAXK = SMM_LOBPCG_MAX_K;
static_assert(3 * MAXK == MB_MAX, "S = [X P W] has 3k columns");

template <typename T>
struct LobpcgState {
	T h[MAXK], coef[MAXK];  // the start block's Gram-Schmidt: the products and their negatives
	T rn2[MAXK];            // |R_j|^2
	int bad;                // a start column without a direction of its own, or with a norm that is not finite
};

template <typename T>
struct LobpcgThetas {
	T v[MAXK];
};

// v = v / d with d = sqrt(v . v) after the two Gram-Schmidt passes and d0 the same before them.  A d or d0 that is not finite, or
// d <= sqrt(eps) d0 (the column lies in the span of those before it to working precision): bad, and every later launch of the start returns.
template <typename T>
__global__ __launch_bounds__(TPB) void lobpcgNormalise(long long n, T* v, const T* __restrict__ parts0, const T* __restrict__ parts1, int nb, LobpcgState<T>* st) {
	__shared__ T red[6];
	if (st->bad) return;
	T a0 = T(0), a1 = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) {
		a0 += parts0[i];
		a1 += parts1[i];
	}
	const T s0 = blockSum256(a0, red);
	const T s1 = blockSum256(a1, red);
	if (threadIdx.x == 0) {
		red[4] = sqrt(s0);
		red[5] = sqrt(s1);
	}
	__syncthreads();
	const T d0 = red[4], d = red[5];
	if (!isfinite(d0) || !isfinite(d) || !(d > sqrt(std::numeric_limits<T>::epsilon()) * d0)) {
		if (blockIdx.x == 0 && threadIdx.x == 0) st->bad = 1;  // (every workgroup comes to the same verdict: none divides)
		return;
	}
	const T* const in[1] = {v};
	T* const out[1] = {v};
	streamMap<T, false, 1, 1>(n, in, out, [&](const T(&e)[1], T(&o)[1]) { o[0] = e[0] / d; });
}

// R_j = AX_j - theta_j X_j (one product, one difference) for column j = blockIdx.y, and this workgroup's share of R_j . R_j
template <typename T>
__global__ __launch_bounds__(TPB) void lobpcgResidual(long long n, const T* X, const T* AX, long long ld, LobpcgThetas<T> theta, T* R, T* __restrict__ parts) {
	__shared__ T red[4];
	const long long off = static_cast<long long>(blockIdx.y) * ld;
	const T th = theta.v[blockIdx.y];
	T acc = T(0);
	const T* const in[2] = {AX + off, X + off};
	T* const out[1] = {R + off};
	streamMap<T, false, 2, 1>(n, in, out, [&](const T(&e)[2], T(&o)[1]) {
		const T r = e[0] - th * e[1];
		o[0] = r;
		acc += r * r;
	});
	const T s = blockSum256(acc, red);
	if (threadIdx.x == 0) parts[static_cast<long long>(blockIdx.y) * NPART + blockIdx.x] = s;
}

// ---- the generalised problem A x = lambda B x ----
template <typename T>
struct LobpcgGenState {
	T h[MAXK], coef[MAXK];  // the start block's B-Gram-Schmidt: the products and their negatives
	T sums[2 * MAXK];       // |R_j|^2, j < k, then |BX_j|^2
	int bad;                // a start column without a direction of its own, or with a B-norm that is not finite or not positive
};

// x = w / d and bx = q / d with d = sqrt(w . q) after the two Gram-Schmidt passes (q = B w) and d0 the same before them: the B-norms.
// A d or d0 that is not finite -- the root of a negative w . q is one -- or !(d > sqrt(eps) d0): bad, as lobpcgNormalise.
template <typename T>
__global__ __launch_bounds__(TPB) void lobpcgGenNormalise(long long n, T* x, T* bx, const T* __restrict__ parts0, const T* __restrict__ parts1, int nb, LobpcgGenState<T>* st) {
	__shared__ T red[6];
	if (st->bad) return;
	T a0 = T(0), a1 = T(0);
	for (int i = threadIdx.x; i < nb; i += TPB) {
		a0 += parts0[i];
		a1 += parts1[i];
	}
	const T s0 = blockSum256(a0, red);
	const T s1 = blockSum256(a1, red);
	if (threadIdx.x == 0) {
		red[4] = sqrt(s0);
		red[5] = sqrt(s1);
	}
	__syncthreads();
	const T d0 = red[4], d = red[5];
	if (!isfinite(d0) || !isfinite(d) || !(d > sqrt(std::numeric_limits<T>::epsilon()) * d0)) {
		if (blockIdx.x == 0 && threadIdx.x == 0) st->bad = 1;  // (every workgroup comes to the same verdict: none divides)
		return;
	}
	const T* const in[2] = {x, bx};
	T* const out[2] = {x, bx};
	streamMap<T, false, 2, 2>(n, in, out, [&](const T(&e)[2], T(&o)[2]) {
		o[0] = e[0] / d;
		o[1] = e[1] / d;
	});
}

// R_j = AX_j - theta_j BX_j (one product, one difference) for column j = blockIdx.y, and this workgroup's shares of R_j . R_j
// (parts[j * NPART + block]) and of BX_j . BX_j (parts[(k + j) * NPART + block], k = gridDim.y): one pass over the two blocks, both sums
template <typename T>
__global__ __launch_bounds__(TPB) void lobpcgGenResidual(long long n, const T* AX, const T* BX, long long ld, LobpcgThetas<T> theta, T* R, T* __restrict__ parts) {
	__shared__ T red[4];
	const long long off = static_cast<long long>(blockIdx.y) * ld;
	const T th = theta.v[blockIdx.y];
	T rr = T(0), bb = T(0);
	const T* const in[2] = {AX + off, BX + off};
	T* const out[1] = {R + off};
	streamMap<T, false, 2, 1>(n, in, out, [&](const T(&e)[2], T(&o)[1]) {
		const T r = e[0] - th * e[1];
		o[0] = r;
		rr += r * r;
		bb += e[1] * e[1];
	});
	const T s = blockSum256(rr, red);
	const T t = blockSum256(bb, red);
	if (threadIdx.x == 0) {
		parts[static_cast<long long>(blockIdx.y) * NPART + blockIdx.x] = s;
		parts[static_cast<long long>(gridDim.y + blockIdx.y) * NPART + blockIdx.x] = t;
	}
}

// The kinds taken: those ConjugateGradient takes, and JACOBI and SGS -- symmetric positive definite for a positive definite matrix as well;
// ConjugateGradient's fused loop has no path for them, here every kind goes through precondApplyDev.
static bool lobpcgKindTaken(int kind) { return precondKindTaken(kind, SOLVER_CG) || kind == SMM_PRECOND_JACOBI || kind == SMM_PRECOND_SGS; }

// The entry check of the preconditioner, the rule of smm_hip_minres_*: M must be symmetric positive definite, so it is asked to fit `a`,
// not to be created for it -- a shifted L - sigma I takes the preconditioner of L.
template <typename T>
static int lobpcgPrecondCheck(const smm_hip_precond* M, const smm_hip_csr* a) {
	if (!M) return SMM_HIP_OK;
	if (M->dtype != dtypeOf<T>()) {
		setError("lobpcg: the preconditioner holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (!M->a || M->a->rows != a->rows) {
		setError("lobpcg: the preconditioner was created for a matrix of %d rows, this one has %d", M->a ? M->a->rows : 0, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	if (!lobpcgKindTaken(M->kind)) {
		std::string names;
		for (int kind = SMM_PRECOND_NONE + 1; kind < N_PRECOND_KINDS; ++kind) {
			if (lobpcgKindTaken(kind)) names += std::string(names.empty() ? "" : " / ") + PRECOND_KINDS[kind].name;
		}
		const char* name = M->kind >= 0 && M->kind < N_PRECOND_KINDS ? PRECOND_KINDS[M->kind].name : "unknown";
		setError("lobpcg: the preconditioner must be symmetric positive definite (%s, created for a positive definite matrix of the same size), not %s", names.c_str(),
		         name);
		return SMM_HIP_ERR_INVALID;
	}
	if (isJsweepKind(M->kind) && !jsweepSymmetric(M)) {
		setError("lobpcg: a %s preconditioner is symmetric only with as many lower steps as upper ones (smm_hip_precond_jsweep_set_sweeps)", PRECOND_KINDS[M->kind].name);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int lobpcgCheck(const smm_hip_csr* a, int k, int which, int maxIterations, const smm_hip_precond* M, const T* X0, long long ldx0, const T* eigenvalues,
                       const T* eigenvectors, long long ldx) {
	SMM_TRY(solverCheck<T>("lobpcg", a));
	if (k < 0 || k > MAXK || (which != SMM_EIGSH_LARGEST && which != SMM_EIGSH_SMALLEST) || maxIterations < 0) {
		setError("lobpcg: bad arguments (0 <= k <= %d, which SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST, maxIterations >= 0)", MAXK);
		return SMM_HIP_ERR_INVALID;
	}
	SMM_TRY(lobpcgPrecondCheck<T>(M, a));
	if (a->rows == 0 || k == 0) return SMM_HIP_OK;
	if (3 * k > a->rows) {
		setError("lobpcg: the basis of 3k = %d columns exceeds the %d rows (a matrix this small is dense work, or smm_hip_eigsh_*'s)", 3 * k, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	if (!eigenvalues) {
		setError("lobpcg: null eigenvalues");
		return SMM_HIP_ERR_INVALID;
	}
	if (eigenvectors && ldx < a->rows) {
		setError("lobpcg: ldx = %lld is less than the %d rows", ldx, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	if (X0 && ldx0 < a->rows) {
		setError("lobpcg: ldx0 = %lld is less than the %d rows", ldx0, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

struct LobpcgOut {
	int status = SMM_SOLVER_SUCCESS, nconv = 0, iterations = 0, matvecs = 0, applies = 0, bmatvecs = 0;
	bool wrote = false;  // the eigenpairs were written to the outputs
};

// y: rows x cols, column-major with leading dimension `rows`, as multiRotate's operand: multiRotatePad(rows) x cols in T, zero rows below.
// `h` is the caller's staging array.
template <typename T>
static int lobpcgStage(int rows, int cols, const std::vector<double>& y, std::vector<T>& h, DevBuf<T>& dY, hipStream_t s) {
	const int MP = multiRotatePad(rows);
	h.assign(static_cast<size_t>(MP) * cols, T(0));
	for (int c = 0; c < cols; ++c) {
		for (int r = 0; r < rows; ++r) h[static_cast<size_t>(c) * MP + r] = static_cast<T>(y[static_cast<size_t>(c) * rows + r]);
	}
	return hostToDev(dY, h.data(), sizeof(T) * h.size(), s);
}

// g (m x m, column-major, in T, from the device) as the row-major fp64 operand of jacobiEigen, symmetrised; false: an entry that is not finite
template <typename T>
static bool lobpcgSymmetrise(int m, const std::vector<T>& g, std::vector<double>& t) {
	t.assign(static_cast<size_t>(m) * m, 0.0);
	for (int i = 0; i < m; ++i) {
		for (int j = 0; j < m; ++j) {
			const double v = 0.5 * (static_cast<double>(g[i + j * m]) + static_cast<double>(g[j + i * m]));
			if (!std::isfinite(v)) return false;
			t[i * m + j] = v;
		}
	}
	return true;
}

// SVQB on the symmetrised Gram matrix t (nz x nz): d = sqrt(diag t);  G' = t / (d d^T) = Q diag(w) Q^T on the columns with d > 0;
// Y = diag(1 / d) Q[:, kept] diag(w_kept^-1/2), the largest w first, into y (nz x *keep, column-major).  false: the eigensolver failed.
static bool lobpcgSvqb(int nz, const std::vector<double>& t, double eps, std::vector<double>& w, std::vector<double>& q, std::vector<double>& y, int* keep) {
	std::vector<int> live;
	std::vector<double> d(nz);
	for (int i = 0; i < nz; ++i) {
		d[i] = std::sqrt(t[i * nz + i]);
		if (d[i] > 0) live.push_back(i);
	}
	const int nl = static_cast<int>(live.size());
	*keep = 0;
	if (nl == 0) return true;
	std::vector<double> gs(static_cast<size_t>(nl) * nl);
	for (int i = 0; i < nl; ++i) {
		for (int j = 0; j < nl; ++j) gs[i * nl + j] = t[live[i] * nz + live[j]] / (d[live[i]] * d[live[j]]);
	}
	if (!jacobiEigen(nl, gs, w, q)) return false;
	const double wmax = w[nl - 1];  // ascending
	while (*keep < nl && w[nl - 1 - *keep] > nl * eps * wmax) ++*keep;
	y.assign(static_cast<size_t>(nz) * *keep, 0.0);
	for (int cc = 0; cc < *keep; ++cc) {
		const int src = nl - 1 - cc;
		for (int i = 0; i < nl; ++i) y[static_cast<size_t>(cc) * nz + live[i]] = q[i * nl + src] / std::sqrt(w[src]) / d[live[i]];
	}
	return true;
}

template <typename T>
static int lobpcgDev(const smm_hip_csr* a, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* X0, long long ldx0, unsigned long long seed,
                     T* d_vals, T* d_X, long long ldx, hipStream_t s, T* residuals, LobpcgOut* out) {
	SMM_TRY(lobpcgCheck<T>(a, k, which, maxIterations, M, X0, ldx0, d_vals, d_X, ldx));
	const int n = a->rows;
	if (n == 0 || k == 0) return SMM_HIP_OK;
	const double eps = static_cast<double>(std::numeric_limits<T>::epsilon());
	const double bound = tol > T(0) ? static_cast<double>(tol) : eps;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	const long long ld = std::max<long long>(64, (static_cast<long long>(n) + 63) / 64 * 64);
	DevBuf<T> S, AS, gparts, parts, parts0, parts1, dG, dH, dY;
	DevBuf<LobpcgState<T>> st;
	SyncOnExit drain{s};
	SMM_TRY(S.alloc(static_cast<size_t>(ld) * 3 * k));
	SMM_TRY(AS.alloc(static_cast<size_t>(ld) * 3 * k));
	SMM_TRY(gparts.alloc(static_cast<size_t>(MB_MAX) * MB_MAX * MG_NPART));
	SMM_TRY(parts.alloc(static_cast<size_t>(MAXK) * NPART));
	SMM_TRY(parts0.alloc(NPART));
	SMM_TRY(parts1.alloc(NPART));
	SMM_TRY(dG.alloc(static_cast<size_t>(MB_MAX) * MB_MAX));
	SMM_TRY(dH.alloc(static_cast<size_t>(MB_MAX) * MB_MAX));
	SMM_TRY(dY.alloc(static_cast<size_t>(32) * MB_MAX));
	SMM_TRY(st.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(LobpcgState<T>), s));
	LobpcgState<T>* sp = st.p;
	const int gmv = gridMV(n, sizeof(T));
	const int g = solverGrid(n);
	auto scol = [&](int j) { return S.p + static_cast<long long>(j) * ld; };
	auto acol = [&](int j) { return AS.p + static_cast<long long>(j) * ld; };
	std::vector<T> hG, hY;
	std::vector<double> t, theta, c, y, w, q;
	LoopWatch none;

	// the start block: the caller's, or the hash columns; classical Gram-Schmidt twice and a division by the norm, column by column
	if (!X0) hashFillKernel<T><<<dim3(g, k), TPB, 0, s>>>(n, seed, 0, S.p, ld);
	for (int j = 0; j < k; ++j) {
		T* xj = scol(j);
		multiAxpyKernel<T, true><<<gmv, TPB, 0, s>>>(n, 0, nullptr, S.p, ld, sp->coef, X0 ? X0 + j * ldx0 : xj, xj, parts0, &sp->bad);  // (no column: a copy and x . x)
		if (j > 0) orthogonaliseTwice<T>(S.p, ld, n, gmv, j, xj, parts, parts1, sp->h, sp->h, sp->coef, &sp->bad, s);
		lobpcgNormalise<T><<<g, TPB, 0, s>>>(n, xj, parts0, j > 0 ? parts1.p : parts0.p, gmv, sp);
	}
	LobpcgState<T> h;
	SMM_TRY(loopFinish(none, &h, sp, sizeof(h), s));
	if (h.bad) {
		out->status = SMM_SOLVER_DIVERGED;
		drain.armed = false;
		return SMM_HIP_OK;
	}
	for (int j = 0; j < k; ++j) SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, scol(j), acol(j), 0, nullptr, nullptr, nullptr, s));
	out->matvecs = k;

	// the Rayleigh-Ritz step on the m leading columns of S and AS: theta (all m, in the order of `which`) and the eigenvectors, column i of
	// `c` (column-major, m x m) that of theta[i].  false: a value that is not finite.
	auto ritz = [&](int m, bool* ok) -> int {
		multiGramLaunch<T>(n, m, m, S.p, ld, AS.p, ld, gparts.p, dG.p, m, s);
		hG.resize(static_cast<size_t>(m) * m);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(devToHost(hG.data(), dG.p, sizeof(T) * hG.size(), s));
		*ok = lobpcgSymmetrise<T>(m, hG, t) && jacobiEigen(m, t, w, q);
		if (!*ok) return SMM_HIP_OK;
		theta.resize(m);
		c.assign(static_cast<size_t>(m) * m, 0.0);
		for (int i = 0; i < m; ++i) {
			const int src = which == SMM_EIGSH_LARGEST ? m - 1 - i : i;
			theta[i] = w[src];
			for (int r = 0; r < m; ++r) c[static_cast<size_t>(i) * m + r] = q[r * m + src];
		}
		return SMM_HIP_OK;
	};
	auto rotateBoth = [&](int from, int m, int cols, const std::vector<double>& yy) -> int {
		SMM_TRY(lobpcgStage<T>(m, cols, yy, hY, dY, s));
		multiRotateLaunch<T>(n, m, cols, scol(from), ld, dY.p, s);
		multiRotateLaunch<T>(n, m, cols, acol(from), ld, dY.p, s);
		return SMM_HIP_OK;
	};

	bool ok = true;
	SMM_TRY(ritz(k, &ok));
	if (!ok) {
		out->status = SMM_SOLVER_DIVERGED;
		drain.armed = false;
		return SMM_HIP_OK;
	}
	SMM_TRY(rotateBoth(0, k, k, c));

	int np = 0;  // kept directions
	double scale = 0;
	std::vector<T> vals(k), rn(k);
	std::vector<int> active;
	int status = SMM_SOLVER_SUCCESS;
	for (int it = 0;; ++it) {
		LobpcgThetas<T> th;
		for (int j = 0; j < MAXK; ++j) th.v[j] = j < k ? static_cast<T>(theta[j]) : T(0);
		T* R = acol(k + np);  // the AW columns: free until the SpMVs below fill them
		lobpcgResidual<T><<<dim3(g, k), TPB, 0, s>>>(n, S.p, AS.p, ld, th, R, parts);
		multiDotFinish<T><<<k, TPB, 0, s>>>(parts, g, sp->rn2, nullptr, nullptr);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(devToHost(rn.data(), sp->rn2, sizeof(T) * k, s));
		bool finite = true;
		for (int j = 0; j < k; ++j) {
			rn[j] = std::sqrt(rn[j]);
			finite = finite && std::isfinite(rn[j]);
		}
		for (double v : theta) {
			finite = finite && std::isfinite(v);
			scale = std::max(scale, std::fabs(v));
		}
		if (!finite) {
			status = SMM_SOLVER_DIVERGED;
			break;
		}
		active.clear();
		for (int j = 0; j < k; ++j) {
			if (!(static_cast<double>(rn[j]) <= bound * scale)) active.push_back(j);
		}
		for (int j = 0; j < k; ++j) vals[j] = th.v[j];
		out->nconv = k - static_cast<int>(active.size());
		out->iterations = it;
		if (active.empty()) break;
		if (it == maxIterations) {
			status = SMM_SOLVER_MAX_ITERATIONS_REACHED;
			break;
		}
		const int na = static_cast<int>(active.size());
		for (int i = 0; i < na; ++i) {
			const T* rj = R + static_cast<long long>(active[i]) * ld;
			if (M) SMM_TRY(precondApplyDev<T>(M, rj, scol(k + np + i), nullptr, s));
			else SMM_TRY(launchCopy2<T>(n, rj, scol(k + np + i), nullptr, s));
		}
		for (int i = 0; i < na; ++i) SMM_TRY(launchSpmv<T>(a, SMM_OP_ASSIGN, nullptr, scol(k + np + i), acol(k + np + i), 0, nullptr, nullptr, nullptr, s));
		out->matvecs += na;
		out->applies += M ? na : 0;

		int nz = np + na;
		for (int pass = 0; pass < 2 && nz > 0; ++pass) {
			multiGramLaunch<T>(n, k, nz, S.p, ld, scol(k), ld, gparts.p, dH.p, k, s);
			multiBlockAxpyLaunch<T>(n, k, nz, S.p, ld, dH.p, k, scol(k), ld, s);
			multiBlockAxpyLaunch<T>(n, k, nz, AS.p, ld, dH.p, k, acol(k), ld, s);
			multiGramLaunch<T>(n, nz, nz, scol(k), ld, scol(k), ld, gparts.p, dG.p, nz, s);
			hG.resize(static_cast<size_t>(nz) * nz);
			SMM_HIP_TRY(hipGetLastError());
			SMM_TRY(devToHost(hG.data(), dG.p, sizeof(T) * hG.size(), s));
			if (!lobpcgSymmetrise<T>(nz, hG, t)) {
				status = SMM_SOLVER_DIVERGED;
				break;
			}
			int keep = 0;
			if (!lobpcgSvqb(nz, t, eps, w, q, y, &keep)) {
				status = SMM_SOLVER_DIVERGED;
				break;
			}
			if (keep > 0) SMM_TRY(rotateBoth(k, nz, keep, y));
			nz = keep;
		}
		if (status != SMM_SOLVER_SUCCESS) break;
		const int m = k + nz;
		SMM_TRY(ritz(m, &ok));
		if (!ok) {
			status = SMM_SOLVER_DIVERGED;
			break;
		}
		// [X P] = S [C | C_P]: C the k wanted eigenvectors, C_P the part of the first npNew active ones that lies in Z (zero in X's rows)
		const int npNew = std::min(na, nz);
		y.assign(static_cast<size_t>(m) * (k + npNew), 0.0);
		std::copy(c.begin(), c.begin() + static_cast<size_t>(m) * k, y.begin());
		for (int i = 0; i < npNew; ++i) {
			for (int r = k; r < m; ++r) y[static_cast<size_t>(k + i) * m + r] = c[static_cast<size_t>(active[i]) * m + r];
		}
		SMM_TRY(rotateBoth(0, m, k + npNew, y));
		np = npNew;
	}
	out->status = status;
	if (status != SMM_SOLVER_DIVERGED) {
		SMM_TRY(hostToDev(d_vals, vals.data(), sizeof(T) * k, s));
		for (int j = 0; d_X && j < k; ++j) SMM_TRY(launchCopy2<T>(n, scol(j), d_X + static_cast<long long>(j) * ldx, nullptr, s));
		if (residuals) std::copy(rn.begin(), rn.end(), residuals);
		out->wrote = true;
	}
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	return M ? precondTakeError(M, s) : SMM_HIP_OK;
}

template <typename T>
static void lobpcgReport(const LobpcgOut& o, int* nconv, int* iterations, int* matvecs, int* applies, int* status) {
	if (nconv) *nconv = o.nconv;
	if (iterations) *iterations = o.iterations;
	if (matvecs) *matvecs = o.matvecs;
	if (applies) *applies = o.applies;
	if (status) *status = o.status;
}

template <typename T>
static int lobpcgDevEntry(const smm_hip_csr* a, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* d_X0, long long ldx0,
                          unsigned long long seed, T* d_vals, T* d_X, long long ldx, smm_hip_stream stream, T* residuals, int* nconv, int* iterations, int* matvecs,
                          int* applies, int* status) {
	SMM_TRY(lobpcgCheck<T>(a, k, which, maxIterations, M, d_X0, ldx0, d_vals, d_X, ldx));
	LobpcgOut o;
	if (a->rows > 0 && k > 0) {
		SMM_TRY(ensureInit());
		SMM_TRY(lobpcgDev<T>(a, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_vals, d_X, ldx, pickStream(stream), residuals, &o));
	}
	lobpcgReport<T>(o, nconv, iterations, matvecs, applies, status);
	return SMM_HIP_OK;
}

// host arrays: X0 (may be null) column-major with ldx0, eigenvalues[k], eigenvectors (may be null) column-major with ldx
template <typename T>
static int lobpcgHost(const smm_hip_csr* a, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* X0, long long ldx0, unsigned long long seed,
                      T* eigenvalues, T* eigenvectors, long long ldx, T* residuals, int* nconv, int* iterations, int* matvecs, int* applies, int* status) {
	SMM_TRY(lobpcgCheck<T>(a, k, which, maxIterations, M, X0, ldx0, eigenvalues, eigenvectors, ldx));
	LobpcgOut o;
	if (a->rows == 0 || k == 0) {
		lobpcgReport<T>(o, nconv, iterations, matvecs, applies, status);
		return SMM_HIP_OK;
	}
	SMM_TRY(ensureInit());
	hipStream_t s = libStream();
	const size_t n = static_cast<size_t>(a->rows);
	DevBuf<T> dX0, dvals, dX;
	SyncOnExit drain{s};
	if (X0) {
		SMM_TRY(dX0.alloc(n * k));
		for (int j = 0; j < k; ++j) SMM_TRY(hostToDev(dX0.p + j * n, X0 + static_cast<long long>(j) * ldx0, sizeof(T) * n, s));
	}
	SMM_TRY(dvals.alloc(k));
	if (eigenvectors) SMM_TRY(dX.alloc(n * k));
	SMM_TRY(lobpcgDev<T>(a, k, which, maxIterations, tol, M, X0 ? dX0.p : nullptr, static_cast<long long>(n), seed, dvals.p, eigenvectors ? dX.p : nullptr,
	                     static_cast<long long>(n), s, residuals, &o));
	if (o.wrote) {
		SMM_TRY(devToHost(eigenvalues, dvals, sizeof(T) * k, s));
		for (int j = 0; eigenvectors && j < k; ++j) SMM_TRY(devToHost(eigenvectors + static_cast<long long>(j) * ldx, dX.p + j * n, sizeof(T) * n, s));
	}
	drain.armed = false;
	lobpcgReport<T>(o, nconv, iterations, matvecs, applies, status);
	return SMM_HIP_OK;
}

// what the generalised entries refuse beyond lobpcgCheck: B must be a matrix of a's dtype and size
template <typename T>
static int lobpcgGenCheck(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, const smm_hip_precond* M, const T* X0, long long ldx0,
                          const T* eigenvalues, const T* eigenvectors, long long ldx) {
	SMM_TRY(lobpcgCheck<T>(a, k, which, maxIterations, M, X0, ldx0, eigenvalues, eigenvectors, ldx));
	if (b->dtype != dtypeOf<T>()) {
		setError("lobpcg: B holds values of the other dtype");
		return SMM_HIP_ERR_INVALID;
	}
	if (b->rows != b->cols) {
		setError("lobpcg: B must be square");
		return SMM_HIP_ERR_INVALID;
	}
	if (b->rows != a->rows) {
		setError("lobpcg: B has %d rows, the matrix has %d", b->rows, a->rows);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

// The loop of lobpcgDev for A x = lambda B x: BS = [BX BP BW] is a third basis beside S and AS, carried through every rotation; the
// orthonormality is B's (X^T BX = I), so the small problem stays the standard one on T = S^T AS.  An iteration, besides the na
// preconditioner applies and the 2 na SpMVs:
//   lobpcgGenResidual + finish   R_j = AX_j - theta_j BX_j, |R_j|^2 and |BX_j|^2 for all j
//   twice:  multiGram            H = BX^T Z
//           multiBlockAxpyBases  Z -= X H;  AZ -= AX H;  BZ -= BX H      (one launch over the three bases)
//           multiGram            G = Z^T BZ                              -> host
//           multiRotateBases     Z = Z Y;  AZ = AZ Y;  BZ = BZ Y         (one launch)
//   multiGram                    T = S^T AS                              -> host
//   multiRotateBases             [X P], [AX AP], [BX BP] by [C | C_P]    (one launch)
// 17 dense launches where three launches per basis would make 25, and the same FOUR host reads.
template <typename T>
static int lobpcgGenDev(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* X0, long long ldx0,
                        unsigned long long seed, T* d_vals, T* d_X, long long ldx, hipStream_t s, T* residuals, LobpcgOut* out) {
	SMM_TRY(lobpcgGenCheck<T>(a, b, k, which, maxIterations, M, X0, ldx0, d_vals, d_X, ldx));
	const int n = a->rows;
	if (n == 0 || k == 0) return SMM_HIP_OK;
	const double eps = static_cast<double>(std::numeric_limits<T>::epsilon());
	const double bound = tol > T(0) ? static_cast<double>(tol) : eps;
	SMM_TRY(ensureCsrReady(a, s, true));
	SMM_TRY(adoptPatternForSolver(a, maxIterations, s));
	if (b != a) {
		SMM_TRY(ensureCsrReady(b, s, true));
		SMM_TRY(adoptPatternForSolver(b, maxIterations, s));
	}
	const long long ld = std::max<long long>(64, (static_cast<long long>(n) + 63) / 64 * 64);
	DevBuf<T> S, AS, BS, gparts, parts, parts0, parts1, dG, dH, dY;
	DevBuf<LobpcgGenState<T>> st;
	SyncOnExit drain{s};
	SMM_TRY(S.alloc(static_cast<size_t>(ld) * 3 * k));
	SMM_TRY(AS.alloc(static_cast<size_t>(ld) * 3 * k));
	SMM_TRY(BS.alloc(static_cast<size_t>(ld) * 3 * k));
	SMM_TRY(gparts.alloc(static_cast<size_t>(MB_MAX) * MB_MAX * MG_NPART));
	SMM_TRY(parts.alloc(static_cast<size_t>(2 * MAXK) * NPART));
	SMM_TRY(parts0.alloc(NPART));
	SMM_TRY(parts1.alloc(NPART));
	SMM_TRY(dG.alloc(static_cast<size_t>(MB_MAX) * MB_MAX));
	SMM_TRY(dH.alloc(static_cast<size_t>(MB_MAX) * MB_MAX));
	SMM_TRY(dY.alloc(static_cast<size_t>(32) * MB_MAX));
	SMM_TRY(st.alloc(1));
	SMM_HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(LobpcgGenState<T>), s));
	LobpcgGenState<T>* sp = st.p;
	const int gmv = gridMV(n, sizeof(T));
	const int g = solverGrid(n);
	auto scol = [&](int j) { return S.p + static_cast<long long>(j) * ld; };
	auto acol = [&](int j) { return AS.p + static_cast<long long>(j) * ld; };
	auto bcol = [&](int j) { return BS.p + static_cast<long long>(j) * ld; };
	auto spmv = [&](const smm_hip_csr* m, const T* x, T* y) { return launchSpmv<T>(m, SMM_OP_ASSIGN, nullptr, x, y, 0, nullptr, nullptr, nullptr, s); };
	std::vector<T> hG, hY;
	std::vector<double> t, theta, c, y, w, q;
	LoopWatch none;

	// the start block: the caller's, or the hash columns; classical Gram-Schmidt in B's inner product twice and a division by the B-norm
	if (!X0) hashFillKernel<T><<<dim3(g, k), TPB, 0, s>>>(n, seed, 0, S.p, ld);
	for (int j = 0; j < k; ++j) {
		T* xj = scol(j);
		T* bxj = bcol(j);
		if (X0) SMM_TRY(launchCopy2<T>(n, X0 + j * ldx0, xj, nullptr, s));
		SMM_TRY(spmv(b, xj, bxj));
		multiDotKernel<T><<<gmv, TPB, 0, s>>>(n, 1, bxj, ld, xj, parts0, &sp->bad);
		if (j > 0) {
			for (int pass = 0; pass < 2; ++pass) {
				multiDotKernel<T><<<gmv, TPB, 0, s>>>(n, j, BS.p, ld, xj, parts, &sp->bad);
				multiDotFinish<T><<<j, TPB, 0, s>>>(parts, gmv, sp->h, sp->coef, &sp->bad);
				multiAxpyKernel<T, false><<<gmv, TPB, 0, s>>>(n, j, nullptr, S.p, ld, sp->coef, xj, xj, nullptr, &sp->bad);
			}
			SMM_TRY(spmv(b, xj, bxj));
			multiDotKernel<T><<<gmv, TPB, 0, s>>>(n, 1, bxj, ld, xj, parts1, &sp->bad);
		}
		lobpcgGenNormalise<T><<<g, TPB, 0, s>>>(n, xj, bxj, parts0, j > 0 ? parts1.p : parts0.p, gmv, sp);
	}
	out->bmatvecs = 2 * k - 1;
	LobpcgGenState<T> h;
	SMM_TRY(loopFinish(none, &h, sp, sizeof(h), s));
	if (h.bad) {
		out->status = SMM_SOLVER_DIVERGED;
		drain.armed = false;
		return SMM_HIP_OK;
	}
	for (int j = 0; j < k; ++j) SMM_TRY(spmv(a, scol(j), acol(j)));
	out->matvecs = k;

	// as in lobpcgDev: the Rayleigh-Ritz step on the m leading columns of S and AS
	auto ritz = [&](int m, bool* ok) -> int {
		multiGramLaunch<T>(n, m, m, S.p, ld, AS.p, ld, gparts.p, dG.p, m, s);
		hG.resize(static_cast<size_t>(m) * m);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(devToHost(hG.data(), dG.p, sizeof(T) * hG.size(), s));
		*ok = lobpcgSymmetrise<T>(m, hG, t) && jacobiEigen(m, t, w, q);
		if (!*ok) return SMM_HIP_OK;
		theta.resize(m);
		c.assign(static_cast<size_t>(m) * m, 0.0);
		for (int i = 0; i < m; ++i) {
			const int src = which == SMM_EIGSH_LARGEST ? m - 1 - i : i;
			theta[i] = w[src];
			for (int r = 0; r < m; ++r) c[static_cast<size_t>(i) * m + r] = q[r * m + src];
		}
		return SMM_HIP_OK;
	};
	auto rotateAll = [&](int from, int m, int cols, const std::vector<double>& yy) -> int {
		SMM_TRY(lobpcgStage<T>(m, cols, yy, hY, dY, s));
		T* const bases[MV_MAX_BASES] = {scol(from), acol(from), bcol(from)};
		multiRotateBasesLaunch<T>(n, m, cols, MV_MAX_BASES, bases, ld, dY.p, s);
		return SMM_HIP_OK;
	};

	bool ok = true;
	SMM_TRY(ritz(k, &ok));
	if (!ok) {
		out->status = SMM_SOLVER_DIVERGED;
		drain.armed = false;
		return SMM_HIP_OK;
	}
	SMM_TRY(rotateAll(0, k, k, c));

	int np = 0;  // kept directions
	double scale = 0;
	std::vector<T> vals(k), rn(k), sums(2 * k);
	std::vector<int> active;
	int status = SMM_SOLVER_SUCCESS;
	for (int it = 0;; ++it) {
		LobpcgThetas<T> th;
		for (int j = 0; j < MAXK; ++j) th.v[j] = j < k ? static_cast<T>(theta[j]) : T(0);
		T* R = acol(k + np);  // the AW columns: free until the SpMVs below fill them
		lobpcgGenResidual<T><<<dim3(g, k), TPB, 0, s>>>(n, AS.p, BS.p, ld, th, R, parts);
		multiDotFinish<T><<<2 * k, TPB, 0, s>>>(parts, g, sp->sums, nullptr, nullptr);
		SMM_HIP_TRY(hipGetLastError());
		SMM_TRY(devToHost(sums.data(), sp->sums, sizeof(T) * 2 * k, s));
		bool finite = true;
		for (int j = 0; j < k; ++j) {
			rn[j] = std::sqrt(sums[j]);
			sums[k + j] = std::sqrt(sums[k + j]);  // bn_j
			finite = finite && std::isfinite(rn[j]) && std::isfinite(sums[k + j]) && sums[k + j] > T(0);
		}
		for (double v : theta) {
			finite = finite && std::isfinite(v);
			scale = std::max(scale, std::fabs(v));
		}
		if (!finite) {
			status = SMM_SOLVER_DIVERGED;
			break;
		}
		active.clear();
		for (int j = 0; j < k; ++j) {
			if (!(static_cast<double>(rn[j]) <= bound * scale * static_cast<double>(sums[k + j]))) active.push_back(j);
		}
		for (int j = 0; j < k; ++j) vals[j] = th.v[j];
		out->nconv = k - static_cast<int>(active.size());
		out->iterations = it;
		if (active.empty()) break;
		if (it == maxIterations) {
			status = SMM_SOLVER_MAX_ITERATIONS_REACHED;
			break;
		}
		const int na = static_cast<int>(active.size());
		for (int i = 0; i < na; ++i) {
			const T* rj = R + static_cast<long long>(active[i]) * ld;
			if (M) SMM_TRY(precondApplyDev<T>(M, rj, scol(k + np + i), nullptr, s));
			else SMM_TRY(launchCopy2<T>(n, rj, scol(k + np + i), nullptr, s));
		}
		for (int i = 0; i < na; ++i) SMM_TRY(spmv(a, scol(k + np + i), acol(k + np + i)));
		for (int i = 0; i < na; ++i) SMM_TRY(spmv(b, scol(k + np + i), bcol(k + np + i)));
		out->matvecs += na;
		out->bmatvecs += na;
		out->applies += M ? na : 0;

		int nz = np + na;
		for (int pass = 0; pass < 2 && nz > 0; ++pass) {
			multiGramLaunch<T>(n, k, nz, BS.p, ld, scol(k), ld, gparts.p, dH.p, k, s);
			const T* const from[MV_MAX_BASES] = {S.p, AS.p, BS.p};
			T* const onto[MV_MAX_BASES] = {scol(k), acol(k), bcol(k)};
			multiBlockAxpyBasesLaunch<T>(n, k, nz, MV_MAX_BASES, from, ld, dH.p, k, onto, ld, s);
			multiGramLaunch<T>(n, nz, nz, scol(k), ld, bcol(k), ld, gparts.p, dG.p, nz, s);
			hG.resize(static_cast<size_t>(nz) * nz);
			SMM_HIP_TRY(hipGetLastError());
			SMM_TRY(devToHost(hG.data(), dG.p, sizeof(T) * hG.size(), s));
			int keep = 0;
			if (!lobpcgSymmetrise<T>(nz, hG, t) || !lobpcgSvqb(nz, t, eps, w, q, y, &keep)) {
				status = SMM_SOLVER_DIVERGED;
				break;
			}
			if (keep > 0) SMM_TRY(rotateAll(k, nz, keep, y));
			nz = keep;
		}
		if (status != SMM_SOLVER_SUCCESS) break;
		const int m = k + nz;
		SMM_TRY(ritz(m, &ok));
		if (!ok) {
			status = SMM_SOLVER_DIVERGED;
			break;
		}
		// [X P] = S [C | C_P], as in lobpcgDev
		const int npNew = std::min(na, nz);
		y.assign(static_cast<size_t>(m) * (k + npNew), 0.0);
		std::copy(c.begin(), c.begin() + static_cast<size_t>(m) * k, y.begin());
		for (int i = 0; i < npNew; ++i) {
			for (int r = k; r < m; ++r) y[static_cast<size_t>(k + i) * m + r] = c[static_cast<size_t>(active[i]) * m + r];
		}
		SMM_TRY(rotateAll(0, m, k + npNew, y));
		np = npNew;
	}
	out->status = status;
	if (status != SMM_SOLVER_DIVERGED) {
		SMM_TRY(hostToDev(d_vals, vals.data(), sizeof(T) * k, s));
		for (int j = 0; d_X && j < k; ++j) SMM_TRY(launchCopy2<T>(n, scol(j), d_X + static_cast<long long>(j) * ldx, nullptr, s));
		if (residuals) std::copy(rn.begin(), rn.end(), residuals);
		out->wrote = true;
	}
	SMM_HIP_TRY(hipGetLastError());
	SMM_HIP_TRY(hipStreamSynchronize(s));
	drain.armed = false;
	return M ? precondTakeError(M, s) : SMM_HIP_OK;
}

template <typename T>
static int lobpcgGenDevEntry(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* d_X0, long long ldx0,
                             unsigned long long seed, T* d_vals, T* d_X, long long ldx, smm_hip_stream stream, T* residuals, int* nconv, int* iterations, int* matvecs,
                             int* bmatvecs, int* applies, int* status) {
	if (!b) {
		SMM_TRY(lobpcgDevEntry<T>(a, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_vals, d_X, ldx, stream, residuals, nconv, iterations, matvecs, applies, status));
		if (bmatvecs) *bmatvecs = 0;
		return SMM_HIP_OK;
	}
	SMM_TRY(lobpcgGenCheck<T>(a, b, k, which, maxIterations, M, d_X0, ldx0, d_vals, d_X, ldx));
	LobpcgOut o;
	if (a->rows > 0 && k > 0) {
		SMM_TRY(ensureInit());
		SMM_TRY(lobpcgGenDev<T>(a, b, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_vals, d_X, ldx, pickStream(stream), residuals, &o));
	}
	lobpcgReport<T>(o, nconv, iterations, matvecs, applies, status);
	if (bmatvecs) *bmatvecs = o.bmatvecs;
	return SMM_HIP_OK;
}

// host arrays, as lobpcgHost
template <typename T>
static int lobpcgGenHost(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, T tol, const smm_hip_precond* M, const T* X0, long long ldx0,
                         unsigned long long seed, T* eigenvalues, T* eigenvectors, long long ldx, T* residuals, int* nconv, int* iterations, int* matvecs, int* bmatvecs,
                         int* applies, int* status) {
	if (!b) {
		SMM_TRY(lobpcgHost<T>(a, k, which, maxIterations, tol, M, X0, ldx0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, iterations, matvecs, applies, status));
		if (bmatvecs) *bmatvecs = 0;
		return SMM_HIP_OK;
	}
	SMM_TRY(lobpcgGenCheck<T>(a, b, k, which, maxIterations, M, X0, ldx0, eigenvalues, eigenvectors, ldx));
	LobpcgOut o;
	if (a->rows > 0 && k > 0) {
		SMM_TRY(ensureInit());
		hipStream_t s = libStream();
		const size_t n = static_cast<size_t>(a->rows);
		DevBuf<T> dX0, dvals, dX;
		SyncOnExit drain{s};
		if (X0) {
			SMM_TRY(dX0.alloc(n * k));
			for (int j = 0; j < k; ++j) SMM_TRY(hostToDev(dX0.p + j * n, X0 + static_cast<long long>(j) * ldx0, sizeof(T) * n, s));
		}
		SMM_TRY(dvals.alloc(k));
		if (eigenvectors) SMM_TRY(dX.alloc(n * k));
		SMM_TRY(lobpcgGenDev<T>(a, b, k, which, maxIterations, tol, M, X0 ? dX0.p : nullptr, static_cast<long long>(n), seed, dvals.p, eigenvectors ? dX.p : nullptr,
		                        static_cast<long long>(n), s, residuals, &o));
		if (o.wrote) {
			SMM_TRY(devToHost(eigenvalues, dvals, sizeof(T) * k, s));
			for (int j = 0; eigenvectors && j < k; ++j) SMM_TRY(devToHost(eigenvectors + static_cast<long long>(j) * ldx, dX.p + j * n, sizeof(T) * n, s));
		}
		drain.armed = false;
	}
	lobpcgReport<T>(o, nconv, iterations, matvecs, applies, status);
	if (bmatvecs) *bmatvecs = o.bmatvecs;
	return SMM_HIP_OK;
}

static int blockCheck(const char* who, int n, int m, int l, bool ldBad, bool nullArray) {
	if (n < 0 || m < 1 || m > MB_MAX || l < 1 || l > MB_MAX || ldBad || nullArray) {
		setError("%s: bad arguments (n >= 0, 1 <= m, l <= %d, every leading dimension at least its column's length, no null array)", who, MB_MAX);
		return SMM_HIP_ERR_INVALID;
	}
	return SMM_HIP_OK;
}

template <typename T>
static int multiGramDev(int n, int m, int l, const T* V, long long ldV, const T* W, long long ldW, T* G, long long ldG, smm_hip_stream stream) {
	SMM_TRY(blockCheck("multi_gram", n, m, l, ldV < n || ldW < n || ldG < m, !G || (n > 0 && (!V || !W))));
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	if (n == 0) {  // the empty sum
		SMM_HIP_TRY(hipMemset2DAsync(G, sizeof(T) * ldG, 0, sizeof(T) * m, l, s));
		return SMM_HIP_OK;
	}
	// one persistent partial-sum buffer per stream and scalar type, the two launches enqueued under one lock (see multiDotDev, smm_solvers_gmres.hip)
	static std::map<hipStream_t, T*> buffers;
	static std::mutex mu;
	std::lock_guard<std::mutex> lock(mu);
	auto it = buffers.find(s);
	if (it == buffers.end()) {
		T* p = nullptr;
		SMM_TRY(devAlloc(reinterpret_cast<void**>(&p), static_cast<size_t>(MB_MAX) * MB_MAX * MG_NPART * sizeof(T)));
		it = buffers.emplace(s, p).first;
	}
	multiGramLaunch<T>(n, m, l, V, ldV, W, ldW, it->second, G, ldG, s);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

template <typename T>
static int multiBlockAxpyDev(int n, int m, int l, const T* V, long long ldV, const T* H, long long ldH, T* W, long long ldW, smm_hip_stream stream) {
	SMM_TRY(blockCheck("multi_block_axpy", n, m, l, ldV < n || ldW < n || ldH < m, !H || (n > 0 && (!V || !W))));
	if (n == 0) return SMM_HIP_OK;
	SMM_TRY(ensureInit());
	multiBlockAxpyLaunch<T>(n, m, l, V, ldV, H, ldH, W, ldW, pickStream(stream));
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// nb in range, the arrays given, and with n > 0 every entry of them
template <typename T>
static bool basesGiven(int n, int nb, const T* const* a) {
	if (nb < 1 || nb > MV_MAX_BASES || !a) return false;
	for (int i = 0; n > 0 && i < nb; ++i) {
		if (!a[i]) return false;
	}
	return true;
}

template <typename T>
static int multiBlockAxpyBasesDev(int n, int m, int l, int nb, const T* const* V, long long ldV, const T* H, long long ldH, T* const* W, long long ldW,
                                  smm_hip_stream stream) {
	const char* who = "multi_block_axpy_bases";
	SMM_TRY(blockCheck(who, n, m, l, ldV < n || ldW < n || ldH < m, !H));
	if (!basesGiven<T>(n, nb, V) || !basesGiven<T>(n, nb, W)) {
		setError("%s: bad arguments (1 <= nb <= %d, no null array and no null entry)", who, MV_MAX_BASES);
		return SMM_HIP_ERR_INVALID;
	}
	if (n == 0) return SMM_HIP_OK;
	for (int i = 0; i < nb; ++i) {  // a V that is read while a W is written: the result would depend on the schedule
		for (int j = 0; j < nb; ++j) {
			const T* vEnd = V[i] + (m - 1) * ldV + n;
			const T* wEnd = W[j] + (l - 1) * ldW + n;
			if (V[i] < wEnd && W[j] < vEnd) {
				setError("%s: V[%d] overlaps W[%d]", who, i, j);
				return SMM_HIP_ERR_INVALID;
			}
		}
	}
	SMM_TRY(ensureInit());
	multiBlockAxpyBasesLaunch<T>(n, m, l, nb, V, ldV, H, ldH, W, ldW, pickStream(stream));
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

// multi_rotate (smm_solvers_eigsh.hip) on several bases: Y is staged once
template <typename T>
static int multiRotateBasesDev(int n, int m, int l, int nb, T* const* V, long long ld, const T* hY, long long ldY, smm_hip_stream stream) {
	if (n < 0 || l < 1 || m < l || m > MR_MAX || ld < n || ldY < m || !hY || !basesGiven<T>(n, nb, V)) {
		setError("multi_rotate_bases: bad arguments (n >= 0, 1 <= l <= m <= %d, ld >= n, ldY >= m, 1 <= nb <= %d, no null array and no null entry)", MR_MAX, MV_MAX_BASES);
		return SMM_HIP_ERR_INVALID;
	}
	if (n == 0) return SMM_HIP_OK;
	SMM_TRY(ensureInit());
	hipStream_t s = pickStream(stream);
	const int MP = multiRotatePad(m);
	std::vector<T> h(static_cast<size_t>(MP) * l, T(0));
	for (int c = 0; c < l; ++c) std::copy(hY + c * ldY, hY + c * ldY + m, h.begin() + static_cast<size_t>(c) * MP);
	DevBuf<T> dY;
	SyncOnExit drain{s};  // (the staged Y is released when this returns)
	SMM_TRY(dY.alloc(h.size()));
	SMM_TRY(hostToDev(dY, h.data(), sizeof(T) * h.size(), s));
	multiRotateBasesLaunch<T>(n, m, l, nb, V, ld, dY.p, s);
	SMM_HIP_TRY(hipGetLastError());
	return SMM_HIP_OK;
}

}  // namespace smm

using namespace smm;

extern "C" {

int smm_hip_lobpcg_f32(const smm_hip_csr* a, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* X0, long long ldx0,
                       unsigned long long seed, float* eigenvalues, float* eigenvectors, long long ldx, float* residuals, int* nconv, int* iterations, int* matvecs,
                       int* applies, int* solver_status) {
	return lobpcgHost<float>(a, k, which, maxIterations, tol, M, X0, ldx0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, iterations, matvecs, applies,
	                         solver_status);
}
int smm_hip_lobpcg_f64(const smm_hip_csr* a, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* X0, long long ldx0,
                       unsigned long long seed, double* eigenvalues, double* eigenvectors, long long ldx, double* residuals, int* nconv, int* iterations, int* matvecs,
                       int* applies, int* solver_status) {
	return lobpcgHost<double>(a, k, which, maxIterations, tol, M, X0, ldx0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, iterations, matvecs, applies,
	                          solver_status);
}
int smm_hip_lobpcg_dev_f32(const smm_hip_csr* a, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* d_X0, long long ldx0,
                           unsigned long long seed, float* d_eigenvalues, float* d_eigenvectors, long long ldx, smm_hip_stream stream, float* residuals, int* nconv,
                           int* iterations, int* matvecs, int* applies, int* solver_status) {
	return lobpcgDevEntry<float>(a, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_eigenvalues, d_eigenvectors, ldx, stream, residuals, nconv, iterations, matvecs,
	                             applies, solver_status);
}
int smm_hip_lobpcg_dev_f64(const smm_hip_csr* a, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* d_X0, long long ldx0,
                           unsigned long long seed, double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream, double* residuals, int* nconv,
                           int* iterations, int* matvecs, int* applies, int* solver_status) {
	return lobpcgDevEntry<double>(a, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_eigenvalues, d_eigenvectors, ldx, stream, residuals, nconv, iterations,
	                              matvecs, applies, solver_status);
}

int smm_hip_lobpcg_gen_f32(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* X0,
                           long long ldx0, unsigned long long seed, float* eigenvalues, float* eigenvectors, long long ldx, float* residuals, int* nconv, int* iterations,
                           int* matvecs, int* bmatvecs, int* applies, int* solver_status) {
	return lobpcgGenHost<float>(a, b, k, which, maxIterations, tol, M, X0, ldx0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, iterations, matvecs, bmatvecs,
	                            applies, solver_status);
}
int smm_hip_lobpcg_gen_f64(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* X0,
                           long long ldx0, unsigned long long seed, double* eigenvalues, double* eigenvectors, long long ldx, double* residuals, int* nconv, int* iterations,
                           int* matvecs, int* bmatvecs, int* applies, int* solver_status) {
	return lobpcgGenHost<double>(a, b, k, which, maxIterations, tol, M, X0, ldx0, seed, eigenvalues, eigenvectors, ldx, residuals, nconv, iterations, matvecs, bmatvecs,
	                             applies, solver_status);
}
int smm_hip_lobpcg_gen_dev_f32(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, float tol, const smm_hip_precond* M, const float* d_X0,
                               long long ldx0, unsigned long long seed, float* d_eigenvalues, float* d_eigenvectors, long long ldx, smm_hip_stream stream,
                               float* residuals, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* solver_status) {
	return lobpcgGenDevEntry<float>(a, b, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_eigenvalues, d_eigenvectors, ldx, stream, residuals, nconv, iterations,
	                                matvecs, bmatvecs, applies, solver_status);
}
int smm_hip_lobpcg_gen_dev_f64(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int maxIterations, double tol, const smm_hip_precond* M, const double* d_X0,
                               long long ldx0, unsigned long long seed, double* d_eigenvalues, double* d_eigenvectors, long long ldx, smm_hip_stream stream,
                               double* residuals, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* solver_status) {
	return lobpcgGenDevEntry<double>(a, b, k, which, maxIterations, tol, M, d_X0, ldx0, seed, d_eigenvalues, d_eigenvectors, ldx, stream, residuals, nconv, iterations,
	                                 matvecs, bmatvecs, applies, solver_status);
}

int smm_hip_multi_block_axpy_bases_dev_f32(int n, int m, int l, int nb, const float* const* d_V, long long ldV, const float* d_H, long long ldH, float* const* d_W,
                                           long long ldW, smm_hip_stream stream) {
	return multiBlockAxpyBasesDev<float>(n, m, l, nb, d_V, ldV, d_H, ldH, d_W, ldW, stream);
}
int smm_hip_multi_block_axpy_bases_dev_f64(int n, int m, int l, int nb, const double* const* d_V, long long ldV, const double* d_H, long long ldH, double* const* d_W,
                                           long long ldW, smm_hip_stream stream) {
	return multiBlockAxpyBasesDev<double>(n, m, l, nb, d_V, ldV, d_H, ldH, d_W, ldW, stream);
}
int smm_hip_multi_rotate_bases_dev_f32(int n, int m, int l, int nb, float* const* d_V, long long ld, const float* h_Y, long long ldY, smm_hip_stream stream) {
	return multiRotateBasesDev<float>(n, m, l, nb, d_V, ld, h_Y, ldY, stream);
}
int smm_hip_multi_rotate_bases_dev_f64(int n, int m, int l, int nb, double* const* d_V, long long ld, const double* h_Y, long long ldY, smm_hip_stream stream) {
	return multiRotateBasesDev<double>(n, m, l, nb, d_V, ld, h_Y, ldY, stream);
}

int smm_hip_multi_gram_dev_f32(int n, int m, int l, const float* d_V, long long ldV, const float* d_W, long long ldW, float* d_G, long long ldG, smm_hip_stream stream) {
	return multiGramDev<float>(n, m, l, d_V, ldV, d_W, ldW, d_G, ldG, stream);
}
int smm_hip_multi_gram_dev_f64(int n, int m, int l, const double* d_V, long long ldV, const double* d_W, long long ldW, double* d_G, long long ldG,
                               smm_hip_stream stream) {
	return multiGramDev<double>(n, m, l, d_V, ldV, d_W, ldW, d_G, ldG, stream);
}
int smm_hip_multi_block_axpy_dev_f32(int n, int m, int l, const float* d_V, long long ldV, const float* d_H, long long ldH, float* d_W, long long ldW,
                                     smm_hip_stream stream) {
	return multiBlockAxpyDev<float>(n, m, l, d_V, ldV, d_H, ldH, d_W, ldW, stream);
}
int smm_hip_multi_block_axpy_dev_f64(int n, int m, int l, const double* d_V, long long ldV, const double* d_H, long long ldH, double* d_W, long long ldW,
                                     smm_hip_stream stream) {
	return multiBlockAxpyDev<double>(n, m, l, d_V, ldV, d_H, ldH, d_W, ldW, stream);
}

}  // extern "C"
