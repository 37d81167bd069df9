// smm_hip/sparse_matrix_math.h -- the reference's C++ API for the hot path, re-implemented on top of the C ABI of
// libsmm_hip.so (include/smm_hip.h).  A program written against vasil-pashov/sparse_matrix_math's
// include/sparse_matrix_math.h ("ref" below) that only uses
//
//     SMM::Vector, SMM::TripletMatrix, SMM::CSRMatrix (init / rMult / rMultAdd / rMultSub / getters / iteration, writable iterators
//     included / getPreconditioner / operator*= / inplaceAdd / inplaceSubtract / updateEntry / addEntry / zeroValues /
//     hasSameNonZeroPattern), SMM::SolverStatus, SMM::SolverPreconditioner, SMM::ConjugateGradient (plain and IC0),
//     SMM::BiCGStab (plain and preconditioned), SMM::BiCGSymmetric, SMM::ConjugateGradientSquared, SMM::GMRES, SMM::MINRES, SMM::LSQR, SMM::eigsh, SMM::svds, SMM::lobpcg (A x = lambda x and A x = lambda B x), SMM::IDRs, SMM::loadMatrix
//     (additions: SMM::transpose, SMM::isSymmetric, SMM::BiCG for matrices that are not symmetric; SMM::multiply, SMM::multiplyInto;
//      SMM::blockMatrix, SMM::blockRefresh, SMM::submatrix, SMM::submatrixRefresh, SMM::diagonal, CSRMatrix::scaleRowsCols;
//     SMM::add, SMM::addInto; SMM::convert, SMM::IterativeRefinement)
//
// compiles against this header unchanged and runs those calls on an MI355X: same names, same argument order and meaning,
// same return values (SolverStatus; int != 0 on failure for init / apply).  Matrix assembly (TripletMatrix, CSR arrays)
// stays on the host exactly as in the reference; the CSR arrays are mirrored to the GPU the first time a hot-path call
// needs them.  Nothing here computes on the CPU: every rMult* / solver / apply call goes through libsmm_hip.so.
//
// FAILURES OF THE GPU PATH ARE OBSERVABLE (the reference's signatures have no room for them, so they are reported beside them):
//   * SMM::lastHipStatus() -- the SMM_HIP_* status of the last hot-path call of this thread (0 = ok), text in smm_hip_last_error();
//   * rMult / rMultAdd / rMultSub fill `out` with NaN, Vector::operator* returns NaN, solvers return SolverStatus::DIVERGED
//     (and lastHipStatus() != 0 tells that apart from a numerical divergence), apply() / init() return non-zero;
//   * compile with -DSMM_HIP_ABORT_ON_ERROR to print the message and abort() instead.
//
// Written from the documented behaviour of the reference; no reference source is reproduced here.
// Additions the reference lacks: CSRMatrix::init(rows, cols, start, positions, values) (raw CSR arrays, ref can only be
// filled through a std::map), JacobiPreconditioner, a working ILU0Preconditioner, Matrix Market `general` matrices, and value edits
// made ON THE GPU once the matrix has a device mirror (the pattern and everything derived from it are kept: see "Editing the values").
// Also an addition: SMM::AssemblyPlan with CSRMatrix::init(plan, values) / assemble(plan, values) -- the triplets sorted once and summed
// on the GPU in list order, for callers that assemble the same pattern again and again; init(TripletMatrix) is unchanged.
#pragma once

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <fstream>
#include <initializer_list>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../smm_hip.h"

#define SMM_MAJOR_VERSION 0
#define SMM_MINOR_VERSION 2
#define SMM_PATCH_VERSION 0

namespace SMM {

// ---- C ABI dispatch on T ------------------------------------------------------------------------------------------
namespace detail {
template <typename T>
struct Abi;
template <>
struct Abi<float> {
	static int create(int r, int c, const int* s, const int* p, const float* v, smm_hip_csr** o) { return smm_hip_csr_create_f32(r, c, s, p, v, o); }
	static int spmv(const smm_hip_csr* m, int op, const float* l, const float* x, float* o) { return smm_hip_spmv_f32(m, op, l, x, o); }
	static int dot(int n, const float* a, const float* b, float* r) { return smm_hip_dot_f32(n, a, b, r); }
	static int cg(const smm_hip_csr* a, const float* b, const float* x0, float* x, int it, float eps, const smm_hip_precond* M, int* st) {
		return smm_hip_cg_f32(a, b, x0, x, it, eps, M, st, nullptr, nullptr);
	}
	static int bicgstab(const smm_hip_csr* a, float* b, float* x, int it, float eps, const smm_hip_precond* M, int* st) {
		return smm_hip_bicgstab_f32(a, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int bicgsym(const smm_hip_csr* a, float* b, float* x, int it, float eps, int* st) { return smm_hip_bicgsymmetric_f32(a, b, x, it, eps, st, nullptr); }
	static int cgs(const smm_hip_csr* a, float* b, float* x, int it, float eps, int* st) { return smm_hip_cgs_f32(a, b, x, it, eps, st, nullptr, nullptr); }
	static int gmres(const smm_hip_csr* a, float* b, float* x, int it, float eps, int restart, const smm_hip_precond* M, int* st) {
		return smm_hip_gmres_f32(a, b, x, it, eps, restart, M, st, nullptr, nullptr);
	}
	static int minres(const smm_hip_csr* a, float* b, float* x, int it, float eps, const smm_hip_precond* M, int* st) {
		return smm_hip_minres_f32(a, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int eigsh(const smm_hip_csr* a, int k, int which, int ncv, int restarts, float tol, const float* v0, unsigned long long seed, float* w, float* x, long long ldx,
	                 float* rho, int* nconv, int* nrestarts, int* matvecs, int* st) {
		return smm_hip_eigsh_f32(a, k, which, ncv, restarts, tol, v0, seed, w, x, ldx, rho, nconv, nrestarts, matvecs, st);
	}
	static int svds(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int restarts, float tol, const float* v0, unsigned long long seed, float* sv, float* u, long long ldu,
	                float* v, long long ldv, float* rho, int* nconv, int* nrestarts, int* matvecs, int* st) {
		return smm_hip_svds_f32(a, at, k, ncv, restarts, tol, v0, seed, sv, u, ldu, v, ldv, rho, nconv, nrestarts, matvecs, st);
	}
	static int lobpcg(const smm_hip_csr* a, int k, int which, int it, float tol, const smm_hip_precond* M, const float* x0, long long ldx0, unsigned long long seed, float* w,
	                  float* x, long long ldx, float* rn, int* nconv, int* iterations, int* matvecs, int* applies, int* st) {
		return smm_hip_lobpcg_f32(a, k, which, it, tol, M, x0, ldx0, seed, w, x, ldx, rn, nconv, iterations, matvecs, applies, st);
	}
	static int lobpcgGen(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int it, float tol, const smm_hip_precond* M, const float* x0, long long ldx0,
	                     unsigned long long seed, float* w, float* x, long long ldx, float* rn, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* st) {
		return smm_hip_lobpcg_gen_f32(a, b, k, which, it, tol, M, x0, ldx0, seed, w, x, ldx, rn, nconv, iterations, matvecs, bmatvecs, applies, st);
	}
	static int idrs(const smm_hip_csr* a, float* b, float* x, int it, float eps, int s, const smm_hip_precond* M, int* st) {
		return smm_hip_idrs_f32(a, b, x, it, eps, s, M, 0ull, st, nullptr, nullptr);
	}
	static int bicg(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int it, float eps, int* st) { return smm_hip_bicg_f32(a, at, b, x, it, eps, st, nullptr, nullptr); }
	static int lsqr(const smm_hip_csr* a, const smm_hip_csr* at, float* b, float* x, int it, float eps, float damp, int* st, int* steps, int* reason) {
		return smm_hip_lsqr_f32(a, at, b, x, it, eps, damp, st, steps, reason, nullptr, nullptr);
	}
	static int apply(const smm_hip_precond* M, const float* r, float* x) { return smm_hip_precond_apply_f32(M, r, x); }
	static int createAmgCandidates(const smm_hip_csr* a, const float* B, int k, int b, double theta, int levels, int coarse, int degree, double ratio, smm_hip_precond** o) {
		return smm_hip_precond_create_amg_candidates_f32(a, B, k, b, theta, levels, coarse, degree, ratio, o);
	}
	static int amgCandidates(const smm_hip_precond* M, int level, float* out, size_t count, int* k, int* dropped) {
		return smm_hip_precond_amg_candidates_f32(M, level, out, count, k, dropped, nullptr);
	}
	static int scale(smm_hip_csr* m, float a) { return smm_hip_csr_scale_f32(m, a, nullptr); }
	static int axpy(smm_hip_csr* m, float a, const smm_hip_csr* o) { return smm_hip_csr_axpy_f32(m, a, o, nullptr); }
	static int zero(smm_hip_csr* m) { return smm_hip_csr_zero_f32(m, nullptr); }
	static int update(smm_hip_csr* m, int n, const int* r, const int* c, const float* v) { return smm_hip_csr_update_entries_f32(m, n, r, c, v, SMM_UPDATE_SET, nullptr); }
	static int getValues(const smm_hip_csr* m, float* v) { return smm_hip_csr_get_values_f32(m, v); }
	static int permuteRefresh(smm_hip_csr* b, const smm_hip_csr* a) { return smm_hip_csr_permute_refresh_f32(b, a, nullptr); }
	static int assembled(const smm_hip_assembly* p, const float* v, smm_hip_csr** o) { return smm_hip_assembly_csr_create_f32(p, v, o); }
	static int refill(const smm_hip_assembly* p, smm_hip_csr* m, const float* v, int mode) { return smm_hip_assembly_refill_f32(p, m, v, mode); }
	static int multiplyInto(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b) { return smm_hip_csr_multiply_into_f32(c, a, b, nullptr); }
	static int addCreate(const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta, smm_hip_csr** o) { return smm_hip_csr_add_create_f32(a, alpha, b, beta, nullptr, o); }
	static int addInto(smm_hip_csr* c, const smm_hip_csr* a, float alpha, const smm_hip_csr* b, float beta) { return smm_hip_csr_add_into_f32(c, a, alpha, b, beta, nullptr); }
	static int blockCreate(int p, int q, const smm_hip_csr* const* blocks, const float* coef, const int* rs, const int* cs, smm_hip_csr** o) {
		return smm_hip_csr_block_create_f32(p, q, blocks, coef, rs, cs, nullptr, o);
	}
	static int blockRefresh(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const float* coef) { return smm_hip_csr_block_refresh_f32(c, p, q, blocks, coef, nullptr); }
	static int submatrixRefresh(smm_hip_csr* s, const smm_hip_csr* a) { return smm_hip_csr_submatrix_refresh_f32(s, a, nullptr); }
	static int diagonal(const smm_hip_csr* a, float* out, int* missing) { return smm_hip_csr_diagonal_f32(a, out, missing); }
	static int scaleRowsCols(smm_hip_csr* m, const float* r, const float* c) { return smm_hip_csr_scale_rows_cols_f32(m, r, c); }
	static int spmm(const smm_hip_csr* m, int op, int k, const float* l, const float* x, float* o) { return smm_hip_spmm_f32(m, op, k, l, x, o); }
	static int bicgstabBatch(const smm_hip_csr* a, int k, float* b, float* x, int it, float eps, const smm_hip_precond* M, int* st) {
		return smm_hip_bicgstab_batch_f32(a, k, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int cgBatch(const smm_hip_csr* a, int k, const float* b, const float* x0, float* x, int it, float eps, int* st) {
		return smm_hip_cg_batch_f32(a, k, b, x0, x, it, eps, st, nullptr, nullptr);
	}
};
template <>
struct Abi<double> {
	static int create(int r, int c, const int* s, const int* p, const double* v, smm_hip_csr** o) { return smm_hip_csr_create_f64(r, c, s, p, v, o); }
	static int spmv(const smm_hip_csr* m, int op, const double* l, const double* x, double* o) { return smm_hip_spmv_f64(m, op, l, x, o); }
	static int dot(int n, const double* a, const double* b, double* r) { return smm_hip_dot_f64(n, a, b, r); }
	static int cg(const smm_hip_csr* a, const double* b, const double* x0, double* x, int it, double eps, const smm_hip_precond* M, int* st) {
		return smm_hip_cg_f64(a, b, x0, x, it, eps, M, st, nullptr, nullptr);
	}
	static int bicgstab(const smm_hip_csr* a, double* b, double* x, int it, double eps, const smm_hip_precond* M, int* st) {
		return smm_hip_bicgstab_f64(a, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int bicgsym(const smm_hip_csr* a, double* b, double* x, int it, double eps, int* st) { return smm_hip_bicgsymmetric_f64(a, b, x, it, eps, st, nullptr); }
	static int cgs(const smm_hip_csr* a, double* b, double* x, int it, double eps, int* st) { return smm_hip_cgs_f64(a, b, x, it, eps, st, nullptr, nullptr); }
	static int gmres(const smm_hip_csr* a, double* b, double* x, int it, double eps, int restart, const smm_hip_precond* M, int* st) {
		return smm_hip_gmres_f64(a, b, x, it, eps, restart, M, st, nullptr, nullptr);
	}
	static int minres(const smm_hip_csr* a, double* b, double* x, int it, double eps, const smm_hip_precond* M, int* st) {
		return smm_hip_minres_f64(a, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int eigsh(const smm_hip_csr* a, int k, int which, int ncv, int restarts, double tol, const double* v0, unsigned long long seed, double* w, double* x, long long ldx,
	                 double* rho, int* nconv, int* nrestarts, int* matvecs, int* st) {
		return smm_hip_eigsh_f64(a, k, which, ncv, restarts, tol, v0, seed, w, x, ldx, rho, nconv, nrestarts, matvecs, st);
	}
	static int svds(const smm_hip_csr* a, const smm_hip_csr* at, int k, int ncv, int restarts, double tol, const double* v0, unsigned long long seed, double* sv, double* u, long long ldu,
	                double* v, long long ldv, double* rho, int* nconv, int* nrestarts, int* matvecs, int* st) {
		return smm_hip_svds_f64(a, at, k, ncv, restarts, tol, v0, seed, sv, u, ldu, v, ldv, rho, nconv, nrestarts, matvecs, st);
	}
	static int lobpcg(const smm_hip_csr* a, int k, int which, int it, double tol, const smm_hip_precond* M, const double* x0, long long ldx0, unsigned long long seed, double* w,
	                  double* x, long long ldx, double* rn, int* nconv, int* iterations, int* matvecs, int* applies, int* st) {
		return smm_hip_lobpcg_f64(a, k, which, it, tol, M, x0, ldx0, seed, w, x, ldx, rn, nconv, iterations, matvecs, applies, st);
	}
	static int lobpcgGen(const smm_hip_csr* a, const smm_hip_csr* b, int k, int which, int it, double tol, const smm_hip_precond* M, const double* x0, long long ldx0,
	                     unsigned long long seed, double* w, double* x, long long ldx, double* rn, int* nconv, int* iterations, int* matvecs, int* bmatvecs, int* applies, int* st) {
		return smm_hip_lobpcg_gen_f64(a, b, k, which, it, tol, M, x0, ldx0, seed, w, x, ldx, rn, nconv, iterations, matvecs, bmatvecs, applies, st);
	}
	static int idrs(const smm_hip_csr* a, double* b, double* x, int it, double eps, int s, const smm_hip_precond* M, int* st) {
		return smm_hip_idrs_f64(a, b, x, it, eps, s, M, 0ull, st, nullptr, nullptr);
	}
	static int bicg(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int it, double eps, int* st) { return smm_hip_bicg_f64(a, at, b, x, it, eps, st, nullptr, nullptr); }
	static int lsqr(const smm_hip_csr* a, const smm_hip_csr* at, double* b, double* x, int it, double eps, double damp, int* st, int* steps, int* reason) {
		return smm_hip_lsqr_f64(a, at, b, x, it, eps, damp, st, steps, reason, nullptr, nullptr);
	}
	static int apply(const smm_hip_precond* M, const double* r, double* x) { return smm_hip_precond_apply_f64(M, r, x); }
	static int createAmgCandidates(const smm_hip_csr* a, const double* B, int k, int b, double theta, int levels, int coarse, int degree, double ratio, smm_hip_precond** o) {
		return smm_hip_precond_create_amg_candidates_f64(a, B, k, b, theta, levels, coarse, degree, ratio, o);
	}
	static int amgCandidates(const smm_hip_precond* M, int level, double* out, size_t count, int* k, int* dropped) {
		return smm_hip_precond_amg_candidates_f64(M, level, out, count, k, dropped, nullptr);
	}
	static int scale(smm_hip_csr* m, double a) { return smm_hip_csr_scale_f64(m, a, nullptr); }
	static int axpy(smm_hip_csr* m, double a, const smm_hip_csr* o) { return smm_hip_csr_axpy_f64(m, a, o, nullptr); }
	static int zero(smm_hip_csr* m) { return smm_hip_csr_zero_f64(m, nullptr); }
	static int update(smm_hip_csr* m, int n, const int* r, const int* c, const double* v) { return smm_hip_csr_update_entries_f64(m, n, r, c, v, SMM_UPDATE_SET, nullptr); }
	static int getValues(const smm_hip_csr* m, double* v) { return smm_hip_csr_get_values_f64(m, v); }
	static int permuteRefresh(smm_hip_csr* b, const smm_hip_csr* a) { return smm_hip_csr_permute_refresh_f64(b, a, nullptr); }
	static int assembled(const smm_hip_assembly* p, const double* v, smm_hip_csr** o) { return smm_hip_assembly_csr_create_f64(p, v, o); }
	static int refill(const smm_hip_assembly* p, smm_hip_csr* m, const double* v, int mode) { return smm_hip_assembly_refill_f64(p, m, v, mode); }
	static int multiplyInto(smm_hip_csr* c, const smm_hip_csr* a, const smm_hip_csr* b) { return smm_hip_csr_multiply_into_f64(c, a, b, nullptr); }
	static int addCreate(const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta, smm_hip_csr** o) { return smm_hip_csr_add_create_f64(a, alpha, b, beta, nullptr, o); }
	static int addInto(smm_hip_csr* c, const smm_hip_csr* a, double alpha, const smm_hip_csr* b, double beta) { return smm_hip_csr_add_into_f64(c, a, alpha, b, beta, nullptr); }
	static int blockCreate(int p, int q, const smm_hip_csr* const* blocks, const double* coef, const int* rs, const int* cs, smm_hip_csr** o) {
		return smm_hip_csr_block_create_f64(p, q, blocks, coef, rs, cs, nullptr, o);
	}
	static int blockRefresh(smm_hip_csr* c, int p, int q, const smm_hip_csr* const* blocks, const double* coef) { return smm_hip_csr_block_refresh_f64(c, p, q, blocks, coef, nullptr); }
	static int submatrixRefresh(smm_hip_csr* s, const smm_hip_csr* a) { return smm_hip_csr_submatrix_refresh_f64(s, a, nullptr); }
	static int diagonal(const smm_hip_csr* a, double* out, int* missing) { return smm_hip_csr_diagonal_f64(a, out, missing); }
	static int scaleRowsCols(smm_hip_csr* m, const double* r, const double* c) { return smm_hip_csr_scale_rows_cols_f64(m, r, c); }
	static int spmm(const smm_hip_csr* m, int op, int k, const double* l, const double* x, double* o) { return smm_hip_spmm_f64(m, op, k, l, x, o); }
	static int bicgstabBatch(const smm_hip_csr* a, int k, double* b, double* x, int it, double eps, const smm_hip_precond* M, int* st) {
		return smm_hip_bicgstab_batch_f64(a, k, b, x, it, eps, M, st, nullptr, nullptr);
	}
	static int cgBatch(const smm_hip_csr* a, int k, const double* b, const double* x0, double* x, int it, double eps, int* st) {
		return smm_hip_cg_batch_f64(a, k, b, x0, x, it, eps, st, nullptr, nullptr);
	}
};
inline int& statusSlot() noexcept {
	static thread_local int st = SMM_HIP_OK;
	return st;
}
// every hot-path call funnels its ABI status through here
inline int note(int abi) noexcept {
	statusSlot() = abi;
#ifdef SMM_HIP_ABORT_ON_ERROR
	if (abi != SMM_HIP_OK) {
		std::fprintf(stderr, "smm_hip: error %d: %s\n", abi, smm_hip_last_error());
		std::abort();
	}
#endif
	return abi;
}
// guards the host / device coherence of the matrices' values (CSRMatrix below): const members that refresh the host copy or flush
// queued entries may run concurrently on one const matrix
inline std::mutex& editMutex() noexcept {
	static std::mutex mu;
	return mu;
}
template <typename T>
inline void fillNaN(T* p, int n) noexcept {
	for (int i = 0; p && i < n; ++i) p[i] = std::numeric_limits<T>::quiet_NaN();
}
}  // namespace detail

// SMM_HIP_* status of the calling thread's last hot-path call (rMult*, dot / norms, solvers, preconditioner init / apply); 0 = ok
inline int lastHipStatus() noexcept { return detail::statusSlot(); }

// ---- Vector<T> (ref:42-381): host buffer that decays to T*, dot product and norms on the GPU ---------------------------
template <typename T>
class Vector {
public:
	using Iterator = T*;
	using ConstIterator = const T*;
	Vector() noexcept = default;
	explicit Vector(const int size) noexcept : buf(static_cast<size_t>(size > 0 ? size : 0)) {}
	Vector(const int size, const T val) noexcept : buf(static_cast<size_t>(size > 0 ? size : 0), val) {}
	Vector(std::initializer_list<T> l) : buf(l) {}
	void init(const int size) { buf.assign(static_cast<size_t>(size), T()); }
	void init(const int size, const T val) { buf.assign(static_cast<size_t>(size), val); }
	int getSize() const noexcept { return static_cast<int>(buf.size()); }
	operator T*() noexcept { return buf.data(); }
	operator const T*() const noexcept { return buf.data(); }
	T& operator[](const int i) { return buf[static_cast<size_t>(i)]; }
	const T& operator[](const int i) const { return buf[static_cast<size_t>(i)]; }
	Iterator begin() noexcept { return buf.data(); }
	Iterator end() noexcept { return buf.data() + buf.size(); }
	ConstIterator begin() const noexcept { return buf.data(); }
	ConstIterator end() const noexcept { return buf.data() + buf.size(); }
	void fill(const T v) { std::fill(buf.begin(), buf.end(), v); }
	Vector& operator+=(const Vector& o) {
		for (size_t i = 0; i < buf.size(); ++i) buf[i] += o.buf[i];
		return *this;
	}
	Vector& operator-=(const Vector& o) {
		for (size_t i = 0; i < buf.size(); ++i) buf[i] -= o.buf[i];
		return *this;
	}
	// dot product (ref:305-328) and norms (ref:287-303) -- reductions of the hot path, computed on the GPU
	const T operator*(const Vector& o) const {
		T r = T(0);
		if (detail::note(detail::Abi<T>::dot(getSize(), buf.data(), o.buf.data(), &r)) != SMM_HIP_OK) r = std::numeric_limits<T>::quiet_NaN();
		return r;
	}
	T secondNormSquared() const { return (*this) * (*this); }
	T secondNorm() const { return std::sqrt(secondNormSquared()); }

private:
	std::vector<T> buf;
};

// ---- TripletMatrix<T> (ref:383-684): ordered COO assembly; duplicates are summed ---------------------------------------
template <typename T>
class TripletEl {
public:
	TripletEl(int r, int c, T v) : row(r), col(c), value(v) {}
	int getRow() const noexcept { return row; }
	int getCol() const noexcept { return col; }
	T getValue() const noexcept { return value; }

private:
	int row, col;
	T value;
};

template <typename T>
class TripletMatrix {
public:
	TripletMatrix() noexcept = default;
	TripletMatrix(int rows, int cols) noexcept : denseRowCount(rows), denseColCount(cols) {}
	TripletMatrix(int rows, int cols, int /*numTriplets*/) noexcept : denseRowCount(rows), denseColCount(cols) {}
	void init(int rows, int cols, int /*numTriplets*/ = 0) {
		denseRowCount = rows;
		denseColCount = cols;
		data.clear();
	}
	int getNonZeroCount() const noexcept { return static_cast<int>(data.size()); }
	int getDenseRowCount() const noexcept { return denseRowCount; }
	int getDenseColCount() const noexcept { return denseColCount; }
	// entries with the same (row, col) add up (ref:612-617)
	void addEntry(int row, int col, T value) { data[key(row, col)] += value; }
	T getValue(int row, int col) const {
		auto it = data.find(key(row, col));
		return it == data.end() ? T(0) : it->second;
	}
	bool updateEntry(int row, int col, T value) {
		auto it = data.find(key(row, col));
		if (it == data.end()) return false;
		it->second = value;
		return true;
	}
	// row-major, column-ascending traversal
	template <typename F>
	void forEach(F&& f) const {
		for (const auto& kv : data) f(static_cast<int>(kv.first >> 32), static_cast<int>(kv.first & 0xFFFFFFFFu), kv.second);
	}

private:
	static uint64_t key(int row, int col) { return (static_cast<uint64_t>(static_cast<uint32_t>(row)) << 32) | static_cast<uint32_t>(col); }
	std::map<uint64_t, T> data;
	int denseRowCount = 0, denseColCount = 0;
};

// ---- AssemblyPlan (addition): one list of (row, col) pairs sorted ONCE on the GPU -- the symbolic half of TripletMatrix + CSRMatrix(triplet).
// CSRMatrix<T>::init(plan, values) / assemble(plan, values) then sum the values of repeated pairs in list order (the bits of addEntry,
// ref:606-618, the first contribution taken as it is) in one device pass; smm_hip.h "assembling a matrix from TRIPLETS".  A pair outside the
// matrix, or no GPU: status() / lastHipStatus() != 0 and the plan is empty (valid() == false).
class AssemblyPlan {
public:
	AssemblyPlan() noexcept = default;
	AssemblyPlan(int rows, int cols, long long n, const int* rowIdx, const int* colIdx) noexcept { init(rows, cols, n, rowIdx, colIdx); }
	AssemblyPlan(const AssemblyPlan&) = delete;
	AssemblyPlan& operator=(const AssemblyPlan&) = delete;
	AssemblyPlan(AssemblyPlan&& o) noexcept { *this = std::move(o); }
	AssemblyPlan& operator=(AssemblyPlan&& o) noexcept {
		if (this != &o) {
			smm_hip_assembly_destroy(plan);
			plan = o.plan;
			st = o.st;
			o.plan = nullptr;
		}
		return *this;
	}
	~AssemblyPlan() { smm_hip_assembly_destroy(plan); }
	int init(int rows, int cols, long long n, const int* rowIdx, const int* colIdx) noexcept {
		smm_hip_assembly_destroy(plan);
		plan = nullptr;
		st = detail::note(smm_hip_assembly_create(rows, cols, n, rowIdx, colIdx, &plan));
		if (st != SMM_HIP_OK) plan = nullptr;
		return st;
	}
	bool valid() const noexcept { return plan != nullptr; }
	int status() const noexcept { return st; }
	int getDenseRowCount() const noexcept { return info(0); }
	int getDenseColCount() const noexcept { return info(1); }
	int getNonZeroCount() const noexcept { return info(2); }
	int getLongestRun() const noexcept { return info(3); }
	long long getTripletCount() const noexcept {
		long long n = 0;
		if (plan) smm_hip_assembly_info(plan, nullptr, nullptr, &n, nullptr, nullptr);
		return n;
	}
	const smm_hip_assembly* handle() const noexcept { return plan; }

private:
	int info(int which) const noexcept {
		int v[4] = {0, 0, 0, 0};
		if (plan) smm_hip_assembly_info(plan, &v[0], &v[1], nullptr, &v[2], &v[3]);
		return v[which];
	}
	smm_hip_assembly* plan = nullptr;
	int st = SMM_HIP_OK;
};

// ref:1002-1006; JACOBI and the BLOCK_ forms (ILU0 / SGS of the block-diagonal part of A, smm_hip.h) are additions
enum class SolverPreconditioner { NONE, SYMMETRIC_GAUS_SEIDEL, ILU0, JACOBI, BLOCK_ILU0, BLOCK_SGS, CHEBYSHEV, AMG };
enum class SolverStatus { SUCCESS = 0, DIVERGED, MAX_ITERATIONS_REACHED };                       // ref:2010-2014

// ---- CSRMatrix<T> (ref:1010-1641) -------------------------------------------------------------------------------------------
template <typename T>
class CSRMatrix {
public:
	using value_type = T;

	// Iterators (ref:722-1000): `*it` / `it->` give an element with getRow / getCol / getValue, and setValue for the non-const kinds.
	// Iterator / ConstIterator walk all stored elements in row-major order (`for (const auto& el : m)`), RowIterator / ConstRowIterator
	// the elements of one row (rowBegin(i) .. rowEnd(i)).  Getting an iterator brings the host copy of the values up to date; setValue
	// writes it and, when the matrix has a device mirror, queues the entry for the mirror (see "Editing the values" below).
	template <bool CONST, bool ROW>
	class IteratorT;
	template <bool CONST>
	class Element {
	public:
		using Matrix = std::conditional_t<CONST, const CSRMatrix, CSRMatrix>;
		Element(Matrix* m, int row, int idx) : m(m), row(row), idx(idx) {}
		int getRow() const noexcept { return row; }
		int getCol() const noexcept { return m->positions[idx]; }
		T getValue() const noexcept { return m->values[idx]; }
		template <bool C = CONST, typename = std::enable_if_t<!C>>
		void setValue(const T v) noexcept {
			m->setValueAt(row, idx, v);
		}

	private:
		template <bool, bool>
		friend class IteratorT;
		Matrix* m;
		int row, idx;
	};
	template <bool CONST, bool ROW>
	class IteratorT {
	public:
		using Matrix = std::conditional_t<CONST, const CSRMatrix, CSRMatrix>;
		using value_type = Element<CONST>;
		using reference = std::conditional_t<CONST, const Element<CONST>&, Element<CONST>&>;
		using pointer = std::conditional_t<CONST, const Element<CONST>*, Element<CONST>*>;
		IteratorT(Matrix* m, int row, int idx) : e(m, row, idx) {
			if (!ROW) skipEmpty();
		}
		template <bool C2, typename = std::enable_if_t<CONST || !C2>>
		IteratorT(const IteratorT<C2, ROW>& o) : e(o.e.m, o.e.row, o.e.idx) {}
		reference operator*() { return e; }
		pointer operator->() { return &e; }
		const Element<CONST>& operator*() const { return e; }
		const Element<CONST>* operator->() const { return &e; }
		IteratorT& operator++() {
			++e.idx;
			if (ROW) {
				if (e.idx == e.m->start[e.row + 1]) ++e.row;
			} else {
				skipEmpty();
			}
			return *this;
		}
		IteratorT operator++(int) {
			IteratorT before = *this;
			++*this;
			return before;
		}
		bool operator!=(const IteratorT& o) const { return e.idx != o.e.idx || e.m != o.e.m; }
		bool operator==(const IteratorT& o) const { return !(*this != o); }

	private:
		template <bool, bool>
		friend class IteratorT;
		void skipEmpty() {
			while (e.row < e.m->denseRowCount && e.idx >= e.m->start[e.row + 1]) ++e.row;
		}
		Element<CONST> e;
	};
	using ConstElement = Element<true>;
	using Iterator = IteratorT<false, false>;
	using ConstIterator = IteratorT<true, false>;
	using RowIterator = IteratorT<false, true>;
	using ConstRowIterator = IteratorT<true, true>;

	// Every preconditioner wraps a device-side smm_hip_precond; `int apply(const T* rhs, T* x) const` as in ref:1173-1235.
	class PreconditionerBase {
	public:
		PreconditionerBase(const PreconditionerBase&) = delete;
		PreconditionerBase& operator=(const PreconditionerBase&) = delete;
		PreconditionerBase(PreconditionerBase&& o) noexcept : m(o.m), kind(o.kind), h(o.h), cheb(o.cheb), amg(o.amg), ainvPower(o.ainvPower), jsweep(o.jsweep) { o.h = nullptr; }
		~PreconditionerBase() { smm_hip_precond_destroy(h); }
		// non-zero on structural failure (missing / tiny diagonal, empty row, non-SPD pivot), like ref:1668-1693
		// (every init / apply / handle goes through m->device(): entries queued by updateEntry / addEntry / setValue reach the matrix's
		// mirror before the preconditioner is made or applied -- SGS reads A's values at every apply)
		int init() const noexcept {
			const smm_hip_csr* dev = m->device();
			if (!dev) return 1;
			if (h) return 0;
			if (kind == SMM_PRECOND_CHEBYSHEV) {
				return detail::note(smm_hip_precond_create_chebyshev(dev, cheb.degree, cheb.boundMode, cheb.eigRatio, cheb.powerSteps, cheb.lambdaMin, cheb.lambdaMax, &h)) == SMM_HIP_OK ? 0 : 1;
			}
			if (kind == SMM_PRECOND_AMG && amg.k > 0) {
				return detail::note(detail::Abi<T>::createAmgCandidates(dev, amg.candidates.data(), amg.k, amg.dofsPerNode, amg.theta, amg.maxLevels, amg.coarseRows,
				                                                        amg.smoothDegree, amg.eigRatio, &h)) == SMM_HIP_OK ? 0 : 1;
			}
			if (kind == SMM_PRECOND_AMG) {
				return detail::note(smm_hip_precond_create_amg(dev, amg.theta, amg.maxLevels, amg.coarseRows, amg.smoothDegree, amg.eigRatio, &h)) == SMM_HIP_OK ? 0 : 1;
			}
			if (kind == SMM_PRECOND_FSAI || kind == SMM_PRECOND_SPAI) {
				return detail::note(smm_hip_precond_create_ainv(dev, kind, ainvPower, &h)) == SMM_HIP_OK ? 0 : 1;
			}
			if (kind >= SMM_PRECOND_JSWEEP_SGS && kind <= SMM_PRECOND_JSWEEP_IC0) {
				return detail::note(smm_hip_precond_create_jsweep(dev, jsweep.baseKind, jsweep.lower, jsweep.upper, &h)) == SMM_HIP_OK ? 0 : 1;
			}
			return detail::note(smm_hip_precond_create(dev, kind, &h)) == SMM_HIP_OK ? 0 : 1;
		}
		int apply(const T* rhs, T* x) const noexcept {
			if (init()) return 1;
			return detail::note(detail::Abi<T>::apply(h, rhs, x)) == SMM_HIP_OK ? 0 : 1;
		}
		const smm_hip_precond* handle() const noexcept { return init() ? nullptr : h; }

	protected:
		PreconditionerBase(const CSRMatrix& m, int kind) noexcept : m(&m), kind(kind) {}
		const CSRMatrix* m;
		int kind;
		mutable smm_hip_precond* h = nullptr;
		struct ChebyshevParameters {  // what smm_hip_precond_create_chebyshev takes (kind CHEBYSHEV only); the defaults of smm_hip_precond_create
			int degree = 3, boundMode = SMM_CHEB_BOUND_GERSHGORIN;
			double eigRatio = 30.0;
			int powerSteps = 10;
			double lambdaMin = 0.0, lambdaMax = 0.0;
		} cheb;
		struct AMGParameters {  // what smm_hip_precond_create_amg takes (kind AMG only); the defaults of smm_hip_precond_create
			double theta = 0.08;
			int maxLevels = 10, coarseRows = 256, smoothDegree = 2;
			double eigRatio = 30.0;
			std::vector<T> candidates;  // k > 0: smm_hip_precond_create_amg_candidates_* with this n x k column-major block
			int k = 0, dofsPerNode = 1;
		} amg;
		int ainvPower = 1;  // what smm_hip_precond_create_ainv takes (kinds FSAI / SPAI only)
		struct JacobiSweepParameters {  // what smm_hip_precond_create_jsweep takes (kinds JSWEEP_* only); 0 steps: the default, 3
			int baseKind = SMM_PRECOND_ILU0, lower = 0, upper = 0;
		} jsweep;
	};
	class IDPreconditioner {  // ref:1166-1170
	public:
		int apply(const T*, T*) const noexcept { return 0; }
		const smm_hip_precond* handle() const noexcept { return nullptr; }
	};
	class SGSPreconditioner : public PreconditionerBase {  // ref:1173-1186
	public:
		SGSPreconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_SGS) {}
		SGSPreconditioner(SGSPreconditioner&&) noexcept = default;
	};
	class JacobiPreconditioner : public PreconditionerBase {  // addition
	public:
		JacobiPreconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_JACOBI) {}
		JacobiPreconditioner(JacobiPreconditioner&&) noexcept = default;
	};
	class ILU0Preconditioner : public PreconditionerBase {  // ref:1189-1212 (declared there, not usable)
	public:
		ILU0Preconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_ILU0) {}
		ILU0Preconditioner(ILU0Preconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
	};
	class IC0Preconditioner : public PreconditionerBase {  // ref:1216-1235
	public:
		IC0Preconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_IC0) {}
		IC0Preconditioner(IC0Preconditioner&&) noexcept = default;
	};
	// additions: ILU0 / SGS of the block-diagonal part of A (blocks of <= 1024 rows -- bricks of the grid when the matrix is a grid
	// stencil, runs of consecutive rows otherwise --, every block's sweeps cut to <= 16 dependent levels; smm_hip.h,
	// SMM_PRECOND_BLOCK_*, smm_hip_precond_create_block_ex for other sizes / cuts / partitions)
	class BlockILU0Preconditioner : public PreconditionerBase {
	public:
		BlockILU0Preconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_BLOCK_ILU0) {}
		BlockILU0Preconditioner(BlockILU0Preconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
	};
	class BlockSGSPreconditioner : public PreconditionerBase {
	public:
		BlockSGSPreconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, SMM_PRECOND_BLOCK_SGS) {}
		BlockSGSPreconditioner(BlockSGSPreconditioner&&) noexcept = default;
	};

	// addition: a Chebyshev polynomial in D^-1 A (smm_hip.h, SMM_PRECOND_CHEBYSHEV): SpMVs and element-wise passes only, symmetric positive
	// definite for such a matrix -- taken by ConjugateGradient, BiCGStab and GMRES.  boundMode: SMM_CHEB_BOUND_GERSHGORIN / _POWER (a heuristic,
	// not a bound) / _USER (lambdaMin, lambdaMax are the caller's).  One object serves one stream at a time (it owns its scratch vectors).
	// Any number of host threads may share it on that stream: an apply is enqueued whole.
	class ChebyshevPreconditioner : public PreconditionerBase {
	public:
		ChebyshevPreconditioner(const CSRMatrix& m, int degree = 3, int boundMode = SMM_CHEB_BOUND_GERSHGORIN, double eigRatio = 30.0, int powerSteps = 10,
		                        double lambdaMin = 0.0, double lambdaMax = 0.0) noexcept
		    : PreconditionerBase(m, SMM_PRECOND_CHEBYSHEV) {
			this->cheb.degree = degree;
			this->cheb.boundMode = boundMode;
			this->cheb.eigRatio = eigRatio;
			this->cheb.powerSteps = powerSteps;
			this->cheb.lambdaMin = lambdaMin;
			this->cheb.lambdaMax = lambdaMax;
		}
		ChebyshevPreconditioner(ChebyshevPreconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
		// degree, bound mode and bounds as the handle keeps them; non-zero when the preconditioner could not be made
		int info(int* degree, int* boundMode, double* lambdaMin, double* lambdaMax) const noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_chebyshev_info(this->h, degree, boundMode, lambdaMin, lambdaMax)) == SMM_HIP_OK ? 0 : 1;
		}
	};

	// addition: smoothed-aggregation multigrid with a symmetric V-cycle (smm_hip.h, SMM_PRECOND_AMG): the one kind whose iteration count does
	// not grow with the grid; symmetric positive definite for such a matrix -- taken by ConjugateGradient, BiCGStab and GMRES (matrices that
	// are not symmetric: the last two only).  A snapshot of the matrix's values: refresh() follows a value edit with the aggregates kept.
	// One object serves one stream at a time (it owns its level vectors).
	// Any number of host threads may share it on that stream: an apply is enqueued whole.
	class AMGPreconditioner : public PreconditionerBase {
	public:
		AMGPreconditioner(const CSRMatrix& m, double theta = 0.08, int maxLevels = 10, int coarseRows = 256, int smoothDegree = 2, double eigRatio = 30.0) noexcept
		    : PreconditionerBase(m, SMM_PRECOND_AMG) {
			this->amg.theta = theta;
			this->amg.maxLevels = maxLevels;
			this->amg.coarseRows = coarseRows;
			this->amg.smoothDegree = smoothDegree;
			this->amg.eigRatio = eigRatio;
		}
		// with near-null-space candidates (smm_hip.h, smm_hip_precond_create_amg_candidates_*): B is rows x k, COLUMN-MAJOR, 1 <= k <= 6, copied
		// here; dofsPerNode (1 .. 4) consecutive rows form a node.  For elasticity: the rigid body modes, 2 or 3 dofs per node.
		AMGPreconditioner(const CSRMatrix& m, const T* B, int k, int dofsPerNode, double theta = 0.08, int maxLevels = 10, int coarseRows = 256, int smoothDegree = 2,
		                  double eigRatio = 30.0)
		    : AMGPreconditioner(m, theta, maxLevels, coarseRows, smoothDegree, eigRatio) {
			this->amg.k = k;
			this->amg.dofsPerNode = dofsPerNode;
			if (B && k > 0) this->amg.candidates.assign(B, B + static_cast<size_t>(m.getDenseRowCount()) * static_cast<size_t>(k));
		}
		AMGPreconditioner(AMGPreconditioner&&) noexcept = default;
		// B_l of a level (rows_l x k column-major, the first `count` values; out may be null with count 0), k and the columns dropped there
		int candidates(int level, T* out, size_t count, int* k, int* dropped) const noexcept {
			if (this->init()) return 1;
			return detail::note(detail::Abi<T>::amgCandidates(this->h, level, out, count, k, dropped)) == SMM_HIP_OK ? 0 : 1;
		}
		int validate() noexcept { return this->init(); }
		// levels, rows / nnz of the first `count` levels (either may be null) and the operator complexity; non-zero when it could not be made
		int info(int* levels, int* rows, int* nnz, size_t count, double* operatorComplexity) const noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_amg_info(this->h, levels, rows, nnz, count, operatorComplexity)) == SMM_HIP_OK ? 0 : 1;
		}
		// the values again from the matrix's present values, aggregates and patterns kept
		int refresh() noexcept {
			if (this->init()) return 1;
			if (!this->m->device()) return 1;  // (queued entry edits reach the device first)
			return detail::note(smm_hip_precond_amg_refresh(this->h)) == SMM_HIP_OK ? 0 : 1;
		}
	};

	// addition: FSAI / SPAI (smm_hip.h, SMM_PRECOND_FSAI / SMM_PRECOND_SPAI): the preconditioner is a sparse matrix, an apply one or two SpMVs.
	// kind SMM_PRECOND_FSAI (symmetric positive definite matrices; taken by ConjugateGradient, BiCGStab and GMRES) or SMM_PRECOND_SPAI (general
	// matrices; BiCGStab and GMRES -- ConjugateGradient refuses it); power 1 .. SMM_AINV_MAX_POWER: the pattern is that of the power-th
	// structural power of the matrix.  A snapshot of the matrix's values: refresh() follows a value edit with every pattern kept.
	// One object serves one stream at a time (it owns the vector between its two SpMVs).
	// Any number of host threads may share it on that stream: an apply is enqueued whole.
	class ApproximateInversePreconditioner : public PreconditionerBase {
	public:
		ApproximateInversePreconditioner(const CSRMatrix& m, int kind = SMM_PRECOND_FSAI, int power = 1) noexcept : PreconditionerBase(m, kind) { this->ainvPower = power; }
		ApproximateInversePreconditioner(ApproximateInversePreconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
		int power() const noexcept { return this->ainvPower; }
		// the power, the longest row of the pattern and the entries of G / M (any may be null); non-zero when the preconditioner could not be made
		int info(int* power, int* maxRow, size_t* nnz) const noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_ainv_info(this->h, power, maxRow, nnz)) == SMM_HIP_OK ? 0 : 1;
		}
		// the values again from the matrix's present values, every pattern kept
		int refresh() noexcept {
			if (this->init()) return 1;
			if (!this->m->device()) return 1;  // (queued entry edits reach the device first)
			return detail::note(smm_hip_precond_ainv_refresh(this->h)) == SMM_HIP_OK ? 0 : 1;
		}
	};

	// addition: SGS / ILU0 / IC0 of the matrix renumbered colour by colour (smm_hip.h, SMM_PRECOND_MULTICOLOR_*): either sweep has as many
	// dependent levels as there are colours.  Base: SGSPreconditioner, ILU0Preconditioner or IC0Preconditioner; usable wherever Base is, and
	// MulticolorPreconditioner<SGSPreconditioner> in ConjugateGradient as well.  A snapshot of the matrix's values: refresh() follows a value
	// edit with the colouring kept.  One object serves one stream at a time (it owns the vector its sweeps work on).
	// Any number of host threads may share it on that stream: an apply is enqueued whole.
	template <typename Base>
	class MulticolorPreconditioner : public PreconditionerBase {
		static_assert(std::is_same<Base, SGSPreconditioner>::value || std::is_same<Base, ILU0Preconditioner>::value || std::is_same<Base, IC0Preconditioner>::value,
		              "MulticolorPreconditioner<Base>: Base is SGSPreconditioner, ILU0Preconditioner or IC0Preconditioner");
		static constexpr int kindOf() noexcept {
			return std::is_same<Base, SGSPreconditioner>::value ? SMM_PRECOND_MULTICOLOR_SGS
			       : std::is_same<Base, ILU0Preconditioner>::value ? SMM_PRECOND_MULTICOLOR_ILU0 : SMM_PRECOND_MULTICOLOR_IC0;
		}

	public:
		MulticolorPreconditioner(const CSRMatrix& m) noexcept : PreconditionerBase(m, kindOf()) {}
		MulticolorPreconditioner(MulticolorPreconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
		// the number of colours and the first `count` of the ncolors + 1 row bounds (either may be null); non-zero when it could not be made
		int info(int* ncolors, int* bounds, size_t count) const noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_multicolor_info(this->h, ncolors, bounds, count)) == SMM_HIP_OK ? 0 : 1;
		}
		// the permuted values and the factor again from the matrix's present values, colouring kept
		int refresh() noexcept {
			if (this->init()) return 1;
			if (!this->m->device()) return 1;  // (queued entry edits reach the device first)
			return detail::note(smm_hip_precond_multicolor_refresh(this->h)) == SMM_HIP_OK ? 0 : 1;
		}
	};

	// addition: the exact SGS / ILU0 / IC0 factor in the natural numbering with each triangular solve replaced by a fixed number of Jacobi
	// steps (smm_hip.h, SMM_PRECOND_JSWEEP_*): no dependent levels, an apply is sweepsLower + sweepsUpper launches shaped like an SpMV over
	// one triangle.  baseKind: SMM_PRECOND_SGS, _ILU0 or _IC0; steps 0 (the default, 3) or 1 .. SMM_JSWEEP_MAX_SWEEPS.  Usable wherever the
	// exact kind is (BiCGStab, GMRES: SGS and ILU0); ConjugateGradient takes IC0 and SGS with as many lower steps as upper ones.  With
	// steps >= levels - 1 (info) the apply is the exact kind's bit for bit.  A snapshot of the matrix's values, SGS included: refresh()
	// follows a value edit.  The iterates belong to the stream: one object serves any number of streams and host threads.
	class JacobiSweepPreconditioner : public PreconditionerBase {
		static constexpr int kindOf(int baseKind) noexcept {
			return baseKind == SMM_PRECOND_SGS ? SMM_PRECOND_JSWEEP_SGS : baseKind == SMM_PRECOND_IC0 ? SMM_PRECOND_JSWEEP_IC0 : SMM_PRECOND_JSWEEP_ILU0;
		}

	public:
		JacobiSweepPreconditioner(const CSRMatrix& m, int baseKind = SMM_PRECOND_ILU0, int sweepsLower = 0, int sweepsUpper = 0) noexcept
		    : PreconditionerBase(m, kindOf(baseKind)) {
			this->jsweep.baseKind = baseKind;  // (one that is none of the three is refused when the handle is made)
			this->jsweep.lower = sweepsLower;
			this->jsweep.upper = sweepsUpper;
		}
		JacobiSweepPreconditioner(JacobiSweepPreconditioner&&) noexcept = default;
		int validate() noexcept { return this->init(); }
		// the base kind, the step counts and the dependency levels of the two exact sweeps (any may be null); non-zero when it could not be made
		int info(int* baseKind, int* sweepsLower, int* sweepsUpper, int* levelsLower, int* levelsUpper) const noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_jsweep_info(this->h, baseKind, sweepsLower, sweepsUpper, levelsLower, levelsUpper)) == SMM_HIP_OK ? 0 : 1;
		}
		// other step counts (0: the default), no rebuild
		int setSweeps(int sweepsLower, int sweepsUpper) noexcept {
			if (this->init()) return 1;
			return detail::note(smm_hip_precond_jsweep_set_sweeps(this->h, sweepsLower, sweepsUpper)) == SMM_HIP_OK ? 0 : 1;
		}
		// the factor and the triangles' values again from the matrix's present values, pattern and split kept
		int refresh() noexcept {
			if (this->init()) return 1;
			if (!this->m->device()) return 1;  // (queued entry edits reach the device first)
			return detail::note(smm_hip_precond_jsweep_refresh(this->h)) == SMM_HIP_OK ? 0 : 1;
		}
	};

	CSRMatrix() noexcept = default;
	CSRMatrix(const TripletMatrix<T>& triplet) noexcept { init(triplet); }
	CSRMatrix(const CSRMatrix&) = delete;
	CSRMatrix& operator=(const CSRMatrix&) = delete;
	CSRMatrix(CSRMatrix&& o) noexcept { *this = std::move(o); }
	CSRMatrix& operator=(CSRMatrix&& o) noexcept {
		release();
		values = std::move(o.values);
		positions = std::move(o.positions);
		start = std::move(o.start);
		denseRowCount = o.denseRowCount;
		denseColCount = o.denseColCount;
		firstActiveStart = o.firstActiveStart;
		dev = o.dev;
		hostStale = o.hostStale;
		queued = std::move(o.queued);
		o.dev = nullptr;
		o.hostStale = false;
		return *this;
	}
	~CSRMatrix() { release(); }

	// ref:1326-1349 / 1606-1641: count per row, prefix sum, scatter in map order (row-major, columns ascending)
	int init(const TripletMatrix<T>& triplet) noexcept {
		release();
		denseRowCount = triplet.getDenseRowCount();
		denseColCount = triplet.getDenseColCount();
		const int nnz = triplet.getNonZeroCount();
		values.reset(new T[nnz > 0 ? nnz : 1]);
		positions.reset(new int[nnz > 0 ? nnz : 1]);
		start.reset(new int[denseRowCount + 1]());
		triplet.forEach([&](int r, int, T) { start[r + 1]++; });
		for (int i = 0; i < denseRowCount; ++i) start[i + 1] += start[i];
		int k = 0;
		triplet.forEach([&](int, int c, T v) {
			positions[k] = c;
			values[k] = v;
			++k;
		});
		computeFirstActive();
		return 0;
	}
	// addition: adopt raw CSR arrays (copied); columns must ascend inside each row
	int init(int rows, int cols, const int* startIn, const int* positionsIn, const T* valuesIn) noexcept {
		release();
		denseRowCount = rows;
		denseColCount = cols;
		const int nnz = startIn[rows];
		values.reset(new T[nnz > 0 ? nnz : 1]);
		positions.reset(new int[nnz > 0 ? nnz : 1]);
		start.reset(new int[rows + 1]);
		std::copy(startIn, startIn + rows + 1, start.get());
		std::copy(positionsIn, positionsIn + nnz, positions.get());
		std::copy(valuesIn, valuesIn + nnz, values.get());
		computeFirstActive();
		return 0;
	}
	// addition: the matrix of an AssemblyPlan's pairs with values[i] the contribution of pair i, assembled on the GPU (repeated pairs add up
	// in list order); the host arrays are filled from the device result, so iterators, getValue and the single-entry edits work as after
	// any other init.  Returns 0, or the SMM_HIP_* status (also in lastHipStatus()) with the matrix left empty.
	int init(const AssemblyPlan& plan, const T* valuesIn) noexcept {
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		if (!plan.valid()) return detail::note(plan.status() != SMM_HIP_OK ? plan.status() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(detail::Abi<T>::assembled(plan.handle(), valuesIn, &d)) != SMM_HIP_OK) return lastHipStatus();
		const int rows = plan.getDenseRowCount(), nnz = plan.getNonZeroCount();
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		int abi = smm_hip_assembly_pattern(plan.handle(), s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = plan.getDenseColCount();
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: this matrix becomes the transpose of `a`, built on the GPU through a's device mirror (smm_hip.h "the TRANSPOSE of a matrix":
	// row j holds column j's entries, source rows ascending; values bit for bit); the host arrays are filled from the device result as
	// init(plan, values) fills them, and the built handle becomes this matrix's mirror.  Returns 0, or the SMM_HIP_* status (also in
	// lastHipStatus()) with the matrix left empty.  SMM::transpose(a, out) is this call.
	int initTransposeOf(const CSRMatrix& a) noexcept {
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		const smm_hip_csr* src = a.device();
		if (!src) return detail::note(a.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_transpose_create(src, nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		const int rows = a.denseColCount, nnz = a.getNonZeroCount();
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		int abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = a.denseRowCount;
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: this matrix becomes P a Pᵀ, built on the GPU through a's device mirror (smm_hip.h "the SYMMETRIC PERMUTATION": row i is a's row
	// perm[i], entry (i, j) its (perm[i], perm[j]); columns ascend, values bit for bit); perm holds a's row count of entries.  The host arrays
	// are filled from the device result and the built handle becomes this matrix's mirror.  Returns 0, or the SMM_HIP_* status (also in
	// lastHipStatus()) with the matrix left empty: SMM_HIP_ERR_INVALID when perm is no permutation.  SMM::permute(a, perm, out) is this call.
	int initPermuteOf(const CSRMatrix& a, const int* perm) noexcept {
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		const smm_hip_csr* src = a.device();
		if (!src) return detail::note(a.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_permute_create(src, perm, static_cast<size_t>(a.denseRowCount), nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		const int rows = a.denseRowCount, nnz = a.getNonZeroCount();
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		int abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = a.denseColCount;
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: a matrix made by initPermuteOf takes over the present values of `a` (its source, or a matrix with that pattern) in one gather
	// pass on the GPU; the host values follow.  Returns 0, or the SMM_HIP_* status with this matrix unchanged.  SMM::permuteRefresh is this call.
	int permuteRefresh(const CSRMatrix& a) noexcept {
		const smm_hip_csr* src = a.device();
		if (!src || !device()) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		int abi = detail::Abi<T>::permuteRefresh(dev, src);
		if (abi == SMM_HIP_OK) abi = smm_hip_stream_synchronize(nullptr);
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(dev, values.get());
		return detail::note(abi);
	}
	// addition: this matrix becomes `a` in THIS matrix's precision, converted on the GPU through a's device mirror (smm_hip.h "a matrix in the
	// OTHER PRECISION": double -> float rounds to nearest even, float -> double is exact, underflow is allowed); the host arrays are filled
	// from the device result and the built handle becomes this matrix's mirror.  Returns 0, or the SMM_HIP_* status (also in lastHipStatus())
	// with the matrix left empty: SMM_HIP_ERR_INVALID for a finite value outside float's range.  SMM::convert<U>(a) is this call.
	template <typename S>
	int initConvertOf(const CSRMatrix<S>& a) noexcept {
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		const smm_hip_csr* src = a.device();
		if (!src) return detail::note(a.rawStart() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_convert_create(src, std::is_same<T, float>::value ? SMM_DTYPE_F32 : SMM_DTYPE_F64, nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		const int rows = a.getDenseRowCount(), nnz = a.getNonZeroCount();
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		int abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = a.getDenseColCount();
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: this matrix becomes the product a b, built on the GPU through the two device mirrors (smm_hip.h "the PRODUCT C = A B": the
	// structural product, columns ascending, every entry the row sum of rMult in a's stored order); the host arrays are filled from the
	// device result and the built handle becomes this matrix's mirror.  Returns 0, or the SMM_HIP_* status (also in lastHipStatus()) with
	// the matrix left empty.  a and b may be one matrix; neither may be this one.  SMM::multiply(a, b, out) is this call.
	int initProductOf(const CSRMatrix& a, const CSRMatrix& b) noexcept {
		if (&a == this || &b == this) return detail::note(SMM_HIP_ERR_INVALID);
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		const smm_hip_csr* da = a.device();
		if (!da) return detail::note(a.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const smm_hip_csr* db = b.device();
		if (!db) return detail::note(b.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_multiply_create(da, db, nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		int rows = 0, cols = 0, nnz = 0;
		int abi = smm_hip_csr_info(d, &rows, &cols, &nnz, nullptr, nullptr);
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		if (abi == SMM_HIP_OK) abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = cols;
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: the numeric phase alone -- this matrix's values become those of a b on ITS pattern (+0.0 where no product lands), a bulk
	// edit on the device like operator*=.  Non-zero (the SMM_HIP_* status, nothing changed): a product falls on an entry this matrix does
	// not store, the shapes do not fit, a or b is this matrix, no GPU.  SMM::multiplyInto(c, a, b) is this call.
	int multiplyInto(const CSRMatrix& a, const CSRMatrix& b) {
		if (&a == this || &b == this) return detail::note(SMM_HIP_ERR_INVALID);
		(void)device();
		if (!flushedMirror()) return detail::note(start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const smm_hip_csr* da = a.device();
		const smm_hip_csr* db = b.device();
		if (!da || !db) return detail::note((a.start && b.start) ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::multiplyInto(dev, da, db);
		deviceEdited(abi);
		return abi;
	}
	// addition: this matrix becomes the sum alpha a + beta b of two matrices with ANY two patterns, built on the GPU through the two device
	// mirrors (smm_hip.h "the SUM C = alpha A + beta B": the union of the patterns, columns ascending, u = alpha a, v = beta b, the entry
	// u + v, u or v); the host arrays are filled from the device result and the built handle becomes this matrix's mirror.  Returns 0, or
	// the SMM_HIP_* status (also in lastHipStatus()) with the matrix left empty.  a and b may be one matrix; neither may be this one (use
	// addInto for that).  SMM::add(a, alpha, b, beta, out) is this call.
	int initSumOf(const CSRMatrix& a, T alpha, const CSRMatrix& b, T beta) noexcept {
		if (&a == this || &b == this) return detail::note(SMM_HIP_ERR_INVALID);
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
		const smm_hip_csr* da = a.device();
		if (!da) return detail::note(a.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const smm_hip_csr* db = b.device();
		if (!db) return detail::note(b.start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(detail::Abi<T>::addCreate(da, alpha, db, beta, &d)) != SMM_HIP_OK) return lastHipStatus();
		int rows = 0, cols = 0, nnz = 0;
		int abi = smm_hip_csr_info(d, &rows, &cols, &nnz, nullptr, nullptr);
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		if (abi == SMM_HIP_OK) abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = cols;
		computeFirstActive();
		dev = d;
		return 0;
	}
	// addition: the numeric phase alone -- this matrix's values become those of alpha a + beta b on ITS pattern (+0.0 where neither stores an
	// entry), a bulk edit on the device like operator*=.  Unlike multiplyInto, a or b (or both) MAY BE THIS MATRIX: A.addInto(A, 1, D, sigma)
	// is the shift A <- A + sigma D in place.  Non-zero (the SMM_HIP_* status, nothing changed): a or b stores an entry this matrix does
	// not, the shapes do not fit, no GPU.  SMM::addInto(c, a, alpha, b, beta) is this call.
	int addInto(const CSRMatrix& a, T alpha, const CSRMatrix& b, T beta) {
		(void)device();
		if (!flushedMirror()) return detail::note(start ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const smm_hip_csr* da = a.device();
		const smm_hip_csr* db = b.device();
		if (!da || !db) return detail::note((a.start && b.start) ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::addInto(dev, da, alpha, db, beta);
		deviceEdited(abi);
		return abi;
	}
	// additions: composing and slicing on the GPU through the device mirrors (smm_hip.h "COMPOSING and SLICING matrices").  The created
	// matrices fill their host arrays from the device result and keep the built handle as their mirror, as initSumOf does; each returns 0,
	// or the SMM_HIP_* status (also in lastHipStatus()) with the matrix left empty (creates) or unchanged (refreshes, scaleRowsCols).
	// An operand without a mirror (no GPU, or left empty by a call that failed) answers the status of that failure, SMM_HIP_ERR_INVALID if none.
	// initBlockOf: this matrix becomes the block matrix of the row-major p x q table `blocks` (nullptr: a zero block; p q <= 64; one matrix
	// may fill several slots, none may be this one); coef nullptr or p q scalars (coef * v, one rounding; 1 copies the bits); rowSizes /
	// colSizes nullptr, or the heights / widths for block rows / columns of nullptr alone (< 0 elsewhere).  SMM::blockMatrix is this call.
	int initBlockOf(int p, int q, const CSRMatrix* const* blocks, const T* coef = nullptr, const int* rowSizes = nullptr, const int* colSizes = nullptr) noexcept {
		std::vector<const smm_hip_csr*> table;
		const int st = blockTable(p, q, blocks, table);
		if (st != SMM_HIP_OK) return detail::note(st);
		clearAll();
		smm_hip_csr* d = nullptr;
		if (detail::note(detail::Abi<T>::blockCreate(p, q, table.data(), coef, rowSizes, colSizes, &d)) != SMM_HIP_OK) return lastHipStatus();
		return adoptBuilt(d);
	}
	// the numeric phase alone into the pattern initBlockOf made, from the blocks' present values (the same table: that the patterns are
	// those of then is the caller's contract); a bulk edit on the device like operator*=.  SMM::blockRefresh is this call.
	int blockRefresh(int p, int q, const CSRMatrix* const* blocks, const T* coef = nullptr) {
		std::vector<const smm_hip_csr*> table;
		const int st = blockTable(p, q, blocks, table);
		if (st != SMM_HIP_OK) return detail::note(st);
		(void)device();
		if (!flushedMirror()) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::blockRefresh(dev, p, q, table.data(), coef);
		deviceEdited(abi);
		return abi;
	}
	// initSubmatrixOf: this matrix becomes the rows rows[0 .. nr) of `a` (any order, repeats allowed; nullptr: all) restricted to the columns
	// cols[0 .. nc) (strictly ascending; nullptr: all), renumbered; values bit for bit.  SMM::submatrix is this call.
	int initSubmatrixOf(const CSRMatrix& a, const int* rows, size_t nr, const int* cols, size_t nc) noexcept {
		if (&a == this) return detail::note(SMM_HIP_ERR_INVALID);
		clearAll();
		const smm_hip_csr* src = a.device();
		if (!src) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_submatrix_create(src, rows, nr, cols, nc, nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		return adoptBuilt(d);
	}
	// ... the rows [r0, r1) and the columns [c0, c1) of `a`
	int initSubmatrixOf(const CSRMatrix& a, int r0, int r1, int c0, int c1) noexcept {
		if (&a == this) return detail::note(SMM_HIP_ERR_INVALID);
		clearAll();
		const smm_hip_csr* src = a.device();
		if (!src) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		smm_hip_csr* d = nullptr;
		if (detail::note(smm_hip_csr_submatrix_range_create(src, r0, r1, c0, c1, nullptr, &d)) != SMM_HIP_OK) return lastHipStatus();
		return adoptBuilt(d);
	}
	// a matrix made by initSubmatrixOf takes over the present values of `a` (its source, or a matrix with that pattern) in one gather pass on
	// the GPU; the host values follow.  SMM::submatrixRefresh is this call.
	int submatrixRefresh(const CSRMatrix& a) {
		const smm_hip_csr* src = a.device();
		(void)device();
		if (!src || !flushedMirror()) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::submatrixRefresh(dev, src);
		deviceEdited(abi);
		return abi;
	}
	// out[i] = a_ii for i < min(rows, cols), 0 where no diagonal entry is stored; *missing (may be null) counts those.  SMM::diagonal is this call.
	int diagonal(T* out, int* missing = nullptr) const noexcept {
		const smm_hip_csr* d = device();
		if (!d) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		return detail::note(detail::Abi<T>::diagonal(d, out, missing));
	}
	// v_ij <- (r_i v_ij) c_j on the GPU, two roundings in this order; r has getDenseRowCount() elements, c getDenseColCount(); nullptr skips
	// the factor.  A bulk edit on the device like operator*=.
	int scaleRowsCols(const T* r, const T* c) {
		(void)device();
		if (!flushedMirror()) return detail::note(lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::scaleRowsCols(dev, r, c);
		deviceEdited(abi);
		return abi;
	}
	// addition: new values for a matrix made by init(plan, ...) from the same plan -- those of init(plan, valuesIn), or added to the present
	// ones (add) -- in one device pass; the pattern and what the library derived from it stay.  Non-zero (the SMM_HIP_* status): not this
	// plan's matrix, no GPU; nothing changed then.
	int assemble(const AssemblyPlan& plan, const T* valuesIn, bool add = false) {
		if (!plan.valid() || !flushedMirror()) return detail::note(SMM_HIP_ERR_INVALID);
		const int abi = detail::Abi<T>::refill(plan.handle(), dev, valuesIn, add ? SMM_UPDATE_ADD : SMM_UPDATE_SET);
		deviceEdited(abi);
		return abi;
	}
	int getNonZeroCount() const noexcept { return start ? start[denseRowCount] : 0; }
	int getDenseRowCount() const noexcept { return denseRowCount; }
	int getDenseColCount() const noexcept { return denseColCount; }
	Iterator begin() noexcept {
		refreshHost();
		return Iterator(this, 0, 0);
	}
	Iterator end() noexcept { return Iterator(this, denseRowCount, getNonZeroCount()); }
	ConstIterator begin() const noexcept { return cbegin(); }
	ConstIterator end() const noexcept { return cend(); }
	ConstIterator cbegin() const noexcept {
		refreshHost();
		return ConstIterator(this, 0, 0);
	}
	ConstIterator cend() const noexcept { return ConstIterator(this, denseRowCount, getNonZeroCount()); }
	// ref:1428-1456: rowEnd(i) of an empty row is rowBegin(i)
	RowIterator rowBegin(const int i) noexcept {
		refreshHost();
		return RowIterator(this, i, start[i]);
	}
	RowIterator rowEnd(const int i) noexcept { return start[i] == start[i + 1] ? rowBegin(i) : RowIterator(this, i + 1, start[i + 1]); }
	ConstRowIterator rowBegin(const int i) const noexcept { return crowBegin(i); }
	ConstRowIterator rowEnd(const int i) const noexcept { return crowEnd(i); }
	ConstRowIterator crowBegin(const int i) const noexcept {
		refreshHost();
		return ConstRowIterator(this, i, start[i]);
	}
	ConstRowIterator crowEnd(const int i) const noexcept { return start[i] == start[i + 1] ? crowBegin(i) : ConstRowIterator(this, i + 1, start[i + 1]); }
	T getValue(int row, int col) const noexcept {
		const int k = indexOf(row, col);
		if (k < 0) return T(0);
		refreshHost();
		return values[k];
	}

	// ---- Editing the values (ref:1366-1385, 1525-1604); the pattern never changes ----
	// No device mirror yet: the edit is made on the host only, as in the reference (no GPU needed).  With a mirror (any hot-path call made
	// one): operator*=, inplaceAdd / inplaceSubtract and zeroValues run on the GPU (libsmm_hip.so) and leave the host copy stale -- the next
	// host read (getValue, iterators, rawValues, or inplaceAdd reading `other`) refreshes it with one device-to-host copy; updateEntry /
	// addEntry / setValue write the host copy and queue the entry, and the queue goes to the GPU as ONE batched update before the next
	// hot-path call (rMult*, the solvers, device(), a preconditioner's init / apply).  Preconditioners made before an edit: SGS applies
	// the edited A, ILU0 / IC0 / JACOBI / BLOCK_* keep their factors (smm_hip.h).  Not while another thread uses the matrix.
	bool hasSameNonZeroPattern(const CSRMatrix& other) const noexcept {
		if (denseRowCount != other.denseRowCount || denseColCount != other.denseColCount) return false;
		const int nnz = getNonZeroCount();
		if (nnz != other.getNonZeroCount()) return false;
		if (nnz == 0) return true;
		return std::equal(start.get(), start.get() + denseRowCount + 1, other.start.get()) && std::equal(positions.get(), positions.get() + nnz, other.positions.get());
	}
	void operator*=(const T scalar) {
		if (!flushedMirror()) {
			const int nnz = getNonZeroCount();
			for (int i = 0; i < nnz; ++i) values[i] *= scalar;
			return;
		}
		deviceEdited(detail::Abi<T>::scale(dev, scalar));
	}
	void inplaceAdd(const CSRMatrix& other) { addScaled(other, T(1)); }
	void inplaceSubtract(const CSRMatrix& other) { addScaled(other, T(-1)); }
	bool updateEntry(const int row, const int col, const T newValue) {
		const int k = indexOf(row, col);
		if (k < 0) return false;
		setValueAt(row, k, newValue);
		return true;
	}
	bool addEntry(const int row, const int col, const T value) {
		const int k = indexOf(row, col);
		if (k < 0) return false;
		refreshHost();
		setValueAt(row, k, values[k] + value);
		return true;
	}
	void zeroValues() {
		if (!flushedMirror()) {
			std::fill_n(values.get(), getNonZeroCount(), T(0));
			return;
		}
		deviceEdited(detail::Abi<T>::zero(dev));
	}

	// ---- the hot path: out = op(lhs, A * mult) on the GPU (ref:1458-1515) ----
	void rMult(const T* const mult, T* const res) const noexcept { spmv(SMM_OP_ASSIGN, nullptr, mult, res); }
	void rMultAdd(const T* const lhs, const T* const mult, T* const out) const noexcept { spmv(SMM_OP_ADD, lhs, mult, out); }
	void rMultSub(const T* const lhs, const T* const mult, T* const out) const noexcept { spmv(SMM_OP_SUB, lhs, mult, out); }
	// additions with no counterpart in the reference: k right-hand sides at once (1 <= k <= SMM_HIP_MAX_RHS).  X is an interleaved block of
	// getDenseColCount() x k elements, Lhs / Out of getDenseRowCount() x k: element (i, j) at i * k + j.  The matrix is streamed once for all k
	// columns; column j of Out is what rMult / rMultAdd / rMultSub give for column j alone (smm_hip.h "CSR SpMM").  Out may be Lhs, not X.
	void rMult(const T* const X, T* const Out, const int k) const noexcept { spmm(SMM_OP_ASSIGN, k, nullptr, X, Out); }
	void rMultAdd(const T* const Lhs, const T* const X, T* const Out, const int k) const noexcept { spmm(SMM_OP_ADD, k, Lhs, X, Out); }
	void rMultSub(const T* const Lhs, const T* const X, T* const Out, const int k) const noexcept { spmm(SMM_OP_SUB, k, Lhs, X, Out); }

	// ref:1643-1651.  WHAT THE KINDS COST ON THE GPU (measured, MI355X, BiCGStab to 1e-8 on the 1.26 M-row convection-diffusion problem of
	// BASELINE config 5; INTEGRATION.md "What a preconditioner costs"): the reference's own kind, SYMMETRIC_GAUS_SEIDEL, and ILU0 are EXACT
	// triangular sweeps -- bit-identical to the sequential loops (ref:1658-1713), and bound by one memory-fabric round trip per dependency
	// level: 79 / 67 iterations but ~200 / ~167 ms, against ~23 ms for 321 iterations with NONE.  They are kept because they are the
	// reference's semantics, not because they are fast.  The kinds that WIN on a GPU are BLOCK_ILU0 / BLOCK_SGS (the same algorithms on
	// the block-diagonal part of A, one wavefront per block: ~18 ms, 105 iterations, create included) and JACOBI (folded into the SpMV
	// rows: the price of NONE).  A caller of getPreconditioner<SYMMETRIC_GAUS_SEIDEL>() (test/cpp/bicgstab.cpp:160-162) gets the slow,
	// exact one -- switching to BLOCK_SGS is a one-word change, but a different preconditioner (different iteration counts).
	template <SolverPreconditioner precond>
	decltype(auto) getPreconditioner() const noexcept {
		if constexpr (precond == SolverPreconditioner::NONE) {
			return IDPreconditioner();
		} else if constexpr (precond == SolverPreconditioner::SYMMETRIC_GAUS_SEIDEL) {
			return SGSPreconditioner(*this);
		} else if constexpr (precond == SolverPreconditioner::ILU0) {
			return ILU0Preconditioner(*this);
		} else if constexpr (precond == SolverPreconditioner::BLOCK_ILU0) {
			return BlockILU0Preconditioner(*this);
		} else if constexpr (precond == SolverPreconditioner::BLOCK_SGS) {
			return BlockSGSPreconditioner(*this);
		} else if constexpr (precond == SolverPreconditioner::CHEBYSHEV) {
			return ChebyshevPreconditioner(*this);  // degree 3, Gershgorin bound, ratio 30
		} else if constexpr (precond == SolverPreconditioner::AMG) {
			return AMGPreconditioner(*this);  // theta 0.08, 10 levels, 256 coarse rows, degree-2 smoother, ratio 30
		} else {
			return JacobiPreconditioner(*this);
		}
	}

	// the Chebyshev preconditioner with chosen parameters (the arguments of smm_hip_precond_create_chebyshev)
	ChebyshevPreconditioner getChebyshevPreconditioner(int degree = 3, int boundMode = SMM_CHEB_BOUND_GERSHGORIN, double eigRatio = 30.0, int powerSteps = 10,
	                                                   double lambdaMin = 0.0, double lambdaMax = 0.0) const noexcept {
		return ChebyshevPreconditioner(*this, degree, boundMode, eigRatio, powerSteps, lambdaMin, lambdaMax);
	}

	// the multigrid preconditioner with chosen parameters (the arguments of smm_hip_precond_create_amg)
	AMGPreconditioner getAMGPreconditioner(double theta = 0.08, int maxLevels = 10, int coarseRows = 256, int smoothDegree = 2, double eigRatio = 30.0) const noexcept {
		return AMGPreconditioner(*this, theta, maxLevels, coarseRows, smoothDegree, eigRatio);
	}
	// ... with near-null-space candidates: B is getDenseRowCount() x k column-major, dofsPerNode consecutive rows form a node
	AMGPreconditioner getAMGPreconditioner(const T* B, int k, int dofsPerNode, double theta = 0.08, int maxLevels = 10, int coarseRows = 256, int smoothDegree = 2,
	                                       double eigRatio = 30.0) const {
		return AMGPreconditioner(*this, B, k, dofsPerNode, theta, maxLevels, coarseRows, smoothDegree, eigRatio);
	}

	// addition: ||A||_2, the largest singular value -- SMM::svds with k = 1 and no vectors (needs min(rows, cols) >= 3).  tol as in SMM::svds.
	// A NaN when the solve does not report SUCCESS or the call failed (lastHipStatus() says why).
	T norm2(T tol = T(1e-6)) const noexcept {
		const smm_hip_csr* d = device();
		T sigma = T(0);
		int st = 0;
		const int rc = d ? detail::note(detail::Abi<T>::svds(d, nullptr, 1, 0, 300, tol, nullptr, 0ull, &sigma, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &st))
		                 : detail::note(SMM_HIP_ERR_NO_DEVICE);
		return rc == SMM_HIP_OK && st == 0 ? sigma : std::numeric_limits<T>::quiet_NaN();
	}

	// device mirror of the three arrays, created on first use; nullptr when there is no GPU
	// (entries queued by updateEntry / addEntry / setValue are sent first, as one batched update)
	const smm_hip_csr* device() const noexcept {
		std::lock_guard<std::mutex> lock(detail::editMutex());
		if (!dev && start) {
			if (detail::note(detail::Abi<T>::create(denseRowCount, denseColCount, start.get(), positions.get(), values.get(), &dev)) != SMM_HIP_OK) dev = nullptr;
			queued.clear();
		}
		if (dev && !queued.empty()) flushLocked();
		return dev;
	}
	// Tuning only (results unchanged): SpMV kernel family and lanes per row for this matrix, e.g. SMM_SPMV_PATTERN for stencil /
	// banded matrices.  Returns the ABI status: non-zero when the matrix does not qualify (the previous choice stays).
	int setSpmvKernel(const int family, const int lanesPerRow = 0) const noexcept {
		(void)device();
		return dev ? smm_hip_csr_set_kernel(dev, family, lanesPerRow) : SMM_HIP_ERR_NO_DEVICE;
	}
	// The BLOCKS family (SMM_SPMV_BLOCKS: one column index per dense b x b block, b = 2, 3, 4).  findBlocks analyses the matrix on the
	// device -- blockSize 0 tries 4, 3, 2 -- and returns the size kept, 0 when the matrix does not fit, a negative number on an error
	// (lastHipStatus() holds the status); setSpmvKernel(SMM_SPMV_BLOCKS) then selects the family.  blocksInfo reports the kept analysis
	// (0 / 0 / 0 without one); any argument may be null.
	int findBlocks(const int blockSize = 0) const noexcept {
		(void)device();
		int found = 0;
		const int st = dev ? smm_hip_csr_find_blocks(dev, blockSize, &found) : static_cast<int>(SMM_HIP_ERR_NO_DEVICE);
		return detail::note(st) == SMM_HIP_OK ? found : -1;
	}
	int blocksInfo(int* blockSize, long long* blocks, int* maxRowEntries) const noexcept {
		(void)device();
		return dev ? smm_hip_csr_blocks_info(dev, blockSize, blocks, maxRowEntries) : SMM_HIP_ERR_NO_DEVICE;
	}
	// The LONGROWS family (SMM_SPMV_LONGROWS: rows of more than splitLen entries are cut into segments of segmentLen that the whole device
	// sums; smm_hip.h states the order and the legal lengths).  configureLongRows sets the two lengths (0 = the default; it replaces a kept
	// analysis) and returns the ABI status; setSpmvKernel(SMM_SPMV_LONGROWS) selects the family and runs the analysis if none is kept.
	// longRowsInfo reports the kept analysis (0 / 0 / 0 / 0 without one); any argument may be null.
	int configureLongRows(const int splitLen = 0, const int segmentLen = 0) const noexcept {
		(void)device();
		return detail::note(dev ? smm_hip_csr_longrows_configure(dev, splitLen, segmentLen) : static_cast<int>(SMM_HIP_ERR_NO_DEVICE));
	}
	int longRowsInfo(int* splitLen, int* segmentLen, int* longRows, long long* segments) const noexcept {
		(void)device();
		return dev ? smm_hip_csr_longrows_info(dev, splitLen, segmentLen, longRows, segments) : SMM_HIP_ERR_NO_DEVICE;
	}
	// call after editing values/positions in place through the raw accessors below
	void invalidateDevice() noexcept {
		refreshHost();  // (a device-side edit not yet copied back would be lost with the mirror)
		smm_hip_csr_destroy(dev);
		dev = nullptr;
		hostStale = false;
		queued.clear();
	}
	const T* rawValues() const noexcept {
		refreshHost();
		return values.get();
	}
	const int* rawPositions() const noexcept { return positions.get(); }
	const int* rawStart() const noexcept { return start.get(); }

private:
	void spmv(int op, const T* lhs, const T* mult, T* out) const noexcept {
		const smm_hip_csr* d = device();  // a failed mirror has already noted its status
		if (!d || detail::note(detail::Abi<T>::spmv(d, op, lhs, mult, out)) != SMM_HIP_OK) detail::fillNaN(out, denseRowCount);
	}
	void spmm(int op, int k, const T* lhs, const T* mult, T* out) const noexcept {
		const smm_hip_csr* d = device();
		if (!d || detail::note(detail::Abi<T>::spmm(d, op, k, lhs, mult, out)) != SMM_HIP_OK) {
			detail::fillNaN(out, k >= 1 && k <= SMM_HIP_MAX_RHS ? denseRowCount * k : 0);  // (a k out of range says nothing about out's size)
		}
	}
	void clearAll() noexcept {
		release();
		values.reset();
		positions.reset();
		start.reset();
		denseRowCount = denseColCount = firstActiveStart = 0;
	}
	// the device mirrors of a p x q table of matrices (nullptr stays nullptr); non-zero: a bad table, this matrix inside it, or a failed mirror
	int blockTable(int p, int q, const CSRMatrix* const* blocks, std::vector<const smm_hip_csr*>& table) const noexcept {
		if (p < 1 || q < 1 || static_cast<long long>(p) * q > 64 || !blocks) return SMM_HIP_ERR_INVALID;
		table.assign(static_cast<size_t>(p) * q, nullptr);
		for (int k = 0; k < p * q; ++k) {
			if (!blocks[k]) continue;
			if (blocks[k] == this) return SMM_HIP_ERR_INVALID;
			table[k] = blocks[k]->device();
			if (!table[k]) return lastHipStatus() ? lastHipStatus() : SMM_HIP_ERR_INVALID;
		}
		return SMM_HIP_OK;
	}
	// this (empty) matrix takes the built handle `d` as its mirror and fills its host arrays from it; on a failure `d` is destroyed
	int adoptBuilt(smm_hip_csr* d) noexcept {
		int rows = 0, cols = 0, nnz = 0;
		int abi = smm_hip_csr_info(d, &rows, &cols, &nnz, nullptr, nullptr);
		std::unique_ptr<T[]> v(new T[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> p(new int[nnz > 0 ? nnz : 1]);
		std::unique_ptr<int[]> s(new int[rows + 1]());
		if (abi == SMM_HIP_OK) abi = smm_hip_csr_get_pattern(d, s.get(), p.get());
		if (abi == SMM_HIP_OK) abi = detail::Abi<T>::getValues(d, v.get());
		if (detail::note(abi) != SMM_HIP_OK) {
			smm_hip_csr_destroy(d);
			return abi;
		}
		values = std::move(v);
		positions = std::move(p);
		start = std::move(s);
		denseRowCount = rows;
		denseColCount = cols;
		computeFirstActive();
		dev = d;
		return 0;
	}
	void computeFirstActive() noexcept {  // ref:1619-1628
		firstActiveStart = denseRowCount;
		for (int i = 0; i < denseRowCount; ++i) {
			if (start[i + 1] != 0) {
				firstActiveStart = i;
				break;
			}
		}
	}
	void release() noexcept {
		smm_hip_csr_destroy(dev);
		dev = nullptr;
		hostStale = false;
		queued.clear();
	}
	int indexOf(int row, int col) const noexcept {  // ref:1551-1570 (out-of-range: not stored)
		if (!start || row < 0 || row >= denseRowCount || col < 0 || col >= denseColCount) return -1;
		const int* b = positions.get() + start[row];
		const int* e = positions.get() + start[row + 1];
		const int* it = std::lower_bound(b, e, col);
		return it != e && *it == col ? static_cast<int>(it - positions.get()) : -1;
	}
	// the host copy after a device-side bulk edit: one device-to-host copy
	void refreshHost() const noexcept {
		std::lock_guard<std::mutex> lock(detail::editMutex());
		if (!hostStale || !dev) return;
		if (detail::note(detail::Abi<T>::getValues(dev, values.get())) == SMM_HIP_OK) hostStale = false;
	}
	void setValueAt(int row, int k, T v) {
		refreshHost();
		values[k] = v;
		std::lock_guard<std::mutex> lock(detail::editMutex());
		if (dev) queued.push_back({row, positions[k], v});
	}
	// the mirror, with every queued entry on it; false when there is none (the edit stays on the host)
	bool flushedMirror() {
		std::lock_guard<std::mutex> lock(detail::editMutex());
		if (!dev) return false;
		if (!queued.empty()) flushLocked();
		return true;
	}
	void flushLocked() const noexcept {
		std::vector<int> r(queued.size()), c(queued.size());
		std::vector<T> v(queued.size());
		for (size_t i = 0; i < queued.size(); ++i) {
			r[i] = queued[i].row;
			c[i] = queued[i].col;
			v[i] = queued[i].value;
		}
		if (detail::note(detail::Abi<T>::update(dev, static_cast<int>(r.size()), r.data(), c.data(), v.data())) == SMM_HIP_OK) queued.clear();
	}
	void addScaled(const CSRMatrix& other, T alpha) {
		if (flushedMirror()) {
			const smm_hip_csr* o = other.device();  // (a failed mirror has noted its status; a matrix never initialised has none)
			deviceEdited(o ? detail::Abi<T>::axpy(dev, alpha, o) : (other.start ? lastHipStatus() : SMM_HIP_ERR_INVALID));
			return;
		}
		other.refreshHost();
		const int nnz = getNonZeroCount();
		for (int i = 0; i < nnz; ++i) values[i] = alpha == T(1) ? values[i] + other.values[i] : values[i] - other.values[i];
	}
	// after a device-side bulk edit: the host copy is stale once the edit has run (a failed call leaves the device values, and so the
	// host copy, as they were; its status is in lastHipStatus())
	void deviceEdited(int abi) {
		if (detail::note(abi) != SMM_HIP_OK) return;
		{
			std::lock_guard<std::mutex> lock(detail::editMutex());
			hostStale = true;
		}
		detail::note(smm_hip_stream_synchronize(nullptr));
	}
	struct Queued {
		int row, col;
		T value;
	};
	// the reference's layout (ref:1243-1259)
	std::unique_ptr<T[]> values;
	std::unique_ptr<int[]> positions;
	std::unique_ptr<int[]> start;
	int denseRowCount = 0;
	int denseColCount = 0;
	int firstActiveStart = 0;
	mutable smm_hip_csr* dev = nullptr;
	mutable bool hostStale = false;      // a device-side bulk edit has not been copied back yet
	mutable std::vector<Queued> queued;  // single-entry edits not yet sent to the mirror
};

// ---- solvers ---------------------------------------------------------------------------------------------------------------
namespace detail {
inline SolverStatus toStatus(int abi, int solver) {
	// no GPU / HIP failure: DIVERGED, with lastHipStatus() != 0 (a numerical DIVERGED leaves it 0) and the text in smm_hip_last_error()
	if (note(abi) != SMM_HIP_OK) return SolverStatus::DIVERGED;
	return static_cast<SolverStatus>(solver);
}
template <typename T>
struct Functor;
template <>
struct Functor<float> {
	static int run(const smm_hip_csr* a, float* b, float* x, int it, float eps, smm_hip_apply_fn_f32 fn, void* user, int* st) {
		return smm_hip_bicgstab_functor_f32(a, b, x, it, eps, fn, user, st, nullptr, nullptr);
	}
};
template <>
struct Functor<double> {
	static int run(const smm_hip_csr* a, double* b, double* x, int it, double eps, smm_hip_apply_fn_f64 fn, void* user, int* st) {
		return smm_hip_bicgstab_functor_f64(a, b, x, it, eps, fn, user, st, nullptr, nullptr);
	}
};
}  // namespace detail

// ref:2316-2398
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const int rc = d ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, nullptr, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ref:2414-2505
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::IC0Preconditioner& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// addition: the same preconditioned loop with the Chebyshev polynomial preconditioner (symmetric positive definite for such a matrix)
template <typename T>
using ChebyshevPreconditioner = typename CSRMatrix<T>::ChebyshevPreconditioner;
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::ChebyshevPreconditioner& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// addition: ... and with the multigrid V-cycle
template <typename T>
using AMGPreconditioner = typename CSRMatrix<T>::AMGPreconditioner;
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::AMGPreconditioner& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// addition: ... and with the factored approximate inverse (kind SMM_PRECOND_FSAI; SMM_PRECOND_SPAI is refused: DIVERGED, lastHipStatus() != 0)
template <typename T>
using ApproximateInversePreconditioner = typename CSRMatrix<T>::ApproximateInversePreconditioner;
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::ApproximateInversePreconditioner& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// addition: ... and with IC0 / SGS of the multicolour reordering (both symmetric positive definite for such a matrix)
template <typename T, typename Base>
using MulticolorPreconditioner = typename CSRMatrix<T>::template MulticolorPreconditioner<Base>;
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::template MulticolorPreconditioner<typename CSRMatrix<T>::IC0Preconditioner>& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::template MulticolorPreconditioner<typename CSRMatrix<T>::SGSPreconditioner>& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// addition: ... and with the iterated sweeps of IC0 / SGS at equal step counts (other bases and unequal counts are refused: DIVERGED,
// lastHipStatus() != 0)
template <typename T>
using JacobiSweepPreconditioner = typename CSRMatrix<T>::JacobiSweepPreconditioner;
template <typename T>
inline SolverStatus ConjugateGradient(const CSRMatrix<T>& a, const T* const b, const T* const x0, T* const x, int maxIterations, T eps,
                                      const typename CSRMatrix<T>::JacobiSweepPreconditioner& M) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = M.handle();
	const int rc = d && h ? detail::Abi<T>::cg(d, b, x0, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ref:2191-2283.  CSRMatrix<T>'s own preconditioner classes live on the GPU and run inside the device-resident loop.  ANY other type
// with the reference's `int apply(const T* rhs, T* x) const` (ref:2199, 2218, 2235, 2251) is accepted as well: the loop then runs
// its SpMVs, reductions and updates on the device and calls the functor on the host around two PCIe copies per apply (the slow
// path: smm_hip_bicgstab_functor_*).
template <typename Preconditioner, typename T>
inline SolverStatus BiCGStab(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, const Preconditioner& preconditioner) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	if (!d) return SolverStatus::DIVERGED;
	if constexpr (std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	              std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value) {
		const smm_hip_precond* h = preconditioner.handle();
		constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
		if (precondition && !h) return SolverStatus::DIVERGED;
		const int rc = detail::Abi<T>::bicgstab(d, b, x, maxIterations, eps, h, &st);
		return detail::toStatus(rc, st);
	} else {
		auto trampoline = +[](void* user, const T* rhs, T* out) -> int { return static_cast<const Preconditioner*>(user)->apply(rhs, out); };
		const int rc = detail::Functor<T>::run(d, b, x, maxIterations, eps, trampoline, const_cast<Preconditioner*>(&preconditioner), &st);
		return detail::toStatus(rc, st);
	}
}

// ref:2294-2303
template <typename T>
inline SolverStatus BiCGStab(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps) {
	return BiCGStab(a, b, x, maxIterations, eps, typename CSRMatrix<T>::IDPreconditioner());
}

// ---- additions with no counterpart in the reference: k right-hand sides at once (smm_hip.h "batched BiCGStab / ConjugateGradient") ----
// B, X (and X0) are interleaved blocks of rows x k elements, element (i, j) at i * k + j, 1 <= k <= SMM_HIP_MAX_RHS; status[j] (k entries, may
// be null) receives what BiCGStab / ConjugateGradient return for column j alone: every column runs the reference's loop for its own b
// (ref:2200-2283, 2330-2398) and is left alone once it has ended.  The return value is SUCCESS when the call ran (whatever the columns'
// statuses) and DIVERGED, with lastHipStatus() != 0, when it could not (no GPU, k out of range, an unsupported preconditioner).
// BiCGStabBatch takes the IDPreconditioner or the JacobiPreconditioner; every other kind is refused.
template <typename Preconditioner, typename T>
inline SolverStatus BiCGStabBatch(const CSRMatrix<T>& a, T* B, T* X, int k, int maxIterations, T eps, const Preconditioner& preconditioner, SolverStatus* status) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "BiCGStabBatch runs the library's own preconditioners only (IDPreconditioner, JacobiPreconditioner)");
	const smm_hip_csr* d = a.device();
	if (!d) return SolverStatus::DIVERGED;
	const smm_hip_precond* h = preconditioner.handle();
	if (!std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value && !h) return SolverStatus::DIVERGED;
	int st[SMM_HIP_MAX_RHS] = {};
	if (detail::note(detail::Abi<T>::bicgstabBatch(d, k, B, X, maxIterations, eps, h, st)) != SMM_HIP_OK) return SolverStatus::DIVERGED;
	for (int j = 0; status && j < k; ++j) status[j] = static_cast<SolverStatus>(st[j]);
	return SolverStatus::SUCCESS;
}
template <typename T>
inline SolverStatus BiCGStabBatch(const CSRMatrix<T>& a, T* B, T* X, int k, int maxIterations, T eps, SolverStatus* status) {
	return BiCGStabBatch(a, B, X, k, maxIterations, eps, typename CSRMatrix<T>::IDPreconditioner(), status);
}
template <typename T>
inline SolverStatus ConjugateGradientBatch(const CSRMatrix<T>& a, const T* B, const T* X0, T* X, int k, int maxIterations, T eps, SolverStatus* status) {
	const smm_hip_csr* d = a.device();
	if (!d) return SolverStatus::DIVERGED;
	int st[SMM_HIP_MAX_RHS] = {};
	if (detail::note(detail::Abi<T>::cgBatch(d, k, B, X0, X, maxIterations, eps, st)) != SMM_HIP_OK) return SolverStatus::DIVERGED;
	for (int j = 0; status && j < k; ++j) status[j] = static_cast<SolverStatus>(st[j]);
	return SolverStatus::SUCCESS;
}

// ref:2021-2102
template <typename T>
inline SolverStatus BiCGSymmetric(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const int rc = d ? detail::Abi<T>::bicgsym(d, b, x, maxIterations, eps, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ref:2104-2178, with `residualSquared` declared before the `do` so that the loop condition reads the value the body has just computed
// (as published, ref:2171-2172, the template cannot be instantiated): the one repair, stated in smm_hip.h
template <typename T>
inline SolverStatus ConjugateGradientSquared(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const int rc = d ? detail::Abi<T>::cgs(d, b, x, maxIterations, eps, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ---- an addition with no counterpart in the reference: restarted GMRES(restart) with right preconditioning (smm_hip.h states the loop) ----
// For general matrices; x is the initial guess and receives the result; maxIterations < 0 means rows, with no other clamp.  Takes the
// IDPreconditioner or any of CSRMatrix<T>'s own preconditioner classes that BiCGStab takes; they run inside the device-resident loop.
template <typename Preconditioner, typename T>
inline SolverStatus GMRES(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, int restart, const Preconditioner& preconditioner) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "GMRES runs the library's own preconditioners only");
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
	if (d && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const int rc = d ? detail::Abi<T>::gmres(d, b, x, maxIterations, eps, restart, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus GMRES(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, int restart = 30) {
	return GMRES(a, b, x, maxIterations, eps, restart, typename CSRMatrix<T>::IDPreconditioner());
}

// ---- an addition with no counterpart in the reference: MINRES with a symmetric positive definite preconditioner (smm_hip.h states the loop) ----
// For symmetric matrices, indefinite ones included (symmetry is the caller's business, as with ConjugateGradient); x is the initial guess and
// receives the result; maxIterations == -1 means rows, otherwise it is clamped to rows.  Takes the IDPreconditioner or one of CSRMatrix<T>'s own
// preconditioner classes of a kind ConjugateGradient takes -- built on a positive definite matrix of the same size, which need not be `a` (a
// preconditioner of an indefinite `a` is not positive definite).  With a preconditioner the stop test reads the residual's M^-1-norm.
template <typename Preconditioner, typename T>
inline SolverStatus MINRES(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, const Preconditioner& preconditioner) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "MINRES runs the library's own preconditioners only");
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
	if (d && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const int rc = d ? detail::Abi<T>::minres(d, b, x, maxIterations, eps, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus MINRES(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps) {
	return MINRES(a, b, x, maxIterations, eps, typename CSRMatrix<T>::IDPreconditioner());
}

// ---- an addition with no counterpart in the reference: the k algebraically largest or smallest eigenpairs of a symmetric matrix by
// thick-restart Lanczos on the device (smm_hip.h states the algorithm) ----
// which: SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST.  eigenvalues[k] come out in the order of `which` (descending / ascending); eigenvectors
// (may be null) receives vector i at eigenvectors + i * rows.  ncv == 0 means min(rows, max(2k + 1, 20)); tol <= 0 the machine epsilon of T;
// v0 == nullptr the hash vector of `seed`.  SUCCESS: all k converged; MAX_ITERATIONS_REACHED: the pairs are the best available; DIVERGED:
// a value that is not finite, or the call failed (lastHipStatus() says why).  No shift-invert, no interior eigenvalues; not preconditioned: SMM::lobpcg is.
struct EigshInfo {
	int nconv = 0, restarts = 0, matvecs = 0;
};
template <typename T>
inline SolverStatus eigsh(const CSRMatrix<T>& a, int k, int which, T* eigenvalues, T* eigenvectors = nullptr, int ncv = 0, T tol = T(0), int maxRestarts = 300,
                          const T* v0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr, EigshInfo* info = nullptr) {
	int st = 0;
	EigshInfo local;
	EigshInfo* o = info ? info : &local;
	const smm_hip_csr* d = a.device();
	const int rc = d ? detail::Abi<T>::eigsh(d, k, which, ncv, maxRestarts, tol, v0, seed, eigenvalues, eigenvectors, static_cast<long long>(a.getDenseRowCount()),
	                                         residuals, &o->nconv, &o->restarts, &o->matvecs, &st)
	                 : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ---- an addition with no counterpart in the reference: the k largest singular triplets of a matrix of any shape by thick-restart
// Golub-Kahan-Lanczos bidiagonalisation on the device (smm_hip.h states the algorithm) ----
// singularValues[k] come out descending; U (may be null) receives left vector i at U + i * rows, V (may be null) right vector i at
// V + i * cols.  ncv == 0 means min(rows, cols, max(2k + 1, 20)); tol <= 0 the machine epsilon of T; v0 == nullptr the hash vector of `seed`,
// otherwise a start vector of cols elements.  `at`: the transpose (SMM::transpose) kept by the caller, null to have one built for the duration
// of the solve, or &a to assert symmetry of a square matrix.  SUCCESS: all k converged; MAX_ITERATIONS_REACHED: the triplets are the best
// available; DIVERGED: a value that is not finite, or the call failed (lastHipStatus() says why).  Not the smallest singular values, no shift,
// no block method.  CSRMatrix<T>::norm2() is the k = 1 case without vectors.
struct SvdsInfo {
	int nconv = 0, restarts = 0, matvecs = 0;
};
template <typename T>
inline SolverStatus svds(const CSRMatrix<T>& a, int k, T* singularValues, T* U = nullptr, T* V = nullptr, int ncv = 0, T tol = T(0), int maxRestarts = 300,
                         const CSRMatrix<T>* at = nullptr, const T* v0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr, SvdsInfo* info = nullptr) {
	int st = 0;
	SvdsInfo local;
	SvdsInfo* o = info ? info : &local;
	const smm_hip_csr* d = a.device();
	const smm_hip_csr* dt = !at ? nullptr : (at == &a ? d : at->device());
	const int rc = d && (!at || dt) ? detail::Abi<T>::svds(d, dt, k, ncv, maxRestarts, tol, v0, seed, singularValues, U, static_cast<long long>(a.getDenseRowCount()), V,
	                                                       static_cast<long long>(a.getDenseColCount()), residuals, &o->nconv, &o->restarts, &o->matvecs, &st)
	                                : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ---- an addition with no counterpart in the reference: the k algebraically largest or smallest eigenpairs of a symmetric matrix by LOBPCG,
// the preconditioned block method (smm_hip.h states the loop) ----
// 1 <= k <= SMM_LOBPCG_MAX_K with 3k <= rows; which: SMM_EIGSH_LARGEST or SMM_EIGSH_SMALLEST.  eigenvalues[k] come out in the order of `which`;
// eigenvectors (may be null) receives vector j at eigenvectors + j * rows.  Takes the IDPreconditioner or one of CSRMatrix<T>'s own
// preconditioner classes of a kind ConjugateGradient takes (or JACOBI / SGS), built on a positive definite matrix of the same size, which need not be `a` (a
// shifted L - sigma I takes the preconditioner of L).  tol <= 0 means the machine epsilon of T; X0 == nullptr the hash columns of `seed`,
// otherwise k start columns, column j at X0 + j * rows.  SUCCESS: all k converged; MAX_ITERATIONS_REACHED: the pairs are the best available;
// DIVERGED: a value that is not finite, a start block of rank below k, or the call failed (lastHipStatus() says why).
struct LobpcgInfo {
	int nconv = 0, iterations = 0, matvecs = 0, applies = 0;
};
template <typename Preconditioner, typename T>
inline SolverStatus lobpcg(const CSRMatrix<T>& a, int k, int which, T* eigenvalues, T* eigenvectors, const Preconditioner& preconditioner, T tol = T(0),
                           int maxIterations = 1000, const T* X0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr, LobpcgInfo* info = nullptr) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "lobpcg runs the library's own preconditioners only");
	int st = 0;
	LobpcgInfo local;
	LobpcgInfo* o = info ? info : &local;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
	if (d && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const long long rows = static_cast<long long>(a.getDenseRowCount());
	const int rc = d ? detail::Abi<T>::lobpcg(d, k, which, maxIterations, tol, h, X0, rows, seed, eigenvalues, eigenvectors, rows, residuals, &o->nconv, &o->iterations,
	                                          &o->matvecs, &o->applies, &st)
	                 : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus lobpcg(const CSRMatrix<T>& a, int k, int which, T* eigenvalues, T* eigenvectors = nullptr, T tol = T(0), int maxIterations = 1000,
                           const T* X0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr, LobpcgInfo* info = nullptr) {
	return lobpcg(a, k, which, eigenvalues, eigenvectors, typename CSRMatrix<T>::IDPreconditioner(), tol, maxIterations, X0, seed, residuals, info);
}

// The GENERALISED problem A x = lambda B x (K x = lambda M x with a mass matrix: the vibration modes), smm_hip_lobpcg_gen_*: `b` is a
// symmetric positive definite matrix of a's size.  Everything else is lobpcg's above; the eigenvectors come out B-orthonormal, the
// preconditioner still approximates A^-1 and fits `a`, and info->bmatvecs counts the products with B.  b may be `a` itself.
struct LobpcgGenInfo : LobpcgInfo {
	int bmatvecs = 0;
};
template <typename Preconditioner, typename T>
inline SolverStatus lobpcg(const CSRMatrix<T>& a, const CSRMatrix<T>& b, int k, int which, T* eigenvalues, T* eigenvectors, const Preconditioner& preconditioner,
                           T tol = T(0), int maxIterations = 1000, const T* X0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr,
                           LobpcgGenInfo* info = nullptr) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "lobpcg runs the library's own preconditioners only");
	int st = 0;
	LobpcgGenInfo local;
	LobpcgGenInfo* o = info ? info : &local;
	const smm_hip_csr* d = a.device();
	const smm_hip_csr* db = &b == &a ? d : b.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
	if (d && db && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const long long rows = static_cast<long long>(a.getDenseRowCount());
	const int rc = d && db ? detail::Abi<T>::lobpcgGen(d, db, k, which, maxIterations, tol, h, X0, rows, seed, eigenvalues, eigenvectors, rows, residuals, &o->nconv,
	                                                   &o->iterations, &o->matvecs, &o->bmatvecs, &o->applies, &st)
	                       : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus lobpcg(const CSRMatrix<T>& a, const CSRMatrix<T>& b, int k, int which, T* eigenvalues, T* eigenvectors = nullptr, T tol = T(0),
                           int maxIterations = 1000, const T* X0 = nullptr, unsigned long long seed = 0, T* residuals = nullptr, LobpcgGenInfo* info = nullptr) {
	return lobpcg(a, b, k, which, eigenvalues, eigenvectors, typename CSRMatrix<T>::IDPreconditioner(), tol, maxIterations, X0, seed, residuals, info);
}

// ---- an addition with no counterpart in the reference: IDR(s), biorthogonal form, with right preconditioning (smm_hip.h states the loop) ----
// For general matrices; x is the initial guess and receives the result; maxIterations < 0 means rows, with no other clamp; 1 <= s <=
// SMM_IDRS_MAX_S shadow vectors, generated by the library from seed 0.  Takes the IDPreconditioner or any of CSRMatrix<T>'s own
// preconditioner classes that GMRES takes; they run inside the device-resident loop.
template <typename Preconditioner, typename T>
inline SolverStatus IDRs(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, int s, const Preconditioner& preconditioner) {
	static_assert(std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value ||
	                  std::is_base_of<typename CSRMatrix<T>::PreconditionerBase, Preconditioner>::value,
	              "IDRs runs the library's own preconditioners only");
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, typename CSRMatrix<T>::IDPreconditioner>::value;
	if (d && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const int rc = d ? detail::Abi<T>::idrs(d, b, x, maxIterations, eps, s, h, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
template <typename T>
inline SolverStatus IDRs(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, int s = 4) {
	return IDRs(a, b, x, maxIterations, eps, s, typename CSRMatrix<T>::IDPreconditioner());
}

// ---- additions with no counterpart in the reference: the transpose, the symmetry check and BiCG for general matrices (smm_hip.h) ----
// out becomes Aᵀ, built on the GPU (CSRMatrix::initTransposeOf); 0, or the SMM_HIP_* status with out left empty
template <typename T>
inline int transpose(const CSRMatrix<T>& a, CSRMatrix<T>& out) noexcept {
	return out.initTransposeOf(a);
}
// the pattern equals the transpose's and every value equals its mirror image by IEEE == (a NaN never does); false also when the check
// could not run (lastHipStatus() != 0 then)
template <typename T>
inline bool isSymmetric(const CSRMatrix<T>& a) noexcept {
	const smm_hip_csr* d = a.device();
	int pattern = 0, vals = 0;
	if (!d || detail::note(smm_hip_csr_is_symmetric(d, &pattern, &vals)) != SMM_HIP_OK) return false;
	return pattern != 0 && vals != 0;
}
// ---- additions: colouring and symmetric permutation (smm_hip.h "a COLOURING of the rows and the SYMMETRIC PERMUTATION") ----
// colors[rows] (0-based) such that no stored off-diagonal entry joins two rows of one colour; *ncolors = the largest colour + 1.  0, or the
// SMM_HIP_* status
template <typename T>
inline int color(const CSRMatrix<T>& a, int* colors, int* ncolors) noexcept {
	const smm_hip_csr* d = a.device();
	return detail::note(d ? smm_hip_csr_color(d, colors, static_cast<size_t>(a.getDenseRowCount()), ncolors) : SMM_HIP_ERR_NO_DEVICE);
}
// out becomes P a Pᵀ (CSRMatrix::initPermuteOf): row i of out is a's row perm[i]; 0, or the SMM_HIP_* status with out left empty
template <typename T>
inline int permute(const CSRMatrix<T>& a, const int* perm, CSRMatrix<T>& out) noexcept {
	return out.initPermuteOf(a, perm);
}
// b, made by SMM::permute, takes over the present values of a (CSRMatrix::permuteRefresh); 0, or the SMM_HIP_* status with b unchanged
template <typename T>
inline int permuteRefresh(CSRMatrix<T>& b, const CSRMatrix<T>& a) noexcept {
	return b.permuteRefresh(a);
}
// ---- additions: bandwidth-reducing ordering (smm_hip.h "a BANDWIDTH-REDUCING ORDERING") ----
// perm becomes the reverse Cuthill-McKee ordering of a's adjacency graph (reverse == false: Cuthill-McKee): perm[i] is the row that becomes
// row i, so SMM::permute(a, perm.data(), out) has its entries near the diagonal.  The information outputs may be null.  0, or the
// SMM_HIP_* status with perm left empty
template <typename T>
inline int rcm(const CSRMatrix<T>& a, std::vector<int>& perm, bool reverse = true, int* components = nullptr, int* levels = nullptr,
               long long* bandwidthBefore = nullptr, long long* bandwidthAfter = nullptr) {
	const smm_hip_csr* d = a.device();
	perm.assign(static_cast<size_t>(a.getDenseRowCount()), 0);
	const int rc = detail::note(d ? smm_hip_csr_rcm(d, perm.data(), perm.size(), reverse ? 1 : 0, components, levels, bandwidthBefore, bandwidthAfter) : SMM_HIP_ERR_NO_DEVICE);
	if (rc != SMM_HIP_OK) perm.clear();
	return rc;
}
// max |i - j| over the stored entries of a and the number of distinct j - i (either may be null); 0, or the SMM_HIP_* status
template <typename T>
inline int bandwidth(const CSRMatrix<T>& a, long long* width, long long* distinctOffsets = nullptr) noexcept {
	const smm_hip_csr* d = a.device();
	return detail::note(d ? smm_hip_csr_bandwidth(d, width, distinctOffsets) : SMM_HIP_ERR_NO_DEVICE);
}
// out becomes the product a b, built on the GPU (CSRMatrix::initProductOf); 0, or the SMM_HIP_* status with out left empty
template <typename T>
inline int multiply(const CSRMatrix<T>& a, const CSRMatrix<T>& b, CSRMatrix<T>& out) noexcept {
	return out.initProductOf(a, b);
}
// the values of c become those of a b on c's own pattern (CSRMatrix::multiplyInto); 0, or the SMM_HIP_* status with c unchanged
template <typename T>
inline int multiplyInto(CSRMatrix<T>& c, const CSRMatrix<T>& a, const CSRMatrix<T>& b) {
	return c.multiplyInto(a, b);
}
// out becomes alpha a + beta b over the union of the two patterns, built on the GPU (CSRMatrix::initSumOf); 0, or the SMM_HIP_* status with
// out left empty
template <typename T>
inline int add(const CSRMatrix<T>& a, typename std::enable_if<true, T>::type alpha, const CSRMatrix<T>& b, typename std::enable_if<true, T>::type beta,
               CSRMatrix<T>& out) noexcept {  // (the scalars are not deduced: add(a, 1, b, -1, out) works for float and double)
	return out.initSumOf(a, alpha, b, beta);
}
// the values of c become those of alpha a + beta b on c's own pattern (CSRMatrix::addInto); c may be a, b or both; 0, or the SMM_HIP_*
// status with c unchanged
template <typename T>
inline int addInto(CSRMatrix<T>& c, const CSRMatrix<T>& a, typename std::enable_if<true, T>::type alpha, const CSRMatrix<T>& b,
                   typename std::enable_if<true, T>::type beta) {
	return c.addInto(a, alpha, b, beta);
}
// ---- composing and slicing (smm_hip.h "COMPOSING and SLICING matrices"); each returns 0 or the SMM_HIP_* status ----
// out becomes the block matrix of the row-major p x q table `blocks` (CSRMatrix::initBlockOf): SMM::blockMatrix(2, 2, {&H, &Bt, &B, nullptr}, K)
template <typename T>
inline int blockMatrix(int p, int q, const CSRMatrix<T>* const* blocks, CSRMatrix<T>& out, const T* coef = nullptr, const int* rowSizes = nullptr,
                       const int* colSizes = nullptr) noexcept {
	return out.initBlockOf(p, q, blocks, coef, rowSizes, colSizes);
}
template <typename T>
inline int blockMatrix(int p, int q, std::initializer_list<const CSRMatrix<T>*> blocks, CSRMatrix<T>& out, const T* coef = nullptr, const int* rowSizes = nullptr,
                       const int* colSizes = nullptr) noexcept {
	if (static_cast<long long>(blocks.size()) != static_cast<long long>(p) * q) return detail::note(SMM_HIP_ERR_INVALID);
	return out.initBlockOf(p, q, blocks.begin(), coef, rowSizes, colSizes);
}
// the values of c (made by blockMatrix from such a table) again from the blocks' present values (CSRMatrix::blockRefresh)
template <typename T>
inline int blockRefresh(CSRMatrix<T>& c, int p, int q, const CSRMatrix<T>* const* blocks, const T* coef = nullptr) {
	return c.blockRefresh(p, q, blocks, coef);
}
template <typename T>
inline int blockRefresh(CSRMatrix<T>& c, int p, int q, std::initializer_list<const CSRMatrix<T>*> blocks, const T* coef = nullptr) {
	if (static_cast<long long>(blocks.size()) != static_cast<long long>(p) * q) return detail::note(SMM_HIP_ERR_INVALID);
	return c.blockRefresh(p, q, blocks.begin(), coef);
}
// out becomes the rows rows[0 .. nr) of a restricted to the ascending columns cols[0 .. nc) (nullptr: all), or the ranges [r0, r1) x [c0, c1)
template <typename T>
inline int submatrix(const CSRMatrix<T>& a, const int* rows, size_t nr, const int* cols, size_t nc, CSRMatrix<T>& out) noexcept {
	return out.initSubmatrixOf(a, rows, nr, cols, nc);
}
template <typename T>
inline int submatrix(const CSRMatrix<T>& a, int r0, int r1, int c0, int c1, CSRMatrix<T>& out) noexcept {
	return out.initSubmatrixOf(a, r0, r1, c0, c1);
}
// the values of s (made by submatrix from a) again from a's present values (CSRMatrix::submatrixRefresh)
template <typename T>
inline int submatrixRefresh(CSRMatrix<T>& s, const CSRMatrix<T>& a) {
	return s.submatrixRefresh(a);
}
// out[i] = a_ii, 0 where none is stored; *missing (may be null) counts those (CSRMatrix::diagonal)
template <typename T>
inline int diagonal(const CSRMatrix<T>& a, T* out, int* missing = nullptr) noexcept {
	return a.diagonal(out, missing);
}
// BiCGSymmetric's text (ref:2021-2102) with the shadow sequence on `at`, the transpose of `a` (SMM::transpose): for matrices that are not
// symmetric.  That `at` is the transpose is the caller's contract; `a` itself as `at` asserts symmetry and gives BiCGSymmetric's bits.
template <typename T>
inline SolverStatus BiCG(const CSRMatrix<T>& a, const CSRMatrix<T>& at, T* b, T* x, int maxIterations, T eps) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_csr* dt = &at == &a ? d : at.device();
	const int rc = d && dt ? detail::Abi<T>::bicg(d, dt, b, x, maxIterations, eps, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}
// ... with a transpose the library builds for the duration of the solve (a device sort per call: keep one when solving more than once)
template <typename T>
inline SolverStatus BiCG(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps) {
	int st = 0;
	const smm_hip_csr* d = a.device();
	const int rc = d ? detail::Abi<T>::bicg(d, nullptr, b, x, maxIterations, eps, &st) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ---- an addition with no counterpart in the reference: LSQR for least-squares and rectangular systems (smm_hip.h states the loop) ----
// min ||a x - b||_2 for a matrix of any shape: b has a.denseRowCount elements, x has a.denseColCount, is the initial guess and receives
// the result.  The stop tests are absolute (eps against the estimates of ||b - a x|| and of ||at (b - a x)||: an inconsistent system ends
// by the second, SUCCESS with *reason == 2 and a residual that is not small); damp > 0 damps the correction x - x0.  `at`: the transpose
// (SMM::transpose) kept by the caller, null to have one built for the duration of the solve, or &a to assert symmetry of a square matrix.
template <typename T>
inline SolverStatus LSQR(const CSRMatrix<T>& a, T* b, T* x, int maxIterations, T eps, typename std::enable_if<true, T>::type damp = T(0),
                         const CSRMatrix<typename std::enable_if<true, T>::type>* at = nullptr, int* iterations = nullptr, int* reason = nullptr) {
	// (damp and at are not deduced: LSQR(a, b, x, -1, eps, 0.5, nullptr) works for float and double)
	int st = 0;
	const smm_hip_csr* d = a.device();
	const smm_hip_csr* dt = !at ? nullptr : (at == &a ? d : at->device());
	const int rc = d && (!at || dt) ? detail::Abi<T>::lsqr(d, dt, b, x, maxIterations, eps, damp, &st, iterations, reason) : SMM_HIP_ERR_NO_DEVICE;
	return detail::toStatus(rc, st);
}

// ---- additions with no counterpart in the reference: the other precision and mixed-precision iterative refinement (smm_hip.h) ----
// out becomes `a` with values of type U, converted on the GPU (CSRMatrix::initConvertOf); 0, or the SMM_HIP_* status with out left empty
template <typename U, typename T>
inline int convert(const CSRMatrix<T>& a, CSRMatrix<U>& out) noexcept {
	return out.initConvertOf(a);
}
// ... returned by value: an empty matrix, with lastHipStatus() != 0, when it could not be made
template <typename U, typename T>
inline CSRMatrix<U> convert(const CSRMatrix<T>& a) noexcept {
	CSRMatrix<U> out;
	out.initConvertOf(a);
	return out;
}
enum class RefinementSolver { CG = SMM_REFINE_INNER_CG, BICGSTAB = SMM_REFINE_INNER_BICGSTAB, GMRES = SMM_REFINE_INNER_GMRES };
struct RefinementInfo {  // what smm_hip_refine_f64 reports beside the status
	int outerIterations = 0, innerIterations = 0;
	double residualNormSquared = 0.0;  // the true ||b - A x||^2 of the returned x, in double
};
// A double answer from float solves (smm_hip.h states the loop): every outer step takes the true residual in double, solves for a correction
// in float with `inner` on a32 -- SMM::convert<float>(a), kept by callers that solve more than once -- and accepts it only if the true
// residual falls: a rejected step (DIVERGED) or a failed call leaves x as it was.  x is the initial guess and receives the result.
// `preconditioner`: the IDPreconditioner or one of a32's own preconditioner objects of a kind the inner solver takes.
template <typename Preconditioner>
inline SolverStatus IterativeRefinement(const CSRMatrix<double>& a, const CSRMatrix<float>& a32, double* b, double* x, double eps, const Preconditioner& preconditioner,
                                        RefinementSolver inner = RefinementSolver::CG, int maxOuter = 20, int maxInner = -1, float innerEps = 1e-4f, int restart = 30,
                                        RefinementInfo* info = nullptr) {
	static_assert(std::is_same<Preconditioner, CSRMatrix<float>::IDPreconditioner>::value || std::is_base_of<CSRMatrix<float>::PreconditionerBase, Preconditioner>::value,
	              "IterativeRefinement runs the library's own preconditioners only");
	int st = 0;
	RefinementInfo out;
	const smm_hip_csr* d = a.device();
	const smm_hip_csr* d32 = a32.device();
	const smm_hip_precond* h = preconditioner.handle();
	constexpr bool precondition = !std::is_same<Preconditioner, CSRMatrix<float>::IDPreconditioner>::value;
	if (d && d32 && precondition && !h) return SolverStatus::DIVERGED;  // (the preconditioner could not be built: lastHipStatus() says why)
	const int rc = d && d32 ? smm_hip_refine_f64(d, d32, b, x, static_cast<int>(inner), maxOuter, maxInner, eps, innerEps, restart, h, &st, &out.outerIterations,
	                                             &out.innerIterations, &out.residualNormSquared)
	                        : SMM_HIP_ERR_NO_DEVICE;
	if (info) *info = out;
	return detail::toStatus(rc, st);
}
inline SolverStatus IterativeRefinement(const CSRMatrix<double>& a, const CSRMatrix<float>& a32, double* b, double* x, double eps,
                                        RefinementSolver inner = RefinementSolver::CG, int maxOuter = 20, int maxInner = -1, float innerEps = 1e-4f, int restart = 30,
                                        RefinementInfo* info = nullptr) {
	return IterativeRefinement(a, a32, b, x, eps, CSRMatrix<float>::IDPreconditioner(), inner, maxOuter, maxInner, innerEps, restart, info);
}
// ... with a float matrix the library converts for the duration of the solve (a pass over the values per call: keep one when solving more than once)
inline SolverStatus IterativeRefinement(const CSRMatrix<double>& a, double* b, double* x, double eps, RefinementSolver inner = RefinementSolver::CG, int maxOuter = 20,
                                        int maxInner = -1, float innerEps = 1e-4f, int restart = 30, RefinementInfo* info = nullptr) {
	int st = 0;
	RefinementInfo out;
	const smm_hip_csr* d = a.device();
	const int rc = d ? smm_hip_refine_f64(d, nullptr, b, x, static_cast<int>(inner), maxOuter, maxInner, eps, innerEps, restart, nullptr, &st, &out.outerIterations,
	                                      &out.innerIterations, &out.residualNormSquared)
	                 : SMM_HIP_ERR_NO_DEVICE;
	if (info) *info = out;
	return detail::toStatus(rc, st);
}

// ---- file loaders (ref:2507-2669) ---------------------------------------------------------------------------------------------
// Same enumerators in the same order as ref:2507-2522; additions follow them.
enum class MatrixLoadStatus {
	SUCCESS = 0,
	FAILED_TO_OPEN_FILE,
	FAILED_TO_OPEN_FILE_UNKNOWN_FORMAT,
	FAILED_TO_PARSE_FILE,
	PARSE_ERROR_MMX_FILE_MISSING_BANNER,
	PARSE_ERROR_MMX_FILE_UNSUPPORTED_TYPE,
	PARSE_ERROR_MMX_FILE_UNSUPPORTED_FORMAT,
	PARSE_ERROR_MMX_FILE_UNSUPPORTED_EL_TYPE,
	PARSE_ERROR_MMX_FILE_UNSUPPORTED_STRUCTURE,
	// additions
	PARSE_ERROR_INDEX_OUT_OF_RANGE,  // an entry outside rows x cols (undefined behaviour in the reference)
	MATRIX_TOO_LARGE                 // more than 2^31 - 1 stored entries after mirroring: start[] is int (ref:1251-1257)
};

namespace detail {
struct MmEntry {
	int row, col;
	double value;
};
struct MmHeader {
	int rows = 0, cols = 0;
	long long declared = 0;
	bool pattern = false, symmetric = false;
};
inline void lower(std::string& s) {
	for (char& c : s) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
}
// Banner, comments and size line exactly as ref:2537-2581 reads them: `%%MatrixMarket` case-sensitive, the four qualifiers
// case-insensitive; `coordinate` only; `real` / `integer` (ref) and `pattern` (addition: every entry is 1); `symmetric` (ref) and
// `general` (addition).
inline MatrixLoadStatus readMmHeader(std::istream& file, MmHeader& h) {
	std::string banner, matrix, format, type, structure;
	file >> banner;
	if (banner != "%%MatrixMarket") return MatrixLoadStatus::PARSE_ERROR_MMX_FILE_MISSING_BANNER;
	file >> matrix;
	lower(matrix);
	if (matrix != "matrix") return MatrixLoadStatus::PARSE_ERROR_MMX_FILE_UNSUPPORTED_TYPE;
	file >> format;
	lower(format);
	if (format != "coordinate") return MatrixLoadStatus::PARSE_ERROR_MMX_FILE_UNSUPPORTED_FORMAT;
	file >> type;
	lower(type);
	h.pattern = type == "pattern";
	if (!h.pattern && type != "real" && type != "integer") return MatrixLoadStatus::PARSE_ERROR_MMX_FILE_UNSUPPORTED_EL_TYPE;
	file >> structure;
	lower(structure);
	h.symmetric = structure == "symmetric";
	if (!h.symmetric && structure != "general") return MatrixLoadStatus::PARSE_ERROR_MMX_FILE_UNSUPPORTED_STRUCTURE;
	while (file.peek() == '%' || std::isspace(file.peek())) file.ignore(std::numeric_limits<std::streamsize>::max(), '\n');
	file >> h.rows >> h.cols >> h.declared;
	if (file.fail() || h.rows < 0 || h.cols < 0) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
	return MatrixLoadStatus::SUCCESS;
}
// Entries until end of file, like the reference's loop (ref:2584-2608: the declared count only sizes the container); every
// entry goes to sink(row, col, value) with 0-based indices, off-diagonal entries of a symmetric file also mirrored (ref:2598-2601).
template <typename Sink>
inline MatrixLoadStatus readMmEntries(std::istream& file, const MmHeader& h, Sink&& sink) {
	while (std::isspace(file.peek())) file.get();
	while (!file.eof() && file.peek() != std::char_traits<char>::eof()) {
		int row = 0, col = 0;
		double value = 1.0;
		file >> row >> col;
		if (!h.pattern) file >> value;
		if (file.fail()) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
		if (row < 1 || col < 1 || row > h.rows || col > h.cols) return MatrixLoadStatus::PARSE_ERROR_INDEX_OUT_OF_RANGE;
		sink(row - 1, col - 1, value);
		if (h.symmetric && row != col) sink(col - 1, row - 1, value);
		while (std::isspace(file.peek())) file.get();
	}
	return MatrixLoadStatus::SUCCESS;
}
}  // namespace detail

// ref:2531-2609, same signature: Matrix Market coordinate file into a TripletMatrix (duplicates add up, ref:612-617)
template <typename T>
inline MatrixLoadStatus loadMatrixMarketMatrix(const char* filepath, TripletMatrix<T>& out) {
	std::ifstream file(filepath);
	if (!file.is_open()) return MatrixLoadStatus::FAILED_TO_OPEN_FILE;
	detail::MmHeader h;
	const MatrixLoadStatus st = detail::readMmHeader(file, h);
	if (st != MatrixLoadStatus::SUCCESS) return st;
	out.init(h.rows, h.cols, static_cast<int>(std::min<long long>(h.declared, std::numeric_limits<int>::max())));
	return detail::readMmEntries(file, h, [&](int r, int c, double v) { out.addEntry(r, c, static_cast<T>(v)); });
}

// Addition: the same file DIRECT TO CSR, without the std::map of the triplet form (ref:606-618 costs ~50 bytes and a tree insertion
// per entry: 5e8 entries do not fit).  Entries are collected, stably sorted by (row, column) and duplicates added in file order --
// the same sums in the same order as TripletMatrix::addEntry forms them -- and the three CSR arrays are written in one pass.
template <typename T>
inline MatrixLoadStatus loadMatrixMarketMatrix(const char* filepath, CSRMatrix<T>& out) {
	std::ifstream file(filepath);
	if (!file.is_open()) return MatrixLoadStatus::FAILED_TO_OPEN_FILE;
	detail::MmHeader h;
	MatrixLoadStatus st = detail::readMmHeader(file, h);
	if (st != MatrixLoadStatus::SUCCESS) return st;
	std::vector<detail::MmEntry> entries;
	if (h.declared > 0) entries.reserve(static_cast<size_t>(h.symmetric ? 2 * h.declared : h.declared));
	st = detail::readMmEntries(file, h, [&](int r, int c, double v) { entries.push_back({r, c, v}); });
	if (st != MatrixLoadStatus::SUCCESS) return st;
	std::stable_sort(entries.begin(), entries.end(), [](const detail::MmEntry& a, const detail::MmEntry& b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
	std::vector<int> start(static_cast<size_t>(h.rows) + 1, 0), positions;
	std::vector<T> values;
	positions.reserve(entries.size());
	values.reserve(entries.size());
	for (size_t i = 0; i < entries.size();) {
		size_t j = i;
		T sum = T(0);  // TripletMatrix::addEntry: data[key] += value starting from T() (ref:612-617)
		for (; j < entries.size() && entries[j].row == entries[i].row && entries[j].col == entries[i].col; ++j) sum += static_cast<T>(entries[j].value);
		if (positions.size() == static_cast<size_t>(std::numeric_limits<int>::max())) return MatrixLoadStatus::MATRIX_TOO_LARGE;
		positions.push_back(entries[i].col);
		values.push_back(sum);
		start[static_cast<size_t>(entries[i].row) + 1]++;
		i = j;
	}
	for (int r = 0; r < h.rows; ++r) start[static_cast<size_t>(r) + 1] += start[static_cast<size_t>(r)];
	return out.init(h.rows, h.cols, start.data(), positions.data(), values.data()) == 0 ? MatrixLoadStatus::SUCCESS : MatrixLoadStatus::FAILED_TO_PARSE_FILE;
}

// The dense text format the reference's saveDenseText writes and ref:2611-2643 reads: `rows cols { {a, b, ...}, {...}, ... }`.
// Written from that format description with a parser of its own: the file is read whole and scanned once as a token stream --
// numbers by strtod, `{` `}` tracked as a nesting depth, commas and white space skipped -- and the shape is CHECKED (exactly `rows`
// inner groups of exactly `cols` numbers, a closed outer group), which the format allows and a stream of >> / ignore calls cannot:
// STRICTER than the reference, which reads `cols` numbers per row and skips whatever else the line holds (INTEGRATION.md lists the
// difference).  Text after the closing brace is ignored, as there.  Zeros are not stored.
template <typename T>
inline MatrixLoadStatus loadSMMDTMatrix(const char* filepath, TripletMatrix<T>& out) {
	std::FILE* f = std::fopen(filepath, "rb");
	if (!f) return MatrixLoadStatus::FAILED_TO_OPEN_FILE;
	std::string text;
	char buf[1 << 16];
	for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
	std::fclose(f);
	const char* p = text.c_str();
	const char* const end = p + text.size();
	long dims[2] = {0, 0};
	for (long& d : dims) {  // the two leading integers
		char* after = nullptr;
		d = std::strtol(p, &after, 10);
		if (after == p || d < 0 || d > std::numeric_limits<int>::max()) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
		p = after;
	}
	const int rows = static_cast<int>(dims[0]), cols = static_cast<int>(dims[1]);
	out.init(rows, cols, 0);
	int depth = 0, row = -1, col = 0;  // depth 1: between rows; depth 2: inside row `row`, `col` numbers read so far
	bool closed = false;
	while (p < end && !closed) {
		const char c = *p;
		if (c == '{') {
			if (++depth > 2) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
			if (depth == 2) {
				if (++row >= rows) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
				col = 0;
			}
			++p;
		} else if (c == '}') {
			if (depth == 2 && col != cols) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
			if (--depth < 0) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
			closed = depth == 0;
			++p;
		} else if (c == ',' || std::isspace(static_cast<unsigned char>(c))) {
			++p;
		} else {
			// a number as `file >> val` with val of type T reads it (ref:2629-2634): parsed straight to T -- strtof for float, so that the
			// rounding is the one-step rounding of the reference and not double -> float --, plain decimal notation only (operator>> takes
			// neither "inf" / "nan" nor hexadecimal floats), and the zero test is made on the T value (a number that underflows to 0 in T
			// is not stored, as in the reference)
			const char* q = p + ((*p == '+' || *p == '-') ? 1 : 0);
			if (!(std::isdigit(static_cast<unsigned char>(*q)) || *q == '.') || (q[0] == '0' && (q[1] == 'x' || q[1] == 'X'))) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
			char* after = nullptr;
			T v;
			if (sizeof(T) == sizeof(float)) v = static_cast<T>(std::strtof(p, &after));
			else v = static_cast<T>(std::strtod(p, &after));
			if (after == p || depth != 2 || col >= cols) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
			if (v != T(0)) out.addEntry(row, col, v);
			++col;
			p = after;
		}
	}
	if (!closed || row + 1 != rows) return MatrixLoadStatus::FAILED_TO_PARSE_FILE;
	return MatrixLoadStatus::SUCCESS;
}

// ref:2645-2656: by file extension
template <typename T>
inline MatrixLoadStatus loadMatrix(const char* filepath, TripletMatrix<T>& out) {
	const char* dot = std::strrchr(filepath, '.');
	if (dot && std::strcmp(dot + 1, "mtx") == 0) return loadMatrixMarketMatrix(filepath, out);
	if (dot && std::strcmp(dot + 1, "smmdt") == 0) return loadSMMDTMatrix(filepath, out);
	return MatrixLoadStatus::FAILED_TO_OPEN_FILE_UNKNOWN_FORMAT;
}

// ref:2658-2669.  `.mtx` goes direct to CSR (above); the dense text format is small by nature and keeps the triplet route.
template <typename T>
inline MatrixLoadStatus loadMatrix(const char* filepath, CSRMatrix<T>& out) {
	const char* dot = std::strrchr(filepath, '.');
	if (dot && std::strcmp(dot + 1, "mtx") == 0) return loadMatrixMarketMatrix(filepath, out);
	TripletMatrix<T> triplet;
	const MatrixLoadStatus status = loadMatrix(filepath, triplet);
	if (status != MatrixLoadStatus::SUCCESS) return status;
	out.init(triplet);
	return MatrixLoadStatus::SUCCESS;
}

}  // namespace SMM
