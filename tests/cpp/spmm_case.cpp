// spmm_case.cpp -- the drop-in header's forms for several right-hand sides: CSRMatrix::rMult / rMultAdd / rMultSub (X, Out, k) and
// SMM::BiCGStabBatch / SMM::ConjugateGradientBatch, every column against the single-vector call of that column (needs a GPU).  The
// matrix: a non-symmetric 5-point convection-diffusion stencil (and its symmetric part for CG).  Prints "OK" last
// (tests/test_gpu_spmm.py); compiled with -fsyntax-only by tests/test_spmm_api_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

static int failures = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		if (!(cond)) {                                                   \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
			++failures;                                                  \
		}                                                                \
	} while (0)

template <typename T>
static void stencil(int nx, T west, T east, SMM::CSRMatrix<T>& out) {
	const int n = nx * nx;
	SMM::TripletMatrix<T> t(n, n);
	for (int i = 0; i < nx; ++i) {
		for (int j = 0; j < nx; ++j) {
			const int row = i * nx + j;
			t.addEntry(row, row, T(4));
			if (i > 0) t.addEntry(row, row - nx, west);
			if (j > 0) t.addEntry(row, row - 1, west);
			if (j + 1 < nx) t.addEntry(row, row + 1, east);
			if (i + 1 < nx) t.addEntry(row, row + nx, east);
		}
	}
	out.init(t);
}

template <typename T>
static T maxAbsDiff(const std::vector<T>& block, int k, int j, const std::vector<T>& col) {
	T worst = 0;
	for (size_t i = 0; i < col.size(); ++i) worst = std::fmax(worst, std::fabs(block[i * k + j] - col[i]));
	return worst;
}

template <typename T>
static void run(T tol) {
	const int nx = 24, n = nx * nx, k = 3;
	SMM::CSRMatrix<T> a, sym;
	stencil<T>(nx, T(-1.3), T(-0.7), a);
	stencil<T>(nx, T(-1), T(-1), sym);
	CHECK(a.setSpmvKernel(SMM_SPMV_STREAM, 1) == SMM_HIP_OK);  // one lane per row: the order of summation the block form keeps
	unsigned s = 12345u;
	auto next = [&s] { return static_cast<T>((s = s * 1664525u + 1013904223u) >> 8) / T(1 << 24) - T(0.5); };
	std::vector<T> X(static_cast<size_t>(n) * k), L(X.size()), Out(X.size(), T(77));
	for (auto& v : X) v = next();
	for (auto& v : L) v = next();

	// rMult / rMultAdd / rMultSub with k columns: bit for bit the single calls
	for (int op = 0; op < 3; ++op) {
		if (op == 0) a.rMult(X.data(), Out.data(), k);
		if (op == 1) a.rMultAdd(L.data(), X.data(), Out.data(), k);
		if (op == 2) a.rMultSub(L.data(), X.data(), Out.data(), k);
		CHECK(SMM::lastHipStatus() == SMM_HIP_OK);
		for (int j = 0; j < k; ++j) {
			std::vector<T> x(n), l(n), y(n);
			for (int i = 0; i < n; ++i) {
				x[i] = X[static_cast<size_t>(i) * k + j];
				l[i] = L[static_cast<size_t>(i) * k + j];
			}
			if (op == 0) a.rMult(x.data(), y.data());
			if (op == 1) a.rMultAdd(l.data(), x.data(), y.data());
			if (op == 2) a.rMultSub(l.data(), x.data(), y.data());
			bool same = true;
			for (int i = 0; i < n; ++i) same = same && std::memcmp(&y[i], &Out[static_cast<size_t>(i) * k + j], sizeof(T)) == 0;
			CHECK(same);
		}
	}
	// a k out of range fails loudly: NaN and a status
	std::vector<T> one(n, T(1));
	a.rMult(X.data(), one.data(), 0);
	CHECK(SMM::lastHipStatus() == SMM_HIP_ERR_INVALID);

	// BiCGStabBatch (none, Jacobi) and ConjugateGradientBatch: five passes, every column against its single solve
	std::vector<T> B(X.size());
	for (auto& v : B) v = T(1) + next();
	const auto jacobi = a.template getPreconditioner<SMM::SolverPreconditioner::JACOBI>();
	for (int variant = 0; variant < 3; ++variant) {
		const SMM::CSRMatrix<T>& m = variant == 2 ? sym : a;
		std::vector<T> Xb(X.size(), T(0)), X0(X.size(), T(0)), Bc(B);
		SMM::SolverStatus st[k];
		SMM::SolverStatus rc;
		if (variant == 0) rc = SMM::BiCGStabBatch(m, Bc.data(), Xb.data(), k, 5, T(1e-30), st);
		else if (variant == 1) rc = SMM::BiCGStabBatch(m, Bc.data(), Xb.data(), k, 5, T(1e-30), jacobi, st);
		else rc = SMM::ConjugateGradientBatch(m, Bc.data(), X0.data(), Xb.data(), k, 5, T(0), st);
		CHECK(rc == SMM::SolverStatus::SUCCESS && SMM::lastHipStatus() == SMM_HIP_OK);
		for (int j = 0; j < k; ++j) {
			std::vector<T> b(n), x(n, T(0)), x0(n, T(0));
			for (int i = 0; i < n; ++i) b[i] = B[static_cast<size_t>(i) * k + j];
			SMM::SolverStatus s1;
			if (variant == 0) s1 = SMM::BiCGStab(m, b.data(), x.data(), 5, T(1e-30));
			else if (variant == 1) s1 = SMM::BiCGStab(m, b.data(), x.data(), 5, T(1e-30), jacobi);
			else s1 = SMM::ConjugateGradient(m, b.data(), x0.data(), x.data(), 5, T(0));
			CHECK(st[j] == s1);
			CHECK(maxAbsDiff(Xb, k, j, x) <= tol);
		}
	}
	// an unsupported preconditioner is refused
	const auto sgs = a.template getPreconditioner<SMM::SolverPreconditioner::SYMMETRIC_GAUS_SEIDEL>();
	std::vector<T> Xb(X.size(), T(0)), Bc(B);
	CHECK(SMM::BiCGStabBatch(a, Bc.data(), Xb.data(), k, 5, T(1e-30), sgs, nullptr) == SMM::SolverStatus::DIVERGED);
	CHECK(SMM::lastHipStatus() == SMM_HIP_ERR_INVALID);
}

int main() {
	// x after five passes is O(1); the batch differs from the single solve only in the order its dot products are added
	run<float>(3e-4f);
	run<double>(1e-10);
	std::printf(failures ? "FAILED\n" : "OK\n");
	return failures ? 1 : 0;
}
