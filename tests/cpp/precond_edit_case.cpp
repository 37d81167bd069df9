// precond_edit_case.cpp -- single-entry edits of a matrix that already has a device mirror reach a preconditioner made BEFORE them
// (drop-in header only; needs a GPU).  An SGSPreconditioner reads A's values at every apply, so after rMult (the mirror exists),
// M.apply, then updateEntry / addEntry / setValue (queued for the mirror), M.apply must give the bits of an SGS made from a fresh matrix
// with the edited arrays -- the queued entries go to the device before the apply.  Prints "sgs <step> <0|1>" per check and
// "status <lastHipStatus>" at the end (tests/test_gpu_csr_update.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

template <typename T>
static bool sameAsFresh(const SMM::CSRMatrix<T>& a, const typename SMM::CSRMatrix<T>::SGSPreconditioner& m, const std::vector<T>& r) {
	SMM::CSRMatrix<T> fresh;
	fresh.init(a.getDenseRowCount(), a.getDenseColCount(), a.rawStart(), a.rawPositions(), a.rawValues());
	auto mf = fresh.template getPreconditioner<SMM::SolverPreconditioner::SYMMETRIC_GAUS_SEIDEL>();
	std::vector<T> x1(r.size(), T(0)), x2(r.size(), T(0));
	if (m.apply(r.data(), x1.data()) != 0 || mf.apply(r.data(), x2.data()) != 0) return false;
	return std::memcmp(x1.data(), x2.data(), x1.size() * sizeof(T)) == 0;
}

template <typename T>
static void run(const char* name) {
	const int nx = 40, n = nx * nx;  // 5-point Poisson
	SMM::TripletMatrix<T> t(n, n);
	for (int i = 0; i < nx; ++i) {
		for (int j = 0; j < nx; ++j) {
			const int r = i * nx + j;
			if (i > 0) t.addEntry(r, r - nx, T(-1));
			if (j > 0) t.addEntry(r, r - 1, T(-1));
			t.addEntry(r, r, T(4));
			if (j + 1 < nx) t.addEntry(r, r + 1, T(-1));
			if (i + 1 < nx) t.addEntry(r, r + nx, T(-1));
		}
	}
	SMM::CSRMatrix<T> a(t);
	auto m = a.template getPreconditioner<SMM::SolverPreconditioner::SYMMETRIC_GAUS_SEIDEL>();
	std::vector<T> r(static_cast<size_t>(n)), y(static_cast<size_t>(n));
	for (int i = 0; i < n; ++i) r[i] = T(1) + T(0.01) * static_cast<T>(i % 37);
	a.rMult(r.data(), y.data());  // the mirror exists from here on
	std::vector<T> x(static_cast<size_t>(n));
	m.apply(r.data(), x.data());  // the preconditioner exists from here on
	std::printf("sgs %s before %d\n", name, sameAsFresh(a, m, r) ? 1 : 0);
	a.updateEntry(5, 5, T(5.5));
	a.updateEntry(nx + 3, nx + 3, T(7.25));
	std::printf("sgs %s updateEntry %d\n", name, sameAsFresh(a, m, r) ? 1 : 0);
	a.addEntry(2 * nx, 2 * nx, T(0.375));
	a.addEntry(2 * nx, nx, T(-0.5));
	std::printf("sgs %s addEntry %d\n", name, sameAsFresh(a, m, r) ? 1 : 0);
	{
		typename SMM::CSRMatrix<T>::RowIterator it = a.rowBegin(n / 2);
		for (; it != a.rowEnd(n / 2); ++it) it->setValue(it->getValue() * T(1.5));
	}
	std::printf("sgs %s setValue %d\n", name, sameAsFresh(a, m, r) ? 1 : 0);
	a *= T(0.5);  // (device-side bulk edit, for contrast)
	std::printf("sgs %s scale %d\n", name, sameAsFresh(a, m, r) ? 1 : 0);
}

int main() {
	run<float>("float");
	run<double>("double");
	std::printf("status %d\n", SMM::lastHipStatus());
	return 0;
}
