// lsqr_case.cpp -- SMM::LSQR through the drop-in header (tests/test_lsqr_cpu.py compiles it; tests/test_gpu_lsqr.py runs it on a GPU).
// The two function pointers below prove that the header declares the template for float and double with its defaulted arguments.
//
//   lsqr_case      the `tall` matrix of tests/lsqr_cases.py, built here: [poisson2d(12, 12); B], 168 x 144, B's rows +e(6 j) - e(6 j + 3);
//                  b from a fixed linear congruential sequence in [-1, 1); solved from x = 0 with maxIterations = -1 in float (eps 1e-3)
//                  and in double (eps 1e-8), the transpose built by the library:
//                  "float status <S> hip <H> steps <K> reason <R> atr <%a> res <%a>" / "double ..."
//                  atr = ||At (b - A x)||_2 and res = ||b - A x||_2, both formed here in double from the triplets
#include <cmath>
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const lsqrFloat)(const SMM::CSRMatrix<float>&, float*, float*, int, float, float, const SMM::CSRMatrix<float>*, int*, int*) =
	&SMM::LSQR<float>;
static SMM::SolverStatus (*const lsqrDouble)(const SMM::CSRMatrix<double>&, double*, double*, int, double, double, const SMM::CSRMatrix<double>*, int*, int*) =
	&SMM::LSQR<double>;

struct Entry {
	int row, col;
	double value;
};

static std::vector<Entry> tallEntries(int grid, int block) {
	std::vector<Entry> e;
	const int n = grid * grid;
	for (int i = 0; i < n; ++i) {
		const int ix = i % grid, iy = i / grid;
		if (iy > 0) e.push_back({i, i - grid, -1.0});
		if (ix > 0) e.push_back({i, i - 1, -1.0});
		e.push_back({i, i, 4.0});
		if (ix < grid - 1) e.push_back({i, i + 1, -1.0});
		if (iy < grid - 1) e.push_back({i, i + grid, -1.0});
	}
	for (int j = 0; j < block; ++j) {
		e.push_back({n + j, 6 * j, 1.0});
		e.push_back({n + j, 6 * j + 3, -1.0});
	}
	return e;
}

template <typename T>
static void tall(const char* name, T eps) {
	const int grid = 12, block = 24, rows = grid * grid + block, cols = grid * grid;
	const std::vector<Entry> entries = tallEntries(grid, block);
	SMM::TripletMatrix<T> t(rows, cols);
	for (const Entry& e : entries) t.addEntry(e.row, e.col, T(e.value));
	SMM::CSRMatrix<T> a(t);
	std::vector<T> b(rows), x(cols, T(0));
	unsigned long long state = 12345;
	for (int i = 0; i < rows; ++i) {
		state = state * 6364136223846793005ull + 1442695040888963407ull;
		b[i] = T(static_cast<double>(state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
	}
	std::vector<T> rhs(b);  // (the entry point takes b as T*, as every solver of the header does)
	int steps = -1, reason = -1;
	const SMM::SolverStatus status = SMM::LSQR(a, rhs.data(), x.data(), -1, eps, T(0), nullptr, &steps, &reason);
	const int hip = SMM::lastHipStatus();
	std::vector<double> r(rows), atr(cols, 0.0);
	for (int i = 0; i < rows; ++i) r[i] = static_cast<double>(b[i]);
	for (const Entry& e : entries) r[e.row] -= e.value * static_cast<double>(x[e.col]);
	for (const Entry& e : entries) atr[e.col] += e.value * r[e.row];
	double rr = 0, aa = 0;
	for (double v : r) rr += v * v;
	for (double v : atr) aa += v * v;
	std::printf("%s status %d hip %d steps %d reason %d atr %a res %a\n", name, static_cast<int>(status), hip, steps, reason, std::sqrt(aa), std::sqrt(rr));
}

int main() {
	(void)lsqrFloat;
	(void)lsqrDouble;
	tall<float>("float", 1e-3f);
	tall<double>("double", 1e-8);
	return 0;
}
