// svds_case.cpp -- SMM::svds and CSRMatrix::norm2 through the drop-in header (tests/test_cpp_svds.py compiles it, and runs it on a GPU
// where there is one).  The two function pointers below prove that the header declares the template for float and double.
//
//   svds_case      the `tall` matrix of tests/lsqr_cases.py, built here: [poisson2d(12, 12); B], 168 x 144, B's rows +e(6 j) - e(6 j + 3);
//                  its four largest singular triplets with ncv = 20, the transpose built by the library, then norm2() with the same tol:
//                  "float status <S> hip <H> nconv <N> restarts <R> matvecs <M> s <%a> <%a> <%a> <%a> res <%a> orth <%a> norm2 <%a>" / "double ..."
//                  res = max_i max(||A v_i - s_i u_i||, ||At u_i - s_i v_i||), orth = max(|Ut U - I|, |Vt V - I|), formed here in double
#include <cmath>
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const svdsFloat)(const SMM::CSRMatrix<float>&, int, float*, float*, float*, int, float, int, const SMM::CSRMatrix<float>*, const float*,
                                            unsigned long long, float*, SMM::SvdsInfo*) = &SMM::svds<float>;
static SMM::SolverStatus (*const svdsDouble)(const SMM::CSRMatrix<double>&, int, double*, double*, double*, int, double, int, const SMM::CSRMatrix<double>*,
                                             const double*, unsigned long long, double*, SMM::SvdsInfo*) = &SMM::svds<double>;

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

static double gramLoss(const std::vector<double>& q, int n, int k) {
	double worst = 0;
	for (int i = 0; i < k; ++i) {
		for (int j = 0; j < k; ++j) {
			double sum = 0;
			for (int r = 0; r < n; ++r) sum += q[i * n + r] * q[j * n + r];
			worst = std::fmax(worst, std::fabs(sum - (i == j ? 1.0 : 0.0)));
		}
	}
	return worst;
}

template <typename T>
static void tall(const char* name, T tol) {
	const int grid = 12, block = 24, rows = grid * grid + block, cols = grid * grid, k = 4;
	const std::vector<Entry> entries = tallEntries(grid, block);
	SMM::TripletMatrix<T> t(rows, cols);
	for (const Entry& e : entries) t.addEntry(e.row, e.col, T(e.value));
	SMM::CSRMatrix<T> a(t);
	T s[k] = {T(0), T(0), T(0), T(0)};
	std::vector<T> U(static_cast<size_t>(rows) * k, T(0)), V(static_cast<size_t>(cols) * k, T(0));
	SMM::SvdsInfo info;
	const SMM::SolverStatus status = SMM::svds(a, k, s, U.data(), V.data(), 20, tol, 100, static_cast<const SMM::CSRMatrix<T>*>(nullptr), static_cast<const T*>(nullptr),
	                                           0ull, static_cast<T*>(nullptr), &info);
	const int hip = SMM::lastHipStatus();
	std::vector<double> u(U.begin(), U.end()), v(V.begin(), V.end());
	double worst = 0;
	for (int i = 0; i < k; ++i) {
		std::vector<double> av(rows, 0.0), atu(cols, 0.0);
		for (const Entry& e : entries) {
			av[e.row] += e.value * v[i * cols + e.col];
			atu[e.col] += e.value * u[i * rows + e.row];
		}
		double left = 0, right = 0;
		for (int r = 0; r < rows; ++r) left += (av[r] - s[i] * u[i * rows + r]) * (av[r] - s[i] * u[i * rows + r]);
		for (int c = 0; c < cols; ++c) right += (atu[c] - s[i] * v[i * cols + c]) * (atu[c] - s[i] * v[i * cols + c]);
		worst = std::fmax(worst, std::fmax(std::sqrt(left), std::sqrt(right)));
	}
	const double orth = std::fmax(gramLoss(u, rows, k), gramLoss(v, cols, k));
	const T norm = a.norm2(tol);
	std::printf("%s status %d hip %d nconv %d restarts %d matvecs %d s %a %a %a %a res %a orth %a norm2 %a\n", name, static_cast<int>(status), hip, info.nconv,
	            info.restarts, info.matvecs, static_cast<double>(s[0]), static_cast<double>(s[1]), static_cast<double>(s[2]), static_cast<double>(s[3]), worst, orth,
	            static_cast<double>(norm));
}

int main() {
	(void)svdsFloat;
	(void)svdsDouble;
	tall<float>("float", 1e-4f);
	tall<double>("double", 1e-10);
	return 0;
}
