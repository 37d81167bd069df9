// eigsh_case.cpp -- SMM::eigsh through the drop-in header (tests/test_cpp_eigsh.py compiles it, and runs it on a GPU where there is one).
// The two function pointers below prove that the header declares the template for float and double.
//
//   eigsh_case      the chain -1 2 -1 of 12 rows in float and in double, its two largest eigenvalues (2 - 2 cos(j pi / 13), j = 12, 11):
//                   "float status <S> hip <H> nconv <N> w <%a> <%a> res <%a>" / "double ..."
//                   res = max_i ||A x_i - w_i x_i||_2, formed here in double from the returned vectors
#include <cmath>
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const eigshFloat)(const SMM::CSRMatrix<float>&, int, int, float*, float*, int, float, int, const float*, unsigned long long, float*,
                                             SMM::EigshInfo*) = &SMM::eigsh<float>;
static SMM::SolverStatus (*const eigshDouble)(const SMM::CSRMatrix<double>&, int, int, double*, double*, int, double, int, const double*, unsigned long long, double*,
                                              SMM::EigshInfo*) = &SMM::eigsh<double>;

template <typename T>
static void chain(const char* name, T tol) {
	const int n = 12, k = 2;
	SMM::TripletMatrix<T> t(n, n);
	for (int r = 0; r < n; ++r) {
		if (r > 0) t.addEntry(r, r - 1, T(-1));
		t.addEntry(r, r, T(2));
		if (r + 1 < n) t.addEntry(r, r + 1, T(-1));
	}
	SMM::CSRMatrix<T> m(t);
	T w[k] = {T(0), T(0)};
	std::vector<T> x(static_cast<size_t>(n) * k, T(0));
	SMM::EigshInfo info;
	SMM::SolverStatus status = SMM::eigsh(m, k, SMM_EIGSH_LARGEST, w, x.data(), 8, tol, 100, static_cast<const T*>(nullptr), 0ull, static_cast<T*>(nullptr), &info);
	double worst = 0;
	for (int i = 0; i < k; ++i) {
		double sum = 0;
		for (int r = 0; r < n; ++r) {
			double ax = 2.0 * x[i * n + r];
			if (r > 0) ax -= x[i * n + r - 1];
			if (r + 1 < n) ax -= x[i * n + r + 1];
			const double d = ax - static_cast<double>(w[i]) * x[i * n + r];
			sum += d * d;
		}
		worst = std::fmax(worst, std::sqrt(sum));
	}
	std::printf("%s status %d hip %d nconv %d w %a %a res %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), info.nconv, static_cast<double>(w[0]),
	            static_cast<double>(w[1]), worst);
}

int main() {
	(void)eigshFloat;
	(void)eigshDouble;
	chain<float>("float", 1e-4f);
	chain<double>("double", 1e-10);
	return 0;
}
