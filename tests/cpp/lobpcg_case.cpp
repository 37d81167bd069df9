// lobpcg_case.cpp -- SMM::lobpcg through the drop-in header (tests/test_cpp_lobpcg.py compiles it, and runs it on a GPU where there is one).
// The two function pointers below prove that the header declares the plain form for float and double.
//
//   lobpcg_case     the five-point Laplacian on a 16 x 12 grid (tests/eigsh_cases.py: lap2d_16x12), its four smallest eigenvalues
//                   (4 - 2 cos(i pi / 17) - 2 cos(j pi / 13)), without a preconditioner and with IC0, in double; in float without:
//                   "<name> status <S> hip <H> nconv <N> iterations <I> applies <P> w <%a> x 4 res <%a>"
//                   res = max_i ||A x_i - w_i x_i||_2, formed here in double from the returned vectors
#include <cmath>
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const lobpcgFloat)(const SMM::CSRMatrix<float>&, int, int, float*, float*, float, int, const float*, unsigned long long, float*,
                                              SMM::LobpcgInfo*) = &SMM::lobpcg<float>;
static SMM::SolverStatus (*const lobpcgDouble)(const SMM::CSRMatrix<double>&, int, int, double*, double*, double, int, const double*, unsigned long long, double*,
                                               SMM::LobpcgInfo*) = &SMM::lobpcg<double>;

template <typename T>
static void grid(const char* name, T tol, bool ic0) {
	const int nx = 16, ny = 12, n = nx * ny, k = 4;
	SMM::TripletMatrix<T> t(n, n);
	for (int y = 0; y < ny; ++y) {
		for (int x = 0; x < nx; ++x) {
			const int r = y * nx + x;
			if (y > 0) t.addEntry(r, r - nx, T(-1));
			if (x > 0) t.addEntry(r, r - 1, T(-1));
			t.addEntry(r, r, T(4));
			if (x + 1 < nx) t.addEntry(r, r + 1, T(-1));
			if (y + 1 < ny) t.addEntry(r, r + nx, T(-1));
		}
	}
	SMM::CSRMatrix<T> m(t);
	T w[k] = {T(0), T(0), T(0), T(0)};
	std::vector<T> v(static_cast<size_t>(n) * k, T(0));
	SMM::LobpcgInfo info;
	SMM::SolverStatus status;
	if (ic0) {
		typename SMM::CSRMatrix<T>::IC0Preconditioner M(m);
		status = SMM::lobpcg(m, k, SMM_EIGSH_SMALLEST, w, v.data(), M, tol, 1000, static_cast<const T*>(nullptr), 0ull, static_cast<T*>(nullptr), &info);
	} else {
		status = SMM::lobpcg(m, k, SMM_EIGSH_SMALLEST, w, v.data(), tol, 1000, static_cast<const T*>(nullptr), 0ull, static_cast<T*>(nullptr), &info);
	}
	double worst = 0;
	for (int i = 0; i < k; ++i) {
		const T* xi = v.data() + static_cast<size_t>(i) * n;
		double sum = 0;
		for (int y = 0; y < ny; ++y) {
			for (int x = 0; x < nx; ++x) {
				const int r = y * nx + x;
				double ax = 4.0 * xi[r];
				if (y > 0) ax -= xi[r - nx];
				if (x > 0) ax -= xi[r - 1];
				if (x + 1 < nx) ax -= xi[r + 1];
				if (y + 1 < ny) ax -= xi[r + nx];
				const double d = ax - static_cast<double>(w[i]) * xi[r];
				sum += d * d;
			}
		}
		worst = std::fmax(worst, std::sqrt(sum));
	}
	std::printf("%s status %d hip %d nconv %d iterations %d applies %d w %a %a %a %a res %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), info.nconv,
	            info.iterations, info.applies, static_cast<double>(w[0]), static_cast<double>(w[1]), static_cast<double>(w[2]), static_cast<double>(w[3]), worst);
}

int main() {
	(void)lobpcgFloat;
	(void)lobpcgDouble;
	grid<float>("float", 1e-4f, false);
	grid<double>("double", 1e-10, false);
	grid<double>("double_ic0", 1e-10, true);
	return 0;
}
