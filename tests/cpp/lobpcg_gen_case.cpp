// lobpcg_gen_case.cpp -- SMM::lobpcg(A, B, ...), the generalised problem A x = lambda B x, through the drop-in header
// (tests/test_cpp_lobpcg_gen.py compiles it, and runs it on a GPU where there is one).  The two function pointers below prove that the
// header declares the plain form for float and double.
//
//   lobpcg_gen_case   the chain of 60 linear elements: A = tridiag(-1, 2, -1), B = tridiag(1, 4, 1) / 6, the two smallest eigenvalues
//                     (6 (1 - c_j) / (2 + c_j), c_j = cos(j pi / 61)), without a preconditioner and with the IC0 of A, in double; in
//                     float without; and B = A in double (every eigenvalue is 1):
//                     "<name> status <S> hip <H> nconv <N> iterations <I> applies <P> bmatvecs <B> w <%a> <%a> res <%a>"
//                     res = max_i ||A x_i - w_i B x_i||_2 / ||B x_i||_2, formed here in double from the returned vectors
#include <cmath>
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const lobpcgFloat)(const SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&, int, int, float*, float*, float, int, const float*,
                                              unsigned long long, float*, SMM::LobpcgGenInfo*) = &SMM::lobpcg<float>;
static SMM::SolverStatus (*const lobpcgDouble)(const SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&, int, int, double*, double*, double, int, const double*,
                                               unsigned long long, double*, SMM::LobpcgGenInfo*) = &SMM::lobpcg<double>;

// y = tridiag(lo, di, lo) x
static void band(int n, double lo, double di, const double* x, double* y) {
	for (int r = 0; r < n; ++r) y[r] = di * x[r] + (r > 0 ? lo * x[r - 1] : 0.0) + (r + 1 < n ? lo * x[r + 1] : 0.0);
}

template <typename T>
static void chain(const char* name, T tol, bool ic0, bool same) {
	const int n = 60, k = 2;
	SMM::TripletMatrix<T> ta(n, n), tb(n, n);
	for (int r = 0; r < n; ++r) {
		if (r > 0) ta.addEntry(r, r - 1, T(-1)), tb.addEntry(r, r - 1, T(1) / T(6));
		ta.addEntry(r, r, T(2)), tb.addEntry(r, r, T(4) / T(6));
		if (r + 1 < n) ta.addEntry(r, r + 1, T(-1)), tb.addEntry(r, r + 1, T(1) / T(6));
	}
	SMM::CSRMatrix<T> a(ta), b(tb);
	const SMM::CSRMatrix<T>& mass = same ? a : b;
	T w[k] = {T(0), T(0)};
	std::vector<T> v(static_cast<size_t>(n) * k, T(0));
	SMM::LobpcgGenInfo info;
	SMM::SolverStatus status;
	if (ic0) {
		typename SMM::CSRMatrix<T>::IC0Preconditioner M(a);
		status = SMM::lobpcg(a, mass, k, SMM_EIGSH_SMALLEST, w, v.data(), M, tol, 1000, static_cast<const T*>(nullptr), 0ull, static_cast<T*>(nullptr), &info);
	} else {
		status = SMM::lobpcg(a, mass, k, SMM_EIGSH_SMALLEST, w, v.data(), tol, 1000, static_cast<const T*>(nullptr), 0ull, static_cast<T*>(nullptr), &info);
	}
	double worst = 0;
	for (int i = 0; i < k; ++i) {
		std::vector<double> x(v.begin() + static_cast<size_t>(i) * n, v.begin() + static_cast<size_t>(i + 1) * n), ax(n), bx(n);
		band(n, -1.0, 2.0, x.data(), ax.data());
		if (same) bx = ax;
		else band(n, 1.0 / 6.0, 4.0 / 6.0, x.data(), bx.data());
		double rr = 0, bb = 0;
		for (int r = 0; r < n; ++r) {
			const double d = ax[r] - static_cast<double>(w[i]) * bx[r];
			rr += d * d;
			bb += bx[r] * bx[r];
		}
		worst = std::fmax(worst, bb > 0 ? std::sqrt(rr / bb) : 0.0);
	}
	std::printf("%s status %d hip %d nconv %d iterations %d applies %d bmatvecs %d w %a %a res %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), info.nconv,
	            info.iterations, info.applies, info.bmatvecs, static_cast<double>(w[0]), static_cast<double>(w[1]), worst);
}

int main() {
	(void)lobpcgFloat;
	(void)lobpcgDouble;
	chain<float>("float", 1e-4f, false, false);
	chain<double>("double", 1e-10, false, false);
	chain<double>("double_ic0", 1e-10, true, false);
	chain<double>("double_same", 1e-10, false, true);
	return 0;
}
