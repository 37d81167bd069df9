// jacobi_case.cpp -- the host-only small eigenproblem and small SVD of sparse_matrix_math_amd/csrc/smm_jacobi.h on their own: host compiler,
// AddressSanitizer + UBSan, no library, no GPU.  The drivers reach them only through whole solves, which rarely project onto a
// rank-deficient matrix.  Every product below is accumulated in long double; every figure is printed before it is judged.
// The bounds: each element of an output is ONE rounding to fp64 (2^-53 relative) of a matrix that is orthogonal in the wider format, so a
// Gram entry of m terms is off by at most m 2^-52 and some slack (4 m 2^-52); a residual entry adds the rounding of the value (8 m 2^-52
// times the largest value).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../sparse_matrix_math_amd/csrc/smm_jacobi.h"

typedef long double R;
static const R EPS = 0x1p-52L;

static int checks = 0, failed = 0;
#define CHECK(cond)                                                     \
	do {                                                                \
		++checks;                                                       \
		if (!(cond)) {                                                  \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
			++failed;                                                   \
		}                                                               \
	} while (0)

static void checkWithin(const char* name, const char* what, R value, R bound) {
	std::printf("%-28s %-18s %.3Le  (bound %.3Le)\n", name, what, value, bound);
	++checks;
	if (!(value <= bound)) {
		std::printf("FAILED %s: %s\n", name, what);
		++failed;
	}
}

// a fixed sequence in (-1, 1): the cases are the same on every run
static unsigned long long lcgState = 0x2545F4914F6CDD1Dull;
static double lcg() {
	lcgState = lcgState * 6364136223846793005ull + 1442695040888963407ull;
	return static_cast<double>(static_cast<long long>(lcgState >> 11) - (1LL << 52)) / static_cast<double>(1LL << 52);
}

static bool allFinite(const std::vector<double>& v) {
	for (double e : v) {
		if (!std::isfinite(e)) return false;
	}
	return true;
}

// max |Q^T Q - I| of the `cols` columns of q (rows x cols, q[r * cols + i])
static R gramError(int rows, int cols, const std::vector<double>& q) {
	R worst = 0;
	for (int i = 0; i < cols; ++i) {
		for (int j = 0; j < cols; ++j) {
			R s = 0;
			for (int r = 0; r < rows; ++r) s += static_cast<R>(q[r * cols + i]) * static_cast<R>(q[r * cols + j]);
			worst = std::max(worst, std::fabs(s - (i == j ? R(1) : R(0))));
		}
	}
	return worst;
}

// max |A Q - P diag(d)|: a (rows x inner, row-major), q (inner x cols), p (rows x cols)
static R residual(int rows, int inner, int cols, const std::vector<double>& a, const std::vector<double>& q, const std::vector<double>& p, const std::vector<double>& d) {
	R worst = 0;
	for (int r = 0; r < rows; ++r) {
		for (int i = 0; i < cols; ++i) {
			R s = 0;
			for (int c = 0; c < inner; ++c) s += static_cast<R>(a[r * inner + c]) * static_cast<R>(q[c * cols + i]);
			worst = std::max(worst, std::fabs(s - static_cast<R>(p[r * cols + i]) * static_cast<R>(d[i])));
		}
	}
	return worst;
}

static void eigenCase(const char* name, int m, const std::vector<double>& t) {
	std::vector<double> theta, y;
	CHECK(smm::jacobiEigen(m, t, theta, y));
	CHECK(static_cast<int>(theta.size()) == m && static_cast<int>(y.size()) == m * m);
	if (static_cast<int>(theta.size()) != m || static_cast<int>(y.size()) != m * m) return;
	CHECK(allFinite(theta) && allFinite(y));
	R thetaMax = 0;
	for (int i = 0; i < m; ++i) {
		if (i + 1 < m) CHECK(theta[i] <= theta[i + 1]);
		thetaMax = std::max(thetaMax, std::fabs(static_cast<R>(theta[i])));
	}
	checkWithin(name, "|Y^T Y - I|", gramError(m, m, y), 4 * m * EPS);
	checkWithin(name, "|T Y - Y theta|", residual(m, m, m, t, y, y, theta), 8 * m * EPS * thetaMax);
}

// bt: p x q, row-major, the transpose of B
static void svdCase(const char* name, int p, int q, const std::vector<double>& bt) {
	std::vector<double> sigma, x, y;
	CHECK(smm::jacobiSvd(p, q, bt, sigma, x, y));
	CHECK(static_cast<int>(sigma.size()) == q && static_cast<int>(x.size()) == q * q && static_cast<int>(y.size()) == p * q);
	if (static_cast<int>(sigma.size()) != q || static_cast<int>(x.size()) != q * q || static_cast<int>(y.size()) != p * q) return;
	CHECK(allFinite(sigma) && allFinite(x) && allFinite(y));  // (a NaN would also slip through every max below)
	for (int i = 0; i < q; ++i) {
		CHECK(sigma[i] >= 0);
		if (i + 1 < q) CHECK(sigma[i] >= sigma[i + 1]);
	}
	checkWithin(name, "|X^T X - I|", gramError(q, q, x), 4 * p * EPS);
	checkWithin(name, "|Y^T Y - I|", gramError(p, q, y), 4 * p * EPS);
	checkWithin(name, "|B^T X - Y sigma|", residual(p, q, q, bt, x, y, sigma), 8 * p * EPS * static_cast<R>(sigma[0]));
}

// what eigsh hands over after a restart that kept l Ritz values: diag(kept), the arrow in row and column l, the new tridiagonal part
static std::vector<double> arrowTridiagonal(int m, int l) {
	std::vector<double> t(static_cast<size_t>(m) * m, 0.0);
	for (int i = 0; i < l; ++i) {
		t[i * m + i] = 8.0 - 0.5 * i + 0.1 * lcg();
		t[i * m + l] = t[l * m + i] = 0.05 * lcg();
	}
	for (int j = l; j < m; ++j) {
		t[j * m + j] = 3.0 * lcg();
		if (j + 1 < m) t[j * m + j + 1] = t[(j + 1) * m + j] = 1.0 + 0.5 * lcg();
	}
	return t;
}

// what svds hands over: B^T (mv x m) with diag(kept), the arrow in B's column l, alpha on the rest of the diagonal and beta above it in B
static std::vector<double> arrowBidiagonal(int mv, int m, int l) {
	std::vector<double> bt(static_cast<size_t>(mv) * m, 0.0);
	for (int i = 0; i < l; ++i) {
		bt[i * m + i] = 8.0 - 0.5 * i + 0.1 * lcg();
		bt[l * m + i] = 0.05 * lcg();
	}
	for (int j = l; j < m; ++j) {
		bt[j * m + j] = 2.0 + lcg();
		if (j + 1 < mv) bt[(j + 1) * m + j] = 1.0 + 0.5 * lcg();
	}
	return bt;
}

int main() {
	const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

	// ---- jacobiEigen
	eigenCase("eigen m=1", 1, {3.5});
	eigenCase("eigen m=2", 2, {2.0, 1.0, 1.0, -1.0});
	const std::vector<double> t20 = arrowTridiagonal(20, 6);
	eigenCase("eigen 20x20 arrow l=6", 20, t20);
	{
		std::vector<double> t = t20, theta, y;
		t[7 * 20 + 8] = t[8 * 20 + 7] = nan;
		CHECK(!smm::jacobiEigen(20, t, theta, y));
	}

	// ---- jacobiSvd, full rank
	svdCase("svd 1x1", 1, 1, {-2.5});
	svdCase("svd 3x2", 3, 2, {1.0, 2.0, -0.5, 0.25, 3.0, 1.5});
	const std::vector<double> bt2120 = arrowBidiagonal(21, 20, 6);  // after a breakdown at an alpha: one more row of V than of U
	svdCase("svd 21x20 arrow l=6", 21, 20, bt2120);
	svdCase("svd 20x20 arrow l=6", 20, 20, arrowBidiagonal(20, 20, 6));

	// ---- jacobiSvd, rank-deficient: Y is completed to orthonormal columns, nothing divides by a zero norm
	svdCase("svd zero 4x3", 4, 3, std::vector<double>(12, 0.0));
	svdCase("svd zero 3x3", 3, 3, std::vector<double>(9, 0.0));
	{
		std::vector<double> bt(25, 0.0);
		for (int i = 0; i < 5; ++i) bt[i * 5 + i] = i == 2 ? 0.0 : 1.0;
		svdCase("svd identity, one zero", 5, 5, bt);
	}
	{
		std::vector<double> bt(20);
		for (int r = 0; r < 5; ++r) {
			for (int c = 0; c < 4; ++c) bt[r * 4 + c] = lcg();
			bt[r * 4 + 3] = bt[r * 4 + 1];
		}
		svdCase("svd two equal columns", 5, 4, bt);
	}
	{
		std::vector<double> bt = bt2120, sigma, x, y;
		bt[9 * 20 + 9] = inf;
		CHECK(!smm::jacobiSvd(21, 20, bt, sigma, x, y));
	}

	std::printf("jacobi_case: %d checks, %d failed\n", checks, failed);
	return failed ? 1 : 0;
}
