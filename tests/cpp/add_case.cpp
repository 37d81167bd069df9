// add_case.cpp -- SMM::add, SMM::addInto and the in-place shift through the drop-in header (tests/test_gpu_add.py compiles and runs it on a
// GPU).  Written against the header's API only: TripletMatrix, CSRMatrix and the call shapes
//     int status = SMM::add(a, alpha, b, beta, c);     int status = SMM::addInto(c, a, alpha, b, beta);     (c may be a, b or both)
// The function pointers below prove that the header declares both for float and double.  Checks itself against sums formed here in the
// same way (u = alpha * a, v = beta * b, u + v; one rounding each -- compile without -ffast-math and without contraction) and prints
// "add_case: OK", or the first difference and exit status 1.
#include <cstdio>
#include <cstring>

#include "sparse_matrix_math.h"

static int (*const addFloat)(const SMM::CSRMatrix<float>&, float, const SMM::CSRMatrix<float>&, float, SMM::CSRMatrix<float>&) noexcept = &SMM::add<float>;
static int (*const addDouble)(const SMM::CSRMatrix<double>&, double, const SMM::CSRMatrix<double>&, double, SMM::CSRMatrix<double>&) noexcept = &SMM::add<double>;
static int (*const intoFloat)(SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&, float, const SMM::CSRMatrix<float>&, float) = &SMM::addInto<float>;
static int (*const intoDouble)(SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&, double, const SMM::CSRMatrix<double>&, double) = &SMM::addInto<double>;

constexpr int M = 6, N = 7;

template <typename T>
static bool sameBits(T x, T y) { return std::memcmp(&x, &y, sizeof(T)) == 0; }

template <typename T>
static bool isStored(const SMM::CSRMatrix<T>& c, int i, int j) {
	for (int k = c.rawStart()[i]; k < c.rawStart()[i + 1]; ++k) {
		if (c.rawPositions()[k] == j) return true;
	}
	return false;
}

// c against alpha a + beta b; `keep` (when given) is the pattern c must have, else the union of sa and sb
template <typename T>
static int check(const char* name, const SMM::CSRMatrix<T>& c, const T (&a)[M][N], const bool (&sa)[M][N], T alpha, const T (&b)[M][N], const bool (&sb)[M][N], T beta,
                 const bool (*keep)[N] = nullptr) {
	for (int i = 0; i < M; ++i) {
		int last = -1;
		for (int k = c.rawStart()[i]; k < c.rawStart()[i + 1]; ++k) {
			if (c.rawPositions()[k] <= last) {
				std::printf("%s: the columns of row %d do not ascend\n", name, i);
				return 1;
			}
			last = c.rawPositions()[k];
		}
		for (int j = 0; j < N; ++j) {
			const bool stored = keep ? keep[i][j] : (sa[i][j] || sb[i][j]);
			volatile T u = alpha * a[i][j];
			volatile T v = beta * b[i][j];
			volatile T sum = u + v;
			const T want = sa[i][j] && sb[i][j] ? sum : sa[i][j] ? u : sb[i][j] ? v : T(0);
			const bool has = isStored(c, i, j);
			if (has != stored) {
				std::printf("%s: entry (%d, %d) stored %d, expected %d\n", name, i, j, has ? 1 : 0, stored ? 1 : 0);
				return 1;
			}
			if (stored && !sameBits<T>(c.getValue(i, j), want)) {
				std::printf("%s: entry (%d, %d) is %a, expected %a\n", name, i, j, static_cast<double>(c.getValue(i, j)), static_cast<double>(want));
				return 1;
			}
		}
	}
	return 0;
}

template <typename T>
static int run(const char* name) {
	T a[M][N] = {}, b[M][N] = {}, d[M][N] = {};
	bool sa[M][N] = {}, sb[M][N] = {}, sd[M][N] = {};
	SMM::TripletMatrix<T> ta(M, N), tb(M, N), td(M, N);
	for (int i = 0; i < M; ++i) {
		for (int j = 0; j < N; ++j) {
			if (i != 3 && (i + 2 * j) % 3 != 1) {  // row 3 of a is empty
				a[i][j] = T(1) / T(3 + i + 5 * j) - T(0.1);
				sa[i][j] = true;
				ta.addEntry(i, j, a[i][j]);
			}
			if (i != 4 && (2 * i + j) % 4 < 2) {  // row 4 of b is empty
				b[i][j] = i == 0 && sa[i][j] ? -a[i][j] : T(2) / T(7 + 3 * i + j) - T(0.2);  // row 0: cancels where a stores the entry too
				sb[i][j] = true;
				tb.addEntry(i, j, b[i][j]);
			}
			if (i == j && sa[i][j]) {  // a diagonal inside a's pattern
				d[i][j] = T(i + 1);
				sd[i][j] = true;
				td.addEntry(i, j, d[i][j]);
			}
		}
	}
	SMM::CSRMatrix<T> A(ta), B(tb), D(td), C;
	if (SMM::add(A, 1, B, 1, C) != 0 || SMM::lastHipStatus() != 0) {
		std::printf("%s: add failed with status %d\n", name, SMM::lastHipStatus());
		return 1;
	}
	if (C.getDenseRowCount() != M || C.getDenseColCount() != N) {
		std::printf("%s: the sum is %d x %d\n", name, C.getDenseRowCount(), C.getDenseColCount());
		return 1;
	}
	if (check<T>(name, C, a, sa, T(1), b, sb, T(1))) return 1;
	bool keep[M][N];
	for (int i = 0; i < M; ++i)
		for (int j = 0; j < N; ++j) keep[i][j] = isStored(C, i, j);
	// other scalars, then the numeric phase alone on the pattern of the first sum
	const T alpha = T(0.3), beta = T(-2.5);
	SMM::CSRMatrix<T> C2;
	if (SMM::add(A, alpha, B, beta, C2) != 0 || check<T>(name, C2, a, sa, alpha, b, sb, beta)) return 1;
	if (SMM::addInto(C, A, alpha, B, beta) != 0) {
		std::printf("%s: addInto failed with status %d\n", name, SMM::lastHipStatus());
		return 1;
	}
	if (check<T>(name, C, a, sa, alpha, b, sb, beta, keep)) return 1;
	// an operand with an entry more than c stores: refused, c unchanged
	if (SMM::addInto(D, A, 1, D, 1) != SMM_HIP_ERR_INVALID || SMM::lastHipStatus() != SMM_HIP_ERR_INVALID) {
		std::printf("%s: an entry outside the pattern was not refused\n", name);
		return 1;
	}
	const T zero[M][N] = {};
	const bool none[M][N] = {};
	if (check<T>(name, D, d, sd, T(1), zero, none, T(0))) return 1;
	// the shift in place: A <- A + sigma D, D's pattern inside A's
	const T sigma = T(0.375);
	bool keepA[M][N];
	for (int i = 0; i < M; ++i)
		for (int j = 0; j < N; ++j) keepA[i][j] = sa[i][j];
	if (SMM::addInto(A, A, 1, D, sigma) != 0) {
		std::printf("%s: the in-place shift failed with status %d\n", name, SMM::lastHipStatus());
		return 1;
	}
	if (check<T>(name, A, a, sa, T(1), d, sd, sigma, keepA)) return 1;
	if (SMM::add(A, 1, B, 1, A) != SMM_HIP_ERR_INVALID) {  // out is an operand
		std::printf("%s: a bad call was not refused\n", name);
		return 1;
	}
	return 0;
}

int main() {
	(void)addFloat;
	(void)addDouble;
	(void)intoFloat;
	(void)intoDouble;
	if (run<float>("float") || run<double>("double")) return 1;
	std::printf("add_case: OK\n");
	return 0;
}
