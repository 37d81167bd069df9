// spgemm_case.cpp -- SMM::multiply and SMM::multiplyInto through the drop-in header (tests/test_gpu_spgemm.py compiles and runs it on a
// GPU).  Written against the header's API only: TripletMatrix, CSRMatrix and the call shapes
//     int status = SMM::multiply(a, b, c);     int status = SMM::multiplyInto(c, a, b);
// The function pointers below prove that the header declares both for float and double.  Checks itself against a dense product formed
// in the same order (p ascending, a * b + c with two roundings -- compile without -ffast-math and without contraction) and prints
// "spgemm_case: OK", or the first difference and exit status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

static int (*const multiplyFloat)(const SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&, SMM::CSRMatrix<float>&) noexcept = &SMM::multiply<float>;
static int (*const multiplyDouble)(const SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&, SMM::CSRMatrix<double>&) noexcept = &SMM::multiply<double>;
static int (*const intoFloat)(SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&) = &SMM::multiplyInto<float>;
static int (*const intoDouble)(SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&) = &SMM::multiplyInto<double>;

constexpr int M = 5, K = 4, N = 6;

template <typename T>
static bool sameBits(T x, T y) { return std::memcmp(&x, &y, sizeof(T)) == 0; }

template <typename T>
static bool isStored(const SMM::CSRMatrix<T>& c, int i, int j) {
	for (int k = c.rawStart()[i]; k < c.rawStart()[i + 1]; ++k) {
		if (c.rawPositions()[k] == j) return true;
	}
	return false;
}

// the stored entries of a (M x K) and b (K x N): value 0 = not stored, except where `stored` says so
template <typename T>
static int check(const char* name, const SMM::CSRMatrix<T>& c, const T (&a)[M][K], const bool (&sa)[M][K], const T (&b)[K][N], const bool (&sb)[K][N],
                 const bool (*keep)[N] = nullptr) {
	for (int i = 0; i < M; ++i) {
		for (int j = 0; j < N; ++j) {
			bool stored = false;
			volatile T acc = T(0);
			for (int p = 0; p < K; ++p) {
				if (sa[i][p] && sb[p][j]) {
					stored = true;
					volatile T prod = a[i][p] * b[p][j];
					acc = prod + acc;
				}
			}
			if (keep) stored = keep[i][j];
			const bool has = isStored(c, i, j);
			if (has != stored) {
				std::printf("%s: entry (%d, %d) stored %d, expected %d\n", name, i, j, has ? 1 : 0, stored ? 1 : 0);
				return 1;
			}
			if (stored && !sameBits<T>(c.getValue(i, j), acc)) {
				std::printf("%s: entry (%d, %d) is %a, expected %a\n", name, i, j, static_cast<double>(c.getValue(i, j)), static_cast<double>(acc));
				return 1;
			}
		}
	}
	return 0;
}

template <typename T>
static int run(const char* name) {
	T a[M][K] = {}, b[K][N] = {};
	bool sa[M][K] = {}, sb[K][N] = {};
	SMM::TripletMatrix<T> ta(M, K), tb(K, N);
	for (int i = 0; i < M; ++i) {
		for (int p = 0; p < K; ++p) {
			if (i == 3 || (i + 2 * p) % 3 == 1) continue;  // row 3 of a is empty
			a[i][p] = T(1) / T(3 + i + 5 * p) - T(0.1);
			sa[i][p] = true;
			ta.addEntry(i, p, a[i][p]);
		}
	}
	for (int p = 0; p < K; ++p) {
		for (int j = 0; j < N; ++j) {
			if (p == 2 || j == 4 || (p + j) % 2 == 1) continue;  // row 2 of b is empty but referenced, column 4 is empty
			b[p][j] = T(2) / T(7 + 3 * p + j) - T(0.2);
			sb[p][j] = true;
			tb.addEntry(p, j, b[p][j]);
		}
	}
	SMM::CSRMatrix<T> A(ta), B(tb), C;
	if (SMM::multiply(A, B, C) != 0 || SMM::lastHipStatus() != 0) {
		std::printf("%s: multiply failed with status %d\n", name, SMM::lastHipStatus());
		return 1;
	}
	if (C.getDenseRowCount() != M || C.getDenseColCount() != N) {
		std::printf("%s: the product is %d x %d\n", name, C.getDenseRowCount(), C.getDenseColCount());
		return 1;
	}
	if (check<T>(name, C, a, sa, b, sb)) return 1;
	bool keep[M][N];
	for (int i = 0; i < M; ++i)
		for (int j = 0; j < N; ++j) keep[i][j] = isStored(C, i, j);
	// new values on the same patterns, then the numeric phase alone
	A *= T(-1.5);
	for (int i = 0; i < M; ++i)
		for (int p = 0; p < K; ++p) a[i][p] = a[i][p] * T(-1.5);
	if (SMM::multiplyInto(C, A, B) != 0) {
		std::printf("%s: multiplyInto failed with status %d\n", name, SMM::lastHipStatus());
		return 1;
	}
	if (check<T>(name, C, a, sa, b, sb, keep)) return 1;
	// a factor with an entry more, whose product has no place in C: refused, C unchanged
	SMM::TripletMatrix<T> tb2(K, N);
	for (int p = 0; p < K; ++p)
		for (int j = 0; j < N; ++j)
			if (sb[p][j]) tb2.addEntry(p, j, b[p][j]);
	tb2.addEntry(0, 4, T(1));
	SMM::CSRMatrix<T> B2(tb2);
	if (SMM::multiplyInto(C, A, B2) != SMM_HIP_ERR_INVALID || SMM::lastHipStatus() != SMM_HIP_ERR_INVALID) {
		std::printf("%s: a product outside the pattern was not refused\n", name);
		return 1;
	}
	if (check<T>(name, C, a, sa, b, sb, keep)) return 1;
	if (SMM::multiplyInto(C, C, B) != SMM_HIP_ERR_INVALID || SMM::multiply(B, B, C) != SMM_HIP_ERR_INVALID) {  // c is a; 6 columns against 4 rows
		std::printf("%s: a bad call was not refused\n", name);
		return 1;
	}
	return 0;
}

int main() {
	(void)multiplyFloat;
	(void)multiplyDouble;
	(void)intoFloat;
	(void)intoDouble;
	if (run<float>("float") || run<double>("double")) return 1;
	std::printf("spgemm_case: OK\n");
	return 0;
}
