// minres_case.cpp -- SMM::MINRES through the drop-in header (tests/test_minres_cpu.py compiles it; tests/test_gpu_minres.py runs it on a
// GPU).  The two function pointers below prove that the header declares the unpreconditioned template for float and double.
//
//   minres_case                                            a 3 x 3 indefinite system in float and in double:
//                                                          "float status <S> hip <H> x <%a> <%a> <%a>" / "double ..."
//   minres_case <matrix> <spd matrix> <rhs> <x> <eps>      the matrix of the first file in double, solved from x0 = 0 with maxIterations = -1,
//                                                          once plainly and once with the IC0 preconditioner of the SECOND matrix (a positive
//                                                          definite relative of the first, of the same size):
//                                                          "plain status <S> hip <H> passes <P> maxdiff <%a>" / "ic0 ..."
//                                                          maxdiff = max|x - x_file| over the values of the file <x>; passes: from the C ABI
//                                                          on the same device handles, which returns the count the header's call drops
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.  vector file: one value per line.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const minresFloat)(const SMM::CSRMatrix<float>&, float*, float*, int, float) = &SMM::MINRES<float>;
static SMM::SolverStatus (*const minresDouble)(const SMM::CSRMatrix<double>&, double*, double*, int, double) = &SMM::MINRES<double>;

template <typename T>
static void small(const char* name) {
	SMM::TripletMatrix<T> t(3, 3);  // symmetric, eigenvalues of both signs (the trace of the leading 2 x 2 block is 0)
	t.addEntry(0, 0, T(2));
	t.addEntry(0, 1, T(1));
	t.addEntry(1, 0, T(1));
	t.addEntry(1, 1, T(-2));
	t.addEntry(1, 2, T(1));
	t.addEntry(2, 1, T(1));
	t.addEntry(2, 2, T(3));
	SMM::CSRMatrix<T> m(t);
	T rhs[3] = {T(3), T(0), T(4)};  // the row sums: x = 1
	T res[3] = {T(0), T(0), T(0)};
	SMM::SolverStatus status = SMM::MINRES(m, rhs, res, 100, T(1e-6));
	std::printf("%s status %d hip %d x %a %a %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), static_cast<double>(res[0]), static_cast<double>(res[1]),
	            static_cast<double>(res[2]));
}

static bool readMatrix(const char* path, SMM::TripletMatrix<double>& t) {
	std::FILE* f = std::fopen(path, "r");
	if (!f) return false;
	int rows = 0, entries = 0;
	if (std::fscanf(f, "%d %d", &rows, &entries) != 2) return false;
	t.init(rows, rows, entries);
	for (int k = 0; k < entries; ++k) {
		int r = 0, c = 0;
		double v = 0;
		if (std::fscanf(f, "%d %d %lf", &r, &c, &v) != 3) return false;
		t.addEntry(r, c, v);
	}
	std::fclose(f);
	return true;
}

static bool readVector(const char* path, std::vector<double>& v) {
	std::FILE* f = std::fopen(path, "r");
	if (!f) return false;
	double e = 0;
	while (std::fscanf(f, "%lf", &e) == 1) v.push_back(e);
	std::fclose(f);
	return true;
}

static double maxDiff(const std::vector<double>& a, const std::vector<double>& b) {
	double worst = 0;
	for (size_t i = 0; i < a.size(); ++i) worst = std::fmax(worst, std::fabs(a[i] - b[i]));
	return worst;
}

static int fromFiles(char** argv) {
	SMM::TripletMatrix<double> ta, tl;
	std::vector<double> rhs, want;
	if (!readMatrix(argv[1], ta) || !readMatrix(argv[2], tl) || !readVector(argv[3], rhs) || !readVector(argv[4], want)) return 2;
	const double eps = std::atof(argv[5]);
	SMM::CSRMatrix<double> a(ta), l(tl);
	const size_t rows = rhs.size();
	if (want.size() != rows) return 2;
	int st = 0, passes = 0;

	std::vector<double> x(rows, 0.0), again(rows, 0.0);
	SMM::SolverStatus status = minresDouble(a, rhs.data(), x.data(), -1, eps);
	const int hipPlain = SMM::lastHipStatus();
	smm_hip_minres_f64(a.device(), rhs.data(), again.data(), -1, eps, nullptr, &st, &passes, nullptr);
	std::printf("plain status %d hip %d passes %d maxdiff %a\n", static_cast<int>(status), hipPlain, passes, maxDiff(x, want));

	SMM::CSRMatrix<double>::IC0Preconditioner M(l);
	std::vector<double> xm(rows, 0.0);
	status = SMM::MINRES(a, rhs.data(), xm.data(), -1, eps, M);
	const int hipIc0 = SMM::lastHipStatus();
	std::fill(again.begin(), again.end(), 0.0);
	passes = 0;
	smm_hip_minres_f64(a.device(), rhs.data(), again.data(), -1, eps, M.handle(), &st, &passes, nullptr);
	std::printf("ic0 status %d hip %d passes %d maxdiff %a\n", static_cast<int>(status), hipIc0, passes, maxDiff(xm, want));
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 6) return fromFiles(argv);
	(void)minresFloat;
	small<float>("float");
	small<double>("double");
	return 0;
}
