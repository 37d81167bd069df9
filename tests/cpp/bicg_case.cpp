// bicg_case.cpp -- SMM::transpose, SMM::isSymmetric and SMM::BiCG through the drop-in header (tests/test_bicg_cpu.py compiles it;
// tests/test_gpu_bicg.py runs it on a GPU).  Written against the header's API only: TripletMatrix, CSRMatrix and the call shapes
//     SMM::transpose(m, mt);   SMM::SolverStatus status = SMM::BiCG(m, mt, rhs, res, maxIterations, L2NormCondition);
// The function pointers below prove that the header declares both overloads of BiCG for float and double.
//
//   bicg_case                     a 3 x 3 system that is not symmetric, in float and in double:
//                                 "<type> status <S> hip <H> x <%a> <%a> <%a> noat <S> sym <0|1> tsym <0|1> t01 <%a>"
//                                 (status / x: BiCG with the built transpose; noat: the overload without `at`; sym: isSymmetric(m);
//                                 tsym: isSymmetric of a symmetric 2 x 2 matrix; t01: entry (0, 1) of the transpose, -2 = m's (1, 0))
//   bicg_case <matrix file> <eps> the matrix of the file in double, rhs = row sums, x0 = 0, maxIterations = -1:
//                                 "status <S> hip <H>" and one "x <%a>" per row
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const bicgFloat)(const SMM::CSRMatrix<float>&, const SMM::CSRMatrix<float>&, float*, float*, int, float) = &SMM::BiCG<float>;
static SMM::SolverStatus (*const bicgDouble)(const SMM::CSRMatrix<double>&, const SMM::CSRMatrix<double>&, double*, double*, int, double) = &SMM::BiCG<double>;
static SMM::SolverStatus (*const bicgNoAtFloat)(const SMM::CSRMatrix<float>&, float*, float*, int, float) = &SMM::BiCG<float>;
static SMM::SolverStatus (*const bicgNoAtDouble)(const SMM::CSRMatrix<double>&, double*, double*, int, double) = &SMM::BiCG<double>;

template <typename T>
static void small(const char* name) {
	SMM::TripletMatrix<T> t(3, 3);  // non-symmetric, diagonally dominant
	t.addEntry(0, 0, T(4));
	t.addEntry(0, 1, T(-1));
	t.addEntry(1, 0, T(-2));
	t.addEntry(1, 1, T(5));
	t.addEntry(1, 2, T(-1));
	t.addEntry(2, 1, T(-2));
	t.addEntry(2, 2, T(6));
	SMM::CSRMatrix<T> m(t);
	SMM::CSRMatrix<T> mt;
	const int made = SMM::transpose(m, mt);
	T rhs[3] = {T(3), T(2), T(4)};  // the row sums: x = 1
	T res[3] = {T(0), T(0), T(0)};
	const int maxIterations = 100;
	const T L2NormCondition = T(1e-6);
	SMM::SolverStatus status = SMM::BiCG(m, mt, rhs, res, maxIterations, L2NormCondition);
	const int hip = made != 0 ? made : SMM::lastHipStatus();
	T res2[3] = {T(0), T(0), T(0)};
	SMM::SolverStatus noAt = SMM::BiCG(m, rhs, res2, maxIterations, L2NormCondition);
	SMM::TripletMatrix<T> s(2, 2);
	s.addEntry(0, 0, T(2));
	s.addEntry(0, 1, T(-1));
	s.addEntry(1, 0, T(-1));
	s.addEntry(1, 1, T(2));
	SMM::CSRMatrix<T> sym(s);
	const bool mSym = SMM::isSymmetric(m), sSym = SMM::isSymmetric(sym);
	std::printf("%s status %d hip %d x %a %a %a noat %d sym %d tsym %d t01 %a\n", name, static_cast<int>(status), hip, static_cast<double>(res[0]),
	            static_cast<double>(res[1]), static_cast<double>(res[2]), static_cast<int>(noAt), mSym ? 1 : 0, sSym ? 1 : 0,
	            made == 0 ? static_cast<double>(mt.getValue(0, 1)) : 0.0);
}

static int fromFile(const char* path, double eps) {
	std::FILE* f = std::fopen(path, "r");
	if (!f) return 2;
	int rows = 0, entries = 0;
	if (std::fscanf(f, "%d %d", &rows, &entries) != 2) return 2;
	SMM::TripletMatrix<double> t(rows, rows);
	std::vector<double> rhs(static_cast<size_t>(rows), 0.0), res(static_cast<size_t>(rows), 0.0);
	for (int k = 0; k < entries; ++k) {
		int r = 0, c = 0;
		double v = 0;
		if (std::fscanf(f, "%d %d %lf", &r, &c, &v) != 3) return 2;
		t.addEntry(r, c, v);
		rhs[static_cast<size_t>(r)] += v;
	}
	std::fclose(f);
	SMM::CSRMatrix<double> m(t);
	SMM::CSRMatrix<double> mt;
	if (SMM::transpose(m, mt) != 0) {
		std::printf("status 1 hip %d\n", SMM::lastHipStatus());
		return 0;
	}
	SMM::SolverStatus status = bicgDouble(m, mt, rhs.data(), res.data(), -1, eps);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 3) return fromFile(argv[1], std::atof(argv[2]));
	(void)bicgFloat;
	(void)bicgNoAtFloat;
	(void)bicgNoAtDouble;
	small<float>("float");
	small<double>("double");
	return 0;
}
