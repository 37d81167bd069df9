// idrs_case.cpp -- SMM::IDRs through the drop-in header (tests/test_idrs_cpu.py compiles it; tests/test_gpu_idrs.py runs it on a
// GPU).  IDR(s) is an addition of this library; the case is written against the reference's types (TripletMatrix, CSRMatrix) and the call
// shape of its solvers plus the number of shadow vectors:
//     SMM::SolverStatus status = SMM::IDRs(m, rhs, res, maxIterations, L2NormCondition, s);
//     SMM::SolverStatus status = SMM::IDRs(m, rhs, res, maxIterations, L2NormCondition, s, preconditioner);
// The two function pointers below prove that the header declares the plain template for float and double.
//
//   idrs_case                      an 8 x 8 system in float and in double (the first three x), plain and with the Jacobi preconditioner:
//                                  "float status <S> hip <H> x ..." / "double ..." / "float-jacobi ..." / "double-jacobi ..."
//   idrs_case <matrix file> <eps>  the matrix of the file in double, rhs = row sums, x0 = 0, maxIterations = -1, s = 4:
//                                  "status <S> hip <H>" and one "x <%a>" per row
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const idrsFloat)(const SMM::CSRMatrix<float>&, float*, float*, int, float, int) = &SMM::IDRs<float>;
static SMM::SolverStatus (*const idrsDouble)(const SMM::CSRMatrix<double>&, double*, double*, int, double, int) = &SMM::IDRs<double>;

template <typename T>
static void small(const char* name, bool jacobi) {
	const int n = 8;  // tridiagonal, non-symmetric, diagonally dominant; more rows than the default s = 4 shadow vectors
	SMM::TripletMatrix<T> t(n, n);
	T rhs[n], res[n];
	for (int i = 0; i < n; ++i) {
		rhs[i] = T(4);
		res[i] = T(0);
		if (i > 0) {
			t.addEntry(i, i - 1, T(-2));
			rhs[i] += T(-2);
		}
		t.addEntry(i, i, T(4));
		if (i + 1 < n) {
			t.addEntry(i, i + 1, T(-1));
			rhs[i] += T(-1);
		}
	}
	SMM::CSRMatrix<T> m(t);  // rhs = the row sums: x = 1
	const int maxIterations = 100;
	const T L2NormCondition = T(1e-6);
	SMM::SolverStatus status;
	if (jacobi) {
		auto preconditioner = m.template getPreconditioner<SMM::SolverPreconditioner::JACOBI>();
		status = SMM::IDRs(m, rhs, res, maxIterations, L2NormCondition, 2, preconditioner);
	} else {
		status = SMM::IDRs(m, rhs, res, maxIterations, L2NormCondition);
	}
	std::printf("%s status %d hip %d x %a %a %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), static_cast<double>(res[0]), static_cast<double>(res[1]),
	            static_cast<double>(res[2]));
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
	SMM::SolverStatus status = idrsDouble(m, rhs.data(), res.data(), -1, eps, 4);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 3) return fromFile(argv[1], std::atof(argv[2]));
	(void)idrsFloat;
	small<float>("float", false);
	small<double>("double", false);
	small<float>("float-jacobi", true);
	small<double>("double-jacobi", true);
	return 0;
}
