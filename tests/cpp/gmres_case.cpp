// gmres_case.cpp -- SMM::GMRES through the drop-in header (tests/test_gmres_cpu.py compiles it; tests/test_gpu_gmres.py runs it on a
// GPU).  GMRES is an addition of this library; the case is written against the reference's types (TripletMatrix, CSRMatrix) and the call
// shape of its solvers plus the restart length:
//     SMM::SolverStatus status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition, restart);
//     SMM::SolverStatus status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition, restart, preconditioner);
// The two function pointers below prove that the header declares the plain template for float and double.
//
//   gmres_case                     a 3 x 3 system in float and in double, plain and with the Jacobi preconditioner:
//                                  "float status <S> hip <H> x ..." / "double ..." / "float-jacobi ..." / "double-jacobi ..."
//   gmres_case <matrix file> <eps> the matrix of the file in double, rhs = row sums, x0 = 0, maxIterations = -1, restart 30:
//                                  "status <S> hip <H>" and one "x <%a>" per row
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static SMM::SolverStatus (*const gmresFloat)(const SMM::CSRMatrix<float>&, float*, float*, int, float, int) = &SMM::GMRES<float>;
static SMM::SolverStatus (*const gmresDouble)(const SMM::CSRMatrix<double>&, double*, double*, int, double, int) = &SMM::GMRES<double>;

template <typename T>
static void small(const char* name, bool jacobi) {
	SMM::TripletMatrix<T> t(3, 3);  // non-symmetric, diagonally dominant
	t.addEntry(0, 0, T(4));
	t.addEntry(0, 1, T(-1));
	t.addEntry(1, 0, T(-2));
	t.addEntry(1, 1, T(5));
	t.addEntry(1, 2, T(-1));
	t.addEntry(2, 1, T(-2));
	t.addEntry(2, 2, T(6));
	SMM::CSRMatrix<T> m(t);
	T rhs[3] = {T(3), T(2), T(4)};  // the row sums: x = 1
	T res[3] = {T(0), T(0), T(0)};
	const int maxIterations = 100;
	const T L2NormCondition = T(1e-6);
	SMM::SolverStatus status;
	if (jacobi) {
		auto preconditioner = m.template getPreconditioner<SMM::SolverPreconditioner::JACOBI>();
		status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition, 2, preconditioner);
	} else {
		status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition);
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
	SMM::SolverStatus status = gmresDouble(m, rhs.data(), res.data(), -1, eps, 30);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 3) return fromFile(argv[1], std::atof(argv[2]));
	(void)gmresFloat;
	small<float>("float", false);
	small<double>("double", false);
	small<float>("float-jacobi", true);
	small<double>("double-jacobi", true);
	return 0;
}
