// ainv_case.cpp -- the FSAI / SPAI preconditioners through the drop-in header (tests/test_ainv_cpu.py compiles it; tests/test_gpu_ainv.py
// runs it on a GPU).  The preconditioners are additions of this library; the case is written against the reference's types
// (TripletMatrix, CSRMatrix) and the call shape of its preconditioned solvers:
//     SMM::ApproximateInversePreconditioner<T> M(m, SMM_PRECOND_FSAI, power);
//     SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M);
//     SMM::SolverStatus status = SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M);
//     SMM::SolverStatus status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition, restart, M);
//
//   ainv_case                     a 3 x 3 symmetric system in float and in double, through the three solvers:
//                                 "<float|double>-<cg|bicgstab|gmres> status <S> hip <H> x ..."
//   ainv_case <matrix file> <eps> the matrix of the file in double, rhs = row sums, x0 = 0, maxIterations = -1, ConjugateGradient with FSAI at
//                                 power 1: "status <S> hip <H>" and one "x <%a>" per row
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

template <typename T>
static void small(const char* name, int solver) {
	SMM::TripletMatrix<T> t(3, 3);  // symmetric, diagonally dominant
	t.addEntry(0, 0, T(4));
	t.addEntry(0, 1, T(-1));
	t.addEntry(1, 0, T(-1));
	t.addEntry(1, 1, T(5));
	t.addEntry(1, 2, T(-2));
	t.addEntry(2, 1, T(-2));
	t.addEntry(2, 2, T(6));
	SMM::CSRMatrix<T> m(t);
	T rhs[3] = {T(3), T(2), T(4)};  // the row sums: x = 1
	T x0[3] = {T(0), T(0), T(0)};
	T res[3] = {T(0), T(0), T(0)};
	const int maxIterations = 100;
	const T L2NormCondition = T(1e-6);
	SMM::SolverStatus status;
	if (solver == 0) {
		SMM::ApproximateInversePreconditioner<T> M(m, SMM_PRECOND_FSAI, 2);
		status = SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M);
	} else if (solver == 1) {
		SMM::ApproximateInversePreconditioner<T> M(m, SMM_PRECOND_SPAI);
		status = SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M);
	} else {
		SMM::ApproximateInversePreconditioner<T> M(m, SMM_PRECOND_SPAI, 2);
		if (M.power() != 2) std::abort();
		status = SMM::GMRES(m, rhs, res, maxIterations, L2NormCondition, 3, M);
		if (status == SMM::SolverStatus::SUCCESS && M.refresh() != 0) std::abort();
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
	std::vector<double> rhs(static_cast<size_t>(rows), 0.0), x0(static_cast<size_t>(rows), 0.0), res(static_cast<size_t>(rows), 0.0);
	for (int k = 0; k < entries; ++k) {
		int r = 0, c = 0;
		double v = 0;
		if (std::fscanf(f, "%d %d %lf", &r, &c, &v) != 3) return 2;
		t.addEntry(r, c, v);
		rhs[static_cast<size_t>(r)] += v;
	}
	std::fclose(f);
	SMM::CSRMatrix<double> m(t);
	SMM::ApproximateInversePreconditioner<double> M(m, SMM_PRECOND_FSAI, 1);
	SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs.data(), x0.data(), res.data(), -1, eps, M);
	int power = -1, maxRow = -1;
	size_t nnz = 0;
	if (M.info(&power, &maxRow, &nnz) == 0) std::fprintf(stderr, "power %d longest row %d entries %zu\n", power, maxRow, nnz);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 3) return fromFile(argv[1], std::atof(argv[2]));
	small<float>("float-cg", 0);
	small<double>("double-cg", 0);
	small<float>("float-bicgstab", 1);
	small<double>("double-bicgstab", 1);
	small<float>("float-gmres", 2);
	small<double>("double-gmres", 2);
	return 0;
}
