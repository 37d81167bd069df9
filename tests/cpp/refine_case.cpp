// refine_case.cpp -- SMM::convert and SMM::IterativeRefinement through the drop-in header (tests/test_refine_cpu.py compiles it;
// tests/test_gpu_refine.py runs it on a GPU).  Both are additions of this library; the case is written against the reference's types
// (TripletMatrix, CSRMatrix) and the call shape of its solvers:
//     SMM::CSRMatrix<float> m32 = SMM::convert<float>(m);
//     SMM::SolverStatus status = SMM::IterativeRefinement(m, m32, rhs, res, L2NormCondition);
//     SMM::SolverStatus status = SMM::IterativeRefinement(m, rhs, res, L2NormCondition);          (converts for the call)
//
//   refine_case                     a 3 x 3 system: "kept status <S> hip <H> outer <O> x ..." with a kept float matrix and BiCGStab + Jacobi
//                                   inside, "call status ..." with the matrix converted for the call and CG inside, and "roundtrip <0|1>":
//                                   whether float -> double -> float gave the float matrix back
//   refine_case <matrix file> <eps> the matrix of the file in double, rhs = row sums, x0 = 0, CG inside:
//                                   "status <S> hip <H>" and one "x <%a>" per row
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static void line(const char* name, SMM::SolverStatus status, const SMM::RefinementInfo& info, const double* res) {
	std::printf("%s status %d hip %d outer %d x %a %a %a\n", name, static_cast<int>(status), SMM::lastHipStatus(), info.outerIterations, res[0], res[1], res[2]);
}

static void small() {
	SMM::TripletMatrix<double> t(3, 3);  // symmetric positive definite; 0.1 is not a float
	t.addEntry(0, 0, 4.1);
	t.addEntry(0, 1, -1.0);
	t.addEntry(1, 0, -1.0);
	t.addEntry(1, 1, 5.1);
	t.addEntry(1, 2, -2.0);
	t.addEntry(2, 1, -2.0);
	t.addEntry(2, 2, 6.1);
	SMM::CSRMatrix<double> m(t);
	double rhs[3] = {4.1 - 1.0, -1.0 + 5.1 - 2.0, -2.0 + 6.1};  // about the row sums: x is about 1
	const double L2NormCondition = 1e-12;
	SMM::RefinementInfo info;
	{
		SMM::CSRMatrix<float> m32 = SMM::convert<float>(m);
		auto preconditioner = m32.getPreconditioner<SMM::SolverPreconditioner::JACOBI>();
		double res[3] = {0, 0, 0};
		SMM::SolverStatus status = SMM::IterativeRefinement(m, m32, rhs, res, L2NormCondition, preconditioner, SMM::RefinementSolver::BICGSTAB, 20, -1, 1e-4f, 30, &info);
		line("kept", status, info, res);
		SMM::CSRMatrix<double> back;
		SMM::CSRMatrix<float> again;
		bool same = SMM::convert(m32, back) == 0 && SMM::convert(back, again) == 0 && again.getNonZeroCount() == m32.getNonZeroCount();
		for (int k = 0; same && k < m32.getNonZeroCount(); ++k) same = again.rawValues()[k] == m32.rawValues()[k] && m32.rawValues()[k] == static_cast<float>(m.rawValues()[k]);
		std::printf("roundtrip %d\n", same ? 1 : 0);
	}
	double res[3] = {0, 0, 0};
	SMM::SolverStatus status = SMM::IterativeRefinement(m, rhs, res, L2NormCondition, SMM::RefinementSolver::CG, 20, -1, 1e-4f, 30, &info);
	line("call", status, info, res);
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
	SMM::CSRMatrix<float> m32 = SMM::convert<float>(m);
	SMM::SolverStatus status = SMM::IterativeRefinement(m, m32, rhs.data(), res.data(), eps);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}

int main(int argc, char** argv) {
	if (argc >= 3) return fromFile(argv[1], std::atof(argv[2]));
	small();
	return 0;
}
