// amg_candidates_case.cpp -- the multigrid preconditioner with near-null-space candidates through the drop-in header
// (tests/test_amg_candidates_cpu.py compiles it; tests/test_gpu_amg_candidates.py runs it on a GPU):
//     SMM::AMGPreconditioner<T> M = m.getAMGPreconditioner(B, k, dofsPerNode, theta, maxLevels, coarseRows);
//     SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M);
//
//   amg_candidates_case <matrix file> <candidates file> <dofs per node> <eps>
// the matrix of the file in double, rhs = row sums, x0 = 0, maxIterations = -1, coarse_rows 64: "status <S> hip <H>",
// "levels <L> k <k> dropped <d on level 0>" and one "x <%a>" per row.  Without arguments: a 4 x 4 system with two candidates, one line.
// matrix file: "rows entries" and then one "row col value" per stored entry, in CSR order; candidates file: "rows k" and then the
// rows x k values row by row.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sparse_matrix_math.h"

static int small() {
	SMM::TripletMatrix<double> t(4, 4);
	const double v[4][4] = {{4, -1, 0, 0}, {-1, 4, -1, 0}, {0, -1, 4, -1}, {0, 0, -1, 4}};
	for (int i = 0; i < 4; ++i) {
		for (int j = 0; j < 4; ++j) {
			if (v[i][j] != 0) t.addEntry(i, j, v[i][j]);
		}
	}
	SMM::CSRMatrix<double> m(t);
	const double B[8] = {1, 0, 1, 0, 0, 1, 0, 1};  // column-major: the two translations of two nodes
	double rhs[4] = {3, 2, 2, 3}, x0[4] = {0, 0, 0, 0}, res[4] = {0, 0, 0, 0};
	SMM::AMGPreconditioner<double> M = m.getAMGPreconditioner(B, 2, 2, 0.08, 10, 1);
	const SMM::SolverStatus status = M.validate() ? SMM::SolverStatus::DIVERGED : SMM::ConjugateGradient(m, rhs, x0, res, 100, 1e-10, M);
	std::printf("small status %d hip %d x %a %a %a %a\n", static_cast<int>(status), SMM::lastHipStatus(), res[0], res[1], res[2], res[3]);
	return 0;
}

int main(int argc, char** argv) {
	if (argc < 5) return small();
	std::FILE* f = std::fopen(argv[1], "r");
	if (!f) return 2;
	int rows = 0, entries = 0;
	if (std::fscanf(f, "%d %d", &rows, &entries) != 2) return 2;
	SMM::TripletMatrix<double> t(rows, rows);
	std::vector<double> rhs(static_cast<size_t>(rows), 0.0), x0(static_cast<size_t>(rows), 0.0), res(static_cast<size_t>(rows), 0.0);
	for (int e = 0; e < entries; ++e) {
		int r = 0, c = 0;
		double v = 0;
		if (std::fscanf(f, "%d %d %lf", &r, &c, &v) != 3) return 2;
		t.addEntry(r, c, v);
		rhs[static_cast<size_t>(r)] += v;
	}
	std::fclose(f);
	f = std::fopen(argv[2], "r");
	if (!f) return 2;
	int brows = 0, k = 0;
	if (std::fscanf(f, "%d %d", &brows, &k) != 2 || brows != rows || k < 1) return 2;
	std::vector<double> B(static_cast<size_t>(rows) * static_cast<size_t>(k));
	for (int i = 0; i < rows; ++i) {
		for (int c = 0; c < k; ++c) {
			if (std::fscanf(f, "%lf", &B[static_cast<size_t>(c) * static_cast<size_t>(rows) + static_cast<size_t>(i)]) != 1) return 2;
		}
	}
	std::fclose(f);
	SMM::CSRMatrix<double> m(t);
	SMM::AMGPreconditioner<double> M = m.getAMGPreconditioner(B.data(), k, std::atoi(argv[3]), 0.08, 10, 64);
	const SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs.data(), x0.data(), res.data(), -1, std::atof(argv[4]), M);
	std::printf("status %d hip %d\n", static_cast<int>(status), SMM::lastHipStatus());
	int levels = 0, kk = 0, dropped = -1;
	M.info(&levels, nullptr, nullptr, 0, nullptr);
	M.candidates(0, nullptr, 0, &kk, &dropped);
	std::printf("levels %d k %d dropped %d\n", levels, kk, dropped);
	for (double v : res) std::printf("x %a\n", v);
	return 0;
}
