// multicolor_case.cpp -- the multicolour preconditioners, the colouring and the symmetric permutation through the drop-in header
// (tests/test_multicolor_cpu.py compiles it; tests/test_gpu_multicolor.py runs it on a GPU).  All are additions of this library; the case
// is written against the reference's types (TripletMatrix, CSRMatrix) and the call shape of its preconditioned solvers:
//     SMM::MulticolorPreconditioner<T, typename SMM::CSRMatrix<T>::SGSPreconditioner> M(m);
//     SMM::SolverStatus status = SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M);
//     SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M);
//
//   multicolor_case   a 6 x 6 symmetric, diagonally dominant system (a path graph: two colours) in float and in double:
//                     "<float|double>-<bicgstab-sgs|bicgstab-ilu0|cg-ic0|cg-sgs> status <S> hip <H> colors <C> x ..." per solve, then
//                     "<float|double>-permute hip <H> colors <C> same <0|1>": SMM::color, SMM::permute by the colour order, SMM::permute of
//                     the result by the inverse permutation, and whether that gives the matrix back bit for bit (pattern and values).
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

constexpr int N = 6;

template <typename T>
static void fill(SMM::TripletMatrix<T>& t) {
	for (int i = 0; i < N; ++i) {
		if (i > 0) t.addEntry(i, i - 1, T(-1) - T(i) / T(8));
		t.addEntry(i, i, T(4) + T(i) / T(4));
		if (i + 1 < N) t.addEntry(i, i + 1, T(-1) - T(i + 1) / T(8));
	}
}

template <typename T, typename M>
static void report(const char* name, const char* what, SMM::SolverStatus status, const M& pre, const T* res) {
	int colors = -1;
	pre.info(&colors, nullptr, 0);
	std::printf("%s-%s status %d hip %d colors %d x", name, what, static_cast<int>(status), SMM::lastHipStatus(), colors);
	for (int i = 0; i < N; ++i) std::printf(" %a", static_cast<double>(res[i]));
	std::printf("\n");
}

template <typename T>
static void solves(const char* name) {
	using Matrix = SMM::CSRMatrix<T>;
	SMM::TripletMatrix<T> t(N, N);
	fill(t);
	Matrix m(t);
	T rhs[N], x0[N], res[N];
	const int maxIterations = 100;
	const T L2NormCondition = T(1e-5);
	auto reset = [&]() {
		for (int i = 0; i < N; ++i) {
			x0[i] = res[i] = T(0);
			rhs[i] = T(0);
		}
		for (auto it = m.begin(); it != m.end(); ++it) rhs[(*it).getRow()] += (*it).getValue();  // the row sums: x = 1
	};
	{
		reset();
		SMM::MulticolorPreconditioner<T, typename Matrix::SGSPreconditioner> M(m);
		report(name, "bicgstab-sgs", SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::MulticolorPreconditioner<T, typename Matrix::ILU0Preconditioner> M(m);
		report(name, "bicgstab-ilu0", M.validate() ? SMM::SolverStatus::DIVERGED : SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::MulticolorPreconditioner<T, typename Matrix::IC0Preconditioner> M(m);
		report(name, "cg-ic0", SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::MulticolorPreconditioner<T, typename Matrix::SGSPreconditioner> M(m);
		report(name, "cg-sgs", SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M), M, res);
	}
	// colour, permute by the colour order, permute back by the inverse: the matrix again, bit for bit
	int colors[N] = {0}, ncolors = 0;
	int same = 0;
	if (SMM::color(m, colors, &ncolors) == 0) {
		std::vector<int> perm, inv(N);
		for (int c = 0; c < ncolors; ++c) {
			for (int i = 0; i < N; ++i) {
				if (colors[i] == c) perm.push_back(i);
			}
		}
		if (static_cast<int>(perm.size()) == N) {
			for (int i = 0; i < N; ++i) inv[static_cast<size_t>(perm[static_cast<size_t>(i)])] = i;
			Matrix b, back;
			if (SMM::permute(m, perm.data(), b) == 0 && SMM::permute(b, inv.data(), back) == 0 && SMM::permuteRefresh(b, m) == 0 &&
			    back.getNonZeroCount() == m.getNonZeroCount()) {
				same = 1;
				auto p = m.begin();
				for (auto q = back.begin(); q != back.end(); ++q, ++p) {
					const T u = (*p).getValue(), v = (*q).getValue();
					if ((*p).getRow() != (*q).getRow() || (*p).getCol() != (*q).getCol() || std::memcmp(&u, &v, sizeof(T)) != 0) same = 0;
				}
			}
		}
	}
	std::printf("%s-permute hip %d colors %d same %d\n", name, SMM::lastHipStatus(), ncolors, same);
}

int main() {
	solves<float>("float");
	solves<double>("double");
	return 0;
}
