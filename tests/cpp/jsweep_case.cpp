// jsweep_case.cpp -- the iterated-sweep preconditioners through the drop-in header (tests/test_gpu_jsweep.py compiles it with its own
// command line and runs it on a GPU).  An addition of this library; the case is written against the reference's types (TripletMatrix,
// CSRMatrix) and the call shape of its preconditioned solvers:
//     SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_ILU0);          // 3 / 3 steps
//     SMM::SolverStatus status = SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M);
//     SMM::SolverStatus status = SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M);
//
//   jsweep_case   a 6 x 6 symmetric, diagonally dominant tridiagonal system in float and in double:
//                 "<float|double>-<bicgstab-ilu0|bicgstab-sgs|cg-ic0|cg-sgs> status <S> hip <H> sweeps <L> <U> x ..." per solve, then
//                 "<float|double>-exact hip <H> levels <L> <U> same <0|1> one_step_same <0|1>": with levels - 1 steps the apply of the ILU0
//                 form equals ILU0Preconditioner's bit for bit (same 1), with one step it does not (one_step_same 0).
#include <cstdio>
#include <cstring>

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
	int lower = -1, upper = -1;
	pre.info(nullptr, &lower, &upper, nullptr, nullptr);
	std::printf("%s-%s status %d hip %d sweeps %d %d x", name, what, static_cast<int>(status), SMM::lastHipStatus(), lower, upper);
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
		SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_ILU0);
		report(name, "bicgstab-ilu0", M.validate() ? SMM::SolverStatus::DIVERGED : SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_SGS);
		report(name, "bicgstab-sgs", SMM::BiCGStab(m, rhs, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_IC0);
		report(name, "cg-ic0", SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M), M, res);
	}
	{
		reset();
		SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_SGS, 3, 3);
		report(name, "cg-sgs", SMM::ConjugateGradient(m, rhs, x0, res, maxIterations, L2NormCondition, M), M, res);
	}
	// levels - 1 steps: the exact kind's apply, bit for bit; one step: not
	reset();
	int lo = 0, up = 0, same = 0, oneStepSame = 0;
	T exact[N], got[N];
	typename Matrix::ILU0Preconditioner X(m);
	SMM::JacobiSweepPreconditioner<T> M(m, SMM_PRECOND_ILU0, 1, 1);
	if (X.apply(rhs, exact) == 0 && M.info(nullptr, nullptr, nullptr, &lo, &up) == 0 && M.apply(rhs, got) == 0) {
		oneStepSame = std::memcmp(exact, got, sizeof(exact)) == 0;
		if (M.setSweeps(lo - 1, up - 1) == 0 && M.refresh() == 0 && M.apply(rhs, got) == 0) same = std::memcmp(exact, got, sizeof(exact)) == 0;
	}
	std::printf("%s-exact hip %d levels %d %d same %d one_step_same %d\n", name, SMM::lastHipStatus(), lo, up, same, oneStepSame);
}

int main() {
	solves<float>("float");
	solves<double>("double");
	return 0;
}
