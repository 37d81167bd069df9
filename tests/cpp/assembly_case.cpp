// assembly_case.cpp -- SMM::AssemblyPlan + CSRMatrix::init(plan, values) / assemble(plan, values) of the drop-in header against a twin
// built the reference's way, TripletMatrix::addEntry in the same list order + CSRMatrix(triplet) (needs a GPU).  The list: a 5-point
// stencil whose entries arrive as 1 to 3 contributions of very different magnitudes, in a scrambled order.  Checked: the pattern and
// every value (getValue, iterators), a single-entry edit after init, the refill with new values through rMult of both, the adding
// refill, the refusal of a foreign matrix and of an out-of-range pair.  Prints "OK" last (tests/test_gpu_assembly.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

static int failures = 0;
#define CHECK(cond)                                                      \
	do {                                                                 \
		if (!(cond)) {                                                   \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
			++failures;                                                  \
		}                                                                \
	} while (0)

template <typename T>
static bool sameBits(const T* a, const T* b, size_t n) { return std::memcmp(a, b, n * sizeof(T)) == 0; }

template <typename T>
struct List {
	std::vector<int> r, c;
	std::vector<T> v;
	void add(int row, int col, T value) {
		r.push_back(row);
		c.push_back(col);
		v.push_back(value);
	}
};

template <typename T>
static List<T> stencilList(int nx, unsigned seed) {
	List<T> l;
	unsigned s = seed;
	auto next = [&s] { return s = s * 1664525u + 1013904223u; };
	auto split = [&](int row, int col, T value) {
		const int parts = 1 + static_cast<int>((next() >> 16) % 3u);
		for (int p = 0; p < parts; ++p) l.add(row, col, value * static_cast<T>(1.0 / (1 << (7 * p))) * static_cast<T>(1 + (next() >> 20) % 7u) / T(3));
	};
	for (int i = 0; i < nx; ++i) {
		for (int j = 0; j < nx; ++j) {
			const int row = i * nx + j;
			split(row, row, T(4));
			if (i > 0) split(row, row - nx, T(-1));
			if (j > 0) split(row, row - 1, T(-1));
			if (j + 1 < nx) split(row, row + 1, T(-1));
			if (i + 1 < nx) split(row, row + nx, T(-1));
		}
	}
	for (size_t k = l.r.size(); k > 1; --k) {  // scramble the list
		const size_t o = next() % k;
		std::swap(l.r[k - 1], l.r[o]);
		std::swap(l.c[k - 1], l.c[o]);
		std::swap(l.v[k - 1], l.v[o]);
	}
	return l;
}

template <typename T>
static void twinOf(const List<T>& l, int n, SMM::CSRMatrix<T>& out) {
	SMM::TripletMatrix<T> t(n, n);
	for (size_t k = 0; k < l.r.size(); ++k) t.addEntry(l.r[k], l.c[k], l.v[k]);
	out.init(t);
}

template <typename T>
static void run() {
	const int nx = 30, n = nx * nx;
	List<T> l = stencilList<T>(nx, 12345u);
	SMM::AssemblyPlan plan(n, n, static_cast<long long>(l.r.size()), l.r.data(), l.c.data());
	CHECK(plan.valid() && plan.status() == 0 && SMM::lastHipStatus() == 0);
	if (!plan.valid()) {
		std::printf("no plan: status %d, %s\n", plan.status(), smm_hip_last_error());
		return;
	}
	SMM::CSRMatrix<T> twin;
	twinOf(l, n, twin);
	CHECK(plan.getNonZeroCount() == twin.getNonZeroCount() && plan.getDenseRowCount() == n && plan.getDenseColCount() == n);
	CHECK(plan.getTripletCount() == static_cast<long long>(l.r.size()) && plan.getLongestRun() == 3);

	SMM::CSRMatrix<T> a;
	CHECK(a.init(plan, l.v.data()) == 0);
	if (SMM::lastHipStatus() != 0) return;
	const int nnz = twin.getNonZeroCount();
	CHECK(a.getNonZeroCount() == nnz && a.getDenseRowCount() == n && a.getDenseColCount() == n);
	CHECK(std::memcmp(a.rawStart(), twin.rawStart(), (n + 1) * sizeof(int)) == 0);
	CHECK(std::memcmp(a.rawPositions(), twin.rawPositions(), nnz * sizeof(int)) == 0);
	CHECK(sameBits(a.rawValues(), twin.rawValues(), nnz));
	CHECK(a.hasSameNonZeroPattern(twin));
	{
		auto ia = a.cbegin();
		auto it = twin.cbegin();
		int seen = 0;
		for (; ia != a.cend() && it != twin.cend(); ++ia, ++it, ++seen) {
			const T va = ia->getValue(), vt = it->getValue();
			if (ia->getRow() != it->getRow() || ia->getCol() != it->getCol() || !sameBits(&va, &vt, 1)) break;
			const T g = a.getValue(ia->getRow(), ia->getCol());
			if (!sameBits(&g, &vt, 1)) break;
		}
		CHECK(seen == nnz);
	}
	std::vector<T> x(static_cast<size_t>(n)), ya(x.size()), yt(x.size());
	for (int i = 0; i < n; ++i) x[i] = T(1) + T(0.01) * static_cast<T>(i % 37);
	a.rMult(x.data(), ya.data());
	twin.rMult(x.data(), yt.data());
	CHECK(SMM::lastHipStatus() == 0 && sameBits(ya.data(), yt.data(), x.size()));
	// the host-side mutator queue works on the assembled matrix
	CHECK(a.updateEntry(5, 5, T(5.5)) && twin.updateEntry(5, 5, T(5.5)));
	a.rMult(x.data(), ya.data());
	twin.rMult(x.data(), yt.data());
	CHECK(sameBits(ya.data(), yt.data(), x.size()));

	// new values for the same pairs
	List<T> l2 = l;
	for (size_t k = 0; k < l2.v.size(); ++k) l2.v[k] = l.v[k] * (T(1) + T(0.125) * static_cast<T>(k % 5));
	SMM::CSRMatrix<T> twin2;
	twinOf(l2, n, twin2);
	CHECK(a.assemble(plan, l2.v.data()) == 0 && SMM::lastHipStatus() == 0);
	a.rMult(x.data(), ya.data());
	twin2.rMult(x.data(), yt.data());
	CHECK(sameBits(ya.data(), yt.data(), x.size()));
	CHECK(sameBits(a.rawValues(), twin2.rawValues(), nnz));
	// ... and added to the present ones: twin2 + twin2, one rounding (exact)
	CHECK(a.assemble(plan, l2.v.data(), true) == 0);
	twin2.inplaceAdd(twin2);
	CHECK(sameBits(a.rawValues(), twin2.rawValues(), nnz));
	const T g = a.getValue(7, 8), w = twin2.getValue(7, 8);
	CHECK(sameBits(&g, &w, 1));

	// refusals: a matrix the plan did not make; a pair outside the matrix
	CHECK(twin.assemble(plan, l2.v.data()) == SMM_HIP_ERR_INVALID && SMM::lastHipStatus() == SMM_HIP_ERR_INVALID);
	CHECK(sameBits(a.rawValues(), twin2.rawValues(), nnz));
	std::vector<int> br(l.r), bc(l.c);
	br[17] = n;
	SMM::AssemblyPlan bad(n, n, static_cast<long long>(br.size()), br.data(), bc.data());
	CHECK(!bad.valid() && bad.status() == SMM_HIP_ERR_INVALID && std::strstr(smm_hip_last_error(), "entry 17 ") != nullptr);
	SMM::CSRMatrix<T> none;
	CHECK(none.init(bad, l.v.data()) == SMM_HIP_ERR_INVALID && none.getNonZeroCount() == 0);
	SMM::AssemblyPlan moved(std::move(plan));
	CHECK(moved.valid() && !plan.valid() && a.assemble(moved, l.v.data()) == 0);
	twinOf(l, n, twin2);
	CHECK(sameBits(a.rawValues(), twin2.rawValues(), nnz));
}

int main() {
	run<float>();
	run<double>();
	if (failures) {
		std::printf("%d checks failed\n", failures);
		return 1;
	}
	std::printf("OK\n");
	return 0;
}
