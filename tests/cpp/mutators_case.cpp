// mutators_case.cpp -- CSRMatrix's value mutators written against the reference's C++ API only: operator*=, inplaceAdd /
// inplaceSubtract, updateEntry / addEntry (stored, missing, repeated), zeroValues, hasSameNonZeroPattern, and the writable
// iterators (Iterator, RowIterator with setValue; ConstIterator / ConstRowIterator to read).  Every step prints the matrix's values
// bit for bit (%a), so the output of a build against the drop-in header can be compared with one against the reference header
// (tests/test_cpp_mutators_cpu.py).  Without a GPU the drop-in header runs all of it on the host; with one (SMM_CASE_MIRROR=1) a
// hot-path call first makes the device mirror, so the same edits go through the device and the printed values must not change.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

static bool g_mirror = false;

template <typename T>
static void dump(const char* step, const SMM::CSRMatrix<T>& m) {
	std::printf("%s:", step);
	for (auto it = m.begin(); it != m.end(); ++it) std::printf(" (%d,%d)=%a", it->getRow(), it->getCol(), static_cast<double>(it->getValue()));
	std::printf("\n");
}

template <typename T>
static void touchDevice(const SMM::CSRMatrix<T>& m) {
#ifdef SMM_HIP_H
	if (g_mirror) {
		std::vector<T> x(static_cast<size_t>(m.getDenseColCount()), T(1)), y(static_cast<size_t>(m.getDenseRowCount()));
		m.rMult(x.data(), y.data());  // makes the mirror: the edits that follow run on the device
	}
#else
	(void)m;
#endif
}

// with a mirror: the edited matrix multiplies like a fresh CSRMatrix made from its (host) arrays, bit for bit -- on stderr, so that
// stdout stays the same with and without the mirror
template <typename T>
static void checkFresh(const char* step, const SMM::CSRMatrix<T>& m) {
#ifdef SMM_HIP_H
	if (!g_mirror) return;
	SMM::CSRMatrix<T> fresh;
	fresh.init(m.getDenseRowCount(), m.getDenseColCount(), m.rawStart(), m.rawPositions(), m.rawValues());
	std::vector<T> x(static_cast<size_t>(m.getDenseColCount())), y1(static_cast<size_t>(m.getDenseRowCount())), y2(y1.size());
	for (size_t i = 0; i < x.size(); ++i) x[i] = T(1) + T(0.25) * static_cast<T>(i);
	m.rMult(x.data(), y1.data());
	fresh.rMult(x.data(), y2.data());
	const bool same = std::memcmp(y1.data(), y2.data(), y1.size() * sizeof(T)) == 0 && SMM::lastHipStatus() == SMM_HIP_OK;
	std::fprintf(stderr, "fresh %s %d\n", step, same ? 1 : 0);
#else
	(void)step;
	(void)m;
#endif
}

// a 5x5 matrix with an empty row (row 3), a missing diagonal entry and entries above and below it
template <typename T>
static void fill(SMM::CSRMatrix<T>& m, T scale) {
	SMM::TripletMatrix<T> t(5, 5);
	t.addEntry(0, 0, T(4) * scale);
	t.addEntry(0, 1, T(-1.25) * scale);
	t.addEntry(0, 4, T(0.1) * scale);
	t.addEntry(1, 0, T(-1) * scale);
	t.addEntry(1, 1, T(3.3) * scale);
	t.addEntry(1, 2, T(-0.7) * scale);
	t.addEntry(2, 1, T(2.5) * scale);
	t.addEntry(2, 3, T(1) / T(3) * scale);
	t.addEntry(4, 0, T(7) * scale);
	t.addEntry(4, 4, T(-9.75) * scale);
	m.init(t);
}

template <typename T>
static void run(const char* name) {
	std::printf("== %s\n", name);
	SMM::CSRMatrix<T> a, b, c;
	fill(a, T(1));
	fill(b, T(0.3));
	SMM::TripletMatrix<T> t(5, 5);  // the same shape, another pattern
	t.addEntry(0, 0, T(1));
	t.addEntry(2, 2, T(1));
	c.init(t);
	touchDevice(a);
	touchDevice(b);
	dump("initial", a);
	std::printf("same a b %d, a c %d, a a %d\n", a.hasSameNonZeroPattern(b) ? 1 : 0, a.hasSameNonZeroPattern(c) ? 1 : 0, a.hasSameNonZeroPattern(a) ? 1 : 0);

	a *= T(1.7);
	dump("scaled", a);
	checkFresh("scaled", a);
	a.inplaceAdd(b);
	dump("added", a);
	a.inplaceSubtract(b);
	dump("subtracted", a);
	a.inplaceAdd(a);
	dump("added to itself", a);

	std::printf("update (1,2) %d\n", a.updateEntry(1, 2, T(11.5)) ? 1 : 0);
	std::printf("update (0,2) %d\n", a.updateEntry(0, 2, T(99)) ? 1 : 0);  // not stored
	std::printf("update (3,3) %d\n", a.updateEntry(3, 3, T(99)) ? 1 : 0);  // empty row
	const bool u1 = a.updateEntry(4, 4, T(-2));
	const bool u2 = a.updateEntry(4, 4, T(6.25));  // the last one stays
	std::printf("update (4,4) %d, again %d\n", u1 ? 1 : 0, u2 ? 1 : 0);
	dump("updated", a);
	const bool d1 = a.addEntry(0, 0, T(0.1));
	const bool d2 = a.addEntry(0, 0, T(0.2));
	const bool d3 = a.addEntry(0, 0, T(1e-3));  // summed in order
	std::printf("add (0,0) %d, again %d, again %d\n", d1 ? 1 : 0, d2 ? 1 : 0, d3 ? 1 : 0);
	std::printf("add (2,2) %d\n", a.addEntry(2, 2, T(5)) ? 1 : 0);  // not stored
	dump("entries added", a);
	std::printf("value (0,0) %a, (4,4) %a, (0,2) %a\n", static_cast<double>(a.getValue(0, 0)), static_cast<double>(a.getValue(4, 4)), static_cast<double>(a.getValue(0, 2)));

	// writable iterators: every element of row 1 through a RowIterator, every element through the general Iterator
	{
		typename SMM::CSRMatrix<T>::RowIterator it = a.rowBegin(1);
		typename SMM::CSRMatrix<T>::RowIterator end = a.rowEnd(1);
		int k = 0;
		for (; it != end; ++it, ++k) it->setValue(it->getValue() * T(2) + T(k));
	}
	dump("row 1 set", a);
	{
		typename SMM::CSRMatrix<T>::RowIterator it = a.rowBegin(3);
		std::printf("row 3 empty %d\n", it == a.rowEnd(3) ? 1 : 0);
	}
	for (typename SMM::CSRMatrix<T>::Iterator it = a.begin(); it != a.end(); ++it) {
		if (it->getRow() == it->getCol()) it->setValue(it->getValue() - T(0.5));
	}
	dump("diagonal set", a);
	checkFresh("diagonal set", a);
	for (int r = 0; r < 5; ++r) {
		std::printf("row %d:", r);
		for (typename SMM::CSRMatrix<T>::ConstRowIterator it = a.crowBegin(r); it != a.crowEnd(r); ++it) std::printf(" %d=%a", it->getCol(), static_cast<double>(it->getValue()));
		std::printf("\n");
	}
	touchDevice(a);  // (with a mirror: the queued entries go to the device here)
	a *= T(-0.5);
	dump("scaled after entries", a);
	a.addEntry(2, 3, T(1));
	a.inplaceAdd(b);
	dump("entry then add", a);
	checkFresh("entry then add", a);

	a.zeroValues();
	dump("zeroed", a);
	a.inplaceSubtract(b);
	dump("zero minus b", a);
	checkFresh("zero minus b", a);
	std::printf("b untouched: ");
	dump("b", b);

	// an empty matrix
	SMM::CSRMatrix<T> e;
	SMM::TripletMatrix<T> te(3, 3);
	e.init(te);
	e *= T(2);
	e.zeroValues();
	std::printf("empty update %d, same %d\n", e.updateEntry(0, 0, T(1)) ? 1 : 0, e.hasSameNonZeroPattern(e) ? 1 : 0);
	dump("empty", e);
}

int main() {
	const char* mirror = std::getenv("SMM_CASE_MIRROR");
	g_mirror = mirror && std::atoi(mirror) != 0;
	run<float>("float");
	run<double>("double");
	return 0;
}
