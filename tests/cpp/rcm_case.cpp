// rcm_case.cpp -- SMM::rcm / SMM::bandwidth / SMM::permute through the drop-in header (tests/test_cpp_rcm.py compiles it and runs it, on a
// GPU where there is one).  A 6 x 5 grid's 5-point Laplacian is numbered by a fixed scramble (row k is grid point 7 k mod 30), ordered by
// reverse Cuthill-McKee and permuted; the permuted matrix must have the bandwidth the ordering announced.
//   "rcm <R> components <C> levels <L> before <B> after <A> width <W> offsets <O> permute <P> hip <H>" and one "p <row>" per entry of perm
#include <cstdio>
#include <vector>

#include "sparse_matrix_math.h"

int main() {
	const int nx = 6, ny = 5, n = nx * ny;
	std::vector<int> name(n);  // the scrambled number of grid point g
	for (int k = 0; k < n; ++k) name[(7 * k) % n] = k;
	SMM::TripletMatrix<double> t(n, n);
	for (int y = 0; y < ny; ++y) {
		for (int x = 0; x < nx; ++x) {
			const int g = y * nx + x;
			t.addEntry(name[g], name[g], 4.0);
			if (x > 0) t.addEntry(name[g], name[g - 1], -1.0);
			if (x < nx - 1) t.addEntry(name[g], name[g + 1], -1.0);
			if (y > 0) t.addEntry(name[g], name[g - nx], -1.0);
			if (y < ny - 1) t.addEntry(name[g], name[g + nx], -1.0);
		}
	}
	SMM::CSRMatrix<double> a(t), b;
	std::vector<int> perm;
	int components = -1, levels = -1;
	long long before = -1, after = -1, width = -1, offsets = -1;
	const int rc = SMM::rcm(a, perm, true, &components, &levels, &before, &after);
	const int pc = rc == 0 ? SMM::permute(a, perm.data(), b) : rc;
	if (pc == 0) SMM::bandwidth(b, &width, &offsets);
	std::printf("rcm %d components %d levels %d before %lld after %lld width %lld offsets %lld permute %d hip %d\n", rc, components, levels, before, after, width, offsets, pc,
	            SMM::lastHipStatus());
	for (int p : perm) std::printf("p %d\n", p);
	return 0;
}
