// blocks_case.cpp -- the BLOCKS SpMV family through the drop-in header (tests/test_cpp_blocks.py compiles it and runs it, on a GPU where
// there is one).  A 12 x 12 matrix of dense 2 x 2 blocks on a 6 x 6 block pattern (diagonal, one block to the right, one wrapped far
// block) is multiplied under STREAM at one lane per row and under BLOCKS; the two results must agree bit for bit.
//   "found <F> blocks <B> size <S> cap <C> set <ST> equal <E> hip <H>" and one "y <%a>" per row
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

int main() {
	const int nb = 6, b = 2, n = nb * b;
	SMM::TripletMatrix<double> t(n, n);
	int blocks = 0;
	for (int R = 0; R < nb; ++R) {
		const int cols[3] = {R, (R + 1) % nb, (R + 3) % nb};
		for (int q = 0; q < 3; ++q) {
			++blocks;
			for (int i = 0; i < b; ++i) {
				for (int j = 0; j < b; ++j) t.addEntry(R * b + i, cols[q] * b + j, 0.1 + 0.37 * (R * b + i) - 0.21 * (cols[q] * b + j) + (i == j ? 3.0 : 0.0));
			}
		}
	}
	SMM::CSRMatrix<double> m(t);
	std::vector<double> x(n), y1(n, -1.0), y2(n, -2.0);
	for (int i = 0; i < n; ++i) x[i] = 1.0 / (i + 3);
	m.setSpmvKernel(SMM_SPMV_STREAM, 1);
	m.rMult(x.data(), y1.data());
	const int found = m.findBlocks(0);
	int size = -1, cap = -1;
	long long kept = -1;
	m.blocksInfo(&size, &kept, &cap);
	const int set = m.setSpmvKernel(SMM_SPMV_BLOCKS);
	m.rMult(x.data(), y2.data());
	const int equal = std::memcmp(y1.data(), y2.data(), sizeof(double) * n) == 0 ? 1 : 0;
	std::printf("found %d blocks %lld of %d size %d cap %d set %d equal %d hip %d\n", found, kept, blocks, size, cap, set, equal, SMM::lastHipStatus());
	for (double v : y2) std::printf("y %a\n", v);
	return 0;
}
