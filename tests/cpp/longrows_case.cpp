// longrows_case.cpp -- the LONGROWS SpMV family through the drop-in header (tests/test_cpp_longrows.py compiles it and runs it, on a GPU
// where there is one).  A 6 x 300 matrix with integer values and rows of 3, 200, 0, 65, 64 and 130 entries is multiplied by an integer x
// with rows of more than 64 entries cut into segments of 64; every summation order is exact, so the result must equal the plain host loop
// below bit for bit (the header itself computes nothing on the CPU).
//   "cfg <C> bad <B> set <ST> split <S> seg <G> long <L> segs <N> equal <E> hip <H>" and one "y <%a>" per row
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

int main() {
	const int rows = 6, cols = 300;
	const int lens[rows] = {3, 200, 0, 65, 64, 130};
	SMM::TripletMatrix<double> t(rows, cols);
	std::vector<double> x(cols), want(rows, 0.0), y(rows, -1.0);
	for (int j = 0; j < cols; ++j) x[j] = j % 17 - 8;
	for (int i = 0; i < rows; ++i) {
		for (int k = 0; k < lens[i]; ++k) {
			const int j = (k * 300) / (lens[i] + 1) + i % 2;  // strictly ascending, inside the matrix
			const double v = (i * 7 + k * 3) % 9 - 4;
			t.addEntry(i, j, v);
			want[i] += v * x[j];
		}
	}
	SMM::CSRMatrix<double> m(t);
	const int bad = m.configureLongRows(64, 100);  // segment_len is a multiple of 64: refused, nothing changes
	const int cfg = m.configureLongRows(64, 64);
	const int set = m.setSpmvKernel(SMM_SPMV_LONGROWS);
	int split = -1, seg = -1, nlong = -1;
	long long segs = -1;
	m.longRowsInfo(&split, &seg, &nlong, &segs);
	m.rMult(x.data(), y.data());
	const int equal = std::memcmp(y.data(), want.data(), sizeof(double) * rows) == 0 ? 1 : 0;
	std::printf("cfg %d bad %d set %d split %d seg %d long %d segs %lld equal %d hip %d\n", cfg, bad, set, split, seg, nlong, segs, equal, SMM::lastHipStatus());
	for (double v : want) std::printf("y %a\n", v);
	return 0;
}
