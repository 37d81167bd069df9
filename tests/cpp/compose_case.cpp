// compose_case.cpp -- composing and slicing through the drop-in header (tests/test_cpp_compose.py compiles it and runs it, on a GPU where
// there is one).  K = [[H, Bt], [B, 0]] is built with SMM::blockMatrix from the 12 x 12 grid Laplacian H and a 20 x 144 constraint block B,
// its (1,1) block is cut back out with SMM::submatrix and compared with H; the diagonal of K and a row / column scaling of the cut follow.
// Without a GPU every call answers SMM_HIP_ERR_NO_DEVICE (the header computes nothing on the CPU).
//   "block <B> sub <S> range <R> pattern <P> values <V> diag <D> missing <M> scale <C> scaled <E> refresh <F> hip <H>"
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_matrix_math.h"

int main() {
	const int n = 12, rows = n * n, m = 20;
	SMM::TripletMatrix<double> th(rows, rows), tb(m, rows);
	for (int y = 0; y < n; ++y) {
		for (int x = 0; x < n; ++x) {
			const int i = y * n + x;
			th.addEntry(i, i, 4.0);
			if (x > 0) th.addEntry(i, i - 1, -1.0);
			if (x + 1 < n) th.addEntry(i, i + 1, -1.0);
			if (y > 0) th.addEntry(i, i - n, -1.0);
			if (y + 1 < n) th.addEntry(i, i + n, -1.0);
		}
	}
	for (int i = 0; i < m; ++i) {
		for (int k = 0; k < 4; ++k) tb.addEntry(i, (i * 7 + k * 31) % rows, 0.25 * (k + 1) - 0.1 * i);
	}
	SMM::CSRMatrix<double> H(th), B(tb), Bt, K, H11, H11r;
	const int tr = SMM::transpose(B, Bt);
	const int block = SMM::blockMatrix<double>(2, 2, {&H, &Bt, &B, nullptr}, K);
	std::vector<int> idx(rows);
	for (int i = 0; i < rows; ++i) idx[i] = i;
	const int sub = SMM::submatrix(K, idx.data(), idx.size(), idx.data(), idx.size(), H11);
	const int range = SMM::submatrix(K, 0, rows, 0, rows, H11r);
	const int pattern = sub == 0 && H11.hasSameNonZeroPattern(H) && H11r.hasSameNonZeroPattern(H) ? 1 : 0;
	int values = 0;
	if (pattern) {
		const size_t bytes = sizeof(double) * static_cast<size_t>(H.getNonZeroCount());
		values = std::memcmp(H11.rawValues(), H.rawValues(), bytes) == 0 && std::memcmp(H11r.rawValues(), H.rawValues(), bytes) == 0 ? 1 : 0;
	}
	std::vector<double> d(rows + m, -1.0), r(rows, 2.0), c(rows, 0.5);
	int missing = -1;
	const int diag = SMM::diagonal(K, d.data(), &missing);
	int diagOk = diag == 0 ? 1 : 0;
	for (int i = 0; diagOk && i < rows + m; ++i) diagOk = d[i] == (i < rows ? 4.0 : 0.0) ? 1 : 0;
	const int scale = H11.scaleRowsCols(r.data(), c.data());  // (2 v) 0.5: the values again, through the device
	const int scaled = scale == 0 && std::memcmp(H11.rawValues(), H.rawValues(), sizeof(double) * static_cast<size_t>(H.getNonZeroCount())) == 0 ? 1 : 0;
	H *= 3.0;
	int refresh = SMM::blockRefresh<double>(K, 2, 2, {&H, &Bt, &B, nullptr});
	if (refresh == 0) refresh = SMM::submatrixRefresh(H11, K);
	const int refreshed = refresh == 0 && H11.getValue(5, 5) == 12.0 && H11.getValue(5, 6) == -3.0 && K.getValue(rows, (0 * 7) % rows) == 0.25 ? 1 : 0;
	std::printf("transpose %d block %d sub %d range %d pattern %d values %d diag %d missing %d scale %d scaled %d refresh %d refreshed %d hip %d\n", tr, block, sub, range,
	            pattern, values, diagOk, missing, scale, scaled, refresh, refreshed, SMM::lastHipStatus());
	return 0;
}
