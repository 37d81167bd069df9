// smm_jacobi.h -- the small symmetric eigenproblem of the eigensolvers' Ritz steps (smm_solvers_eigsh.hip, smm_solvers_lobpcg.hip), on the host.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace smm {

// The eigenpairs of the symmetric m x m matrix `a` (row-major) by cyclic Jacobi: theta ascending, column i of y (y[r * m + i]) the unit
// eigenvector of theta[i], both rounded to fp64 at the end.  The rotations are accumulated in the host's long double: a restart multiplies
// the kept basis by Y, nothing re-orthogonalises the kept columns among themselves afterwards, and Y's own departure from orthogonality
// -- some tens of fp64 roundings when some thousand rotations are accumulated in fp64 -- would add up over the restarts.  Rounded from
// the wider format it is one rounding per element.  false: a value that is not finite.
inline bool jacobiEigen(int m, const std::vector<double>& t, std::vector<double>& theta, std::vector<double>& y) {
	typedef long double R;
	std::vector<R> a(t.begin(), t.end()), v(static_cast<size_t>(m) * m, R(0));
	for (int i = 0; i < m; ++i) v[i * m + i] = R(1);
	for (double e : t) {
		if (!std::isfinite(e)) return false;
	}
	for (int sweep = 0; sweep < 100; ++sweep) {
		R off = 0;
		for (int p = 0; p < m; ++p) {
			for (int q = p + 1; q < m; ++q) off += a[p * m + q] * a[p * m + q];
		}
		if (off == R(0)) break;
		for (int p = 0; p < m; ++p) {
			for (int q = p + 1; q < m; ++q) {
				const R apq = a[p * m + q];
				if (apq == R(0)) continue;
				const R app = a[p * m + p], aqq = a[q * m + q];
				const R g = R(100) * std::fabs(apq);
				if (sweep > 3 && std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {  // negligible beside both diagonals
					a[p * m + q] = a[q * m + p] = R(0);
					continue;
				}
				const R tau = (aqq - app) / (R(2) * apq);
				const R tn = (tau >= 0 ? R(1) : R(-1)) / (std::fabs(tau) + std::sqrt(R(1) + tau * tau));
				const R c = R(1) / std::sqrt(R(1) + tn * tn), s = tn * c;
				for (int r = 0; r < m; ++r) {  // columns p and q
					const R rp = a[r * m + p], rq = a[r * m + q];
					a[r * m + p] = c * rp - s * rq;
					a[r * m + q] = s * rp + c * rq;
				}
				for (int r = 0; r < m; ++r) {  // rows p and q
					const R pr = a[p * m + r], qr = a[q * m + r];
					a[p * m + r] = c * pr - s * qr;
					a[q * m + r] = s * pr + c * qr;
				}
				a[p * m + q] = a[q * m + p] = R(0);
				for (int r = 0; r < m; ++r) {
					const R rp = v[r * m + p], rq = v[r * m + q];
					v[r * m + p] = c * rp - s * rq;
					v[r * m + q] = s * rp + c * rq;
				}
			}
		}
	}
	std::vector<int> order(m);
	std::iota(order.begin(), order.end(), 0);
	std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return a[i * m + i] < a[j * m + j]; });
	theta.resize(m);
	y.assign(static_cast<size_t>(m) * m, 0.0);
	for (int i = 0; i < m; ++i) {
		theta[i] = static_cast<double>(a[order[i] * m + order[i]]);
		if (!std::isfinite(theta[i])) return false;
		for (int r = 0; r < m; ++r) y[r * m + i] = static_cast<double>(v[r * m + order[i]]);
	}
	return true;
}

}  // namespace smm
