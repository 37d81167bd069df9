// smm_jacobi.h -- the small dense problems of the Ritz steps, on the host: the symmetric eigenproblem (smm_solvers_eigsh.hip,
// smm_solvers_lobpcg.hip) and the SVD (smm_solvers_svds.hip).  Host code only: tests/cpp/jacobi_case.cpp includes nothing else.
#pragma once
#include <algorithm>
#include <cfloat>
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

// The SVD of the small matrix whose TRANSPOSE is `bt` (p x q, row-major, p >= q -- B is q x p): B = X diag(sigma) Y^T with sigma (q of
// them) descending, X (q x q, x[r * q + i]) orthogonal and Y (p x q, y[r * q + i]) with orthonormal columns, by one-sided Jacobi
// (Hestenes) on the columns of B^T: B^T X = Y diag(sigma).  X is the accumulated rotations: it is what rho and the arrow are read from,
// and a restart multiplies the kept basis by it, so -- as in jacobiEigen -- the rotations run in the host's long double
// and are rounded to fp64 once.  A column of Y whose sigma is at rounding level beside sigma_0 has no direction of its own: it is
// completed to a unit vector orthogonal to the others (any such vector is a singular vector of that sigma to rounding), so that a
// rank-deficient B never divides by zero.  false: a value that is not finite.
inline bool jacobiSvd(int p, int q, const std::vector<double>& bt, std::vector<double>& sigma, std::vector<double>& x, std::vector<double>& y) {
	typedef long double R;
	for (double e : bt) {
		if (!std::isfinite(e)) return false;
	}
	std::vector<R> g(bt.begin(), bt.end()), w(static_cast<size_t>(q) * q, R(0));
	for (int i = 0; i < q; ++i) w[i * q + i] = R(1);
	const R tiny = R(4) * LDBL_EPSILON;
	for (int sweep = 0; sweep < 100; ++sweep) {
		bool rotated = false;
		for (int a = 0; a < q; ++a) {
			for (int b = a + 1; b < q; ++b) {
				R aa = 0, bb = 0, ab = 0;
				for (int r = 0; r < p; ++r) {
					aa += g[r * q + a] * g[r * q + a];
					bb += g[r * q + b] * g[r * q + b];
					ab += g[r * q + a] * g[r * q + b];
				}
				if (ab == R(0) || std::fabs(ab) <= tiny * std::sqrt(aa * bb)) continue;
				rotated = true;
				const R zeta = (bb - aa) / (R(2) * ab);
				const R tn = (zeta >= 0 ? R(1) : R(-1)) / (std::fabs(zeta) + std::sqrt(R(1) + zeta * zeta));
				const R c = R(1) / std::sqrt(R(1) + tn * tn), s = tn * c;
				for (int r = 0; r < p; ++r) {
					const R ga = g[r * q + a], gb = g[r * q + b];
					g[r * q + a] = c * ga - s * gb;
					g[r * q + b] = s * ga + c * gb;
				}
				for (int r = 0; r < q; ++r) {
					const R wa = w[r * q + a], wb = w[r * q + b];
					w[r * q + a] = c * wa - s * wb;
					w[r * q + b] = s * wa + c * wb;
				}
			}
		}
		if (!rotated) break;
	}
	std::vector<R> nrm(q);
	for (int i = 0; i < q; ++i) {
		R s = 0;
		for (int r = 0; r < p; ++r) s += g[r * q + i] * g[r * q + i];
		nrm[i] = std::sqrt(s);
	}
	std::vector<int> order(q);
	std::iota(order.begin(), order.end(), 0);
	std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return nrm[i] > nrm[j]; });
	sigma.resize(q);
	x.assign(static_cast<size_t>(q) * q, 0.0);
	y.assign(static_cast<size_t>(p) * q, 0.0);
	std::vector<R> z(static_cast<size_t>(p) * q, R(0));  // Y in the wide format, column i at z[r * q + i]
	const R cut = q > 0 ? R(DBL_EPSILON) * nrm[order[0]] : R(0);
	for (int i = 0; i < q; ++i) {
		const int o = order[i];
		sigma[i] = static_cast<double>(nrm[o]);
		if (!std::isfinite(sigma[i])) return false;
		for (int r = 0; r < q; ++r) x[r * q + i] = static_cast<double>(w[r * q + o]);
		if (nrm[o] > cut) {
			for (int r = 0; r < p; ++r) z[r * q + i] = g[r * q + o] / nrm[o];
		}
	}
	for (int i = 0; i < q; ++i) {  // (descending: the columns at rounding level are the last ones)
		if (nrm[order[i]] > cut) continue;
		std::vector<R> best(p, R(0)), t(p);
		R bestNorm = R(-1);
		for (int e = 0; e < p; ++e) {  // the unit vector that keeps most of itself
			std::fill(t.begin(), t.end(), R(0));
			t[e] = R(1);
			for (int pass = 0; pass < 2; ++pass) {
				for (int c = 0; c < i; ++c) {
					R d = 0;
					for (int r = 0; r < p; ++r) d += z[r * q + c] * t[r];
					for (int r = 0; r < p; ++r) t[r] -= d * z[r * q + c];
				}
			}
			R s = 0;
			for (int r = 0; r < p; ++r) s += t[r] * t[r];
			if (s > bestNorm) {
				bestNorm = s;
				best = t;
			}
		}
		const R d = std::sqrt(bestNorm);
		for (int r = 0; r < p; ++r) z[r * q + i] = best[r] / d;
	}
	for (size_t i = 0; i < z.size(); ++i) y[i] = static_cast<double>(z[i]);
	return true;
}

}  // namespace smm
