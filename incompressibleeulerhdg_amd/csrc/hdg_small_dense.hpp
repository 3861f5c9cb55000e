// Small dense host mathematics of the solvers: eigenvalues of a Hessenberg matrix (Ritz values of a GMRES cycle), the
// least-squares step of an s-step cycle from its Gram matrix, a dense transpose.  Plain C++ (no HIP header,
// tests/host/small_dense_check.cpp compiles it with g++).
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace hdg {

// row-major r x c -> c x r
inline std::vector<double> transpose(const std::vector<double>& a, int r, int c) {
  std::vector<double> t(a.size());
  for (int i = 0; i < r; i++)
    for (int j = 0; j < c; j++) t[(size_t)j * r + i] = a[(size_t)i * c + j];
  return t;
}

// eigenvalues of a small upper Hessenberg matrix: shifted QR iteration in complex arithmetic with
// deflation (n <= 32, used for Ritz values only)
inline std::vector<std::complex<double>> hessenberg_eig(const std::vector<double>& Hin, int n) {
  typedef std::complex<double> cd;
  std::vector<cd> H((size_t)n * n);
  for (int i = 0; i < n * n; i++) H[i] = Hin[i];
  std::vector<cd> ev;
  int hi = n - 1;
  int guard = 0;
  while (hi >= 0 && guard++ < 10000) {
    if (hi == 0) { ev.push_back(H[0]); break; }
    // deflate
    double sub = std::abs(H[(size_t)hi * n + hi - 1]);
    double diag = std::abs(H[(size_t)hi * n + hi]) + std::abs(H[(size_t)(hi - 1) * n + hi - 1]);
    if (sub <= 1e-14 * (diag > 0 ? diag : 1.0)) { ev.push_back(H[(size_t)hi * n + hi]); hi--; continue; }
    // Wilkinson shift from the trailing 2x2 block
    cd a = H[(size_t)(hi - 1) * n + hi - 1], b = H[(size_t)(hi - 1) * n + hi], c = H[(size_t)hi * n + hi - 1], d = H[(size_t)hi * n + hi];
    cd tr = a + d, det = a * d - b * c, disc = std::sqrt(tr * tr - 4.0 * det);
    cd l1 = 0.5 * (tr + disc), l2 = 0.5 * (tr - disc);
    cd mu = (std::abs(l1 - d) < std::abs(l2 - d)) ? l1 : l2;
    if (guard % 11 == 10) mu += cd(0.37 * sub, 0.11 * sub);  // exceptional shift
    // QR step on the active block 0..hi by Givens rotations
    std::vector<cd> cs_(hi), sn_(hi);
    for (int i = 0; i <= hi; i++) H[(size_t)i * n + i] -= mu;
    for (int k = 0; k < hi; k++) {
      cd x = H[(size_t)k * n + k], y = H[(size_t)(k + 1) * n + k];
      double r = std::sqrt(std::norm(x) + std::norm(y));
      cd cc = (r == 0) ? cd(1) : x / r, ss = (r == 0) ? cd(0) : y / r;
      cs_[k] = cc; sn_[k] = ss;
      for (int col = k; col <= hi; col++) {
        cd u = H[(size_t)k * n + col], v = H[(size_t)(k + 1) * n + col];
        H[(size_t)k * n + col] = std::conj(cc) * u + std::conj(ss) * v;
        H[(size_t)(k + 1) * n + col] = -ss * u + cc * v;
      }
    }
    for (int k = 0; k < hi; k++) {
      int rmax = std::min(hi, k + 1);
      for (int row = 0; row <= rmax; row++) {
        cd u = H[(size_t)row * n + k], v = H[(size_t)row * n + k + 1];
        H[(size_t)row * n + k] = u * cs_[k] + v * sn_[k];
        H[(size_t)row * n + k + 1] = -u * std::conj(sn_[k]) + v * std::conj(cs_[k]);
      }
    }
    for (int i = 0; i <= hi; i++) H[(size_t)i * n + i] += mu;
  }
  return ev;
}

// s-step minimal-residual cycle (Engine::sstep_mr), power basis K_0 .. K_sl:
// least-squares coefficients of min |K_0 - sum_{i=1..sl} y_i K_i| from the Gram matrix G ((sl+1) x (sl+1), row-major):
// scaled normal equations, Cholesky in long double truncated at the first pivot below 1e-13; returns the rank and the
// predicted residual norm (from the Gram matrix: reliable down to reductions of ~1e-6 of |K_0|)
inline int sstep_ls(const std::vector<long double>& G, int nv, int sl, std::vector<long double>& y, double& rho) {
  std::vector<long double> d(sl), L((size_t)sl * sl, 0.0L), rhs(sl);
  y.assign(sl, 0.0L);
  for (int i = 0; i < sl; i++) d[i] = std::sqrt(std::max(G[(size_t)(i + 1) * nv + (i + 1)], (long double)1e-300));
  int rank = 0;
  for (int j = 0; j < sl; j++) {
    long double piv = 1.0L;
    for (int q = 0; q < j; q++) piv -= L[(size_t)j * sl + q] * L[(size_t)j * sl + q];
    if (!(piv > 1e-13L)) break;
    L[(size_t)j * sl + j] = std::sqrt(piv);
    for (int i = j + 1; i < sl; i++) {
      long double v = G[(size_t)(i + 1) * nv + (j + 1)] / (d[i] * d[j]);
      for (int q = 0; q < j; q++) v -= L[(size_t)i * sl + q] * L[(size_t)j * sl + q];
      L[(size_t)i * sl + j] = v / L[(size_t)j * sl + j];
    }
    rank = j + 1;
  }
  for (int i = 0; i < rank; i++) {  // forward, then backward substitution on the leading rank x rank block
    long double v = G[(size_t)(i + 1) * nv] / d[i];
    for (int q = 0; q < i; q++) v -= L[(size_t)i * sl + q] * rhs[q];
    rhs[i] = v / L[(size_t)i * sl + i];
  }
  for (int i = rank - 1; i >= 0; i--) {
    long double v = rhs[i];
    for (int q = i + 1; q < rank; q++) v -= L[(size_t)q * sl + i] * y[q];
    y[i] = v / L[(size_t)i * sl + i];
  }
  for (int i = 0; i < rank; i++) y[i] /= d[i];
  long double r2 = G[0];
  for (int i = 0; i < rank; i++) {
    r2 -= 2.0L * y[i] * G[(size_t)(i + 1) * nv];
    for (int q = 0; q < rank; q++) r2 += y[i] * y[q] * G[(size_t)(i + 1) * nv + (q + 1)];
  }
  rho = std::sqrt((double)std::max(r2, 0.0L));
  return rank;
}

}  // namespace hdg
