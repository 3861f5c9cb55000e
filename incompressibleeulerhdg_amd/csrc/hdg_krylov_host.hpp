// Host arithmetic of the restarted Krylov solvers (Engine::arnoldi_cycle, Engine::fgmres_blocks): the least-squares problem
// min_y |beta e1 - H y| of one cycle, kept triangular by Givens rotations as the columns of the Hessenberg matrix arrive.
// Plain C++, no HIP: tests/host/tent_policy_check.cpp compiles it with g++ and checks it against the normal equations.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace hdg {

struct GivensLsq {
  int m;  // restart length: columns of H, and its row stride
  std::vector<double> H, cs, sn, gv;
  std::vector<double> Hraw;  // the unrotated matrix (m x m), kept only where the Ritz values are wanted
  explicit GivensLsq(int m_, bool keep_unrotated = false)
      : m(m_), H((size_t)(m_ + 1) * m_, 0.0), cs(m_), sn(m_), gv(m_ + 1), Hraw(keep_unrotated ? (size_t)m_ * m_ : 0, 0.0) {}
  // a cycle begins from a residual of norm beta
  void start(double beta) {
    std::fill(gv.begin(), gv.end(), 0.0);
    gv[0] = beta;
  }
  // column j: h[l] = (w, V_l), l <= j, and hn = |w - V h|.  Applies the earlier rotations to it, forms the one that removes
  // hn, and returns the residual norm of the least-squares problem with columns 0 .. j
  double add_column(int j, const double* h, double hn) {
    for (int l = 0; l <= j; l++) H[(size_t)l * m + j] = h[l];
    H[(size_t)(j + 1) * m + j] = hn;
    if (!Hraw.empty()) {
      for (int l = 0; l <= j; l++) Hraw[(size_t)l * m + j] = h[l];
      if (j + 1 < m) Hraw[(size_t)(j + 1) * m + j] = hn;
    }
    for (int l = 0; l < j; l++) {
      double a1 = H[(size_t)l * m + j], a2 = H[(size_t)(l + 1) * m + j];
      H[(size_t)l * m + j] = cs[l] * a1 + sn[l] * a2;
      H[(size_t)(l + 1) * m + j] = -sn[l] * a1 + cs[l] * a2;
    }
    double a1 = H[(size_t)j * m + j], a2 = H[(size_t)(j + 1) * m + j];
    double rr = std::hypot(a1, a2);
    cs[j] = (rr == 0) ? 1.0 : a1 / rr;
    sn[j] = (rr == 0) ? 0.0 : a2 / rr;
    H[(size_t)j * m + j] = rr;
    H[(size_t)(j + 1) * m + j] = 0.0;
    gv[j + 1] = -sn[j] * gv[j];
    gv[j] = cs[j] * gv[j];
    return std::fabs(gv[j + 1]);
  }
  // the minimiser over the first j columns (back-substitution in the rotated triangle)
  std::vector<double> solve(int j) const {
    std::vector<double> y(j, 0.0);
    for (int l = j - 1; l >= 0; l--) {
      double acc = gv[l];
      for (int q = l + 1; q < j; q++) acc -= H[(size_t)l * m + q] * y[q];
      y[l] = acc / H[(size_t)l * m + l];
    }
    return y;
  }
  // leading j x j block of the unrotated matrix, dense row-major: what hessenberg_eig takes
  std::vector<double> unrotated(int j) const {
    std::vector<double> Hs((size_t)j * j);
    for (int a = 0; a < j; a++) for (int c = 0; c < j; c++) Hs[(size_t)a * j + c] = Hraw[(size_t)a * m + c];
    return Hs;
  }
};

}  // namespace hdg
