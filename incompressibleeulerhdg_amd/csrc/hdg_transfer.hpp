// Transfer of broken fields between two nested structured meshes of any two degrees (hdg_transfer_state /
// hdg_transfer_difference): the host side.  Plain C++, no HIP: the child enumeration, the class of a
// child and the table C of L2 inner products between coarse and fine modes, checked on the host by
// tests/host/transfer_check.cpp.
//
// Meshes: a coarse square of side H holds r x r fine squares of side h = H / r.  Fine cell (i, j, s) lies in coarse square
// (i / r, j / r) at sub-square (a, b) = (i % r, j % r) -- integer arithmetic, no floating-point location.  With the shapes of
// hdg_tables.hpp (lower s = 0: x = (x_i, y_j) + h xi, upper s = 1: x = (x_{i+1}, y_{j+1}) - h xi) the lower sub-triangle lies in
// the coarse lower triangle iff a + b <= r - 1, the upper one iff a + b <= r - 2.
//
// Classes: in the reference coordinates of its parent a child is xi_c = (o + sigma xi_f) / r with integer o and sigma = +-1.
// An upper parent is the point reflection of a lower one: child (a, b, s) of an upper parent has the map of child
// (r-1-a, r-1-b, 1-s) of a lower parent.  So r^2 maps serve both parent shapes: r (r+1) / 2 children of the parent's own shape
// (sigma = +1, o = (a', b'), a' + b' <= r - 1) and r (r-1) / 2 of the other one (sigma = -1, o = (a'+1, b'+1), a' + b' <= r - 2);
// the second kind is stored at the reflected slot, which fills the r x r index square exactly once.
//
// Table: C[class][m][n] = int_ref phi_m(xi_c(xi_f)) phi_n(xi_f) dxi_f for the orthonormal Dubiner modes (Dubiner, ordered by
// total degree: the table of two lower degrees is the leading block).  With the physically orthonormal bases phi / h of the
// engine,  prolongation  a_f = (1 / r) C^T a_c,  restriction  a_c = (1 / r) sum_children C a_f.
#pragma once
#include <string>
#include <vector>

#include "hdg_tables.hpp"

namespace hdg {
namespace transfer {

constexpr int MAX_RATIO = 16;
constexpr int MAX_DEGREE = 5;  // of a polynomial space: velocity P_{k+1}, k <= 4

struct Child { int a, b, s; };

// shape of the coarse triangle that holds fine cell (a, b, s) of a coarse square
inline int parent_shape(int r, int a, int b, int s) { return a + b <= r - 1 - s ? 0 : 1; }

// the r^2 children of the coarse triangle of shape S, row by row
inline std::vector<Child> children(int r, int S) {
  std::vector<Child> c;
  for (int b = 0; b < r; b++)
    for (int a = 0; a < r; a++)
      for (int s = 0; s < 2; s++)
        if (parent_shape(r, a, b, s) == S) c.push_back(Child{a, b, s});
  return c;
}

// class of child (a, b, s) of a parent of shape S, in 0 .. r^2 - 1
inline int child_class(int r, int S, int a, int b, int s) {
  const int a1 = S ? r - 1 - a : a, b1 = S ? r - 1 - b : b;  // the same child seen from a lower parent
  return s == S ? b1 * r + a1 : (r - 1 - b1) * r + (r - 1 - a1);
}

// the map of a class: xi_c = (ox + sigma xi_f, oy + sigma eta_f) / r
inline void class_map(int r, int cls, int& sigma, int& ox, int& oy) {
  const int qa = cls % r, qb = cls / r;
  if (qa + qb <= r - 1) { sigma = 1; ox = qa; oy = qb; }
  else { sigma = -1; ox = r - qa; oy = r - qb; }
}

inline void check_pair(int dc, int df, int r) {
  if (dc < 0 || dc > MAX_DEGREE || df < 0 || df > MAX_DEGREE) throw std::string("transfer tables: degree out of range");
  if (r < 1 || r > MAX_RATIO) throw std::string("transfer tables: ratio out of range");
}

// C[class][m][n] by quadrature in long double: coarse modes m of degree <= dc, fine modes n of degree <= df.  The collapsed
// Gauss-Jacobi rule with 6 x 6 points is exact to degree 11 >= dc + df.
inline std::vector<real> child_tables_quadrature(int dc, int df, int r) {
  check_pair(dc, df, r);
  const Dubiner Bc(dc), Bf(df);
  const int nc = Bc.n, nf = Bf.n, mq = 6;
  std::vector<real> xa, wa, xb, wb;
  gaussJacobi(mq, 0, 0, xa, wa);
  gaussJacobi(mq, 1, 0, xb, wb);
  std::vector<real> C((size_t)r * r * nc * nf, 0), vc(nc), vf((size_t)mq * mq * nf);
  for (int i = 0; i < mq; i++)  // the fine modes at the points of the rule: the same for every class
    for (int j = 0; j < mq; j++) {
      const real eta = (xb[j] + 1) / 2, xi = (xa[i] + 1) / 2 * (1 - eta);
      Bf.eval(xi, eta, vf.data() + (size_t)(i * mq + j) * nf, nullptr, nullptr);
    }
  for (int cls = 0; cls < r * r; cls++) {
    int sigma, ox, oy;
    class_map(r, cls, sigma, ox, oy);
    real* Cc = C.data() + (size_t)cls * nc * nf;
    for (int i = 0; i < mq; i++)
      for (int j = 0; j < mq; j++) {
        const real eta = (xb[j] + 1) / 2, xi = (xa[i] + 1) / 2 * (1 - eta);
        const real w = wa[i] * wb[j] / 8;
        const real* vfq = vf.data() + (size_t)(i * mq + j) * nf;
        Bc.eval((ox + sigma * xi) / r, (oy + sigma * eta) / r, vc.data(), nullptr, nullptr);
        for (int m = 0; m < nc; m++)
          for (int n = 0; n < nf; n++) Cc[m * nf + n] += w * vc[m] * vfq[n];
      }
  }
  return C;
}

// the table the kernels read, rounded to double.  r = 1 has one class whose map is the identity: the modes are orthonormal,
// C = delta_mn, and it is stored as exactly that (a field transferred to its own space, or compared with itself, comes back
// bit for bit).
inline dvec child_tables(int dc, int df, int r) {
  const std::vector<real> C = child_tables_quadrature(dc, df, r);
  dvec out(C.begin(), C.end());
  if (r == 1) {
    const int nc = n_scalar(dc), nf = n_scalar(df);
    for (int m = 0; m < nc; m++)
      for (int n = 0; n < nf; n++) out[(size_t)m * nf + n] = m == n ? 1.0 : 0.0;
  }
  return out;
}

}  // namespace transfer
}  // namespace hdg
