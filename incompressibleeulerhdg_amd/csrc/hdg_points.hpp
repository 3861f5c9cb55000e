// Point values of the broken fields (hdg_evaluate_points / hdg_set_probes): the parts shared by host
// and device.  Plain C++ outside HIP (__host__ / __device__ are defined away), so that a host check compiles it with g++.
//
//   * dubiner_at<D>: the orthonormal Dubiner basis of degree D <= 5 and its reference gradients at any (xi, eta), in the
//     ordering and normalisation of Dubiner::eval (hdg_tables.hpp).  Dubiner::eval works in the collapsed coordinate
//     a = 2 (1 + r) / (1 - s) - 1, which is undefined at the vertex eta = 1; here the factor ((1 - s) / 2)^i P_i(a) is
//     carried as one homogeneous polynomial Q_i(A, B) of A = a (1 - s) / 2 = 2 xi + eta - 1 and B = (1 - s) / 2 = 1 - eta
//     through the three-term recurrence of P_i, so values and gradients are polynomials in (xi, eta) with no division:
//     finite and exact at the vertex, and at points a rounding error outside the triangle.
//   * square_locate: the ownership rule on the structured square meshes (closed form), on the host and on the device.
#pragma once
#include <cmath>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace hdg {

constexpr int POINT_NCOL = 5;           // ux, uy, p, q, omega
constexpr double POINT_TOL = 1e-12;     // barycentric (general meshes) / relative to L (unit square) tolerance of location

// orthonormal Jacobi polynomial P_N^(a, b) (weight (1-x)^a (1+x)^b on [-1, 1]) for integer a, b >= 0: jacobiP of
// hdg_tables.hpp with the Gamma functions of the norm written as factorials
__host__ __device__ inline double jacobi_at(double x, int a, int b, int N) {
  double fr = 1.0;  // a! b! / (a + b)!
  for (int t = 1; t <= b; t++) fr = fr * t / (a + t);
  const double g0 = std::ldexp(1.0, a + b + 1) / (a + b + 1) * fr;
  double p0 = 1.0 / std::sqrt(g0);
  if (N == 0) return p0;
  const double g1 = (a + 1.0) * (b + 1.0) / (a + b + 3.0) * g0;
  double p1 = ((a + b + 2.0) * x / 2 + (a - b) / 2.0) / std::sqrt(g1);
  double aold = 2.0 / (2 + a + b) * std::sqrt((a + 1.0) * (b + 1.0) / (a + b + 3.0));
  for (int i = 1; i < N; i++) {
    const double h1 = 2.0 * i + a + b;
    const double anew = 2.0 / (h1 + 2) * std::sqrt((i + 1.0) * (i + 1.0 + a + b) * (i + 1.0 + a) * (i + 1.0 + b) / (h1 + 1) / (h1 + 3));
    const double bnew = -(double)(a * a - b * b) / h1 / (h1 + 2);
    const double p2 = (-aold * p0 + (x - bnew) * p1) / anew;
    p0 = p1;
    p1 = p2;
    aold = anew;
  }
  return p1;
}

// values val[m] and reference gradients gx[m] = d/dxi, gy[m] = d/deta of the (D + 1)(D + 2) / 2 modes of degree <= D
template <int D>
__host__ __device__ inline void dubiner_at(double xi, double eta, double* val, double* gx, double* gy) {
  static_assert(D >= 0 && D <= 5, "point basis: degree <= 5");
  // Q_i = B^i P_i(A / B) for the orthonormal Legendre P_i (a = b = 0), and its derivatives in xi and eta
  const double A = 2.0 * xi + eta - 1.0, B = 1.0 - eta;
  double Q[D + 1], Qx[D + 1], Qy[D + 1];
  Q[0] = 1.0 / std::sqrt(2.0); Qx[0] = 0.0; Qy[0] = 0.0;
  if (D >= 1) { const double c1 = std::sqrt(1.5); Q[1] = c1 * A; Qx[1] = 2.0 * c1; Qy[1] = c1; }
  {
    double aold = 2.0 / 2.0 * std::sqrt(1.0 / 3.0);
    for (int i = 1; i < D; i++) {
      const double h1 = 2.0 * i;
      const double anew = 2.0 / (h1 + 2) * std::sqrt((i + 1.0) * (i + 1.0) * (i + 1.0) * (i + 1.0) / (h1 + 1) / (h1 + 3));
      // P_{i+1} = (x P_i - aold P_{i-1}) / anew, times B^{i+1}
      Q[i + 1] = (A * Q[i] - aold * B * B * Q[i - 1]) / anew;
      Qx[i + 1] = (2.0 * Q[i] + A * Qx[i] - aold * B * B * Qx[i - 1]) / anew;
      Qy[i + 1] = (Q[i] + A * Qy[i] + aold * (2.0 * B * Q[i - 1] - B * B * Qy[i - 1])) / anew;
      aold = anew;
    }
  }
  const double b = 2.0 * eta - 1.0;
  int m = 0;
  for (int t = 0; t <= D; t++)
    for (int i = t; i >= 0; i--, m++) {
      const int j = t - i;
      const double gb = jacobi_at(b, 2 * i + 1, 0, j);
      const double dgb = j > 0 ? std::sqrt((double)j * (j + 2 * i + 2)) * jacobi_at(b, 2 * i + 2, 1, j - 1) : 0.0;
      const double sc = 2.0 * std::ldexp(std::sqrt(2.0), i);  // 2 * 2^(i + 1/2)
      val[m] = sc * Q[i] * gb;
      gx[m] = sc * Qx[i] * gb;
      gy[m] = sc * (Qy[i] * gb + Q[i] * 2.0 * dgb);
    }
}

// Location on the structured square meshes: nx x ny squares of side h = L / nx (cell (i, j) = lower triangle s = 0 plus
// upper triangle s = 1).  Returns false for a point outside the unit square (more than POINT_TOL * L outside [0, L]^2); on
// the periodic square every finite point is located after wrapping into [0, L).  Reference coordinates: the lower shape maps
// x = (x_i, y_j) + h (xi, eta), the upper one x = (x_{i+1}, y_{j+1}) - h (xi, eta) (hdg_tables.hpp).  One operation per
// statement: no contraction into fma (the pragma holds it on the device too, where the particle kernels of hdg_particles.hpp
// locate every step), so that tests/probe_reference.py reproduces every rounding and host and device locate alike.
__host__ __device__ inline bool square_locate(double x, double y, int nx, int ny, double L, bool periodic, int& i, int& j,
                                              int& s, double& xi, double& eta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double h = L / nx;
  const double Lx = L, Ly = ny == nx ? L : ny * h;
  if (!(std::isfinite(x) && std::isfinite(y))) return false;
  if (periodic) {
    const double wx = std::floor(x / Lx) * Lx;
    const double wy = std::floor(y / Ly) * Ly;
    x -= wx;
    y -= wy;
    if (x >= Lx || x < 0.0) x = 0.0;
    if (y >= Ly || y < 0.0) y = 0.0;
  } else {
    const double tx = POINT_TOL * Lx, ty = POINT_TOL * Ly;
    if (x < -tx || x > Lx + tx || y < -ty || y > Ly + ty) return false;
    x = std::fmin(std::fmax(x, 0.0), Lx);
    y = std::fmin(std::fmax(y, 0.0), Ly);
  }
  i = (int)std::floor(x / h);
  j = (int)std::floor(y / h);
  if (i > nx - 1) i = nx - 1;
  if (j > ny - 1) j = ny - 1;
  const double fx = x / h - i;
  const double fy = y / h - j;
  s = (fx + fy <= 1.0) ? 0 : 1;
  xi = s == 0 ? fx : 1.0 - fx;
  eta = s == 0 ? fy : 1.0 - fy;
  return true;
}

}  // namespace hdg
