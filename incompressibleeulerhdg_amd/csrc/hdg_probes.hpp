// Point values on the device (hdg_evaluate_points / hdg_set_probes).
//
// A point set is located once on the host (hdg_points.hpp square_locate, hdg_general.hpp GLocator) into a table of
// PointLoc entries: the cell layout index c, the shape s, and the reference coordinates (xi, eta) in that shape.  One thread
// per point then evaluates the modal coefficients of its cell with dubiner_at<K + 1> and writes one row of POINT_NCOL values
//   ux, uy, p, q, omega = d_x u_y - d_y u_x   (omega: the curl of the broken velocity inside the owning cell)
// A column whose field pointer is null is NaN; a point outside the domain (s = PT_OUTSIDE) is a NaN row.  A point another rank
// owns (s = PT_OTHER_RANK) is a zero row, so that one all-reduce sum over the ranks gives every rank the full row (each entry
// has exactly one non-zero contributor; NaN columns stay NaN).
#pragma once
#include <hip/hip_runtime.h>
#include "hdg_points.hpp"

namespace hdg {

constexpr int PT_OUTSIDE = -2;     // PointLoc::s: outside the domain
constexpr int PT_OTHER_RANK = -1;  // PointLoc::s: owned by another rank of a strip partition
struct PointLoc {
  double xi, eta;
  long c;  // cell layout index: rowbase(g, s, j) + i (structured), the cell number (general)
  int s;   // structured: 0 lower, 1 upper shape; general: 0; or PT_OUTSIDE / PT_OTHER_RANK
  int pad;
};
constexpr int POINT_BLOCK = 64;

__device__ __forceinline__ void point_row_fill(double* __restrict__ r, double v) {
#pragma unroll
  for (int col = 0; col < POINT_NCOL; col++) r[col] = v;
}

// shared tail: velocity values and physical gradients from the reference ones, via (vsc, the map of reference to physical
// gradients d/dx = a00 d/dxi + a10 d/deta, d/dy = a01 d/dxi + a11 d/deta)
template <int K>
__device__ __forceinline__ void point_row(const double (&val)[Dim<K>::NU], const double (&gx)[Dim<K>::NU],
                                          const double (&gy)[Dim<K>::NU], const double (&x)[2 * Dim<K>::NU], bool hasQ,
                                          const double* pp, const double* qq, double vsc, double a00, double a01, double a10,
                                          double a11, double* __restrict__ r) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP;
  const double nan = __builtin_nan("");
  if (hasQ) {
    double ux = 0, uy = 0, dxi_y = 0, deta_y = 0, dxi_x = 0, deta_x = 0;
#pragma unroll
    for (int m = 0; m < NU; m++) {
      ux = fma(val[m], x[m], ux); uy = fma(val[m], x[NU + m], uy);
      dxi_x = fma(gx[m], x[m], dxi_x); deta_x = fma(gy[m], x[m], deta_x);
      dxi_y = fma(gx[m], x[NU + m], dxi_y); deta_y = fma(gy[m], x[NU + m], deta_y);
    }
    const double dyx_dx = a00 * dxi_y + a10 * deta_y;  // d_x u_y
    const double dxy_dy = a01 * dxi_x + a11 * deta_x;  // d_y u_x
    r[0] = vsc * ux;
    r[1] = vsc * uy;
    r[4] = dyx_dx - dxy_dy;
  } else {
    r[0] = r[1] = r[4] = nan;
  }
  double pv = 0, qv = 0;
#pragma unroll
  for (int m = 0; m < NP; m++) {
    if (pp) pv = fma(val[m], pp[m], pv);
    if (qq) qv = fma(val[m], qq[m], qv);
  }
  r[2] = pp ? vsc * pv : nan;
  r[3] = qq ? vsc * qv : nan;
}

// structured meshes: modal coefficients of cell c in the plane layouts (velocity pair planes, pressure planes, stride Nc);
// the basis is 1 / h times the reference one, reference gradients scale by +-1 / h^2 (upper shape: x = x_{i+1} - h xi)
template <int K>
__global__ __launch_bounds__(POINT_BLOCK) void k_point_eval(int n, const PointLoc* __restrict__ loc, long Nc, double h,
                                                            const double* __restrict__ Q, const double* __restrict__ p,
                                                            const double* __restrict__ q, double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const PointLoc L = loc[t];
  double* __restrict__ r = out + (long)t * POINT_NCOL;
  if (L.s == PT_OUTSIDE) { point_row_fill(r, __builtin_nan("")); return; }
  if (L.s == PT_OTHER_RANK) {
    point_row_fill(r, 0.0);
    if (!Q) r[0] = r[1] = r[4] = __builtin_nan("");
    if (!p) r[2] = __builtin_nan("");
    if (!q) r[3] = __builtin_nan("");
    return;
  }
  double val[NU], gx[NU], gy[NU], x[2 * NU], pp[NP], qq[NP];
  dubiner_at<K + 1>(L.xi, L.eta, val, gx, gy);
  if (Q) {
#pragma unroll
    for (int m = 0; m < NU; m++) { x[m] = Q[((m * Nc + L.c) << 1)]; x[NU + m] = Q[((m * Nc + L.c) << 1) + 1]; }
  } else {
#pragma unroll
    for (int m = 0; m < 2 * NU; m++) x[m] = 0.0;
  }
#pragma unroll
  for (int m = 0; m < NP; m++) { pp[m] = p ? p[m * Nc + L.c] : 0.0; qq[m] = q ? q[m * Nc + L.c] : 0.0; }
  const double sg = (L.s == 0 ? 1.0 : -1.0) / (h * h);
  point_row<K>(val, gx, gy, x, Q != nullptr, p ? pp : nullptr, q ? qq : nullptr, 1.0 / h, sg, 0.0, 0.0, sg, r);
}

// general meshes: per-cell layout c * 2NU (x components, then y) / c * NP, basis inv_sdet times the reference one, gradients
// through the cell's inverse Jacobian (as k_g_diag_cell)
template <int K>
__global__ __launch_bounds__(POINT_BLOCK) void k_g_point_eval(GGeo G, int n, const PointLoc* __restrict__ loc,
                                                              const double* __restrict__ Q, const double* __restrict__ p,
                                                              const double* __restrict__ q, double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP, N2 = 2 * NU;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const PointLoc L = loc[t];
  double* __restrict__ r = out + (long)t * POINT_NCOL;
  if (L.s < 0) { point_row_fill(r, __builtin_nan("")); return; }
  const long c = L.c;
  double val[NU], gx[NU], gy[NU], x[N2], pp[NP], qq[NP];
  dubiner_at<K + 1>(L.xi, L.eta, val, gx, gy);
#pragma unroll
  for (int m = 0; m < N2; m++) x[m] = Q ? Q[c * N2 + m] : 0.0;
#pragma unroll
  for (int m = 0; m < NP; m++) { pp[m] = p ? p[c * NP + m] : 0.0; qq[m] = q ? q[c * NP + m] : 0.0; }
  const double s = G.inv_sdet[c];
  point_row<K>(val, gx, gy, x, Q != nullptr, p ? pp : nullptr, q ? qq : nullptr, s, G.Jinv[4 * c + 0] * s,
               G.Jinv[4 * c + 1] * s, G.Jinv[4 * c + 2] * s, G.Jinv[4 * c + 3] * s, r);
}

}  // namespace hdg
