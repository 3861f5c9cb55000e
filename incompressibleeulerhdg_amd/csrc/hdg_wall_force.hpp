// Viscous wall force: the force on the fluid through side w of the unit square, the viscous form with
// its moving-wall load tested against the constants e_c and restricted to w,
//   F_w . e_c = nu int_w (e_c.n)( n.dn u - eta_b u.n ) ds                     always
//             + nu int_w (e_c.t)( t.dn u - eta_b (u.t - U_w) ) ds             no slip only
// so that sum_w F_w = int nu M^-1 (V u + l(U)) dx for every broken u: the drag counterpart of the tracers' wall flux.
//
// Every wall is axis-aligned, so in the orthonormal modal basis the force of one cell through its leg (s, e) is, per component d,
//   - lvec[s][e] . u_d  (+ U_w wone on the tangential component),   wone = eta_b h,
// the normal component always, the tangential one with no slip only (ViscosityTables::packed_moving holds lvec behind the blocks).
//
// k_wall_force: one thread per wall-leg cell -- 2 (nx + ny) of them, a corner cell once per leg; gridDim.y = the four sides
// bottom, right, top, left, so the side and with it the shape and the leg are uniform over a workgroup and lvec arrives through
// scalar loads.  Every thread forms both components; a workgroup leaves one partial per component in
// part[(side * 2 + c) * gridDim.x + block].  k_wall_force_finish (one workgroup) adds the partials of a (side, component) in block
// order and scales by nu.  No floating-point atomics, every sum in a fixed order: two calls give the same bits.
// Owned rows only.  On a strip the bottom belongs to the rank that owns global row 0 and the top to the one that owns the last
// row; a rank's share of left and right is its own rows (the caller adds the eight values over the ranks).
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

#define HDG_WALL_FORCE_BLOCK 128
template <int K>
__global__ __launch_bounds__(HDG_WALL_FORCE_BLOCK) void k_wall_force(Geo g, const double* __restrict__ tab, int no_slip, double wone, WallSpeed W,
                                                                      const double* __restrict__ u, double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU, BL = NU * NU;
  const int side = blockIdx.y;                       // 0 bottom, 1 right, 2 top, 3 left
  const int s = (side == 1 || side == 2) ? 1 : 0;    // the shape whose leg lies on that side
  const int e = (side == 0 || side == 2) ? 0 : 2;    // horizontal / vertical leg
  const int len = e == 0 ? g.nx : g.ny;
  const int pos = blockIdx.x * HDG_WALL_FORCE_BLOCK + threadIdx.x;
  // the side exists on this rank: bottom with global row 0, top with the last global row; no side on the periodic square
  const bool mine = side == 0 ? g.joff == 0 : (side == 2 ? g.joff + g.ny == g.nyg : g.px == 0);
  const bool live = mine && pos < len;
  const int i = e == 0 ? pos : (side == 1 ? g.nx - 1 : 0);
  const int j = e == 2 ? pos : (side == 2 ? g.ny - 1 : 0);
  const long c = live ? rowbase(g, s, j) + i : rowbase(g, s, 0);  // a dead lane reads a valid cell and adds zero
  const double* __restrict__ lv = tab + 2 * 9 * BL + (2 * s + (e == 0 ? 0 : 1)) * NU;
  const double side_u = side == 0 ? W.bottom : (side == 1 ? W.right : (side == 2 ? W.top : W.left));
  const VelBuf U(u);
  const unsigned lane_b = (unsigned)c * 16u;
  double dx = 0.0, dy = 0.0;
#pragma unroll
  for (int m = 0; m < NU; m++) {
    const hdg_d2 x = U.ld(pair_bytes(m, g.Nc), lane_b);
    dx = fma(lv[m], x.x, dx);
    dy = fma(lv[m], x.y, dy);
  }
  // horizontal wall (e = 0): y is the normal component, x the tangential one; vertical wall: the other way round
  const double tang = no_slip ? side_u * wone - (e == 0 ? dx : dy) : 0.0;
  const double norm = -(e == 0 ? dy : dx);
  const double fx = live ? (e == 0 ? tang : norm) : 0.0;
  const double fy = live ? (e == 0 ? norm : tang) : 0.0;
  __shared__ double sm[2][HDG_WALL_FORCE_BLOCK / 64];
  const double wx = wave_sum(fx), wy = wave_sum(fy);
  if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = wx; sm[1][threadIdx.x >> 6] = wy; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double a = 0.0;
    for (int v = 0; v < HDG_WALL_FORCE_BLOCK / 64; v++) a += sm[threadIdx.x][v];
    part[((long)side * 2 + threadIdx.x) * gridDim.x + blockIdx.x] = a;
  }
}

// F[side * 2 + c] = nu * (the partials of (side, c) in block order); one workgroup, thread side * 2 + c
__global__ void k_wall_force_finish(int nblk, int nx, int ny, double nu, const double* __restrict__ part, double* __restrict__ F) {
  const int n = threadIdx.x;
  if (n >= 8) return;
  const int side = n >> 1;
  const int len = (side == 0 || side == 2) ? nx : ny;
  const int used = (len + HDG_WALL_FORCE_BLOCK - 1) / HDG_WALL_FORCE_BLOCK;  // the blocks of this side that hold cells
  double a = 0.0;
  for (int b = 0; b < used && b < nblk; b++) a += part[(long)n * nblk + b];
  F[n] = nu * a;
}

}  // namespace hdg
