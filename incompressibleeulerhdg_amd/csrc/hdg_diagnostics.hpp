// Flow diagnostics on the device (hdg_compute_diagnostics / hdg_set_diagnostics).
//
// For the velocity u (broken [P_{k+1}]^2), pressure p and tracer q (P_k) of one state:
//   0 energy          1/2 int |u|^2
//   1 enstrophy       1/2 sum_K int_K (d_x u_y - d_y u_x)^2        (broken curl, no edge terms)
//   2 div_l2          (sum_K int_K (div u)^2)^(1/2)
//   3 jump_l2         (sum_F int_F [u.n]^2)^(1/2)   interior edges, and the boundary edges (u.n) of a non-periodic mesh;
//                                                   every edge once
//   4 p_integral      int p
//   5 tracer_integral int q                       (NaN without a tracer)
//   6 tracer_half_sq  1/2 int q^2                 (NaN without a tracer)
//   7 max_speed       max |u| over the nodes of V_Q (hdg_node_coordinates)
//   8 cfl             dt max_K (max nodal |u| in K) / h_K,   h_K = shortest edge of K
//
// The bases are physically orthonormal and hierarchical (the pressure modes are the first NP velocity modes, mode 0 is the
// constant 1 / sqrt|K|), so 0 and 6 are sums of squared coefficients and 4, 5 are sqrt|K| times mode 0.  1 and 2 use the
// advection cell rule (exact to degree 3k + 2 >= 2k), 3 the advection edge rule (Gauss, exact to degree >= 3k + 3).  Nodal
// values come from the modal -> nodal matrix of the library boundary.
//
// Two passes and a second reduction stage, nothing leaves the device:
//   cell pass  (k_diag_cell / k_g_diag_cell): one thread per cell reads u, p, q once; per-workgroup partials
//              part[b * DIAG_NPART + 0..5] (sums 0, 1, 2^2, 4, 5, 6) and [6, 7] (maxima of |u| and |u| / h_K);
//   edge pass  (k_diag_edge / k_g_diag_edge): the corner / edge gathers of k_dg_avg_trace / k_g_dg_avg_trace, per-workgroup
//              sums of int_F [u.n]^2;
//   k_diag_reduce: one workgroup, fixed order -> acc[0..6] sums (the edge sum last), acc[7..8] maxima;
//   (strip partitions: all-reduce of the sums, all-gather of the maxima);  k_diag_row: the nine columns.
#pragma once
#include <hip/hip_runtime.h>

#include "hdg_step_rate.hpp"

namespace hdg {

constexpr int DIAG_NPART = 8;  // per-workgroup partials of the cell pass: 6 sums, 2 maxima
constexpr int DIAG_NACC = 9;   // k_diag_reduce: 7 sums (the 6 cell sums, the edge sum), 2 maxima
constexpr int DIAG_NCOL = 9;   // columns of a diagnostics row
constexpr int DIAG_BLOCK = 128;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// workgroup reduction of NS sums and NM maxima into part[blockIdx.x * (NS + NM) + ...] (blockDim.x <= 256, a multiple of 64)
template <int NS, int NM>
__device__ __forceinline__ void diag_block_store(const double (&sm)[NS], const double (&mx)[NM], double* __restrict__ part) {
  __shared__ double red[4][NS + NM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const double v = wave_sum(sm[k]);
    if (lane == 0) red[wv][k] = v;
  }
#pragma unroll
  for (int k = 0; k < NM; k++) {
    const double v = wave_max(mx[k]);
    if (lane == 0) red[wv][NS + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS + NM) {
    const int k = threadIdx.x;
    double v = red[0][k];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) v = k < NS ? v + red[w][k] : fmax(v, red[w][k]);
    part[(long)blockIdx.x * (NS + NM) + k] = v;
  }
}

// per-cell accumulation shared by both cell passes.  x: velocity coefficients (x components, then y components), pp / qq:
// pressure / tracer coefficients; phys(qp, m, gx, gy): physical gradient of velocity mode m at rule point qp; w(qp): weight
// incl. |K|; Vu (NU x NU, row = node) times vsc: modal -> nodal, or Qn != null: the cell's nodal values Qn[2 n + d] as given
// (hdg_compute_diagnostics: the maxima of the caller's own nodal values, not of a round trip through the modal basis);
// sqK = sqrt|K|, hK = shortest edge
template <int K, typename Grad, typename Wt>
__device__ __forceinline__ void diag_cell_acc(const double (&x)[2 * Dim<K>::NU], const double (&pp)[Dim<K>::NP],
                                              const double (&qq)[Dim<K>::NP], bool tracer, int nqc, Grad phys, Wt wt,
                                              const double* __restrict__ Vu, double vsc, const double* __restrict__ Qn,
                                              double sqK, double hK,
                                              double (&sm)[6], double (&mx)[2]) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP;
  double e = 0.0;
#pragma unroll
  for (int n = 0; n < 2 * NU; n++) e = fma(x[n], x[n], e);
  sm[0] += 0.5 * e;
  double ens = 0.0, dv = 0.0;
#pragma unroll 1
  for (int qp = 0; qp < nqc; qp++) {
    double dxx = 0, dxy = 0, dyx = 0, dyy = 0;  // dab = d_b u_a
#pragma unroll
    for (int m = 1; m < NU; m++) {  // mode 0 is constant
      double gx, gy;
      phys(qp, m, gx, gy);
      dxx = fma(gx, x[m], dxx); dxy = fma(gy, x[m], dxy);
      dyx = fma(gx, x[NU + m], dyx); dyy = fma(gy, x[NU + m], dyy);
    }
    const double w = wt(qp), cu = dyx - dxy, di = dxx + dyy;
    ens = fma(w * cu, cu, ens);
    dv = fma(w * di, di, dv);
  }
  sm[1] += 0.5 * ens;
  sm[2] += dv;
  sm[3] += sqK * pp[0];
  if (tracer) {
    double t2 = 0.0;
#pragma unroll
    for (int r = 0; r < NP; r++) t2 = fma(qq[r], qq[r], t2);
    sm[4] += sqK * qq[0];
    sm[5] += 0.5 * t2;
  }
  const double sp = cell_max_speed<K, false>(x, Vu, vsc, Qn);  // hdg_step_rate.hpp: shared with the step-rate kernels
  mx[0] = fmax(mx[0], sp);
  mx[1] = fmax(mx[1], sp / hK);
}

// ---- structured meshes: the cell index math of HDG_CELL_PROLOGUE, but every thread reaches the workgroup reduction
template <int K>
__global__ __launch_bounds__(DIAG_BLOCK) void k_diag_cell(Geo g, DevTables T, const double* __restrict__ Q,
                                                           const double* __restrict__ p, const double* __restrict__ q,
                                                           const double* __restrict__ Qn, double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP;
  const CellAt at = cell_at(g);
  const int s = at.s, i = at.i, j = at.j;
  const bool live = at.live;
  double sm[6] = {0, 0, 0, 0, 0, 0}, mx[2] = {0, 0};
  if (live) {
    const long c = rowbase(g, s, j) + i;
    double x[2 * NU], pp[NP], qq[NP];
    load_vel<NU>(Q, g.Nc, c, x);
    load_cell<NP>(p, g.Nc, c, pp);
    if (q) load_cell<NP>(q, g.Nc, c, qq);
    else {
#pragma unroll
      for (int r = 0; r < NP; r++) qq[r] = 0.0;
    }
    const double* __restrict__ Gx = T.cGx[s];
    const double* __restrict__ Gy = T.cGy[s];
    const double* __restrict__ cw = T.cw;
    diag_cell_acc<K>(x, pp, qq, q != nullptr, T.nqc,
                     [&](int qp, int m, double& gx, double& gy) { gx = Gx[qp * NU + m]; gy = Gy[qp * NU + m]; },
                     [&](int qp) { return cw[qp]; }, T.Vu, 1.0,
                     Qn ? Qn + (2 * ((long)j * g.nx + i) + s) * (2 * NU) : nullptr, g.h * 0.70710678118654752440, g.h, sm, mx);
  }
  diag_block_store<6, 2>(sm, mx, part);
}

// edge pass: the corner threads of k_dg_avg_trace (three edges per grid corner), int_F [u.n]^2 per workgroup
template <int K>
__global__ __launch_bounds__(DIAG_BLOCK) void k_diag_edge(Geo g, DevTables T, const double* __restrict__ Q,
                                                           double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU;
  const int xcd_ = blockIdx.x & 7, q_ = blockIdx.x >> 3;
  const int jj_ = q_ / g.nbxc;
  const int i = (q_ - jj_ * g.nbxc) * blockDim.x + threadIdx.x;
  const int r_ = xcd_ * g.rows_xcdc + jj_;
  const int j = launch_row(g, r_);
  const bool live = jj_ < g.rows_xcdc && r_ < g.wrowsc && i <= g.nx - g.px;
  double sm[1] = {0.0}, mx[1] = {0.0};  // the maximum slot stays zero
  if (live) {
    const bool in_x = i < g.nx, in_y = j < g.ny + g.ehi;
    const bool below = (g.joff + j) > 0;
    const bool left = i > 0 || g.px;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int e = (t == 0) ? 0 : (t == 1 ? 2 : 1);
      bool valid, hasL, hasU;
      long cL, cU;
      if (t == 0) { valid = in_x; hasL = in_y; hasU = below; cL = cidx(g, 0, j, i); cU = cidx(g, 1, j - 1, i); }
      else if (t == 1) { valid = in_y; hasL = in_x; hasU = left; cL = cidx(g, 0, j, i); cU = cidx(g, 1, j, xm1(g, i)); }
      else { valid = in_x && in_y; hasL = hasU = true; cL = cidx(g, 0, j, i); cU = cidx(g, 1, j, i); }
      if (!valid) continue;
      // normal components of the coefficients: a = n.x_L, b = n.x_U (zero for a missing side)
      const double nx_ = T.enx[e], ny_ = T.eny[e];
      double a[NU], b[NU];
      {
        double xs[2 * NU];
        if (hasL) load_vel<NU>(Q, g.Nc, cL, xs);
#pragma unroll
        for (int m = 0; m < NU; m++) a[m] = hasL ? fma(nx_, xs[m], ny_ * xs[NU + m]) : 0.0;
        if (hasU) load_vel<NU>(Q, g.Nc, cU, xs);
#pragma unroll
        for (int m = 0; m < NU; m++) b[m] = hasU ? fma(nx_, xs[m], ny_ * xs[NU + m]) : 0.0;
      }
      const double* __restrict__ PL = T.ePhi[0][e];
      const double* __restrict__ PU = T.ePhi[1][e];
      const double* __restrict__ ew = T.ew[e];
#pragma unroll 1
      for (int qp = 0; qp < T.nqe; qp++) {
        double jn = 0.0;
#pragma unroll
        for (int m = 0; m < NU; m++) jn = fma(PL[qp * NU + m], a[m], fma(-PU[qp * NU + m], b[m], jn));
        sm[0] = fma(ew[qp] * jn, jn, sm[0]);
      }
    }
  }
  diag_block_store<1, 1>(sm, mx, part);
}

// ---- general meshes: one thread per cell / edge, per-cell geometry as in k_g_adv
template <int K>
__global__ __launch_bounds__(DIAG_BLOCK) void k_g_diag_cell(GGeo G, const double* __restrict__ Vu, const double* __restrict__ hmin,
                                                             const double* __restrict__ Q, const double* __restrict__ p,
                                                             const double* __restrict__ q, const double* __restrict__ Qn,
                                                             double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP, N2 = 2 * NU;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  double sm[6] = {0, 0, 0, 0, 0, 0}, mx[2] = {0, 0};
  if (c < G.nc) {
    double x[N2], pp[NP], qq[NP];
#pragma unroll
    for (int n = 0; n < N2; n++) x[n] = Q[(long)c * N2 + n];
#pragma unroll
    for (int r = 0; r < NP; r++) { pp[r] = p[(long)c * NP + r]; qq[r] = q ? q[(long)c * NP + r] : 0.0; }
    const double s = G.inv_sdet[c], dj = G.detJ[c];
    const double j00 = G.Jinv[4 * (long)c + 0] * s, j01 = G.Jinv[4 * (long)c + 1] * s, j10 = G.Jinv[4 * (long)c + 2] * s,
                 j11 = G.Jinv[4 * (long)c + 3] * s;
    const double* __restrict__ Gxi = G.cGxi;
    const double* __restrict__ Get = G.cGeta;
    const double* __restrict__ cw = G.cw;
    diag_cell_acc<K>(x, pp, qq, q != nullptr, G.nqc,
                     [&](int qp, int m, double& gx, double& gy) {
                       const double a = Gxi[qp * NU + m], b = Get[qp * NU + m];
                       gx = j00 * a + j10 * b; gy = j01 * a + j11 * b;
                     },
                     [&](int qp) { return cw[qp] * dj; }, Vu, s, Qn ? Qn + (long)c * N2 : nullptr,
                     sqrt(0.5 * dj), hmin[c], sm, mx);
  }
  diag_block_store<6, 2>(sm, mx, part);
}

// ecl[2 e + side] = 3 c + l of the cells of edge e (-1: none), as for k_g_dg_avg_trace
template <int K>
__global__ __launch_bounds__(DIAG_BLOCK) void k_g_diag_edge(GGeo G, int ne, const int* __restrict__ ecl, const double* __restrict__ Q,
                                                             double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU, N2 = 2 * NU;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  double sm[1] = {0.0}, mx[1] = {0.0};
  if (e < ne) {
    const int s0 = ecl[2 * (long)e], s1 = ecl[2 * (long)e + 1];
    const double nx_ = G.cenx[s0], ny_ = G.ceny[s0], len = G.celen[s0];
    const double* __restrict__ P0 = G.ePhi + (long)G.ctab[s0] * G.nqe * NU;
    const double* __restrict__ P1 = G.ePhi + (long)(s1 >= 0 ? G.ctab[s1] : 0) * G.nqe * NU;
    double a[NU], b[NU];
    {
      const int c0 = s0 / 3;
      const double sc = G.inv_sdet[c0];
#pragma unroll
      for (int m = 0; m < NU; m++) a[m] = sc * fma(nx_, Q[(long)c0 * N2 + m], ny_ * Q[(long)c0 * N2 + NU + m]);
      if (s1 >= 0) {
        const int c1 = s1 / 3;
        const double sn = G.inv_sdet[c1];
#pragma unroll
        for (int m = 0; m < NU; m++) b[m] = sn * fma(nx_, Q[(long)c1 * N2 + m], ny_ * Q[(long)c1 * N2 + NU + m]);
      } else {
#pragma unroll
        for (int m = 0; m < NU; m++) b[m] = 0.0;
      }
    }
    for (int qp = 0; qp < G.nqe; qp++) {
      double jn = 0.0;
#pragma unroll
      for (int m = 0; m < NU; m++) jn = fma(P0[qp * NU + m], a[m], fma(-P1[qp * NU + m], b[m], jn));
      sm[0] = fma(G.ew[qp] * len * jn, jn, sm[0]);
    }
  }
  diag_block_store<1, 1>(sm, mx, part);
}

// second stage, one workgroup of 1024 threads, fixed order: acc[0..5] cell sums, acc[6] edge sum, acc[7..8] maxima
__global__ __launch_bounds__(1024) void k_diag_reduce(int ncb, const double* __restrict__ cpart, int neb,
                                                      const double* __restrict__ epart, double* __restrict__ acc) {
  double sm[7] = {0, 0, 0, 0, 0, 0, 0}, mx[2] = {0, 0};
  for (int b = threadIdx.x; b < ncb; b += blockDim.x) {
#pragma unroll
    for (int k = 0; k < 6; k++) sm[k] += cpart[(long)b * DIAG_NPART + k];
    mx[0] = fmax(mx[0], cpart[(long)b * DIAG_NPART + 6]);
    mx[1] = fmax(mx[1], cpart[(long)b * DIAG_NPART + 7]);
  }
  for (int b = threadIdx.x; b < neb; b += blockDim.x) sm[6] += epart[2 * (long)b];
  __shared__ double red[16][9];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const double v = wave_sum(sm[k]);
    if (lane == 0) red[wv][k] = v;
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const double v = wave_max(mx[k]);
    if (lane == 0) red[wv][7 + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < DIAG_NACC) {
    const int k = threadIdx.x;
    double v = red[0][k];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) v = k < 7 ? v + red[w][k] : fmax(v, red[w][k]);
    acc[k] = v;
  }
}

// the nine columns from the (rank-summed) sums acc[0..6] and the maxima of every rank, mxs[r * 2 + 0..1]
__global__ void k_diag_row(const double* __restrict__ acc, const double* __restrict__ mxs, int nranks, double dt, int tracer,
                           double* __restrict__ row) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double m0 = 0.0, m1 = 0.0;
  for (int r = 0; r < nranks; r++) { m0 = fmax(m0, mxs[2 * r]); m1 = fmax(m1, mxs[2 * r + 1]); }
  const double nan = __builtin_nan("");
  row[0] = acc[0];
  row[1] = acc[1];
  row[2] = sqrt(acc[2]);
  row[3] = sqrt(acc[6]);
  row[4] = acc[3];
  row[5] = tracer ? acc[4] : nan;
  row[6] = tracer ? acc[5] : nan;
  row[7] = m0;
  row[8] = dt * m1;
}

}  // namespace hdg
