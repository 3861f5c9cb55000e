// Linear drag and volume penalisation: out (+)= sgn M^-1 D u (+ load),  D(w, u) = sum_K int_K sigma w.u,
// sigma >= 0 linear on every cell (three vertex values, broken across cells) on [DG_{k+1}]^2 in the orthonormal modal basis.
// The term is cell-local: no facet terms, no neighbour, no ghost rows.  A cell's block is
//   (sigma_0 I + (sigma_1 - sigma_0) L_1 + (sigma_2 - sigma_0) L_2) (x) I_2
// with the reference tables L_v = int lambda_v phi_r phi_m (hdg_tables.hpp: CoriolisTables::general(): L_1 then L_2; both
// symmetric, so a row serves as the column of mode m).  What differs from k_coriolis: the three coefficients change from cell
// to cell and are read per lane, and the block acts on both components alike.
//
// The step path calls with sgn = -1 and load = M^-1 D u_s (LOAD; without it u_s = 0), which gives - M^-1 D (u - u_s): the slot
// stays affine in u.  LOAD is a template flag, not a test of the pointer: a branch inside the unrolled row loop splits it into
// basic blocks, the scheduling barriers no longer hold the loads back and the kernel needs 88 instead of 54 VGPRs at k = 2.
// The load itself is built once per setting by the same kernel with sgn = +1 and no load.
// ACC = false writes the result, ACC = true adds it to what out holds (a slot k_viscosity or k_coriolis has written): every
// thread reads and writes the rows of its own cell only, so accumulating in place needs no second vector.  No LDS, no scratch
// in the apply kernels; the force kernels use LDS for their workgroup sums only.
#pragma once
#include <hip/hip_runtime.h>

#include "hdg_step_rate.hpp"

namespace hdg {

#define HDG_DRAG_FORCE_NVAL 12  // 4 regions x (F_x, F_y, P)

// Structured meshes, the per-cell block code of k_drag and k_drag_force: F = (ACC: out) + (load) + sgn B u of cell c.
// coef: three planes of Nc doubles in the kernels' own cell order (hdg_drag_host.hpp: drag_pack_planes), so a lane's three
// 8-byte loads are coalesced across the wave.  The accumulator of both components stays live: it starts as the diagonal part
// sgn sigma_0 u_r (plus what out and load hold), built row by row so that few operand pairs are in flight beside it, then u is
// streamed mode by mode as in k_coriolis (the mode loop is a loop, the row loop is unrolled: the accumulator is never indexed
// dynamically) and adds sgn (d_1 L_1 + d_2 L_2) u; the second read of u comes from the cache.  tab is uniform over the
// workgroup: scalar loads.  A wave none of whose cells has a gradient of sigma (uniform friction, the inside of a mask, the
// cells outside it) takes a scalar branch around the table.
template <int K, bool ACC, bool LOAD>
__device__ __forceinline__ void drag_cell(const Geo& g, long c, const double* __restrict__ tab, const double* __restrict__ coef,
                                          double sgn, const VelBuf& U, const double* __restrict__ load, const VelBuf& O,
                                          hdg_d2 (&F)[Dim<K>::NU]) {
  constexpr int NU = Dim<K>::NU;
  const CellBuf Cf(coef);
  const unsigned lane_c = (unsigned)c * 8u, lane_b = (unsigned)c * 16u;
  const double s0 = sgn * Cf.ld(plane_bytes(0, g.Nc), lane_c);
  const double d1 = sgn * Cf.ld(plane_bytes(1, g.Nc), lane_c);
  const double d2 = sgn * Cf.ld(plane_bytes(2, g.Nc), lane_c);
  const VelBuf Ld(load);
#pragma unroll
  for (int r = 0; r < NU; r++) {
    F[r] = hdg_d2{0.0, 0.0};
    if (ACC) {
      F[r] = O.ld(pair_bytes(r, g.Nc), lane_b);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (LOAD) {
      const hdg_d2 l = Ld.ld(pair_bytes(r, g.Nc), lane_b);
      F[r] += l;
      __builtin_amdgcn_sched_barrier(0);
    }
    const hdg_d2 x = U.ld(pair_bytes(r, g.Nc), lane_b);
    F[r] = hdg_d2{fma(s0, x.x, F[r].x), fma(s0, x.y, F[r].y)};
    __builtin_amdgcn_sched_barrier(0);
  }
  if (__builtin_amdgcn_ballot_w64(d1 != 0.0 || d2 != 0.0) != 0) {
#pragma unroll 1
    for (int m = 0; m < NU; m++) {
      const hdg_d2 x = U.ld(pair_bytes(m, g.Nc), lane_b);
#pragma unroll
      for (int v = 0; v < 2; v++) {  // one vertex after the other: one scaled pair live beside the accumulator
        const double d = v == 0 ? d1 : d2;
        const hdg_d2 y{d * x.x, d * x.y};
        const double* __restrict__ col = tab + v * NU * NU + m * NU;
#pragma unroll
        for (int r = 0; r < NU; r++) {
          const double a = col[r];
          F[r].x = fma(a, y.x, F[r].x);
          F[r].y = fma(a, y.y, F[r].y);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// the thread <-> cell mapping, grid and block size of k_coriolis, component-pair layout (one 16-byte access per mode), owned
// rows only
template <int K, bool ACC, bool LOAD>
__global__ __launch_bounds__(128) void k_drag(Geo g, const double* __restrict__ tab, const double* __restrict__ coef, double sgn,
                                              const double* __restrict__ u, const double* __restrict__ load,
                                              double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU;
  HDG_CELL_PROLOGUE
  const VelBuf U(u), O(out);
  hdg_d2 F[NU];
  drag_cell<K, ACC, LOAD>(g, c, tab, coef, sgn, U, load, O, F);
  const unsigned lane_b = (unsigned)c * 16u;
#pragma unroll
  for (int r = 0; r < NU; r++) O.st(pair_bytes(r, g.Nc), lane_b, F[r]);
}

// General meshes, cell-major layout (c * 2NU + d * NU + m), one thread per cell: the per-cell block code of k_g_drag and
// k_g_drag_force.  coef: (sigma_0, sigma_1 - sigma_0, sigma_2 - sigma_0) per cell, nc x 3.  The basis of hdg_general.hpp is
// orthonormal on the cell like the structured one: the tables apply as they are.
template <int K, bool ACC, bool LOAD>
__device__ __forceinline__ void drag_cell_general(long c, const double* __restrict__ tab, const double* __restrict__ coef, double sgn,
                                                  const double* __restrict__ u, const double* __restrict__ load,
                                                  const double* __restrict__ out, double (&Fx)[Dim<K>::NU], double (&Fy)[Dim<K>::NU]) {
  constexpr int NU = Dim<K>::NU;
  const double s0 = sgn * coef[3 * c], d1 = sgn * coef[3 * c + 1], d2 = sgn * coef[3 * c + 2];
  const double* __restrict__ uc = u + c * 2 * NU;
#pragma unroll
  for (int r = 0; r < NU; r++) {
    Fx[r] = (ACC ? out[c * 2 * NU + r] : 0.0) + (LOAD ? load[c * 2 * NU + r] : 0.0);
    Fy[r] = (ACC ? out[c * 2 * NU + NU + r] : 0.0) + (LOAD ? load[c * 2 * NU + NU + r] : 0.0);
    Fx[r] = fma(s0, uc[r], Fx[r]);
    Fy[r] = fma(s0, uc[NU + r], Fy[r]);
  }
  if (d1 != 0.0 || d2 != 0.0) {
#pragma unroll 1
    for (int m = 0; m < NU; m++) {
      const double x = uc[m], y = uc[NU + m];
      const double* __restrict__ c1 = tab + m * NU;
      const double* __restrict__ c2 = tab + NU * NU + m * NU;
#pragma unroll
      for (int r = 0; r < NU; r++) {
        const double a = fma(d1, c1[r], d2 * c2[r]);
        Fx[r] = fma(a, x, Fx[r]);
        Fy[r] = fma(a, y, Fy[r]);
      }
    }
  }
}

template <int K, bool ACC, bool LOAD>
__global__ __launch_bounds__(64) void k_g_drag(int nc, const double* __restrict__ tab, const double* __restrict__ coef, double sgn,
                                               const double* __restrict__ u, const double* __restrict__ load,
                                               double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU;
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double Fx[NU], Fy[NU];
  drag_cell_general<K, ACC, LOAD>(c, tab, coef, sgn, u, load, out, Fx, Fy);
  double* __restrict__ oc = out + c * 2 * NU;
#pragma unroll
  for (int r = 0; r < NU; r++) {
    oc[r] = Fx[r];
    oc[NU + r] = Fy[r];
  }
}

// ---- the force of the term (section 26): per region r of the cells,
//   (F_x, F_y) = - int sigma (u - u_s) dx,   P = - int sigma (u - u_s) . u dx.
// With R = - M^-1 D (u - u_s) of a cell (what the apply kernel writes) the force is int phi_0 = sqrt|K| times mode 0 of R, and
// the power is R . u (the basis is orthonormal).  Each workgroup leaves its 12 sums in part[block * 12 + 3 r + n]: lanes of other
// regions add zero, sums over the wave by shuffles and over the waves in wave order.  k_drag_force_finish (one workgroup of 256)
// adds the partials: thread t takes the blocks t, t + 256, ... in rising order, then the same wave and LDS sums.  No
// floating-point atomics, every sum in a fixed order: two calls give the same bits.
__device__ __forceinline__ void drag_force_store(int region, double fx, double fy, double pw, double* __restrict__ part) {
  __shared__ double sm[4][HDG_DRAG_FORCE_NVAL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const bool in = region == r;
    const double a = wave_sum(in ? fx : 0.0), b = wave_sum(in ? fy : 0.0), p = wave_sum(in ? pw : 0.0);
    if (lane == 0) { sm[wv][3 * r] = a; sm[wv][3 * r + 1] = b; sm[wv][3 * r + 2] = p; }
  }
  __syncthreads();
  if (threadIdx.x < HDG_DRAG_FORCE_NVAL) {
    double v = sm[0][threadIdx.x];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) v += sm[w][threadIdx.x];
    part[(long)blockIdx.x * HDG_DRAG_FORCE_NVAL + threadIdx.x] = v;
  }
}

// structured meshes, launched on cell_grid() like k_drag; every thread reaches the workgroup sums (cell_at), a dead lane reads
// a valid cell and adds zero.  region: the tags in the kernels' cell order.
template <int K, bool LOAD>
__global__ __launch_bounds__(128) void k_drag_force(Geo g, const double* __restrict__ tab, const double* __restrict__ coef,
                                                    const int* __restrict__ region, const double* __restrict__ u,
                                                    const double* __restrict__ load, double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU;
  const CellAt at = cell_at(g);
  const long c = at.live ? rowbase(g, at.s, at.j) + at.i : rowbase(g, 0, 0);
  const VelBuf U(u);
  hdg_d2 F[NU];
  drag_cell<K, false, LOAD>(g, c, tab, coef, -1.0, U, load, U, F);
  const unsigned lane_b = (unsigned)c * 16u;
  double pw = 0.0;
#pragma unroll
  for (int r = 0; r < NU; r++) {
    const hdg_d2 x = U.ld(pair_bytes(r, g.Nc), lane_b);
    pw = fma(F[r].x, x.x, fma(F[r].y, x.y, pw));
  }
  const double sqK = g.h * 0.70710678118654752440;
  const double lv = at.live ? 1.0 : 0.0;
  drag_force_store(region[c], lv * sqK * F[0].x, lv * sqK * F[0].y, lv * pw, part);
}

// general meshes: one thread per cell; detJ: |K| = detJ / 2
template <int K, bool LOAD>
__global__ __launch_bounds__(128) void k_g_drag_force(int nc, const double* __restrict__ detJ, const double* __restrict__ tab,
                                                      const double* __restrict__ coef, const int* __restrict__ region,
                                                      const double* __restrict__ u, const double* __restrict__ load,
                                                      double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU;
  const long c0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = c0 < nc;
  const long c = live ? c0 : 0;
  double Fx[NU], Fy[NU];
  drag_cell_general<K, false, LOAD>(c, tab, coef, -1.0, u, load, nullptr, Fx, Fy);
  double pw = 0.0;
#pragma unroll
  for (int r = 0; r < NU; r++) pw = fma(Fx[r], u[c * 2 * NU + r], fma(Fy[r], u[c * 2 * NU + NU + r], pw));
  const double sqK = sqrt(0.5 * detJ[c]), lv = live ? 1.0 : 0.0;
  drag_force_store(region[c], lv * sqK * Fx[0], lv * sqK * Fy[0], lv * pw, part);
}

// F[0 .. 11] = the sums of the nblk partials, in a fixed order
__global__ __launch_bounds__(256) void k_drag_force_finish(int nblk, const double* __restrict__ part, double* __restrict__ F) {
  double v[HDG_DRAG_FORCE_NVAL];
#pragma unroll
  for (int k = 0; k < HDG_DRAG_FORCE_NVAL; k++) v[k] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
#pragma unroll
    for (int k = 0; k < HDG_DRAG_FORCE_NVAL; k++) v[k] += part[(long)b * HDG_DRAG_FORCE_NVAL + k];
  }
  __shared__ double sm[4][HDG_DRAG_FORCE_NVAL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < HDG_DRAG_FORCE_NVAL; k++) {
    const double a = wave_sum(v[k]);
    if (lane == 0) sm[wv][k] = a;
  }
  __syncthreads();
  if (threadIdx.x < HDG_DRAG_FORCE_NVAL) F[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

}  // namespace hdg
