// The advective rate A = max_K (max nodal |u| in K) / h_K of a velocity (hdg_get_step_rates): the CFL
// number of the diagnostics row without its factor dt, from one pass over the velocity that produces one double.
//
// cell_max_speed is the per-cell piece of the diagnostics' columns 7 and 8 (modal -> nodal values, largest nodal speed); the
// diagnostics cell passes (hdg_diagnostics.hpp) and the two kernels here call the one function.  The diagnostics take their
// maxima with fmax, which drops a NaN; the rate must not, so the function takes the maximum as a policy.
//
// Reduction: a non-negative double orders like its bit pattern read as an unsigned 64-bit integer, and every NaN pattern sorts
// above +inf, so the maximum of the patterns is the maximum of the values and a non-finite speed anywhere survives to the end.
// Cross-lane maximum per wave, one value per workgroup through LDS, stored to the workgroup's own slot; k_step_rate_reduce, one
// workgroup, takes the maximum of the slots into the one device word, as k_diag_reduce does for the diagnostics.  Two launches,
// no atomic, no host synchronisation but the caller's 8-byte read.  (One atomic maximum per workgroup on the word itself was
// measured at C3 size: the 16 384 reads and atomics on one address cost 29 of 112 us, profiles/adaptive_dt_cost.txt.)
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

constexpr int STEP_RATE_BLOCK = 128;

// Largest nodal speed of one cell.  x: velocity coefficients (x components, then y components); Vu (NU x NU, row = node) times
// vsc: modal -> nodal, or Qn != null: the cell's nodal values Qn[2 n + d] as given.  KEEP_NAN = false: fmax, a NaN entry is
// passed over (the diagnostics row); true: a NaN entry makes the result NaN.
template <int K, bool KEEP_NAN>
__device__ __forceinline__ double cell_max_speed(const double (&x)[2 * Dim<K>::NU], const double* __restrict__ Vu, double vsc,
                                                 const double* __restrict__ Qn) {
  constexpr int NU = Dim<K>::NU;
  double s2 = 0.0;
#pragma unroll 1
  for (int n = 0; n < NU; n++) {
    double vx = 0.0, vy = 0.0;
    if (Qn) {
      vx = Qn[2 * n]; vy = Qn[2 * n + 1];
    } else {
#pragma unroll
      for (int m = 0; m < NU; m++) {  // the order of k_q_modal_to_nodal: the values hdg_get_field returns
        const double a = Vu[n * NU + m];
        vx = fma(a, x[m], vx);
        vy = fma(a, x[NU + m], vy);
      }
      vx *= vsc; vy *= vsc;
    }
    const double v2 = __dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy));  // no contraction: |u| as a host computes it
    if (KEEP_NAN) s2 = (v2 > s2 || v2 != v2) ? v2 : s2;  // once NaN, s2 stays NaN: both tests are false from then on
    else s2 = fmax(s2, v2);
  }
  return sqrt(s2);
}

// the cell of this thread in a cell_grid() launch: the index math of HDG_CELL_PROLOGUE without its early return, for kernels
// whose every thread has to reach a workgroup reduction
struct CellAt {
  int s, i, j;
  bool live;
};
__device__ __forceinline__ CellAt cell_at(const Geo& g) {
  const int xcd_ = blockIdx.x & 7, q_ = blockIdx.x >> 3;
  const int jj_ = q_ / (2 * g.nbx), rem_ = q_ - jj_ * 2 * g.nbx;
  CellAt a;
  a.s = rem_ / g.nbx;
  a.i = (rem_ - a.s * g.nbx) * blockDim.x + threadIdx.x;
  const int r_ = xcd_ * g.rows_xcd + jj_;
  a.j = launch_row(g, r_);
  a.live = jj_ < g.rows_xcd && r_ < g.wrows && a.i < g.nx;  // owned rows only: no ghost row, no padding row
  return a;
}

// maximum over the workgroup of v (>= +0, or not finite) into part[blockIdx.x] (blockDim.x <= STEP_RATE_BLOCK, a multiple of 64)
__device__ __forceinline__ void rate_block_max(double v, unsigned long long* __restrict__ part) {
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(b, off, 64);
    b = o > b ? o : b;
  }
  __shared__ unsigned long long red[STEP_RATE_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) b = red[w] > b ? red[w] : b;
    part[blockIdx.x] = b;
  }
}

// second stage, one workgroup of 1024 threads: the maximum of the n slots into out[0]
__global__ __launch_bounds__(1024) void k_step_rate_reduce(int n, const unsigned long long* __restrict__ part,
                                                           unsigned long long* __restrict__ out) {
  unsigned long long b = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) b = part[i] > b ? part[i] : b;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(b, off, 64);
    b = o > b ? o : b;
  }
  __shared__ unsigned long long red[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) b = red[w] > b ? red[w] : b;
    out[0] = b;
  }
}

// structured meshes: one thread per cell over the plane layouts (loads coalesced across cells), launched on cell_grid()
template <int K>
__global__ __launch_bounds__(STEP_RATE_BLOCK) void k_step_rate(Geo g, const double* __restrict__ Vu, const double* __restrict__ Q,
                                                                unsigned long long* __restrict__ part) {
  constexpr int NU = Dim<K>::NU;
  const CellAt a = cell_at(g);
  double r = 0.0;
  if (a.live) {
    double x[2 * NU];
    load_vel<NU>(Q, g.Nc, rowbase(g, a.s, a.j) + a.i, x);
    r = cell_max_speed<K, true>(x, Vu, 1.0, nullptr) / g.h;
  }
  rate_block_max(r, part);
}

// general meshes: one thread per cell, the cell-major layout and the per-cell scale of k_g_diag_cell
template <int K>
__global__ __launch_bounds__(STEP_RATE_BLOCK) void k_g_step_rate(int nc, const double* __restrict__ inv_sdet, const double* __restrict__ Vu,
                                                                  const double* __restrict__ hmin, const double* __restrict__ Q,
                                                                  unsigned long long* __restrict__ part) {
  constexpr int N2 = 2 * Dim<K>::NU;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  double r = 0.0;
  if (c < nc) {
    double x[N2];
#pragma unroll
    for (int n = 0; n < N2; n++) x[n] = Q[(long)c * N2 + n];
    r = cell_max_speed<K, true>(x, Vu, inv_sdet[c], nullptr) / hmin[c];
  }
  rate_block_max(r, part);
}

}  // namespace hdg
