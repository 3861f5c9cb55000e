// Implicit tracer diffusion: per tracer with tau_t = dt kappa_t != 0 the backward-Euler system
//   A_t x = (I - tau_t M^-1 D_w) x = b_t = q~_t + tau_t l_w
// in the orthonormal modal basis (mass = identity, A_t symmetric positive definite, spectrum in [1, 1 + tau_t rho]), solved by
// conjugate gradients for all tracers together with every scalar on the device.
//
// The recurrences are those of CG written with ONE reduction point per iteration (Chronopoulos & Gear 1989): the operator is
// applied to the residual, w = A r, and  y = A p  follows the direction by its own recurrence, so that a single scalar kernel
// sits between the operator pass and the one fused update pass:
//   k_tracer_helm     w = r - tau D_w r, partial sums of (r, w)                                 [thread <-> cell, TB tracers]
//   k_tdi_scalars     rr = (r, r) from the last update, beta = rr / rr_old, alpha = rr / ((r, w) - beta rr / alpha_old), flags
//   k_tdi_update      p = r + beta p, y = w + beta y, x += alpha p, r -= alpha y, partial sums of the new (r, r)
// Start: x_0 = q~ (the transported tracer; it is b wherever no wall is fixed), r_0 = b - A x_0 = tau (D_w q~ + l_w), formed with
// (b, b) by the INIT form of the operator kernel.  Stop: (r, r) <= rtol^2 (b, b), per tracer.
//
// Per tracer t the device keeps eight doubles sc[8 t + ..]: 0 rr, 1 alpha, 2 beta, 3 (b, b), 4 iterations, 5 state, 6 |r| / |b|
// (hdg_tracer_implicit_host.hpp).
// state: 0 iterating, 1 converged, 2 out of iterations, 3 broke down (a NaN or a non-positive curvature), 4 not part of the solve
// (tau_t = 0).  A tracer whose state is not 0 is frozen: no kernel reads or writes a vector entry of it.  Per tracer the
// floating-point operations and their order depend neither on TB nor on the other tracers: a thread's sums run over its own
// cell's modes in index order, a workgroup's over its waves in index order, the scalar kernel's over the workgroups in a fixed
// pattern, and the launch geometry is that of the mesh.
#pragma once
#include "hdg_cg.hpp"
#include "hdg_tracer_implicit_host.hpp"

namespace hdg {

// HDG_CELL_PROLOGUE for a kernel that ends in a workgroup reduction: a thread without a cell stays (live = false)
#define HDG_TDI_CELL_PROLOGUE                                      \
  const int xcd_ = blockIdx.x & 7, q_ = blockIdx.x >> 3;           \
  const int jj_ = q_ / (2 * g.nbx), rem_ = q_ - jj_ * 2 * g.nbx;   \
  const int s = rem_ / g.nbx;                                      \
  const int i_ = (rem_ - s * g.nbx) * blockDim.x + threadIdx.x;    \
  const int r_ = xcd_ * g.rows_xcd + jj_;                          \
  const bool live = jj_ < g.rows_xcd && r_ < g.wrows && i_ < g.nx; \
  const int i = live ? i_ : 0;                                     \
  const int j = live ? launch_row(g, r_) : 0;                      \
  const long c = rowbase(g, s, j) + i;

// sum of v over the workgroup (64 or 128 threads), in thread 0: waves in index order
__device__ __forceinline__ double tdi_block_sum(double v, double* sm) {
  const double w = wave_sum(v);
  __syncthreads();  // sm may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
  __syncthreads();
  double t = sm[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); k++) t += sm[k];
  return t;
}

// The operator pass.  Thread <-> cell map, tracer blocks (gridDim.y), TB and the short last block are k_tracer_diff's, and so are
// the tables: Vol / Own / Nbr (and the wall blocks of section 23) through scalar loads, the accumulation order per tracer.
// tau_t[t]: a small device array (the engine: dt kappa_t, written once per solve; the test hook: the numbers it was given).
//   INIT = false:  out_t = in_t - tau_t (D + D_w) in_t,  part0[t][block] = sum in_t . out_t                       (w = A r)
//   INIT = true:   out_t = tau_t ((D + D_w) in_t + l_w),  x_t = in_t,  part0 = sum out_t . out_t,  part1 = sum b_t . b_t,
//                  b_t = in_t + tau_t l_w                                                                           (r_0, x_0)
// in has its ghost rows filled on the periodic square (Engine::halo_rows).  A tracer whose state is not 0 is skipped.
// K = 3 with one tracer: the register allocator is told 5 waves per SIMD, the occupancy it reaches anyway.  Left to itself it
// reserves a 20-byte private segment in some of these instantiations (spill bookkeeping of the scalar table operands that it
// parks in vector lanes; no instruction touches it), and with it every launch would set up scratch memory.
template <int K, int TB, bool WALLS, bool INIT>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, (K == 3 && TB == 1) ? 5 : 8))) void k_tracer_helm(Geo g, const double* __restrict__ tab, const double* __restrict__ tau_t,
                                                      const double* __restrict__ sc, int nt, long tstride, const double* __restrict__ in,
                                                      double* __restrict__ out, double* __restrict__ x, double* __restrict__ part0,
                                                      double* __restrict__ part1, const double* __restrict__ wtab,
                                                      const int* __restrict__ wkind, const double* __restrict__ wval) {
  constexpr int NP = Dim<K>::NP, BL = NP * NP;
  __shared__ double sm[2];
  HDG_TDI_CELL_PROLOGUE
  const int t0 = blockIdx.y * TB;
  const int nb = nt - t0 < TB ? nt - t0 : TB;
  bool act[TB];  // uniform over the workgroup
  bool any = false;
#pragma unroll
  for (int b = 0; b < TB; b++) {
    act[b] = b < nb && sc[(t0 + b) * TDI_NSC + TDI_STATE] == (double)TDI_ITERATING;
    any = any || act[b];
  }
  if (!any) return;
  const double* __restrict__ T = tab + (long)s * 7 * BL;
  double qc[TB][NP], F[TB][NP], L[INIT && WALLS ? TB : 1][NP];
#pragma unroll
  for (int b = 0; b < TB; b++) {
    if (act[b] && live) load_cell<NP>(in + (t0 + b) * tstride, g.Nc, c, qc[b]);
#pragma unroll
    for (int r = 0; r < NP; r++) { F[b][r] = 0.0; if (!(act[b] && live)) qc[b][r] = 0.0; }
  }
#pragma unroll
  for (int b = 0; b < (INIT && WALLS ? TB : 1); b++)
#pragma unroll
    for (int r = 0; r < NP; r++) L[b][r] = 0.0;
  auto apply = [&](const double* __restrict__ A, const double (&v)[TB][NP]) {
#pragma unroll
    for (int r = 0; r < NP; r++)
#pragma unroll
      for (int m = 0; m < NP; m++) {
        const double a = A[r * NP + m];
#pragma unroll
        for (int b = 0; b < TB; b++) F[b][r] = fma(a, v[b][m], F[b][r]);
      }
  };
  apply(T, qc);
#pragma unroll
  for (int e = 0; e < 3; e++) {
    long cn;
    const bool has = nbr(s, e, i, j, g, cn) && live;
    if (__builtin_amdgcn_ballot_w64(has) != 0) {
      if (!has) cn = c;  // a valid address; the operand is zero
      double qn[TB][NP];
#pragma unroll
      for (int b = 0; b < TB; b++) {
        if (act[b] && has) load_cell<NP>(in + (t0 + b) * tstride, g.Nc, cn, qn[b]);
        else {
#pragma unroll
          for (int r = 0; r < NP; r++) qn[b][r] = 0.0;
        }
      }
      if (has) {
        apply(T + (1 + e) * BL, qc);
        apply(T + (4 + e) * BL, qn);
      }
    }
    if constexpr (WALLS) {
      const bool wall = !has && live;
      if (e != 1 && __builtin_amdgcn_ballot_w64(wall) != 0) {  // uniform over the wave
        const int side = s == 0 ? (e == 0 ? 0 : 3) : (e == 0 ? 2 : 1);
        const double* __restrict__ W = wtab + (long)s * (2 * BL + 2 * NP) + (e == 0 ? 0 : BL);
        const double* __restrict__ wv = wtab + (long)s * (2 * BL + 2 * NP) + 2 * BL + (e == 0 ? 0 : NP);
        bool on[TB];
        double gv[TB];
#pragma unroll
        for (int b = 0; b < TB; b++) {
          const bool fixed = act[b] && wkind[(t0 + b) * 4 + side] != 0;  // uniform over the workgroup
          double gb = 0.0;
          if constexpr (INIT) gb = fixed ? wval[(t0 + b) * 4 + side] : 0.0;
          on[b] = wall && fixed;
          gv[b] = wall ? gb : 0.0;
        }
#pragma unroll
        for (int m = 0; m < NP; m++) {
          double v[TB];
#pragma unroll
          for (int b = 0; b < TB; b++) v[b] = on[b] ? qc[b][m] : 0.0;
#pragma unroll
          for (int r = 0; r < NP; r++) {
            const double a = W[r * NP + m];
#pragma unroll
            for (int b = 0; b < TB; b++) F[b][r] = fma(a, v[b], F[b][r]);
          }
        }
        if constexpr (INIT) {  // the load l_w, kept apart from the operator: b needs it alone
#pragma unroll
          for (int r = 0; r < NP; r++) {
            const double a = wv[r];
#pragma unroll
            for (int b = 0; b < TB; b++) L[b][r] = fma(a, gv[b], L[b][r]);
          }
        }
      }
    }
  }
  const long blk = blockIdx.x;
#pragma unroll
  for (int b = 0; b < TB; b++) {
    if (!act[b]) continue;  // uniform over the workgroup
    const int t = t0 + b;
    const double tau = tau_t[t];
    double o[NP], s0 = 0.0, s1 = 0.0;
    if constexpr (INIT) {
#pragma unroll
      for (int r = 0; r < NP; r++) {
        double load = 0.0;
        if constexpr (WALLS) load = L[b][r];
        o[r] = tau * (F[b][r] + load);
        const double bv = fma(tau, load, qc[b][r]);
        s0 = fma(o[r], o[r], s0);
        s1 = fma(bv, bv, s1);
      }
      if (live) store_cell<NP>(x + t * tstride, g.Nc, c, qc[b]);
    } else {
#pragma unroll
      for (int r = 0; r < NP; r++) {
        o[r] = fma(-tau, F[b][r], qc[b][r]);
        s0 = fma(qc[b][r], o[r], s0);
      }
    }
    if (live) store_cell<NP>(out + t * tstride, g.Nc, c, o);
    const double v0 = tdi_block_sum(live ? s0 : 0.0, sm);
    if (threadIdx.x == 0) part0[(long)t * gridDim.x + blk] = v0;
    if constexpr (INIT) {
      const double v1 = tdi_block_sum(live ? s1 : 0.0, sm);
      if (threadIdx.x == 0) part1[(long)t * gridDim.x + blk] = v1;
    }
  }
}

// The fused update of one iteration, one tracer per blockIdx.y, thread <-> cell: every entry of p, y, x, r is read once and
// written once, w is read once.  beta = 0 (the first iteration of a solve): p and y are written, not read.
template <int K>
__global__ __launch_bounds__(128) void k_tdi_update(Geo g, const double* __restrict__ sc, long tstride, const double* __restrict__ w,
                                                     double* __restrict__ p, double* __restrict__ y, double* __restrict__ x,
                                                     double* __restrict__ r, double* __restrict__ part) {
  constexpr int NP = Dim<K>::NP;
  __shared__ double sm[2];
  HDG_TDI_CELL_PROLOGUE
  const int t = blockIdx.y;
  const double* __restrict__ st = sc + t * TDI_NSC;
  if (st[TDI_STATE] != (double)TDI_ITERATING) return;  // uniform over the workgroup
  const double alpha = st[TDI_ALPHA], beta = st[TDI_BETA];
  const long off = t * tstride;
  double s0 = 0.0;
  if (live) {
    double rv[NP], wv[NP], pv[NP], yv[NP], xv[NP];
    load_cell<NP>(r + off, g.Nc, c, rv);
    load_cell<NP>(w + off, g.Nc, c, wv);
    load_cell<NP>(x + off, g.Nc, c, xv);
    if (beta != 0.0) {
      load_cell<NP>(p + off, g.Nc, c, pv);
      load_cell<NP>(y + off, g.Nc, c, yv);
#pragma unroll
      for (int n = 0; n < NP; n++) { pv[n] = fma(beta, pv[n], rv[n]); yv[n] = fma(beta, yv[n], wv[n]); }
    } else {
#pragma unroll
      for (int n = 0; n < NP; n++) { pv[n] = rv[n]; yv[n] = wv[n]; }
    }
#pragma unroll
    for (int n = 0; n < NP; n++) {
      xv[n] = fma(alpha, pv[n], xv[n]);
      rv[n] = fma(-alpha, yv[n], rv[n]);
      s0 = fma(rv[n], rv[n], s0);
    }
    store_cell<NP>(p + off, g.Nc, c, pv);
    store_cell<NP>(y + off, g.Nc, c, yv);
    store_cell<NP>(x + off, g.Nc, c, xv);
    store_cell<NP>(r + off, g.Nc, c, rv);
  }
  const double v0 = tdi_block_sum(s0, sm);
  if (threadIdx.x == 0) part[(long)t * gridDim.x + blockIdx.x] = v0;
}

// One workgroup of 256: wave v finishes the sums of tracers v, v + 4, ... (lane l adds the workgroups l, l + 64, ... in order,
// then the wave sum) and applies the rule; thread 0 then counts the tracers still iterating into the host's flag word.
#define HDG_TDI_SC_BLOCK 256
__global__ __launch_bounds__(HDG_TDI_SC_BLOCK) void k_tdi_scalars(int nt, int nblk, int first, int last, double rtol2,
                                                                 const double* __restrict__ part_rr, const double* __restrict__ part_rw,
                                                                 const double* __restrict__ part_bb, double* sc, double* hflag) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wv; t < nt; t += HDG_TDI_SC_BLOCK / 64) {
    double* st = sc + t * TDI_NSC;
    if (st[TDI_STATE] != (double)TDI_ITERATING) continue;  // uniform over the wave
    double a = 0.0, b = 0.0, d = 0.0;
    for (int k = lane; k < nblk; k += 64) {
      a += part_rr[(long)t * nblk + k];
      if (!last) b += part_rw[(long)t * nblk + k];
      if (first) d += part_bb[(long)t * nblk + k];
    }
    a = wave_sum(a); b = wave_sum(b); d = wave_sum(d);
    if (lane == 0) tdi_scalar_rule(st, a, b, d, first != 0, last != 0, rtol2);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int open = 0;
    for (int t = 0; t < nt; t++) open += sc[t * TDI_NSC + TDI_STATE] == (double)TDI_ITERATING;
    hflag[0] = (double)open;
  }
}

// the end of a solve: a converged tracer takes its solution, every other tracer keeps the transported values
template <int K>
__global__ __launch_bounds__(128) void k_tdi_accept(Geo g, const double* __restrict__ sc, long tstride, const double* __restrict__ x,
                                                     double* __restrict__ q) {
  constexpr int NP = Dim<K>::NP;
  HDG_CELL_PROLOGUE
  const int t = blockIdx.y;
  if (sc[t * TDI_NSC + TDI_STATE] != (double)TDI_CONVERGED) return;
  double v[NP];
  load_cell<NP>(x + t * tstride, g.Nc, c, v);
  store_cell<NP>(q + t * tstride, g.Nc, c, v);
}

}  // namespace hdg
