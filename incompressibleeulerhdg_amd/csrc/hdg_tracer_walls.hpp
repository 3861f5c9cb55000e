// Wall flux of the tracers: Phi_{t,w} = kappa_t int_w ( dn q_t - eta_b (q_t - g_{t,w}) ) ds on a side w
// of the unit square where tracer t is held at g_{t,w}, 0 on a no-flux side; positive into the domain.  It is the diffusion form
// tested against chi = 1, so d/dt int q_t = sum_w Phi_{t,w} holds for the discrete operator at zero velocity.
//
// In the orthonormal modal basis the flux through the wall leg (s, e) of one cell is  kappa (g wone - wvec[s][e] . q_K),
// wone = eta_b h (TracerDiffusionTables: Wall^T coef(1) = - wvec, so the table of k_tracer_diff<., ., true> serves).
//
// k_tracer_wall_flux: one thread per wall leg-edge cell -- 2 (nx + ny) of them, a corner cell once per leg; gridDim.y = the four
// sides bottom, right, top, left, so the side and with it the shape and the leg are uniform over a workgroup and wvec arrives
// through scalar loads.  Every thread forms wvec . q_K of all nt tracers; a workgroup leaves one partial per tracer in
// part[(t * 4 + side) * gridDim.x + block].  k_tracer_wall_flux_finish (one workgroup) adds the partials of a (tracer, side) in
// block order and forms the flux.  No floating-point atomics, every sum in a fixed order: two calls give the same bits.
// Owned rows only (j = 0 .. ny - 1); a single rank (tracers are refused on strips).
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

#define HDG_WALL_FLUX_BLOCK 128
template <int K>
__global__ __launch_bounds__(HDG_WALL_FLUX_BLOCK) void k_tracer_wall_flux(Geo g, const double* __restrict__ wtab, int nt, long tstride,
                                                                           const double* __restrict__ q, double* __restrict__ part) {
  constexpr int NP = Dim<K>::NP, BL = NP * NP;
  const int side = blockIdx.y;                       // 0 bottom, 1 right, 2 top, 3 left
  const int s = (side == 1 || side == 2) ? 1 : 0;    // the shape whose leg lies on that side
  const int e = (side == 0 || side == 2) ? 0 : 2;    // horizontal / vertical leg
  const int len = e == 0 ? g.nx : g.ny;
  const int pos = blockIdx.x * HDG_WALL_FLUX_BLOCK + threadIdx.x;
  const bool live = pos < len;
  const int i = e == 0 ? pos : (side == 1 ? g.nx - 1 : 0);
  const int j = e == 2 ? pos : (side == 2 ? g.ny - 1 : 0);
  const long c = live ? rowbase(g, s, j) + i : rowbase(g, s, 0);  // a dead lane reads a valid cell and adds zero
  const double* __restrict__ wv = wtab + (long)s * (2 * BL + 2 * NP) + 2 * BL + (e == 0 ? 0 : NP);
  __shared__ double sm[HDG_WALL_FLUX_BLOCK / 64];
  for (int t = 0; t < nt; t++) {
    double qc[NP];
    load_cell<NP>(q + t * tstride, g.Nc, c, qc);
    double d = 0.0;
#pragma unroll
    for (int m = 0; m < NP; m++) d = fma(wv[m], qc[m], d);
    const double w = wave_sum(live ? d : 0.0);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0.0;
      for (int v = 0; v < HDG_WALL_FLUX_BLOCK / 64; v++) a += sm[v];
      part[((long)t * 4 + side) * gridDim.x + blockIdx.x] = a;
    }
    __syncthreads();
  }
}

// flux[t * 4 + w] = kind ? kappa_t (g wone cells_w - sum of the partials) : 0; one workgroup, thread t * 4 + w
__global__ void k_tracer_wall_flux_finish(int nt, int nblk, int nx, int ny, double wone, const double* __restrict__ kappa,
                                          const int* __restrict__ wkind, const double* __restrict__ wval,
                                          const double* __restrict__ part, double* __restrict__ flux) {
  const int n = threadIdx.x;
  if (n >= nt * 4) return;
  const int side = n & 3;
  const int len = (side == 0 || side == 2) ? nx : ny;
  const int used = (len + HDG_WALL_FLUX_BLOCK - 1) / HDG_WALL_FLUX_BLOCK;  // the blocks of this side that hold cells
  double a = 0.0;
  for (int b = 0; b < used && b < nblk; b++) a += part[(long)n * nblk + b];
  flux[n] = wkind[n] != 0 ? kappa[n >> 2] * (wval[n] * wone * len - a) : 0.0;
}

}  // namespace hdg
