// Boussinesq buoyancy: the tracers force the flow,  B(q) = sum_t beta_t q_t g  in the velocity space.
//
// The device bases are hierarchical (orthonormal Dubiner modes ordered by total degree, the same scaling in every space), so
// the tracer space DG_k IS the span of the first NP modes of each velocity component's DG_{k+1}: the embedding is the
// identity on modes 0 .. NP-1 and zero on modes NP .. NU-1.  The kernels below therefore only form a_m = sum_t beta_t q_t[m]
// and write (g_x a_m, g_y a_m) into mode m of the force vector; the modes NP .. NU-1 of that vector are zeroed once when it
// is allocated and never written.  beta (HDG_MAX_TRACERS doubles, zero beyond the engine's tracer count) and g are kernel
// arguments passed by value: they sit in scalar registers, the test beta_t != 0 is a scalar branch, and a tracer with
// beta_t = 0 is not read.  The sum runs over t in ascending order, one fma per tracer and mode.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

struct BuoyCoef {
  double beta[HDG_MAX_TRACERS];
  double gx, gy;
};

// Structured meshes: thread <-> cell mapping, grid and block size of k_tracer_adv (one thread per owned cell); q holds the
// tracers tracer-major (tracer t starts at t * tstride), f is a velocity vector in the component-pair layout: one 16-byte
// store per mode.  Owned rows only: a consumer that reads f across rows (the pressure-reconstruction right-hand side) fills
// the ghost rows of what it reads itself (Engine::precon_rhs).
template <int K>
__global__ __launch_bounds__(128) void k_buoyancy(Geo g, BuoyCoef B, long tstride, const double* __restrict__ q,
                                                  double* __restrict__ f) {
  constexpr int NP = Dim<K>::NP;
  HDG_CELL_PROLOGUE
  double a[NP];
#pragma unroll
  for (int m = 0; m < NP; m++) a[m] = 0.0;
#pragma unroll
  for (int t = 0; t < HDG_MAX_TRACERS; t++) {
    if (B.beta[t] == 0.0) continue;
    double qc[NP];
    load_cell<NP>(q + t * tstride, g.Nc, c, qc);
#pragma unroll
    for (int m = 0; m < NP; m++) a[m] = fma(B.beta[t], qc[m], a[m]);
  }
  const VelBuf F(f);
  const unsigned lane_b = (unsigned)c * 16u;
#pragma unroll
  for (int m = 0; m < NP; m++) F.st(pair_bytes(m, g.Nc), lane_b, hdg_d2{B.gx * a[m], B.gy * a[m]});
}

// General meshes, cell-major layouts: tracer (c * NP + m), velocity (c * 2NU + d * NU + m).  The same arithmetic.
template <int K>
__global__ __launch_bounds__(64) void k_g_buoyancy(int nc, BuoyCoef B, long tstride, const double* __restrict__ q,
                                                   double* __restrict__ f) {
  constexpr int NU = Dim<K>::NU, NP = Dim<K>::NP;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double a[NP];
#pragma unroll
  for (int m = 0; m < NP; m++) a[m] = 0.0;
#pragma unroll
  for (int t = 0; t < HDG_MAX_TRACERS; t++) {
    if (B.beta[t] == 0.0) continue;
#pragma unroll
    for (int m = 0; m < NP; m++) a[m] = fma(B.beta[t], q[t * tstride + (long)c * NP + m], a[m]);
  }
#pragma unroll
  for (int m = 0; m < NP; m++) {
    f[(long)c * 2 * NU + m] = B.gx * a[m];
    f[(long)c * 2 * NU + NU + m] = B.gy * a[m];
  }
}

}  // namespace hdg
