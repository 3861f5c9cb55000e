// Coriolis term: out (+)= M^-1 C u,  C(w, u) = sum_K int_K f_c (w_x u_y - w_y u_x),  f_c = f0 + beta y,
// the rotation  - f_c k x u = (f_c u_y, - f_c u_x)  on [DG_{k+1}]^2 in the orthonormal modal basis.  The term is cell-local:
// no facet terms, no neighbour, no ghost rows.  f_c is linear, so a cell's block is (f_ref I + sum_v d_v L_v) (x) J with the
// reference tables L_v = int lambda_v phi_r phi_m (hdg_tables.hpp: CoriolisTables), f_ref = f_c at the cell's reference vertex,
// d_v the difference of f_c between vertex v and the reference vertex, J = [[0, 1], [-1, 0]].
//
// ACC = false writes the result, ACC = true adds it to what out holds (a slot k_viscosity has written): every thread reads
// and writes the rows of its own cell only, so accumulating in place needs no second vector.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

// Structured meshes: the thread <-> cell mapping, grid and block size of k_viscosity, component-pair layout (one 16-byte
// access per mode), owned rows only.  The reference vertex of shape s in global cell row gj lies at y = (gj + s) h and the
// block is (f_ref I + beta h Y_s) (x) J, Y_s transposed in tab (uniform over a workgroup: scalar loads).  The accumulator of
// both components stays live: it starts as the diagonal part J f_ref u_r (plus what out holds with ACC), built row by row so
// that at most one operand pair is in flight beside it, then u is streamed mode by mode as in k_viscosity (the mode loop is a
// loop, the row loop is unrolled: the accumulator is never indexed dynamically) and adds beta h Y_s J u; the second read of u
// comes from the cache.  f0, beta and h sit in scalar registers, so beta == 0 is a scalar branch around the table: a
// pointwise rotation by f0, one load and one store per mode.
template <int K, bool ACC>
__global__ __launch_bounds__(128) void k_coriolis(Geo g, const double* __restrict__ tab, double f0, double beta, double h,
                                                  const double* __restrict__ u, double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU;
  HDG_CELL_PROLOGUE
  const VelBuf U(u), O(out);
  const unsigned lane_b = (unsigned)c * 16u;
  const double fr = fma(beta, h * (double)(g.joff + j + s), f0);  // f_c at the reference vertex
  hdg_d2 F[NU];
#pragma unroll
  for (int r = 0; r < NU; r++) {
    if (ACC) {
      F[r] = O.ld(pair_bytes(r, g.Nc), lane_b);
      __builtin_amdgcn_sched_barrier(0);
    }
    const hdg_d2 x = U.ld(pair_bytes(r, g.Nc), lane_b);
    F[r] = ACC ? hdg_d2{fma(fr, x.y, F[r].x), fma(-fr, x.x, F[r].y)} : hdg_d2{fr * x.y, -fr * x.x};  // J w = (w.y, -w.x)
    __builtin_amdgcn_sched_barrier(0);
  }
  if (beta != 0.0) {
    const double* __restrict__ Y = tab + (long)s * NU * NU;
    const double bh = beta * h;
#pragma unroll 1
    for (int m = 0; m < NU; m++) {
      const hdg_d2 x = U.ld(pair_bytes(m, g.Nc), lane_b);
      const hdg_d2 jx{bh * x.y, -bh * x.x};
      const double* __restrict__ col = Y + m * NU;
#pragma unroll
      for (int r = 0; r < NU; r++) {
        const double a = col[r];
        F[r].x = fma(a, jx.x, F[r].x);
        F[r].y = fma(a, jx.y, F[r].y);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NU; r++) O.st(pair_bytes(r, g.Nc), lane_b, F[r]);
}

// General meshes, cell-major layout (c * 2NU + d * NU + m), one thread per cell.  yv: the ordinates of the cell's three
// vertices (nc x 3); tab: L_1 then L_2, row-major (symmetric, so a row serves as the column of mode m).  The basis of
// hdg_general.hpp is Dub / sqrt(detJ), orthonormal on the cell like the structured one: the tables apply as they are.
template <int K, bool ACC>
__global__ __launch_bounds__(64) void k_g_coriolis(int nc, const double* __restrict__ tab, const double* __restrict__ yv,
                                                   double f0, double beta, const double* __restrict__ u,
                                                   double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const double y0 = yv[3 * (long)c], fr = fma(beta, y0, f0);
  const double d1 = beta * (yv[3 * (long)c + 1] - y0), d2 = beta * (yv[3 * (long)c + 2] - y0);
  const double* __restrict__ uc = u + (long)c * 2 * NU;
  double* __restrict__ oc = out + (long)c * 2 * NU;
  double Fx[NU], Fy[NU];
#pragma unroll
  for (int r = 0; r < NU; r++) {
    Fx[r] = (ACC ? oc[r] : 0.0) + fr * uc[NU + r];
    Fy[r] = (ACC ? oc[NU + r] : 0.0) - fr * uc[r];
  }
  if (beta != 0.0) {
#pragma unroll 1
    for (int m = 0; m < NU; m++) {
      const double jx = uc[NU + m], jy = -uc[m];
      const double* __restrict__ c1 = tab + m * NU;
      const double* __restrict__ c2 = tab + NU * NU + m * NU;
#pragma unroll
      for (int r = 0; r < NU; r++) {
        const double a = fma(d1, c1[r], d2 * c2[r]);
        Fx[r] = fma(a, jx, Fx[r]);
        Fy[r] = fma(a, jy, Fy[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NU; r++) {
    oc[r] = Fx[r];
    oc[NU + r] = Fy[r];
  }
}

}  // namespace hdg
