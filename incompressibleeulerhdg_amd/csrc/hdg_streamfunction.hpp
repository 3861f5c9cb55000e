// Stream function of the velocity in the continuous space CG_{k+1}: psi minimises |u - curl psi|_{L2}
// over the whole space, curl psi = (d_y psi, -d_x psi), no essential boundary condition:
//   (grad psi, grad tau) = int (u_x d_y tau - u_y d_x tau) dx   for all tau          (singular by constants, right-hand side sums to 0)
// solved by conjugate gradients on the stiffness matrix K, preconditioned by  z = r / diag(K) + P Acoarse^-1 P^T r  with one
// V-cycle of the P1 vertex grid (hdg_vertex_mg.hpp) for Acoarse^-1: the 5-point Laplacian of that grid IS P^T K P under the
// nested P1 interpolation P.  The idioms are those of hdg_cg.hpp: a cell computes its planes of cg_y and k_cg_gather sums per
// dof, a corner owns the dofs attached to it, no atomics, every sum in a fixed order (two calls give the same bits).
// The right-hand side is k_cg_cell<K, 4> (hdg_cg.hpp): MODE 3 without its boundary term.
#pragma once
#include "hdg_cg.hpp"
#include "hdg_step_rate.hpp"

namespace hdg {

// weights of the nested P1 interpolation at the nodes of CG_{k+1} (host: Engine::psi_setup, from the node coordinates)
struct PsiTabs {
  double et[4];          // parameter t of the p - 1 interior nodes of an edge: the value there is (1 - t) a + t b
  double plam[2][6][3];  // interior dof q of shape s: weights of the cell's vertex nodes (a = b = 0 | a = p | b = p of CgTabs::fwd)
  double vlam[6][6];     // CgTabs::vtx entry e, interior dof q of that cell: the weight of the vertex the entry stands for
};

// y = Kloc[shape] * (nodal values gathered from the continuous vector cg);  Kloc: 2 x NU x NU, the element stiffness matrices
// (no h in 2-D).  y: NU planes y[n*Nc + c]; k_cg_gather sums per dof.
template <int K>
__global__ __launch_bounds__(128) void k_psi_stiff(Geo g, CgTabs C, const double* __restrict__ Kloc, const double* __restrict__ cg,
                                                   double* __restrict__ y) {
  constexpr int NU = Dim<K>::NU;
  HDG_CELL_PROLOGUE
  double v[NU], o[NU];
#pragma unroll
  for (int n = 0; n < NU; n++) {
    const short* f = C.fwd[s][n];
    v[n] = cg[cg_dof(C, f[0], i + f[1], j + f[2], f[3], s)];
    o[n] = 0.0;
  }
  mv_acc<NU, NU>(Kloc + (long)s * NU * NU, v, o, 1.0);
#pragma unroll
  for (int n = 0; n < NU; n++) y[(long)n * g.Nc + c] = o[n];
}

// ---- CG_{k+1} <-> P1 vertex grid.  Vertex (i, j) of the grid is the vertex dof (i, j) of the continuous space (same index).
// Restriction, one thread per mesh vertex: rc_v = sum_n lambda_v(x_n) r_n over the vertex dof, the interior nodes of the six
// incident edges H(i,j), H(i-1,j), V(i,j), V(i,j-1), D(i-1,j), D(i,j-1) and the interior dofs of the six incident cells
// (CgTabs::vtx), each dof once, in this order.  Launched on the corner grid of every local row (g_all).
template <int K>
__global__ __launch_bounds__(128) void k_psi_restrict(Geo g, CgTabs C, PsiTabs T, const double* __restrict__ r, double* __restrict__ rc) {
  HDG_CORNER_PROLOGUE
  const bool per = C.per != 0;
  const bool xl = i > 0 || per, yl = j > 0 || per;
  const int im = i > 0 ? i - 1 : g.nx - 1, jm = j > 0 ? j - 1 : g.ny - 1;  // (used where xl / yl hold)
  double acc = r[cg_dof(C, 0, i, j, 0, 0)];
  for (int t = 0; t < C.p - 1; t++) {
    const double w = T.et[t], w1 = 1.0 - w;
    if (in_x) acc = fma(w1, r[cg_dof(C, 1, i, j, t, 0)], acc);
    if (xl) acc = fma(w, r[cg_dof(C, 1, im, j, t, 0)], acc);
    if (in_y) acc = fma(w1, r[cg_dof(C, 2, i, j, t, 0)], acc);
    if (yl) acc = fma(w, r[cg_dof(C, 2, i, jm, t, 0)], acc);
    if (xl && in_y) acc = fma(w1, r[cg_dof(C, 3, im, j, t, 0)], acc);  // D(i-1, j) starts at (i, j)
    if (in_x && yl) acc = fma(w, r[cg_dof(C, 3, i, jm, t, 0)], acc);   // D(i, j-1) ends at (i, j)
  }
  for (int e = 0; e < 6; e++) {
    const short* f = C.vtx[e];
    int ci = i + f[1], cj = j + f[2];
    if (per) { ci = ci < 0 ? ci + g.nx : ci; cj = cj < 0 ? cj + g.ny : cj; }
    if (ci < 0 || cj < 0 || ci >= g.nx || cj >= g.ny) continue;
    for (int q = 0; q < C.nint; q++) acc = fma(T.vlam[e][q], r[cg_dof(C, 4, ci, cj, q, f[0])], acc);
  }
  rc[(long)j * C.vs + i] = acc;
}

// Prolongation fused with the Jacobi term, one thread per grid corner (the dofs attached to it, as in k_cg_gather):
//   out = r / dg + P xc;   r == nullptr: out = P xc;   xc == nullptr: out = r / dg
template <int K>
__global__ __launch_bounds__(128) void k_psi_prolong(Geo g, CgTabs C, PsiTabs T, const double* __restrict__ xc, const double* __restrict__ r,
                                                     const double* __restrict__ dg, double* __restrict__ out) {
  HDG_CORNER_PROLOGUE
  auto xv = [&](int I, int J) -> double {
    if (!xc) return 0.0;
    if (C.per) { I = I >= g.nx ? I - g.nx : I; J = J >= g.ny ? J - g.ny : J; }
    return xc[(long)J * C.vs + I];
  };
  auto put = [&](long dof, double val) { out[dof] = r ? r[dof] / dg[dof] + val : val; };
  const double a = xv(i, j), b = in_x ? xv(i + 1, j) : 0.0, c = in_y ? xv(i, j + 1) : 0.0, d = in_x && in_y ? xv(i + 1, j + 1) : 0.0;
  put(cg_dof(C, 0, i, j, 0, 0), a);
  for (int t = 0; t < C.p - 1; t++) {
    const double w = T.et[t], w1 = 1.0 - w;
    if (in_x) put(cg_dof(C, 1, i, j, t, 0), fma(w1, a, w * b));
    if (in_y) put(cg_dof(C, 2, i, j, t, 0), fma(w1, a, w * c));
    if (in_x && in_y) put(cg_dof(C, 3, i, j, t, 0), fma(w1, b, w * c));  // D(i, j): from (i+1, j) to (i, j+1)
  }
  if (in_x && in_y) {
    for (int q = 0; q < C.nint; q++) {
      put(cg_dof(C, 4, i, j, q, 0), fma(T.plam[0][q][0], a, fma(T.plam[0][q][1], b, T.plam[0][q][2] * c)));  // L: (i,j), (i+1,j), (i,j+1)
      put(cg_dof(C, 4, i, j, q, 1), fma(T.plam[1][q][0], d, fma(T.plam[1][q][1], c, T.plam[1][q][2] * b)));  // U: (i+1,j+1), (i,j+1), (i+1,j)
    }
  }
}

// ---- reductions in a fixed order.  A workgroup leaves NV sums in part[block * NV + v]: over the wave by shuffles, over the waves
// in wave order.  k_psi_finish (one workgroup of 256) adds the partials: thread t takes the blocks t, t + 256, ... in rising order.
#define HDG_PSI_BLOCK 256
template <int NV>
__device__ __forceinline__ void psi_block_store(const double (&v)[NV], double* __restrict__ part) {
  __shared__ double sm[HDG_PSI_BLOCK / 64][NV];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const double s = wave_sum(v[q]);
    if (lane == 0) sm[wv][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = sm[0][threadIdx.x];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) t += sm[w][threadIdx.x];
    part[(long)blockIdx.x * NV + threadIdx.x] = t;
  }
}
template <int NV>
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_finish(int nb, const double* __restrict__ part, double* __restrict__ res) {
  double v[NV];
#pragma unroll
  for (int q = 0; q < NV; q++) v[q] = 0.0;
  for (int b = threadIdx.x; b < nb; b += HDG_PSI_BLOCK) {
#pragma unroll
    for (int q = 0; q < NV; q++) v[q] += part[(long)b * NV + q];
  }
  __shared__ double sm[HDG_PSI_BLOCK / 64][NV];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; q++) {
    const double s = wave_sum(v[q]);
    if (lane == 0) sm[wv][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = sm[0][threadIdx.x];
    for (int w = 1; w < HDG_PSI_BLOCK / 64; w++) t += sm[w][threadIdx.x];
    res[threadIdx.x] = t;
  }
}

// Component d of curl psi = (d_y psi, -d_x psi) as a broken modal velocity: per cell, gather the nodal psi and apply the nodal
// derivative table Dxy[shape][1 - d] (NU x NU, row = mode: the derivative blocks W of the vorticity times Vinv, combined on the
// host) with the sign of the component.  One table per launch, the shape of k_psi_stiff.
template <int K>
__global__ __launch_bounds__(128) void k_psi_curl(Geo g, CgTabs C, const double* __restrict__ Dxy, const double* __restrict__ psi, int d,
                                                  double* __restrict__ out) {
  constexpr int NU = Dim<K>::NU;
  HDG_CELL_PROLOGUE
  double v[NU], o[NU];
#pragma unroll
  for (int n = 0; n < NU; n++) {
    const short* f = C.fwd[s][n];
    v[n] = psi[cg_dof(C, f[0], i + f[1], j + f[2], f[3], s)];
    o[n] = 0.0;
  }
  mv_acc<NU, NU>(Dxy + (long)(2 * s + 1 - d) * NU * NU, v, o, d == 0 ? 1.0 : -1.0);
#pragma unroll
  for (int m = 0; m < NU; m++) out[vix<NU>(d * NU + m, g.Nc, c)] = o[m];
}
// Defect and mean flow, launched on cell_grid(): e = u - ubar - curl psi in the orthonormal modal basis (curl: k_psi_curl's
// output).  Workgroup sums:
//   part[4 b + 0, 1] = int u_x, int u_y;   part[4 b + 2] = int |u|^2;   part[4 b + 3] = int |e|^2
// Iphi[s][l] = int psi_l over a cell of shape s.  ub: the mean flow to subtract (two values on the device; nullptr: none).  Every
// thread reaches the workgroup sums (cell_at); a dead lane reads a valid cell and adds zero.
template <int K>
__global__ __launch_bounds__(128) void k_psi_defect(Geo g, const double* __restrict__ Iphi, const double* __restrict__ curl,
                                                    const double* __restrict__ vel, const double* __restrict__ ub, double* __restrict__ part) {
  constexpr int NU = Dim<K>::NU;
  const CellAt at = cell_at(g);
  const int s = at.s;
  const long c = at.live ? rowbase(g, s, at.j) + at.i : rowbase(g, 0, 0);
  double q[2 * NU], w[2 * NU];
  load_vel<NU>(vel, g.Nc, c, q);
  load_vel<NU>(curl, g.Nc, c, w);
  const double* __restrict__ I = Iphi + s * NU;
  const double ubx = ub ? ub[0] : 0.0, uby = ub ? ub[1] : 0.0;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int l = 0; l < NU; l++) {
    const double ex = fma(-ubx, I[l], q[l]) - w[l], ey = fma(-uby, I[l], q[NU + l]) - w[NU + l];
    sum[0] = fma(I[l], q[l], sum[0]);
    sum[1] = fma(I[l], q[NU + l], sum[1]);
    sum[2] = fma(q[l], q[l], fma(q[NU + l], q[NU + l], sum[2]));
    sum[3] = fma(ex, ex, fma(ey, ey, sum[3]));
  }
  const double lv = at.live ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) sum[k] *= lv;
  psi_block_store<4>(sum, part);
}
// ub = (int u_x, int u_y) / area   (periodic square: the mean flow a periodic psi cannot carry)
__global__ void k_psi_mean_flow(const double* __restrict__ res, double area, double* __restrict__ ub) {
  if (threadIdx.x < 2) ub[threadIdx.x] = res[threadIdx.x] / area;
}

// ---- the gauge.  One workgroup: the arithmetic mean of psi over nv mesh vertices, taken in index order -- the 4 nx boundary
// vertices of the unit square (walk: bottom, right, top, left), every vertex of the periodic square (the first nv dofs).
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_gauge_mean(int nx, int boundary, const double* __restrict__ psi, double* __restrict__ mean) {
  const long nv = boundary ? 4L * nx : (long)nx * nx;
  double s = 0.0;
  for (long q = threadIdx.x; q < nv; q += HDG_PSI_BLOCK) {
    long id = q;
    if (boundary) {
      const int side = (int)(q / nx), k = (int)(q - (long)side * nx);
      const int I = side == 0 ? k : side == 1 ? nx : side == 2 ? nx - k : 0;
      const int J = side == 0 ? 0 : side == 1 ? k : side == 2 ? nx : nx - k;
      id = (long)J * (nx + 1) + I;
    }
    s += psi[id];
  }
  __shared__ double sm[HDG_PSI_BLOCK / 64];
  const double w = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sm[0];
    for (int k = 1; k < HDG_PSI_BLOCK / 64; k++) t += sm[k];
    mean[0] = t / (double)nv;
  }
}
// psi -= mean; workgroup minima and maxima of the shifted values in part[2 b], part[2 b + 1]
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_shift(long n, const double* __restrict__ mean, double* __restrict__ psi, double* __restrict__ part) {
  const double m = mean[0];
  double lo = INFINITY, hi = -INFINITY;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = psi[i] - m;
    psi[i] = v;
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_down(lo, off, 64)); hi = fmax(hi, __shfl_down(hi, off, 64)); }
  __shared__ double sm[HDG_PSI_BLOCK / 64][2];
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = lo; sm[threadIdx.x >> 6][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < HDG_PSI_BLOCK / 64; k++) { lo = fmin(lo, sm[k][0]); hi = fmax(hi, sm[k][1]); }
    part[2L * blockIdx.x] = lo;
    part[2L * blockIdx.x + 1] = hi;
  }
}
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_minmax(int nb, const double* __restrict__ part, double* __restrict__ res) {
  double lo = INFINITY, hi = -INFINITY;
  for (int b = threadIdx.x; b < nb; b += HDG_PSI_BLOCK) { lo = fmin(lo, part[2L * b]); hi = fmax(hi, part[2L * b + 1]); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_down(lo, off, 64)); hi = fmax(hi, __shfl_down(hi, off, 64)); }
  __shared__ double sm[HDG_PSI_BLOCK / 64][2];
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = lo; sm[threadIdx.x >> 6][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < HDG_PSI_BLOCK / 64; k++) { lo = fmin(lo, sm[k][0]); hi = fmax(hi, sm[k][1]); }
    res[0] = lo;
    res[1] = hi;
  }
}

// ---- preconditioned CG on K, one right-hand side, scalars on the device (the pattern of k_cgm_*): per iteration a stiffness
// application, (p, K p), the update of x and r, the preconditioner, (r, z), the new direction, and two one-workgroup launches that
// finish the sums and form alpha and beta.  sc: 0 rz, 1 alpha, 2 beta, 3 rz0, 4 converged.  No host synchronisation inside an iteration.
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_dot(long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ part) {
  double s[1] = {0.0};
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s[0] = b ? fma(a[i], b[i], s[0]) : s[0] + a[i];  // b == nullptr: the sum
  psi_block_store<1>(s, part);
}
// x -= sum / n
__global__ void k_psi_shift_mean(long n, const double* __restrict__ sum, double* __restrict__ x) {
  const double m = sum[0] / (double)n;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] -= m;
}
// finishes a reduction and forms the scalars.  mode 0: the value is (p, K p): alpha = rz / pKp;  mode 1: the new (r, z): beta =
// new / old, convergence flag;  mode 2: the first (r, z): rz = rz0, beta = 0.  hflag (pinned host memory): converged, rz, rz0
__global__ __launch_bounds__(HDG_PSI_BLOCK) void k_psi_scalars(int nb, int mode, double tol2, const double* __restrict__ part, double* __restrict__ sc,
                                                               double* __restrict__ hflag) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += HDG_PSI_BLOCK) s += part[b];
  __shared__ double sm[HDG_PSI_BLOCK / 64];
  const double w = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double v = sm[0];
  for (int k = 1; k < HDG_PSI_BLOCK / 64; k++) v += sm[k];
  if (mode == 0) sc[1] = (v > 0.0 && sc[0] > 0.0) ? sc[0] / v : 0.0;  // a converged (or zero) iteration stands still
  else if (mode == 1) { sc[2] = sc[0] > 0.0 ? v / sc[0] : 0.0; sc[0] = v; }
  else { sc[0] = sc[3] = v; sc[2] = 0.0; }
  sc[4] = !(sc[0] > tol2 * sc[3]) ? 1.0 : 0.0;
  if (hflag) { hflag[0] = sc[4]; hflag[1] = sc[0]; hflag[2] = sc[3]; }
}
// x += alpha p ; r -= alpha K p
__global__ void k_psi_update(long n, const double* __restrict__ sc, const double* __restrict__ p, const double* __restrict__ Kp,
                             double* __restrict__ x, double* __restrict__ r) {
  const double al = sc[1];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    x[i] = fma(al, p[i], x[i]);
    r[i] = fma(-al, Kp[i], r[i]);
  }
}
// p = z + beta p   (beta = 0: the buffer may hold anything)
__global__ void k_psi_dir(long n, const double* __restrict__ sc, const double* __restrict__ z, double* __restrict__ p) {
  const double be = sc[2];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = be == 0.0 ? z[i] : fma(be, p[i], z[i]);
}

}  // namespace hdg
