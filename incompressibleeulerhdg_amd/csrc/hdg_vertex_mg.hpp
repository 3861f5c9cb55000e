// Geometric multigrid on the P1 vertex grid (coarse space of the GTMG preconditioner, hdg_imex.py:97-118,139-167): the
// kernels of every form a level of the V-cycle runs as (hdg_vertex_levels.hpp decides which), the trace <-> P1 transfers
// and the vertex-row exchange of a strip partition.  Orchestration is Engine::vcycle.
//
// Two grids, one set of kernels (template <bool PER>, P1Grid):
//   unit square      (n+1) x (n+1) vertices, vertex (i,j) at j*(n+1) + i.  Operator: P1 stiffness matrix of the
//                    right-triangle mesh = 5-point Laplacian with half weights along boundary edges (homogeneous Neumann).
//   periodic square  n x n vertices, vertex (i,j) at j*n + i, indices wrap.  Operator: the full 5-point stencil (diagonal 4;
//                    singular: constants).
// Every value of a cycle -- relaxed vertex, residual, restricted residual, prolongated correction -- is computed by ONE
// function below, whichever form calls it (per-level kernel, LDS-tile leg, one-workgroup tail): that, not a comparison by
// eye, is why the forms agree bit for bit (one exception: the tail kernel sums its seven restriction terms in place, over
// the shared residual function; the reason is beside it).  The two grids differ in rounding in two places, and each keeps
// its own form under `if constexpr (PER)`: the relaxation (p1_relax) and the restriction (p1_restrict_at).
#pragma once
#include "hdg_kernels.hpp"
#include "hdg_vertex_levels.hpp"

namespace hdg {

template <bool PER>
struct P1Grid {
  int n;
  __device__ __forceinline__ int pitch() const { return PER ? n : n + 1; }  // row pitch
  __device__ __forceinline__ int last() const { return PER ? n - 1 : n; }   // last vertex index of a row / column
  // index of a neighbour (a within n of the grid): wrapped on the periodic grid; on the unit square the caller tests the boundary
  __device__ __forceinline__ int wrap(int a) const { return PER ? (a < 0 ? a + n : (a >= n ? a - n : a)) : a; }
  __device__ __forceinline__ int next(int a) const { return PER ? (a + 1 == n ? 0 : a + 1) : a + 1; }  // wrap(a + 1) for 0 <= a < n
};

// diagonal entry and the sum of the off-diagonal terms (signs flipped) of row (i,j)
template <bool PER>
__device__ __forceinline__ void p1_stencil(const double* x, const P1Grid<PER> g, int i, int j, double& diag, double& off) {
  const int n = g.n, st = g.pitch();
  if constexpr (PER) {
    diag = 4.0;
    off = x[j * st + g.wrap(i - 1)] + x[j * st + g.wrap(i + 1)] + x[g.wrap(j - 1) * st + i] + x[g.wrap(j + 1) * st + i];
  } else {
    const double wx = (j == 0 || j == n) ? 0.5 : 1.0;  // weight of horizontal edges in this row
    const double wy = (i == 0 || i == n) ? 0.5 : 1.0;
    diag = 0.0;
    off = 0.0;
    if (i > 0) { diag += wx; off += wx * x[j * st + i - 1]; }
    if (i < n) { diag += wx; off += wx * x[j * st + i + 1]; }
    if (j > 0) { diag += wy; off += wy * x[(j - 1) * st + i]; }
    if (j < n) { diag += wy; off += wy * x[(j + 1) * st + i]; }
  }
}
// Gauss-Seidel value of a vertex.  Periodic: times 0.25.  Unit square: divided by the diagonal, which is 4 (interior),
// 2 (boundary edge) or 1 (corner) -- its reciprocal is exact, so the kernels that relax in LDS multiply by it (RECIP), bit
// for bit the same as the division.
template <bool PER, bool RECIP>
__device__ __forceinline__ double p1_relax(double b, double diag, double off) {
  if constexpr (PER) return (b + off) * 0.25;
  else if constexpr (RECIP) {
    const double inv = diag == 4.0 ? 0.25 : (diag == 2.0 ? 0.5 : 1.0 / diag);
    return (b + off) * inv;
  } else return (b + off) / diag;
}
template <bool PER>
__device__ __forceinline__ double p1_residual_at(const double* x, const double* b, const P1Grid<PER> g, int i, int j) {
  double diag, off;
  p1_stencil<PER>(x, g, i, j, diag, off);
  return b[j * g.pitch() + i] - (diag * x[j * g.pitch() + i] - off);
}
// restriction = transpose of the nested P1 interpolation (the coarse diagonal joins (I+1,J) and (I,J+1)): the coarse value
// at fine vertex (i,j) = (2I,2J) of grid g; r(di, dj) = the fine residual at (i+di, j+dj).  Unit square: 0.5 r added term
// by term; periodic: the six neighbours summed and halved once.
template <bool PER, class Load>
__device__ __forceinline__ double p1_restrict_at(const P1Grid<PER> g, int i, int j, Load r) {
  if constexpr (PER) return r(0, 0) + 0.5 * (r(-1, 0) + r(1, 0) + r(0, -1) + r(0, 1) + r(-1, 1) + r(1, -1));
  else {
    const int n = g.n;
    double acc = r(0, 0);
    if (i > 0) acc += 0.5 * r(-1, 0);
    if (i < n) acc += 0.5 * r(1, 0);
    if (j > 0) acc += 0.5 * r(0, -1);
    if (j < n) acc += 0.5 * r(0, 1);
    if (i > 0 && j < n) acc += 0.5 * r(-1, 1);
    if (i < n && j > 0) acc += 0.5 * r(1, -1);
    return acc;
  }
}
// nested P1 interpolation: the value at fine vertex (i,j) of the coarse function xc on grid gc
template <bool PER>
__device__ __forceinline__ double p1_prolong_value(const double* xc, const P1Grid<PER> gc, int i, int j) {
  const int I = i >> 1, J = j >> 1, sc = gc.pitch(), I1 = gc.next(I), J1 = gc.next(J);
  double v;
  if (!(i & 1) && !(j & 1)) v = xc[J * sc + I];
  else if ((i & 1) && !(j & 1)) v = 0.5 * (xc[J * sc + I] + xc[J * sc + I1]);
  else if (!(i & 1) && (j & 1)) v = 0.5 * (xc[J * sc + I] + xc[J1 * sc + I]);
  else v = 0.5 * (xc[J * sc + I1] + xc[J1 * sc + I]);
  return v;
}

// ------------------------------------------------------------------------------------------
// Per-level kernels: one thread per vertex, blockIdx.y = the vertex row
// ------------------------------------------------------------------------------------------
// red-black Gauss-Seidel half sweep on A x = b
template <bool PER>
__global__ void k_p1_rbgs(int n, double* __restrict__ x, const double* __restrict__ b, int colour) {
  const P1Grid<PER> g{n};
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > g.last() || ((i + j) & 1) != colour) return;
  double diag, off;
  p1_stencil<PER>(x, g, i, j, diag, off);
  x[j * g.pitch() + i] = p1_relax<PER, false>(b[j * g.pitch() + i], diag, off);
}
template <bool PER>
__global__ void k_p1_residual(int n, const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ r) {
  const P1Grid<PER> g{n};
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > g.last()) return;
  r[j * g.pitch() + i] = p1_residual_at<PER>(x, b, g, i, j);
}
template <bool PER>
__global__ void k_p1_restrict(int nc, const double* __restrict__ rf, double* __restrict__ rc) {
  const P1Grid<PER> gc{nc}, gf{2 * nc};
  const int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y;
  if (I > gc.last()) return;
  const int i = 2 * I, j = 2 * J, st = gf.pitch();
  rc[J * gc.pitch() + I] = p1_restrict_at<PER>(gf, i, j, [&](int di, int dj) { return rf[gf.wrap(j + dj) * st + gf.wrap(i + di)]; });
}
template <bool PER>
__global__ void k_p1_prolong_add(int nc, const double* __restrict__ xc, double* __restrict__ xf) {
  const P1Grid<PER> gc{nc}, gf{2 * nc};
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i > gf.last()) return;
  xf[j * gf.pitch() + i] += p1_prolong_value<PER>(xc, gc, i, j);
}

// ------------------------------------------------------------------------------------------
// Fused legs of one V-cycle level (levels too large for the LDS tail below).  Per level the unfused path
// is 12 launches of ~6 us latency-bound kernels (fill, 2 nsw half sweeps, residual, restriction | prolongation,
// 2 nsw half sweeps); here each leg is ONE kernel: a workgroup holds a TS x TS tile of vertices plus a halo in
// LDS and recomputes the halo (temporal blocking; a half sweep has dependency radius 1, so after m half
// sweeps everything further than m from the edge of the loaded region is exact).
// ------------------------------------------------------------------------------------------
#define HDG_P1_TS 32
#define HDG_P1_THREADS 1024
// Side job of a leg launch (Engine::trace_cg_sr, one rank): the legs are latency-bound (8 barrier-separated LDS phases on a
// grid of at most 33 x 33 tiles) and leave HBM idle, so the half of the CG update that nothing reads before the next
// update -- p = (z - c n) + beta p ; x += alpha p (k_cg_sr_update_xp) -- rides along: the workgroups of the tile rows
// >= nrows of a leg launch each take 1024 sixteen-byte pairs of the slice [i0, i1) instead of a tile, and apply to them the whole
// batch of queued updates in order (XpBatch, hdg_cg_pending.hpp: one pass over p and x for up to 16 iterations).  (A second stream
// for the same purpose gained 14 us per CG iteration of the 64 possible: two cross-stream dependencies cost 17 us.)
struct SideXP {
  XpBatch b;  // the queued updates the slice applies in one pass (hdg_kernels.hpp)
  const double* nvec;
  double* p;
  double* x;
  long i0, i1;
};
__device__ __forceinline__ void side_xp(const SideXP& sj, long blk, long nblk) {
  for (long i = sj.i0 + blk * HDG_P1_THREADS + threadIdx.x; i < sj.i1; i += nblk * HDG_P1_THREADS) xp_batch_pair(sj.b, i, sj.nvec, sj.p, sj.x);
}
// by = the tile row of a workgroup that has one; side rows do their share of the side job and leave (hdg_side_rows.hpp)
#define HDG_P1_SIDE_JOB                                                                                              \
  const SideRow srow_ = side_row_of((int)blockIdx.y, (int)gridDim.y, extra, period);                                 \
  if (srow_.side) {                                                                                                  \
    side_xp(sj, (long)srow_.idx * gridDim.x + blockIdx.x, (long)extra * gridDim.x);                                  \
    return;                                                                                                          \
  }                                                                                                                  \
  const int by = srow_.idx;
// region-local stencil: (gi, gj) global vertex, (li, lj) local; false if a neighbour inside the domain lies
// outside the loaded region (the point is then part of the garbage ring and is skipped).  Tile-local coordinates: on the
// periodic grid the loads of a leg have wrapped already and every vertex is interior (the four terms in p1_stencil's order).
template <int W, bool PER = false>
__device__ __forceinline__ bool p1_stencil_tile(const double* X, int n, int gi, int gj, int li, int lj, double& diag,
                                                double& off) {
  if (PER) {
    diag = 4.0;
    off = 0.0;
    if (li == 0 || li == W - 1 || lj == 0 || lj == W - 1) return false;
    off = X[lj * W + li - 1] + X[lj * W + li + 1] + X[(lj - 1) * W + li] + X[(lj + 1) * W + li];
    return true;
  }
  const double wx = (gj == 0 || gj == n) ? 0.5 : 1.0;
  const double wy = (gi == 0 || gi == n) ? 0.5 : 1.0;
  diag = 0.0;
  off = 0.0;
  if ((gi > 0 && li == 0) || (gi < n && li == W - 1) || (gj > 0 && lj == 0) || (gj < n && lj == W - 1)) return false;
  if (gi > 0) { diag += wx; off += wx * X[lj * W + li - 1]; }
  if (gi < n) { diag += wx; off += wx * X[lj * W + li + 1]; }
  if (gj > 0) { diag += wy; off += wy * X[(lj - 1) * W + li]; }
  if (gj < n) { diag += wy; off += wy * X[(lj + 1) * W + li]; }
  return true;
}
// 2 nsw half sweeps; each thread owns the q-th vertex of the active colour (W even: W/2 per row and colour)
template <int W, bool PER = false>
__device__ __forceinline__ void p1_tile_sweeps(double* X, const double* B, int n, int gi0, int gj0, int nsw, bool reverse) {
  for (int hs = 0; hs < 2 * nsw; hs++) {
    const int colour = ((hs & 1) == 0) ? (reverse ? 1 : 0) : (reverse ? 0 : 1);
    for (int q = threadIdx.x; q < W * W / 2; q += HDG_P1_THREADS) {
      const int lj = q / (W / 2), li = 2 * (q - lj * (W / 2)) + ((colour + gi0 + gj0 + lj) & 1);
      const int gi = gi0 + li, gj = gj0 + lj;
      if (!PER && (gi < 0 || gj < 0 || gi > n || gj > n)) continue;
      double diag, off;
      if (p1_stencil_tile<W, PER>(X, n, gi, gj, li, lj, diag, off)) X[lj * W + li] = p1_relax<PER, true>(B[lj * W + li], diag, off);
    }
    __syncthreads();
  }
}
// down leg: x = 0, nsw sweeps on A x = b, r = b - A x, bc = R r (coarse right-hand side); x is stored to xpre
template <int NSW, bool PER = false>
__global__ __launch_bounds__(HDG_P1_THREADS) void k_p1_down(int n, const double* __restrict__ b, double* __restrict__ xpre,
                                                            double* __restrict__ bc, int jt0 = 0, int extra = 0, int period = 2, SideXP sj = SideXP{}) {
  constexpr int H = 2 * NSW + 2, W = HDG_P1_TS + 2 * H;
  __shared__ double X[W * W];
  __shared__ double B[W * W];
  HDG_P1_SIDE_JOB
  const P1Grid<PER> g{n}, gc{n >> 1};
  const int st = g.pitch(), last = g.last();
  const int i0 = blockIdx.x * HDG_P1_TS, j0 = (by + jt0) * HDG_P1_TS, gi0 = i0 - H, gj0 = j0 - H;  // jt0: first tile row of this launch
  for (int p = threadIdx.x; p < W * W; p += HDG_P1_THREADS) {
    const int lj = p / W, li = p - lj * W, gi = gi0 + li, gj = gj0 + lj;
    if (PER) B[p] = b[g.wrap(gj) * st + g.wrap(gi)];
    else {
      const bool in = gi >= 0 && gj >= 0 && gi <= n && gj <= n;
      B[p] = in ? b[gj * st + gi] : 0.0;
    }
    X[p] = 0.0;
  }
  __syncthreads();
  p1_tile_sweeps<W, PER>(X, B, n, gi0, gj0, NSW, false);
  // store the tile's x, then overwrite B by the residual (r_p needs b_p and x only)
  {
    const int p = threadIdx.x;  // HDG_P1_TS^2 == HDG_P1_THREADS
    const int tj = p / HDG_P1_TS, ti = p - tj * HDG_P1_TS, gi = i0 + ti, gj = j0 + tj;
    if (gi <= last && gj <= last) xpre[gj * st + gi] = X[(tj + H) * W + ti + H];
  }
  for (int p = threadIdx.x; p < W * W; p += HDG_P1_THREADS) {
    const int lj = p / W, li = p - lj * W, gi = gi0 + li, gj = gj0 + lj;
    if (!PER && (gi < 0 || gj < 0 || gi > n || gj > n)) continue;
    double diag, off;
    if (p1_stencil_tile<W, PER>(X, n, gi, gj, li, lj, diag, off)) B[p] = B[p] - (diag * X[p] - off);
  }
  __syncthreads();
  constexpr int HT = HDG_P1_TS / 2;
  if (threadIdx.x < HT * HT) {
    const int p = threadIdx.x;
    const int tJ = p / HT, tI = p - tJ * HT, i = i0 + 2 * tI, j = j0 + 2 * tJ;
    if (i <= last && j <= last) {
      const int li = i - gi0, lj = j - gj0;
      bc[(j >> 1) * gc.pitch() + (i >> 1)] = p1_restrict_at<PER>(g, i, j, [&](int di, int dj) { return B[(lj + dj) * W + li + di]; });
    }
  }
}
// up leg: x = xpre + P xc, nsw sweeps with the colours reversed.  xpre (the down leg's result) and x are
// DIFFERENT buffers: a workgroup reads the halo of its tile while its neighbours store theirs.
template <int NSW, bool PER = false>
__global__ __launch_bounds__(HDG_P1_THREADS) void k_p1_up(int n, const double* __restrict__ xc, const double* __restrict__ b,
                                                          const double* __restrict__ xpre, double* __restrict__ x, int jt0 = 0, int extra = 0, int period = 2,
                                                          SideXP sj = SideXP{}) {
  constexpr int H = 2 * NSW, W = HDG_P1_TS + 2 * H;
  __shared__ double X[W * W];
  __shared__ double B[W * W];
  HDG_P1_SIDE_JOB
  const P1Grid<PER> g{n}, gc{n >> 1};
  const int st = g.pitch(), last = g.last();
  const int i0 = blockIdx.x * HDG_P1_TS, j0 = (by + jt0) * HDG_P1_TS, gi0 = i0 - H, gj0 = j0 - H;  // jt0: first tile row of this launch
  for (int p = threadIdx.x; p < W * W; p += HDG_P1_THREADS) {
    const int lj = p / W, li = p - lj * W;
    int i = gi0 + li, j = gj0 + lj;
    if (PER) { i = g.wrap(i); j = g.wrap(j); }
    else if (i < 0 || j < 0 || i > n || j > n) { X[p] = 0.0; B[p] = 0.0; continue; }
    X[p] = xpre[j * st + i] + p1_prolong_value<PER>(xc, gc, i, j);
    B[p] = b[j * st + i];
  }
  __syncthreads();
  p1_tile_sweeps<W, PER>(X, B, n, gi0, gj0, NSW, true);
  {
    const int p = threadIdx.x;
    const int tj = p / HDG_P1_TS, ti = p - tj * HDG_P1_TS, gi = i0 + ti, gj = j0 + tj;
    if (gi <= last && gj <= last) x[gj * st + gi] = X[(tj + H) * W + ti + H];
  }
}

// ------------------------------------------------------------------------------------------
// The coarse tail of the unit square's V-cycle (all levels with n <= 32, i.e. <= 33^2 vertices) in ONE workgroup with
// every level resident in LDS: replaces ~70 launches of 1-4 us kernels per V-cycle by one.
// Same algorithm as the per-level kernels: V(nsw,nsw) with red-black Gauss-Seidel (colours swapped on
// the way up), residual restriction by the transpose of the nested P1 interpolation, ncoarse+ncoarse
// sweeps on the coarsest level.
// ------------------------------------------------------------------------------------------
struct P1Tail {
  int nlev;
  int n[8];
};
__device__ __forceinline__ void p1_sweeps_lds(double* x, const double* b, int n, int sweeps, bool reverse) {
  const P1Grid<false> g{n};
  const int npts = (n + 1) * (n + 1);
  // n even (every level of the tail): the row length is odd, so the points of colour c are exactly the odd / even linear
  // indices: every thread of a trip has work (n = 32: one trip of 545 points instead of two over 1089).
  const int step = (n & 1) ? 1 : 2;
  for (int sw = 0; sw < 2 * sweeps; sw++) {
    const int colour = ((sw & 1) == 0) ? (reverse ? 1 : 0) : (reverse ? 0 : 1);
    for (int p = step * threadIdx.x + (step == 2 ? colour : 0); p < npts; p += step * blockDim.x) {
      const int j = p / (n + 1), i = p - j * (n + 1);
      if (step == 2 || ((i + j) & 1) == colour) {
        double diag, off;
        p1_stencil<false>(x, g, i, j, diag, off);
        x[p] = p1_relax<false, true>(b[p], diag, off);
      }
    }
    __syncthreads();
  }
}
// unit_pitch > 0 (set-up of the dense form, k_p1_dense_tail): workgroup c solves for the c-th UNIT right-hand side and writes its
// result to x_out + c * unit_pitch -- every column of the tail's matrix in ONE launch
__global__ __launch_bounds__(1024) void k_p1_vcycle_tail(P1Tail tl, const double* __restrict__ b_in,
                                                          double* __restrict__ x_out, int nsw, int ncoarse, int unit_pitch = 0) {
  __shared__ double X[HDG_P1_TAIL_MAX];
  __shared__ double B[HDG_P1_TAIL_MAX];
  int offs[9];
  offs[0] = 0;
  for (int l = 0; l < tl.nlev; l++) offs[l + 1] = offs[l] + (tl.n[l] + 1) * (tl.n[l] + 1);
  if (unit_pitch > 0) {
    for (int p = threadIdx.x; p < offs[1]; p += blockDim.x) B[p] = p == (int)blockIdx.x ? 1.0 : 0.0;
    x_out += (long)blockIdx.x * unit_pitch;
  } else {
    for (int p = threadIdx.x; p < offs[1]; p += blockDim.x) B[p] = b_in[p];
  }
  for (int p = threadIdx.x; p < offs[tl.nlev]; p += blockDim.x) X[p] = 0.0;
  __syncthreads();
  for (int l = 0; l < tl.nlev - 1; l++) {
    const int n = tl.n[l], nc = tl.n[l + 1];
    const P1Grid<false> g{n};
    double* x = X + offs[l];
    const double* b = B + offs[l];
    p1_sweeps_lds(x, b, n, nsw, false);
    double* bc = B + offs[l + 1];
    for (int p = threadIdx.x; p < (nc + 1) * (nc + 1); p += blockDim.x) {
      const int J = p / (nc + 1), I = p - J * (nc + 1), i = 2 * I, j = 2 * J;
      // (written out, not p1_restrict_at over the residual: through the helper the compiler allocates 56 instead of 44 VGPRs here)
      double acc = p1_residual_at<false>(x, b, g, i, j);
      if (i > 0) acc += 0.5 * p1_residual_at<false>(x, b, g, i - 1, j);
      if (i < n) acc += 0.5 * p1_residual_at<false>(x, b, g, i + 1, j);
      if (j > 0) acc += 0.5 * p1_residual_at<false>(x, b, g, i, j - 1);
      if (j < n) acc += 0.5 * p1_residual_at<false>(x, b, g, i, j + 1);
      if (i > 0 && j < n) acc += 0.5 * p1_residual_at<false>(x, b, g, i - 1, j + 1);
      if (i < n && j > 0) acc += 0.5 * p1_residual_at<false>(x, b, g, i + 1, j - 1);
      bc[p] = acc;
    }
    __syncthreads();
  }
  {
    const int l = tl.nlev - 1;
    p1_sweeps_lds(X + offs[l], B + offs[l], tl.n[l], ncoarse, false);
    p1_sweeps_lds(X + offs[l], B + offs[l], tl.n[l], ncoarse, true);
  }
  for (int l = tl.nlev - 2; l >= 0; l--) {
    const int n = tl.n[l];
    const P1Grid<false> gc{tl.n[l + 1]};
    double* x = X + offs[l];
    const double* xc = X + offs[l + 1];
    for (int p = threadIdx.x; p < (n + 1) * (n + 1); p += blockDim.x) {
      const int j = p / (n + 1), i = p - j * (n + 1);
      x[p] += p1_prolong_value<false>(xc, gc, i, j);
    }
    __syncthreads();
    p1_sweeps_lds(x, B + offs[l], n, nsw, true);
  }
  for (int p = threadIdx.x; p < offs[1]; p += blockDim.x) x_out[p] = X[p];
}

// Dense form of the tail.  The tail is a fixed LINEAR map of its right-hand side (zero start, fixed sweeps), so
// it is one matrix M of (n+1)^2 <= 1089 rows: k_p1_vcycle_tail walks through ~48 barrier-separated phases in ONE workgroup
// (33.7 us at every mesh size, a quarter of a V-cycle at C3); M b is 9.5 MB of matrix from the L2 / Infinity Cache spread
// over 273 workgroups.  M is built once per engine by applying the tail to the unit vectors (the same operator up
// to the rounding of the summation order); one wave per row, 16-byte loads, deterministic wave reduction.
__global__ __launch_bounds__(256) void k_p1_dense_tail(int N, int pitch, const double* __restrict__ M, const double* __restrict__ b,
                                                       double* __restrict__ x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const double* __restrict__ mr = M + (long)row * pitch;
  double acc0 = 0.0, acc1 = 0.0;
  for (int c = 2 * lane; c < N; c += 128) {
    const hdg_d2 m = *reinterpret_cast<const hdg_d2*>(mr + c);
    acc0 = fma(m.x, b[c], acc0);
    if (c + 1 < N) acc1 = fma(m.y, b[c + 1], acc1);
  }
  const double acc = wave_sum(acc0 + acc1);
  if (lane == 0) x[row] = acc;
}
__global__ void k_transpose_sq(int N, int pitch, const double* __restrict__ in, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c < N) out[(long)r * pitch + c] = in[(long)c * pitch + r];
}

// ------------------------------------------------------------------------------------------
// trace <-> P1 transfer: P = edge-wise L2 projection of the P1 function (hdg_imex.py:491-503,
// without the reference's 1/2 on interior edges - a preconditioner detail).  One pair per grid: their
// ghost-row logic differs for real (cut rows of a strip partition | wrapped ghost rows).
// ------------------------------------------------------------------------------------------
__global__ void k_p1_to_trace(Geo g, int NL, const double* __restrict__ xc, double* __restrict__ l, double accumulate,
                              double lH, double lV, double lD) {
  HDG_CORNER_PROLOGUE
  const int st = g.nx + 1;
  const long J = g.joff + j;  // global vertex row; xc is the global (replicated) vertex vector
  const double r3 = 0.57735026918962576451;
  const double v00 = xc[J * st + i];
  if (in_x) {
    const double vb = xc[J * st + i + 1], sl = sqrt(lH);
    double* p0 = l + ((long)0 * NL) * g.G + o;
    double* p1 = l + ((long)0 * NL + 1) * g.G + o;
    *p0 = accumulate * (*p0) + sl * 0.5 * (v00 + vb);
    *p1 = accumulate * (*p1) + sl * r3 * 0.5 * (vb - v00);
  }
  if (in_y) {
    const double vb = xc[(J + 1) * st + i], sl = sqrt(lV);
    double* p0 = l + ((long)1 * NL) * g.G + o;
    double* p1 = l + ((long)1 * NL + 1) * g.G + o;
    *p0 = accumulate * (*p0) + sl * 0.5 * (v00 + vb);
    *p1 = accumulate * (*p1) + sl * r3 * 0.5 * (vb - v00);
  }
  if (in_x && in_y) {
    const double va = xc[J * st + i + 1], vb = xc[(J + 1) * st + i], sl = sqrt(lD);
    double* p0 = l + ((long)2 * NL) * g.G + o;
    double* p1 = l + ((long)2 * NL + 1) * g.G + o;
    *p0 = accumulate * (*p0) + sl * 0.5 * (va + vb);
    *p1 = accumulate * (*p1) + sl * r3 * 0.5 * (vb - va);
  }
}
// transpose: a vertex row gathers from its (up to six) incident edges (rows j and j-1); writes the rank's rows
// joff .. joff+ny of the global vertex vector.  Strip partition (partial != 0, launched over rows 0..ny): every
// rank sums its OWNED edges only, so no halo of the residual is needed -- the vertex row on a cut receives the
// edges of the row below from the lower rank (its extra row ny: only those terms) and everything else from the
// upper rank (its row 0 without them); k_p1_assemble adds the two parts.
__global__ void k_trace_to_p1(Geo g, int NL, const double* __restrict__ l, double* __restrict__ rc, double lH, double lV,
                              double lD, int partial) {
  HDG_CORNER_PROLOGUE
  const int st = g.nx + 1;
  const double r3 = 0.57735026918962576451;
  const double* H0 = l + ((long)0 * NL) * g.G;
  const double* H1 = l + ((long)0 * NL + 1) * g.G;
  const double* V0 = l + ((long)1 * NL) * g.G;
  const double* V1 = l + ((long)1 * NL + 1) * g.G;
  const double* D0 = l + ((long)2 * NL) * g.G;
  const double* D1 = l + ((long)2 * NL + 1) * g.G;
  const double sH = 0.5 * sqrt(lH), sV = 0.5 * sqrt(lV), sD = 0.5 * sqrt(lD);
  const bool cut_lo = partial && g.joff > 0 && j == 0;                      // edges of row -1 belong to the lower rank
  const bool extra = partial && (g.joff + g.ny < g.nyg) && j == g.ny;       // lower side of the cut above: row ny-1 only
  const bool from_below = below && !cut_lo;
  double acc = 0.0;
  if (!extra) {
    if (i < g.nx) acc += sH * (H0[o] - r3 * H1[o]);                            // H(i,j): a-end
    if (i > 0) acc += sH * (H0[o - 1] + r3 * H1[o - 1]);                       // H(i-1,j): b-end
    if (in_y) acc += sV * (V0[o] - r3 * V1[o]);                                // V(i,j): a-end
  }
  if (from_below) acc += sV * (V0[o - g.P] + r3 * V1[o - g.P]);                // V(i,j-1): b-end
  if (!extra && i > 0 && in_y) acc += sD * (D0[o - 1] - r3 * D1[o - 1]);       // D(i-1,j): a-end (x_i,y_j)
  if (i < g.nx && from_below) acc += sD * (D0[o - g.P] + r3 * D1[o - g.P]);    // D(i,j-1): b-end (x_i,y_j)
  rc[(long)(g.joff + j) * st + i] = acc;
}
// trace <-> periodic P1 grid (ghost trace rows must be current for the restriction)
__global__ void k_p1p_to_trace(Geo g, int NL, const double* __restrict__ xc, double* __restrict__ l, double accumulate,
                               double lH, double lV, double lD) {
  HDG_CORNER_PROLOGUE
  const P1Grid<true> pg{g.nx};
  const int n = g.nx, J = g.pj0 + j, i1 = pg.wrap(i + 1), j1 = pg.wrap(J + 1);  // (owned corner rows: J < n)
  const double r3 = 0.57735026918962576451;
  const double v00 = xc[J * n + i], v10 = xc[J * n + i1], v01 = xc[j1 * n + i];
  const double ea[3] = {v00, v00, v10}, eb[3] = {v10, v01, v01}, len[3] = {lH, lV, lD};
#pragma unroll
  for (int t = 0; t < 3; t++) {
    const double sl = sqrt(len[t]);
    double* p0 = l + ((long)t * NL) * g.G + o;
    double* p1 = l + ((long)t * NL + 1) * g.G + o;
    *p0 = accumulate * (*p0) + sl * 0.5 * (ea[t] + eb[t]);
    *p1 = accumulate * (*p1) + sl * r3 * 0.5 * (eb[t] - ea[t]);
  }
}
__global__ void k_trace_to_p1p(Geo g, int NL, const double* __restrict__ l, double* __restrict__ rc, double lH, double lV, double lD) {
  HDG_CORNER_PROLOGUE
  const double r3 = 0.57735026918962576451;
  const double* H0 = l + ((long)0 * NL) * g.G;
  const double* H1 = l + ((long)0 * NL + 1) * g.G;
  const double* V0 = l + ((long)1 * NL) * g.G;
  const double* V1 = l + ((long)1 * NL + 1) * g.G;
  const double* D0 = l + ((long)2 * NL) * g.G;
  const double* D1 = l + ((long)2 * NL + 1) * g.G;
  const double sH = 0.5 * sqrt(lH), sV = 0.5 * sqrt(lV), sD = 0.5 * sqrt(lD);
  double acc = sH * (H0[o] - r3 * H1[o]) + sH * (H0[oL] + r3 * H1[oL])          // H(i,j) a-end, H(i-1,j) b-end
             + sV * (V0[o] - r3 * V1[o]) + sV * (V0[o - g.P] + r3 * V1[o - g.P])  // V(i,j) a-end, V(i,j-1) b-end (ghost row for j = 0)
             + sD * (D0[oL] - r3 * D1[oL]) + sD * (D0[o - g.P] + r3 * D1[o - g.P]);  // D(i-1,j) a-end, D(i,j-1) b-end
  rc[(g.pj0 + j) * g.nx + i] = acc;
}

// ------------------------------------------------------------------------------------------
// Distributed finest level of the vertex-grid V-cycle (strip partition): after the restriction from the rank's own edges
// the neighbours swap `depth` vertex rows next to the cut plus their PARTIAL sums of the cut row itself.  A message holds
// depth + 1 rows of st values; from_lo = [rows J0-depth .. J0-1, partial row J0], from_hi = [partial row J1, rows J1+1 ..
// J1+depth] (J0 / J1: the rank's lowest / highest vertex row).  The partial rows are added, the others stored.
// ------------------------------------------------------------------------------------------
__global__ void k_p1_merge_halo(int st, int depth, int J0, int J1, int has_lo, int has_hi, const double* __restrict__ from_lo,
                                const double* __restrict__ from_hi, double* __restrict__ b) {
  const long n = (long)(depth + 1) * st;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
    const int row = (int)(idx / st), i = (int)(idx - (long)row * st);
    if (has_lo) {
      if (row < depth) b[(long)(J0 - depth + row) * st + i] = from_lo[idx];
      else b[(long)J0 * st + i] += from_lo[idx];
    }
    if (has_hi) {
      if (row == 0) b[(long)J1 * st + i] += from_hi[idx];
      else b[(long)(J1 + row) * st + i] = from_hi[idx];
    }
  }
}
// global vertex vector from the all-gathered blocks of (ny+1) rows per rank, in ONE launch: rank r owns the rows
// r*ny .. (r+1)*ny-1 (the last rank also the top row); on a cut the lower rank's extra row is added (partial sums)
__global__ void k_p1_assemble(int P, int ny, int st, const double* __restrict__ gathered, double* __restrict__ out,
                              int partial) {
  const long n = ((long)P * ny + 1) * st, blk = (long)(ny + 1) * st;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
    const int R = (int)(idx / st), i = (int)(idx - (long)R * st);
    int r = R / ny;
    if (r > P - 1) r = P - 1;
    const int lr = R - r * ny;
    double v = gathered[r * blk + (long)lr * st + i];
    if (partial && lr == 0 && r > 0) v += gathered[(r - 1) * blk + (long)ny * st + i];
    out[idx] = v;
  }
}

}  // namespace hdg
