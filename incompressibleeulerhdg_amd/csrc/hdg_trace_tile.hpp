// The two smoother applications of the trace preconditioner (GTMG of hdg_imex.py:139-167: Chebyshev(2) + edge block-Jacobi
// around the coarse-grid correction) as TWO kernels instead of five row-stencil launches per CG iteration:
//
//   k_trace_pre_tile   z = S_pre(r)            (zero start: d0 = Dinv r / theta, d1 = c1 d0 + c2 Dinv (r - T d0), z = d0 + d1)
//                      res = r - T z           (what the restriction to the vertex grid consumes)
//   k_trace_post_tile  z0 = z + P xc           (prolongation of the vertex-grid correction)
//                      r0 = r - T z0, d0 = Dinv r0 / theta, z1 = z0 + d0
//                      r1 = r0 - T d0, d1 = c1 d0 + c2 Dinv r1, z2 = z1 + d1
//                      w  = T z2               (the operator application the single-reduction CG needs next)
//
// Why: each of the five stencil launches (k_trace_smooth x 3, k_trace_apply x 2) is bound by its own dependent-latency
// chain (27 loads -> products -> block-Jacobi -> stores: 37-97 us for 150-390 MB at C3), not by bytes; folding pointwise
// work into them bought 1-2 %.  Here a workgroup owns a tile of TW x TH grid corners, keeps the
// stencil inputs of every stage in LDS with a halo that shrinks by one corner per operator application (2 for the pre
// kernel, 3 for the post kernel: recomputed, not exchanged) and walks through the stages between barriers -- the scheme
// of the vertex-grid kernels k_p1_down / k_p1_up.  One thread keeps the same corners through all stages (the index map of
// the halo-2 region; stages that act on a smaller region mask the rest).  The post kernel holds every value ONCE: only r / r0,
// which no LDS array has, crosses a barrier in registers.  d0 lives in Ds and z0 in Zs; the stage that needs them pointwise
// reads them back at the thread's own slot (d0 is own[] of the stencil read it does anyway), and z1 = z0 + d0 is formed
// where it is consumed.  Held in registers as well (36 VGPRs at k = 2) they kept it at 157 VGPRs, three workgroups per CU;
// without them it fits four.  The pre kernel keeps r and d0 in registers (four workgroups per CU either way).
//
// Same arithmetic per corner as trace_stencil / k_trace_smooth.  Round 4: strips as well, and the doubly periodic square
// (corner_info: wrapped columns; in y a strip whose ghost rows are its own opposite rows).  A launch
// COMPUTES the corner rows [jlo, jhi) of the rank's strip (local numbering, ghost rows included) and READS the rows
// [rlo, rhi) = the computed rows +- the kernel's halo; a corner outside that window or outside the GLOBAL mesh is a zero
// (it lies beyond the dependency cone of every computed row).  One rank: jlo = 0, jhi = ny + 1, the window is the mesh.
// On a strip the pre kernel computes 3 ghost rows towards every neighbour (z valid where the post kernel's halo reads it),
// so r has to be valid 5 ghost rows deep: ONE exchange per CG iteration (Geo: GH = 6).
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

template <int K>
struct TraceTile {
  static constexpr int NL = Dim<K>::NL, NT = 3 * NL;
  // Tile 16 x 8 corners, 256 threads: one corner of the halo-2 region (20 x 12 = 240) per thread.  Measured at C3 (k = 2),
  // us per launch pre / post: 32 x 8 tiles with two corners per thread 93 / 148 (212 VGPRs in the post kernel), 32 x 8 with
  // 512 threads 124 / 180, 16 x 8 87 / 135 (166 VGPRs, 3 workgroups per CU), 16 x 4 with 192 threads 103 / 166, 16 x 8 forced
  // to 4 waves per SIMD 90 / 188 (spills).  The five row-stencil launches they replace: 60 + 37 and 97 + 78 + 37.
  static constexpr int TW = 16, TH = 8, NTHREADS = 256;
  static constexpr int W2 = TW + 4, H2 = TH + 4, N2 = W2 * H2;  // halo-2 region: the index map of every stage
  // waves per SIMD the post kernel is held to (with the inner products too): the step its registers reach without scratch and
  // its LDS fits (k = 1, 2, 3: 87 / 123 / 159 VGPRs; 5 x 26464, 4 x 39616, 3 x 52768 B of the CU's 160 KiB)
  static constexpr int WPE_POST = K == 1 ? 5 : (K == 2 ? 4 : (K == 3 ? 3 : 1));
  static constexpr int W3 = TW + 6, H3 = TH + 6, N3 = W3 * H3;  // halo-3 region (post kernel, stage 0)
  static constexpr int W1 = TW + 2, H1 = TH + 2, N1 = W1 * H1;  // halo-1 region
  static constexpr int KMAX = (N2 + NTHREADS - 1) / NTHREADS;   // corners per thread
};

// (-S) v at the three edges of a corner from an LDS array A[(t * NL + m)][row][col] (region pitch RW, RH rows), corner at
// (li, lj) of that region; own[] = the corner's own edges in local-edge order (H, D, V)
template <int K, int RW, int RH>
__device__ __forceinline__ void lds_trace_stencil(const double* __restrict__ A, int li, int lj, bool in_x, bool in_y, bool below,
                                                  bool left, const DevTables& T, double* own, double* yH, double* yV, double* yD) {
  constexpr int NL = Dim<K>::NL, NT = 3 * NL;
  auto at = [&](int t, int m, int dj, int di) { return A[((t * NL + m) * RH + (lj + dj)) * RW + (li + di)]; };
  double uA[NT], uB[NT], uC[NT];
#pragma unroll
  for (int m = 0; m < NL; m++) {
    own[m] = at(0, m, 0, 0); own[NL + m] = at(2, m, 0, 0); own[2 * NL + m] = at(1, m, 0, 0);
    uA[m] = at(0, m, 1, 0); uA[2 * NL + m] = at(1, m, 0, 1);         // U(i,j):   H(i,j+1), V(i+1,j)
    uB[NL + m] = at(2, m, -1, 0); uB[2 * NL + m] = at(1, m, -1, 1);  // U(i,j-1): D(i,j-1), V(i+1,j-1)
    uC[m] = at(0, m, 1, -1); uC[NL + m] = at(2, m, 0, -1);           // U(i-1,j): H(i-1,j+1), D(i-1,j)
    yH[m] = yV[m] = yD[m] = 0.0;
  }
  const bool vL = in_x && in_y, vB = in_x && below, vW = in_y && left;
#pragma unroll
  for (int m = 0; m < NL; m++) {
    if (!in_x) own[m] = 0.0;
    if (!vL) own[NL + m] = 0.0;
    if (!in_y) own[2 * NL + m] = 0.0;
    uA[NL + m] = own[NL + m];
    uB[m] = own[m];
    uC[2 * NL + m] = own[2 * NL + m];
  }
  const double* __restrict__ SL = T.SK[0];
  const double* __restrict__ SU = T.SK[1];
  if (vL) {
    mv_acc_ld<NL, NT>(SL + 0 * NL * NT, NT, own, yH, -1.0);
    mv_acc_ld<NL, NT>(SL + 1 * NL * NT, NT, own, yD, -1.0);
    mv_acc_ld<NL, NT>(SL + 2 * NL * NT, NT, own, yV, -1.0);
    mv_acc_ld<NL, NT>(SU + 1 * NL * NT, NT, uA, yD, -1.0);
  }
  if (vB) mv_acc_ld<NL, NT>(SU + 0 * NL * NT, NT, uB, yH, -1.0);
  if (vW) mv_acc_ld<NL, NT>(SU + 2 * NL * NT, NT, uC, yV, -1.0);
}

// per-corner facts on a single-rank, non-periodic mesh
// Tile of a workgroup.  The launch is one-dimensional with 8 * ceil(tiles / 8) workgroups; the hardware deals consecutive
// workgroups round-robin to the 8 XCDs, so workgroup b runs on XCD b % 8 and takes the (b / 8)-th tile of that XCD's
// CONTIGUOUS range of tiles (row-major: a band of tile rows): the halos that neighbouring tiles share are then served by
// the XCD's own L2 instead of the fabric (PMC before: 1.8x / 2.2x the algorithmic bytes for the pre / post kernel).
#define HDG_TILE_OF_BLOCK                                              \
  const int tiles_per_xcd_ = (int)(gridDim.x >> 3);                    \
  const int tile_v = (int)(blockIdx.x & 7) * tiles_per_xcd_ + (int)(blockIdx.x >> 3); \
  if (tile_v >= ntx * nty) return;                                     \
  const int tile_y = tile_v / ntx, tile_x = tile_v - tile_y * ntx;
struct CornerInfo {
  bool exists, in_x, in_y, below, left;
  bool own_x;  // the column is one of the mesh's own (periodic in x: a wrapped halo column is NOT; stores / inner products skip it)
  int vH, vV;  // block-Jacobi variants of the corner's H and V edge
  long o;      // offset of the corner inside a trace plane
};
// rows of a tile launch: computed [jlo, jhi), readable [rlo, rhi) (local corner rows of the strip)
struct TileRows {
  int jlo, jhi, rlo, rhi;
};
__device__ __forceinline__ CornerInfo corner_info(const Geo& g, const TileRows& tr, int i, int j) {
  CornerInfo c;
  const int gj = g.joff + j;  // global corner row
  if (g.px) {
    // doubly periodic square: nx corner columns, every column index wraps; in y the strip pretends to lie inside a taller mesh
    // (Engine::construct) and its ghost rows hold the rows of the opposite side, as on a strip between two neighbours
    c.exists = gj >= 0 && gj <= g.nyg && j >= tr.rlo && j < tr.rhi;
    c.own_x = i >= 0 && i < g.nx;
    const int iw = i < 0 ? i + g.nx : (i >= g.nx ? i - g.nx : i);  // tiles reach at most 3 columns beyond either end; nx >= 16 (use_trace_tile)
    c.in_x = c.exists;
    c.in_y = c.exists && gj < g.nyg;
    c.below = gj > 0;
    c.left = true;
    c.vH = gj == 0 ? 1 : (gj == g.nyg ? 2 : 0);
    c.vV = 0;
    c.o = (long)(j + GH) * g.P + iw;
    return c;
  }
  c.exists = i >= 0 && i <= g.nx && gj >= 0 && gj <= g.nyg && j >= tr.rlo && j < tr.rhi;
  c.own_x = true;
  c.in_x = c.exists && i < g.nx;
  c.in_y = c.exists && gj < g.nyg;
  c.below = gj > 0;
  c.left = i > 0;
  c.vH = gj == 0 ? 1 : (gj == g.nyg ? 2 : 0);
  c.vV = i == 0 ? 1 : (i == g.nx ? 2 : 0);
  c.o = (long)(j + GH) * g.P + i;
  return c;
}
// the corner's edge values of a global trace vector, local-edge order (H, D, V), zero where the edge does not exist
template <int NL>
__device__ __forceinline__ void load_corner(const double* __restrict__ v, const Geo& g, const CornerInfo& c, double* e) {
#pragma unroll
  for (int m = 0; m < NL; m++) {
    e[m] = c.in_x ? v[((long)0 * NL + m) * g.G + c.o] : 0.0;
    e[NL + m] = (c.in_x && c.in_y) ? v[((long)2 * NL + m) * g.G + c.o] : 0.0;
    e[2 * NL + m] = c.in_y ? v[((long)1 * NL + m) * g.G + c.o] : 0.0;
  }
}
template <int NL>
__device__ __forceinline__ void store_corner(double* __restrict__ v, const Geo& g, const CornerInfo& c, const double* e) {
#pragma unroll
  for (int m = 0; m < NL; m++) {
    v[((long)0 * NL + m) * g.G + c.o] = c.in_x ? e[m] : 0.0;
    v[((long)2 * NL + m) * g.G + c.o] = (c.in_x && c.in_y) ? e[NL + m] : 0.0;
    v[((long)1 * NL + m) * g.G + c.o] = c.in_y ? e[2 * NL + m] : 0.0;
  }
}
// z = sc * Dinv r at the corner's three edges (local-edge order), zero where the edge does not exist
// The interior variant (both cells present) is applied to every lane through WAVE-UNIFORM table pointers (scalar loads);
// the few lanes on the mesh boundary redo their edge with the one-cell variant.  (With the variant chosen per lane every
// table entry became a vector load: 27 per application and corner.)  r holds zeros where an edge does not exist.
template <int NL>
__device__ __forceinline__ void corner_dinv(const DevTables& T, const CornerInfo& c, double sc, const double* r, double* z) {
#pragma unroll
  for (int q = 0; q < 3 * NL; q++) z[q] = 0.0;
  mv_acc_ld<NL, NL>(T.trDinv[0][0], NL, r, z, sc);
  mv_acc_ld<NL, NL>(T.trDinv[2][0], NL, r + NL, z + NL, sc);
  mv_acc_ld<NL, NL>(T.trDinv[1][0], NL, r + 2 * NL, z + 2 * NL, sc);
  if (c.vH != 0) {
#pragma unroll
    for (int q = 0; q < NL; q++) z[q] = 0.0;
    mv_acc_ld<NL, NL>(T.trDinv[0][c.vH], NL, r, z, sc);
  }
  if (c.vV != 0) {
#pragma unroll
    for (int q = 0; q < NL; q++) z[2 * NL + q] = 0.0;
    mv_acc_ld<NL, NL>(T.trDinv[1][c.vV], NL, r + 2 * NL, z + 2 * NL, sc);
  }
}
// LDS slot of local-edge entry q (0..NT-1: H modes, D modes, V modes) in plane order (H = 0, V = 1, D = 2)
template <int NL>
__device__ __forceinline__ int plane_of(int q) { return q < NL ? q : (q < 2 * NL ? 2 * NL + (q - NL) : NL + (q - 2 * NL)); }

template <int K>
__global__ __launch_bounds__(TraceTile<K>::NTHREADS) void k_trace_pre_tile(int ntx, int nty, Geo g, TileRows tr, DevTables T, const double* __restrict__ r, double c0, double c1,
                                                         double c2, double* __restrict__ z_out, double* __restrict__ res_out) {
  typedef TraceTile<K> TT;
  constexpr int NL = TT::NL, NT = TT::NT, TW = TT::TW, TH = TT::TH, W2 = TT::W2, H2 = TT::H2, W1 = TT::W1, H1 = TT::H1, KMAX = TT::KMAX;
  __shared__ double Ds[NT * TT::N2];  // d0 on the halo-2 region
  __shared__ double Zs[NT * TT::N1];  // z on the halo-1 region
  HDG_TILE_OF_BLOCK
  const int i0 = tile_x * TW, j0 = tr.jlo + tile_y * TH;
  double rr[KMAX][NT], dd[KMAX][NT];
  // stage 1: d0 = c0 Dinv r on the halo-2 region (pointwise); r and d0 of this thread's corners stay in registers (d0 taken
  // from the stencil's own[] as in the post kernel stops short of the five-wave step and is no faster: DESIGN.md section 9)
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      const int jc = j0 - 2 + lj;
      const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
      load_corner<NL>(r, g, c, rr[k]);
      corner_dinv<NL>(T, c, c0, rr[k], dd[k]);
#pragma unroll
      for (int q = 0; q < NT; q++) Ds[(plane_of<NL>(q) * H2 + lj) * W2 + li] = dd[k][q];
    }
  }
  __syncthreads();
  // stage 2 on the halo-1 region: z = d0 + c1 d0 + c2 Dinv (r - T d0)
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      if (li >= 1 && li < W2 - 1 && lj >= 1 && lj < H2 - 1) {
        const int jc = j0 - 2 + lj;
        const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
        double z[NT];
#pragma unroll
        for (int q = 0; q < NT; q++) z[q] = 0.0;
        if (c.exists) {
          double own[NT], y[3][NL], r1[NT], zz[NT];
          lds_trace_stencil<K, W2, H2>(Ds, li, lj, c.in_x, c.in_y, c.below, c.left, T, own, y[0], y[1], y[2]);
#pragma unroll
          for (int m = 0; m < NL; m++) {  // y[0] = H, y[1] = V, y[2] = D; local-edge order is H, D, V
            r1[m] = rr[k][m] - y[0][m];
            r1[NL + m] = rr[k][NL + m] - y[2][m];
            r1[2 * NL + m] = rr[k][2 * NL + m] - y[1][m];
          }
          corner_dinv<NL>(T, c, c2, r1, zz);
#pragma unroll
          for (int q = 0; q < NT; q++) z[q] = dd[k][q] + fma(c1, dd[k][q], zz[q]);
        }
#pragma unroll
        for (int q = 0; q < NT; q++) Zs[(plane_of<NL>(q) * H1 + (lj - 1)) * W1 + (li - 1)] = z[q];
        if (c.exists && c.own_x && li >= 2 && li < W2 - 2 && lj >= 2 && lj < H2 - 2 && jc < tr.jhi) store_corner<NL>(z_out, g, c, z);
      }
    }
  }
  __syncthreads();
  // stage 3 on the tile: res = r - T z
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      if (li >= 2 && li < W2 - 2 && lj >= 2 && lj < H2 - 2) {
        const int jc = j0 - 2 + lj;
        const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
        if (c.exists && c.own_x && jc < tr.jhi) {
          double own[NT], y[3][NL], res[NT];
          lds_trace_stencil<K, W1, H1>(Zs, li - 1, lj - 1, c.in_x, c.in_y, c.below, c.left, T, own, y[0], y[1], y[2]);
#pragma unroll
          for (int m = 0; m < NL; m++) {
            res[m] = rr[k][m] - y[0][m];
            res[NL + m] = rr[k][NL + m] - y[2][m];
            res[2 * NL + m] = rr[k][2 * NL + m] - y[1][m];
          }
          store_corner<NL>(res_out, g, c, res);
        }
      }
    }
  }
}

template <int K, bool DOTS>
__global__ __launch_bounds__(TraceTile<K>::NTHREADS) __attribute__((amdgpu_waves_per_eu(TraceTile<K>::WPE_POST))) void k_trace_post_tile(int ntx, int nty, Geo g, TileRows tr, DevTables T, const double* __restrict__ z_in, const double* __restrict__ r,
                                                          const double* __restrict__ xc, double sH, double sV, double sD, double c0,
                                                          double c1, double c2, double* __restrict__ z_out, double* __restrict__ w_out,
                                                          double* __restrict__ part) {
  typedef TraceTile<K> TT;
  constexpr int NL = TT::NL, NT = TT::NT, TW = TT::TW, TH = TT::TH, W2 = TT::W2, H2 = TT::H2, W3 = TT::W3, H3 = TT::H3, KMAX = TT::KMAX;
  __shared__ double Zs[NT * TT::N3];  // z0 on the halo-3 region; later z2 on its halo-1 part
  __shared__ double Ds[NT * TT::N2];  // d0 on the halo-2 region
  HDG_TILE_OF_BLOCK
  const int i0 = tile_x * TW, j0 = tr.jlo + tile_y * TH;
  const int st = g.nx + 1;
  // stage 0: z0 = z + P xc on the halo-3 region (pointwise; zero outside the mesh)
  for (int idx = threadIdx.x; idx < TT::N3; idx += TT::NTHREADS) {
    const int lj = idx / W3, li = idx - lj * W3;
    const int i = i0 - 3 + li, j = j0 - 3 + lj;
    const CornerInfo c = corner_info(g, tr, i, j);
    double z[NT];
    load_corner<NL>(z_in, g, c, z);
    if (c.exists && g.px) {
      // periodic vertex grid: nx x nx vertices (square mesh), both indices wrap (j, i within 3 of the strip; global row pj0 + j)
      const int n = g.nx, m = g.nx, jg = g.pj0 + j;
      const int iw = i < 0 ? i + n : (i >= n ? i - n : i), i1 = iw + 1 == n ? 0 : iw + 1;
      const int jw = jg < 0 ? jg + m : (jg >= m ? jg - m : jg), j1 = jw + 1 == m ? 0 : jw + 1;
      const double v00 = xc[(long)jw * n + iw], v10 = xc[(long)jw * n + i1], v01 = xc[(long)j1 * n + iw];
      edge_prolong(v00, v10, sH, z);
      if (c.in_y) edge_prolong(v10, v01, sD, z + NL);
      if (c.in_y) edge_prolong(v00, v01, sV, z + 2 * NL);
    } else if (c.exists) {
      const long J = g.joff + j;  // xc is the global (replicated) vertex vector
      const double v00 = xc[J * st + i];
      const double v10 = c.in_x ? xc[J * st + i + 1] : 0.0, v01 = c.in_y ? xc[(J + 1) * st + i] : 0.0;
      if (c.in_x) edge_prolong(v00, v10, sH, z);
      if (c.in_x && c.in_y) edge_prolong(v10, v01, sD, z + NL);
      if (c.in_y) edge_prolong(v00, v01, sV, z + 2 * NL);
    }
#pragma unroll
    for (int q = 0; q < NT; q++) Zs[(plane_of<NL>(q) * H3 + lj) * W3 + li] = z[q];
  }
  // r of this thread's stage-1 corners: requested BEFORE the barrier, so that the loads travel together with those of stage 0
  // (the compiler does not move a load across s_barrier; behind it the round trip was exposed once more per workgroup)
  double r0[KMAX][NT];
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    const int lj = idx / W2, li = idx - lj * W2;
    CornerInfo c = corner_info(g, tr, i0 - 2 + li, j0 - 2 + lj);
    if (idx >= TT::N2) c.in_x = c.in_y = false;
    load_corner<NL>(r, g, c, r0[k]);
  }
  __syncthreads();
  double dots[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // (z,n), (z,r), (z,z), (z,w), (n,r) of this thread's tile corners
  // stage 1 on the halo-2 region: r0 = r - T z0, d0 = c0 Dinv r0 (to Ds only; z1 = z0 + d0 is formed in stage 2)
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      const int jc = j0 - 2 + lj;
      const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
      double d0[NT];
#pragma unroll
      for (int q = 0; q < NT; q++) d0[q] = 0.0;  // (r0 holds r: zeros where the corner or an edge does not exist)
      if (c.exists) {
        double own[NT], y[3][NL];
        lds_trace_stencil<K, W3, H3>(Zs, li + 1, lj + 1, c.in_x, c.in_y, c.below, c.left, T, own, y[0], y[1], y[2]);
#pragma unroll
        for (int m = 0; m < NL; m++) {
          r0[k][m] -= y[0][m];
          r0[k][NL + m] -= y[2][m];
          r0[k][2 * NL + m] -= y[1][m];
        }
        corner_dinv<NL>(T, c, c0, r0[k], d0);
      }
#pragma unroll
      for (int q = 0; q < NT; q++) Ds[(plane_of<NL>(q) * H2 + lj) * W2 + li] = d0[q];
    }
  }
  __syncthreads();
  // stage 2 on the halo-1 region: z1 = z0 + d0, r1 = r0 - T d0, d1 = c1 d0 + c2 Dinv r1, z2 = z1 + d1 (stored over z0, which is
  // dead).  d0 of the corner is own[] of the Ds stencil and z0 the corner's own slot of Zs, which only this thread writes
  // in this stage and no thread reads before the next barrier.  An entry of an edge that does not exist is +0.0 in both
  // arrays: stage 0 stores the zero load_corner gives and prolongs onto existing edges only, and corner_dinv maps the zero
  // of r0 there to +0.0 (Dinv is block diagonal over the edges) -- the same values the masks of the stencil give.
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      if (li >= 1 && li < W2 - 1 && lj >= 1 && lj < H2 - 1) {
        const int jc = j0 - 2 + lj;
        const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
        double z2[NT];
#pragma unroll
        for (int q = 0; q < NT; q++) z2[q] = 0.0;
        if (c.exists) {
          double own[NT], y[3][NL], r1[NT], zz[NT];
          lds_trace_stencil<K, W2, H2>(Ds, li, lj, c.in_x, c.in_y, c.below, c.left, T, own, y[0], y[1], y[2]);
#pragma unroll
          for (int m = 0; m < NL; m++) {
            r1[m] = r0[k][m] - y[0][m];
            r1[NL + m] = r0[k][NL + m] - y[2][m];
            r1[2 * NL + m] = r0[k][2 * NL + m] - y[1][m];
          }
          corner_dinv<NL>(T, c, c2, r1, zz);
#pragma unroll
          for (int q = 0; q < NT; q++) {
            const double z1 = Zs[(plane_of<NL>(q) * H3 + (lj + 1)) * W3 + (li + 1)] + own[q];
            z2[q] = z1 + fma(c1, own[q], zz[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < NT; q++) Zs[(plane_of<NL>(q) * H3 + (lj + 1)) * W3 + (li + 1)] = z2[q];
        if (c.exists && c.own_x && li >= 2 && li < W2 - 2 && lj >= 2 && lj < H2 - 2 && jc < tr.jhi) store_corner<NL>(z_out, g, c, z2);
      }
    }
  }
  if (!w_out) return;  // uniform
  // r of the tile corners for the inner products: requested before the barrier as well (r0, z1, d0 are dead)
  double rr3[KMAX][NT];
  if (DOTS) {
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      const int idx = threadIdx.x + k * TT::NTHREADS;
      const int lj = idx / W2, li = idx - lj * W2;
      const int jc = j0 - 2 + lj;
      CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
      if (!(idx < TT::N2 && li >= 2 && li < W2 - 2 && lj >= 2 && lj < H2 - 2 && c.exists && c.own_x && jc < tr.jhi)) c.in_x = c.in_y = false;
      load_corner<NL>(r, g, c, rr3[k]);
    }
  }
  __syncthreads();
  // stage 3 on the tile: w = T z2
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    const int idx = threadIdx.x + k * TT::NTHREADS;
    if (idx < TT::N2) {
      const int lj = idx / W2, li = idx - lj * W2;
      if (li >= 2 && li < W2 - 2 && lj >= 2 && lj < H2 - 2) {
        const int jc = j0 - 2 + lj;
        const CornerInfo c = corner_info(g, tr, i0 - 2 + li, jc);
        if (c.exists && c.own_x && jc < tr.jhi) {
          double own[NT], y[3][NL], w[NT];
          lds_trace_stencil<K, W3, H3>(Zs, li + 1, lj + 1, c.in_x, c.in_y, c.below, c.left, T, own, y[0], y[1], y[2]);
#pragma unroll
          for (int m = 0; m < NL; m++) { w[m] = y[0][m]; w[NL + m] = y[2][m]; w[2 * NL + m] = y[1][m]; }
          store_corner<NL>(w_out, g, c, w);
          if (DOTS) {
            // the five inner products of the single-reduction CG from what is in registers (+ r of this corner): the
            // separate multi-dot pass over z, n, r, w is not needed.  The null vector n (the constant) has the entry
            // sqrt(edge length) in mode 0 of every edge that exists and zeros elsewhere -- what edge_prolong gives for
            // vertex values 1; entries of edges that do not exist are zero in z and r.
            const double* rr = rr3[k];
            dots[0] += sH * own[0] + sD * own[NL] + sV * own[2 * NL];  // own = z2 of this corner (from LDS)
            dots[4] += sH * rr[0] + sD * rr[NL] + sV * rr[2 * NL];
#pragma unroll
            for (int q = 0; q < NT; q++) {
              const double zq = own[q];
              dots[1] = fma(zq, rr[q], dots[1]);
              dots[2] = fma(zq, zq, dots[2]);
              dots[3] = fma(zq, w[q], dots[3]);
            }
          }
        }
      }
    }
  }
  if (DOTS) {  // deterministic two-stage reduction (per workgroup here, k_reduce_parts over the workgroups)
    __shared__ double sm[TT::NTHREADS / 64][5];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; q++) {
      const double sv = wave_sum(dots[q]);
      if (lane == 0) sm[wv][q] = sv;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
      double sv = 0.0;
      for (int w2 = 0; w2 < TT::NTHREADS / 64; w2++) sv += sm[w2][threadIdx.x];
      part[(long)threadIdx.x * (ntx * nty) + tile_v] = sv;  // [inner product][tile]
    }
  }
}

}  // namespace hdg
