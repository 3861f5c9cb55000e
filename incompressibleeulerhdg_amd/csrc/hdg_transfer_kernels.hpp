// Device side of the transfer between two engines on nested structured meshes (hdg_transfer.hpp has the host tables and the
// conventions).  One thread per cell of the mesh the launch runs on, laid out by that engine's cell grid
// (HDG_CELL_PROLOGUE: owned rows only, so ghost and padding rows are left to the later exchanges as put_Q / put_P leave them).
// The other engine's cell is found by integer arithmetic and gathered from its planes.
//
// Table operand: T[(class * LDC + m) * LDF + n], the velocity table of the pair of degrees (coarse modes m, fine modes n); the
// scalar fields read its leading block.  The class differs from lane to lane, so the table is read with vector loads (r^2
// blocks of at most 21 x 21 doubles: they stay in L2); the accumulators are the only per-thread array, indexed statically.
// Every kernel is templated on the degrees of the coarse-mesh and the fine-mesh field and on VEL (velocity pair planes of
// P_{k+1}, or scalar planes of P_k; fields of one launch are grid.y apart by a stride).
#pragma once
#include "hdg_kernels.hpp"

namespace hdg {

template <int K, bool VEL> struct XferModes { static constexpr int N = VEL ? Dim<K>::NU : Dim<K>::NP; };

// class of fine cell (a, b, s) of a coarse square in a parent of shape S (transfer::child_class)
__device__ __forceinline__ int xfer_class(int r, int S, int a, int b, int s) {
  const int a1 = S ? r - 1 - a : a, b1 = S ? r - 1 - b : b;
  return s == S ? b1 * r + a1 : (r - 1 - b1) * r + (r - 1 - a1);
}
__device__ __forceinline__ int xfer_parent_shape(int r, int a, int b, int s) { return a + b <= r - 1 - s ? 0 : 1; }

template <bool VEL> struct XferVal;
template <> struct XferVal<true> {
  typedef hdg_d2 T;
  static __device__ __forceinline__ T ld(const double* v, long Nc, int m, long c) { return reinterpret_cast<const hdg_d2*>(v)[(long)m * Nc + c]; }
  static __device__ __forceinline__ void st(double* v, long Nc, int m, long c, T x) { reinterpret_cast<hdg_d2*>(v)[(long)m * Nc + c] = x; }
  static __device__ __forceinline__ T zero() { return hdg_d2{0.0, 0.0}; }
  static __device__ __forceinline__ double sq(T x) { return x.x * x.x + x.y * x.y; }
};
template <> struct XferVal<false> {
  typedef double T;
  static __device__ __forceinline__ T ld(const double* v, long Nc, int m, long c) { return v[(long)m * Nc + c]; }
  static __device__ __forceinline__ void st(double* v, long Nc, int m, long c, T x) { v[(long)m * Nc + c] = x; }
  static __device__ __forceinline__ T zero() { return 0.0; }
  static __device__ __forceinline__ double sq(T x) { return x * x; }
};

// prolongation (g: the destination, finer or equal mesh; gs: the source):  a_f = (1 / r) C^T a_c
template <int KS, int KD, bool VEL>
__global__ void k_xfer_prolong(Geo g, Geo gs, int r, const double* __restrict__ T, const double* __restrict__ src, long sstride,
                               double* __restrict__ dst, long dstride) {
  typedef XferVal<VEL> V;
  constexpr int NS = XferModes<KS, VEL>::N, ND = XferModes<KD, VEL>::N, LDC = Dim<KS>::NU, LDF = Dim<KD>::NU;
  HDG_CELL_PROLOGUE
  src += (long)blockIdx.y * sstride;
  dst += (long)blockIdx.y * dstride;
  const int I = i / r, J = j / r, a = i - I * r, b = j - J * r;
  const int S = xfer_parent_shape(r, a, b, s);
  const double* Tc = T + (long)xfer_class(r, S, a, b, s) * (LDC * LDF);
  const long cs = rowbase(gs, S, J) + I;
  typename V::T acc[ND];
#pragma unroll
  for (int n = 0; n < ND; n++) acc[n] = V::zero();
#pragma unroll 1
  for (int m = 0; m < NS; m++) {
    const typename V::T am = V::ld(src, gs.Nc, m, cs);
#pragma unroll
    for (int n = 0; n < ND; n++) acc[n] += Tc[m * LDF + n] * am;
  }
  const double rinv = 1.0 / r;
#pragma unroll
  for (int n = 0; n < ND; n++) V::st(dst, g.Nc, n, c, acc[n] * rinv);
}

// restriction (g: the destination, coarser mesh; gs: the source):  a_c = (1 / r) sum_children C a_f
template <int KS, int KD, bool VEL>
__global__ void k_xfer_restrict(Geo g, Geo gs, int r, const double* __restrict__ T, const double* __restrict__ src, long sstride,
                                double* __restrict__ dst, long dstride) {
  typedef XferVal<VEL> V;
  constexpr int NS = XferModes<KS, VEL>::N, ND = XferModes<KD, VEL>::N, LDC = Dim<KD>::NU, LDF = Dim<KS>::NU;
  HDG_CELL_PROLOGUE
  src += (long)blockIdx.y * sstride;
  dst += (long)blockIdx.y * dstride;
  typename V::T acc[ND];
#pragma unroll
  for (int m = 0; m < ND; m++) acc[m] = V::zero();
#pragma unroll 1
  for (int b = 0; b < r; b++)
#pragma unroll 1
    for (int a = 0; a < r; a++)
#pragma unroll 1
      for (int sf = 0; sf < 2; sf++) {
        if (xfer_parent_shape(r, a, b, sf) != s) continue;
        const double* Tc = T + (long)xfer_class(r, s, a, b, sf) * (LDC * LDF);
        const long cf = rowbase(gs, sf, j * r + b) + (i * r + a);
#pragma unroll 1
        for (int n = 0; n < NS; n++) {
          const typename V::T af = V::ld(src, gs.Nc, n, cf);
#pragma unroll
          for (int m = 0; m < ND; m++) acc[m] += Tc[m * LDF + n] * af;
        }
      }
  const double rinv = 1.0 / r;
#pragma unroll
  for (int m = 0; m < ND; m++) V::st(dst, g.Nc, m, c, acc[m] * rinv);
}

// squared L2 norm of the difference per cell of the finer mesh (g; gc: the coarser or equal mesh): both fields in degree
// max(KC, KF) on the fine cell -- the coarse-mesh field through the table (exact injection), the fine-mesh field zero-padded --
// and the squares of the modal coefficients of the difference summed (orthonormal basis).  out: one value per cell, in the
// layout of a scalar plane; the engine's dot against the ones vector sums the owned cells.
template <int KC, int KF, bool VEL>
__global__ void k_xfer_diff(Geo g, Geo gc, int r, const double* __restrict__ T, const double* __restrict__ coarse,
                            const double* __restrict__ fine, double* __restrict__ out) {
  typedef XferVal<VEL> V;
  constexpr int KM = KC > KF ? KC : KF;
  constexpr int NC = XferModes<KC, VEL>::N, NF = XferModes<KF, VEL>::N, NM = XferModes<KM, VEL>::N, LDF = Dim<KM>::NU, LDC = Dim<KC>::NU;
  HDG_CELL_PROLOGUE
  const int I = i / r, J = j / r, a = i - I * r, b = j - J * r;
  const int S = xfer_parent_shape(r, a, b, s);
  const double* Tc = T + (long)xfer_class(r, S, a, b, s) * (LDC * LDF);
  const long cc = rowbase(gc, S, J) + I;
  typename V::T acc[NM];
#pragma unroll
  for (int n = 0; n < NM; n++) acc[n] = V::zero();
#pragma unroll 1
  for (int m = 0; m < NC; m++) {
    const typename V::T am = V::ld(coarse, gc.Nc, m, cc);
#pragma unroll
    for (int n = 0; n < NM; n++) acc[n] += Tc[m * LDF + n] * am;
  }
  const double rinv = 1.0 / r;
  double ss = 0.0;
#pragma unroll
  for (int n = 0; n < NM; n++) {
    typename V::T d = acc[n] * rinv;
    if (n < NF) d -= V::ld(fine, g.Nc, n, c);
    ss += V::sq(d);
  }
  out[c] = ss;
}

}  // namespace hdg
