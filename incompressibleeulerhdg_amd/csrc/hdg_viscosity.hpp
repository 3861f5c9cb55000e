// Viscous term: out = nu M^-1 V u, the symmetric interior-penalty form on [DG_{k+1}]^2 with Nitsche walls,
// in the orthonormal modal basis, on the structured meshes.  Every wall there is axis-aligned, so the two components decouple
// and M^-1 V is nine scalar NU x NU blocks per element shape (hdg_tables.hpp, ViscosityTables::packed: Vol, Own[0..2], Nbr[0..2],
// Wall[0], Wall[2], each transposed).  The shape is uniform over a workgroup, so the blocks arrive through scalar loads.
//
// A cell's row is  Vol u_K + sum_{e with a neighbour} (Own[e] u_K + Nbr[e] u_K') + sum_{wall e} Wall[e] (u_K restricted to the
// wall's normal component; to both components with no slip).  Registers: the accumulator of both components (NU pairs) stays
// live, every operand -- the cell itself, once per block, and each neighbour -- is streamed mode by mode as one 16-byte load of
// the component pair, so NU = 21 at k = 4 costs 42 accumulator doubles, not the 126 doubles of cell + neighbour + accumulator.
// The mode loop is a loop (not unrolled), the row loop is unrolled: the accumulator is never indexed dynamically.
// Which blocks a cell takes depends on the lane (the cells at a wall), but every branch around a block is taken by the whole
// wave (a ballot) and a lane the block does not concern contributes an operand of zero: with branches that diverge inside a
// wave the compiler kept a second copy of the accumulator (174 VGPRs at k = 4 against 92).  An interior wave runs seven
// blocks, a wave that touches a wall nine; a neighbour is read only where there is one.
// No LDS, no scratch.  Owned rows only; the caller has filled the ghost rows of u (Engine::stencil_in).
//
// Moving no-slip walls: MOVING = true runs instead of the plain kernel while a wall speed is set.  The
// tangential Nitsche term then acts on u.t - U_w, which adds U_w lvec[s][e] (ViscosityTables::packed_moving: four vectors behind
// the nine blocks) to the tangential component of a cell at a wall, inside the wall branch and before the scaling by nu.  The
// side w follows from (s, e), both uniform over a workgroup, so the speed is a scalar select among the four kernel arguments.
#pragma once
#include <hip/hip_runtime.h>

namespace hdg {

struct WallSpeed { double bottom, right, top, left; };  // the Cartesian tangential speed of every side, in the order of the C-ABI

template <int K, bool MOVING>
__global__ __launch_bounds__(128) void k_viscosity(Geo g, const double* __restrict__ tab, double nu, int no_slip,
                                                   const double* __restrict__ u, double* __restrict__ out, WallSpeed W) {
  constexpr int NU = Dim<K>::NU, BL = NU * NU;
  HDG_CELL_PROLOGUE
  const double* __restrict__ T = tab + (long)s * 9 * BL;
  const VelBuf U(u), O(out);
  const unsigned lane_b = (unsigned)c * 16u;
  hdg_d2 F[NU];
#pragma unroll
  for (int r = 0; r < NU; r++) F[r] = hdg_d2{0.0, 0.0};
  // F += A x, A one transposed block, x the cell at lane offset lb where the lane's predicate holds for the component, else 0
  auto apply = [&](const double* __restrict__ A, unsigned lb, bool px, bool py) {
#pragma unroll 1
    for (int m = 0; m < NU; m++) {
      hdg_d2 x = U.ld(pair_bytes(m, g.Nc), lb);
      x.x = px ? x.x : 0.0;
      x.y = py ? x.y : 0.0;
      const double* __restrict__ col = A + m * NU;
#pragma unroll
      for (int r = 0; r < NU; r++) {
        const double a = col[r];
        F[r].x = fma(a, x.x, F[r].x);
        F[r].y = fma(a, x.y, F[r].y);
      }
    }
  };
  apply(T, lane_b, true, true);
  // the branches are uniform over a wave (ballots): an interior wave runs seven blocks, a wave that touches a wall nine
#pragma unroll
  for (int e = 0; e < 3; e++) {
    long cn;
    const bool has = nbr(s, e, i, j, g, cn);
    if (__builtin_amdgcn_ballot_w64(has) != 0) {
      apply(T + (1 + e) * BL, lane_b, has, has);
      apply(T + (4 + e) * BL, has ? (unsigned)cn * 16u : lane_b, has, has);
    }
    if (e != 1 && __builtin_amdgcn_ballot_w64(!has) != 0) {  // a wall: horizontal (e = 0, normal along y) or vertical (e = 2, normal along x)
      apply(T + (e == 0 ? 7 : 8) * BL, lane_b, !has && (no_slip || e == 2), !has && (no_slip || e == 0));
      if constexpr (MOVING) {
        const double* __restrict__ lv = tab + 2 * 9 * BL + (2 * s + (e == 0 ? 0 : 1)) * NU;
        const double side_u = s == 0 ? (e == 0 ? W.bottom : W.left) : (e == 0 ? W.top : W.right);
        const double uw = (!has && no_slip) ? side_u : 0.0;
#pragma unroll
        for (int r = 0; r < NU; r++) {
          if (e == 0) F[r].x = fma(uw, lv[r], F[r].x);
          else F[r].y = fma(uw, lv[r], F[r].y);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NU; r++) O.st(pair_bytes(r, g.Nc), lane_b, hdg_d2{nu * F[r].x, nu * F[r].y});
}

}  // namespace hdg
