// Lagrangian particles on the device (hdg_set_particles / hdg_get_particles / hdg_advance_particles).
//
// n positions X follow dX/dt = u(X, t), u the broken velocity of the engine's current state (the ux, uy of
// hdg_evaluate_points, with its ownership rule: square_locate of hdg_points.hpp, here run on the device every evaluation).
// Heun's method over each step of the flow solver:
//   k1 = u^n(X^n),  X* = X^n + dt k1,  k2 = u^{n+1}(X*),  X^{n+1} = X^n + dt/2 (k1 + k2)
// k1 and X* are formed as soon as X^n and u^n exist and live in per-particle buffers across the step, so no copy of the old
// velocity is kept.  One thread per particle; the pieces of a step are bits of `phase`, so that one rank runs the whole step
// (evaluate k2, correct, evaluate the next k1, predict) in one launch and a strip partition cuts it where the two all-reduce
// sums go.  A rank evaluates the particles whose owning cell row is its own and writes zeros for the rest (the geometry
// carries the rows it owns; one rank owns all of them): every entry of the sum has one non-zero contributor.
// nsteps > 1 repeats the step inside the launch on the same field: the frozen-field mode of hdg_advance_particles.
//
// Unit square: every coordinate is clamped to [0, L] after each of the two position updates (the broken velocity has
// u.n = 0 on the boundary only weakly) and the clamped updates are counted.  Periodic square: positions are not wrapped
// (displacements can be read off), location wraps.  A position that becomes non-finite is located nowhere, gets a NaN
// velocity, stays NaN and is counted as lost once; it reads no field entry.
#pragma once
#include <hip/hip_runtime.h>
#include "hdg_points.hpp"

namespace hdg {

constexpr int PARTICLE_BLOCK = 64;
// pieces of a step (bits of `phase`)
constexpr int PF_EVAL_STAR = 1;  // k2 = u(X*)                        (alone: written to the k2 buffer)
constexpr int PF_CORRECT = 2;    // X = clamp(X + dt/2 (k1 + k2))     (k2 from the buffer unless PF_EVAL_STAR), row <- X
constexpr int PF_EVAL_X = 4;     // k1 = u(X)                         (written to the k1 buffer)
constexpr int PF_PREDICT = 8;    // X* = clamp(X + dt k1)             (k1 from the buffer unless PF_EVAL_X)
constexpr int PF_STEP = PF_EVAL_STAR | PF_CORRECT | PF_EVAL_X | PF_PREDICT;
constexpr int PARTICLE_NCOUNT = 2;  // device counters: clamped updates, lost particles

struct ParticleGeo {
  int nx, ny;    // cells of the global mesh
  int j0, nyl;   // first cell row this rank owns and their number (one rank: 0, ny)
  int periodic;
  long R, Nc;    // rows of one shape's plane (ghost and padding rows included), stride of a coefficient plane
  double L, h;
};

// velocity at (x, y): the owner's value, zero for a cell row of another rank, NaN for a point located nowhere
template <int K>
__device__ __forceinline__ void particle_velocity(const ParticleGeo& G, const double* __restrict__ Q, double x, double y,
                                                  double& ux, double& uy) {
  constexpr int NU = Dim<K>::NU;
  int i, j, s;
  double xi, eta;
  if (!square_locate(x, y, G.nx, G.ny, G.L, G.periodic != 0, i, j, s, xi, eta)) {
    ux = uy = __builtin_nan("");
    return;
  }
  const int jl = j - G.j0;
  if (jl < 0 || jl >= G.nyl) { ux = uy = 0.0; return; }
  // plane layouts as k_point_eval reads them: cell rowbase(g, s, jl) + i, velocity pair planes of stride Nc; the basis is
  // 1 / h times the reference one; (xi, eta) of the upper shape are the rotated (1 - fx, 1 - fy) of square_locate
  const long c = ((long)s * G.R + (jl + GH)) * G.nx + i;
  double val[NU], gx[NU], gy[NU];
  dubiner_at<K + 1>(xi, eta, val, gx, gy);
  double ax = 0.0, ay = 0.0;
#pragma unroll
  for (int m = 0; m < NU; m++) {
    ax = fma(val[m], Q[(m * G.Nc + c) << 1], ax);
    ay = fma(val[m], Q[((m * G.Nc + c) << 1) + 1], ay);
  }
  const double sc = 1.0 / G.h;
  ux = sc * ax;
  uy = sc * ay;
}

// clamps onto [0, L]^2 (unit square only; NaN stays NaN); true when a coordinate moved
__device__ __forceinline__ bool particle_clamp(const ParticleGeo& G, double& x, double& y) {
  if (G.periodic) return false;
  bool moved = false;
  if (x < 0.0) { x = 0.0; moved = true; }
  if (x > G.L) { x = G.L; moved = true; }
  if (y < 0.0) { y = 0.0; moved = true; }
  if (y > G.L) { y = G.L; moved = true; }
  return moved;
}

template <int K>
__global__ __launch_bounds__(PARTICLE_BLOCK) void k_particles_step(ParticleGeo G, int n, int phase, int nsteps, double dt,
                                                                   const double* __restrict__ Q, double* __restrict__ X,
                                                                   double* __restrict__ Xs, double* __restrict__ k1,
                                                                   double* __restrict__ k2, double* __restrict__ row,
                                                                   unsigned long long* __restrict__ counts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const long o = 2L * t;
  double x = X[o], y = X[o + 1], xs = Xs[o], ys = Xs[o + 1], kx = k1[o], ky = k1[o + 1];
  double ax = 0.0, ay = 0.0;
  unsigned nclamp = 0, nlost = 0;
  for (int it = 0; it < nsteps; it++) {
    if (phase & PF_EVAL_STAR) particle_velocity<K>(G, Q, xs, ys, ax, ay);
    else if (phase & PF_CORRECT) { ax = k2[o]; ay = k2[o + 1]; }
    if (phase & PF_CORRECT) {
      const bool was = std::isfinite(x) && std::isfinite(y);
      double px = x + dt * kx, py = y + dt * ky;  // the predictor this update uses: counted here, once, when it is used
      if (particle_clamp(G, px, py)) nclamp++;
      x = x + 0.5 * dt * (kx + ax);
      y = y + 0.5 * dt * (ky + ay);
      if (particle_clamp(G, x, y)) nclamp++;
      if (was && !(std::isfinite(x) && std::isfinite(y))) {
        nlost++;
        x = y = __builtin_nan("");
      }
    }
    if (phase & PF_EVAL_X) particle_velocity<K>(G, Q, x, y, kx, ky);
    if (phase & PF_PREDICT) {
      xs = x + dt * kx;
      ys = y + dt * ky;
      particle_clamp(G, xs, ys);
    }
  }
  if ((phase & PF_EVAL_STAR) && !(phase & PF_CORRECT)) { k2[o] = ax; k2[o + 1] = ay; }
  if (phase & PF_CORRECT) {
    X[o] = x; X[o + 1] = y;
    if (row) { row[o] = x; row[o + 1] = y; }
  }
  if (phase & PF_EVAL_X) { k1[o] = kx; k1[o + 1] = ky; }
  if (phase & PF_PREDICT) { Xs[o] = xs; Xs[o + 1] = ys; }
  if (counts) {  // rare events: plain vector atomics
    if (nclamp) atomicAdd(&counts[0], (unsigned long long)nclamp);
    if (nlost) atomicAdd(&counts[1], (unsigned long long)nlost);
  }
}

}  // namespace hdg
