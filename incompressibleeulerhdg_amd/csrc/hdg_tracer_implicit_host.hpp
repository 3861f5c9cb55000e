// Implicit tracer diffusion: the per-tracer scalars of the conjugate-gradient solve and the rule that
// advances them, shared by host and device.  Plain C++ outside HIP (__host__ / __device__ are defined away), so that a host
// check compiles it with g++.  The layout and the states are described in hdg_tracer_implicit.hpp.
#pragma once
#include <cmath>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace hdg {

constexpr int TDI_NSC = 8;
enum { TDI_RR = 0, TDI_ALPHA, TDI_BETA, TDI_BB, TDI_ITS, TDI_STATE, TDI_RES };
enum { TDI_ITERATING = 0, TDI_CONVERGED, TDI_OUT_OF_ITERATIONS, TDI_BROKE_DOWN, TDI_IDLE };

// The scalar rule of one tracer, on the sums of an iteration (k_tdi_scalars applies it on the device,
// tests/host/tracer_implicit_scalars_check.cpp on the host).  rr = (r, r) of the current residual, rw = (r, A r); first: the
// first iteration of a solve, bb = (b, b) arrives with it; last: no iteration follows (the check after max_iterations
// updates), rw is not read.
__host__ __device__ inline void tdi_scalar_rule(double* st, double rr, double rw, double bb, bool first, bool last, double rtol2) {
  if (st[TDI_STATE] != (double)TDI_ITERATING) return;
  if (first) { st[TDI_BB] = bb; st[TDI_ITS] = 0.0; }
  const double b2 = st[TDI_BB];
  st[TDI_RES] = b2 > 0.0 ? sqrt(rr / b2) : (rr == 0.0 ? 0.0 : rr);
  if (!(rr == rr)) { st[TDI_STATE] = (double)TDI_BROKE_DOWN; return; }
  if (rr <= rtol2 * b2) { st[TDI_STATE] = (double)TDI_CONVERGED; return; }
  if (last) { st[TDI_STATE] = (double)TDI_OUT_OF_ITERATIONS; return; }
  const double beta = first ? 0.0 : rr / st[TDI_RR];
  const double curv = first ? rw : rw - beta * rr / st[TDI_ALPHA];  // (p, A p) of the direction that the update will form
  if (!(curv > 0.0)) { st[TDI_STATE] = (double)TDI_BROKE_DOWN; return; }
  st[TDI_BETA] = beta;
  st[TDI_ALPHA] = rr / curv;
  st[TDI_RR] = rr;
  st[TDI_ITS] += 1.0;
}

}  // namespace hdg
