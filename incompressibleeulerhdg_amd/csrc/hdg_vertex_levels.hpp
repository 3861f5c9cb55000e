// The level plan of the P1 vertex-grid V-cycle (coarse solve of the condensed-trace preconditioner on the structured
// square): the hierarchy of grids and, for every level, the ONE form it runs as.  Host only (plain C++, no HIP):
// tests/host/vertex_levels_check.cpp compiles it with g++ and states the plan of a dozen meshes as literal values.
//
// The engine builds the plan once (Engine::setup_trace_solver); the V-cycle, the builder of the dense tail, the
// distributed finest level of a strip partition and the side-job weights of the condensed CG read it and decide nothing
// themselves.  The kernels of every form are in hdg_vertex_mg.hpp.
#pragma once
#include <vector>

#include "hdg_options.hpp"

// doubles of x and of b a workgroup of the one-workgroup tail holds in LDS (k_p1_vcycle_tail): every level of the tail
#define HDG_P1_TAIL_MAX 1600
// smoothing sweeps the fused legs are built for (k_p1_down<NSW> / k_p1_up<NSW>: the halo of a tile grows with them)
#define HDG_P1_MAXSW 3

namespace hdg {

enum class VForm {
  Legs,        // one kernel per leg: LDS tiles with recomputed halos (k_p1_down / k_p1_up)
  PerLevel,    // one launch per half sweep, residual, restriction, prolongation
  TailKernel,  // this level and every coarser one in one workgroup (k_p1_vcycle_tail)
  DenseTail,   // the same linear map as one dense matrix (k_p1_dense_tail)
  Coarsest     // the last level: 2 * mg_coarse sweeps by per-level launches
};

struct VLevel {
  int n;      // cells per side
  long nv;    // vertices: (n + 1)^2, periodic n^2
  int pitch;  // row pitch: n + 1, periodic n
  VForm form;
};

struct VertexPlan {
  bool periodic = false;
  std::vector<VLevel> lev;
  int dense_lev = -1;  // level at which the dense tail is built and applied (-1: none)
  int tail_nlev = 0;   // levels a tail of either kind covers (it always reaches the coarsest; they carry the tail's form)

  int size() const { return (int)lev.size(); }
  long tail_vertices() const {
    long tot = 0;
    for (int l = size() - tail_nlev; l < size(); l++) tot += lev[l].nv;
    return tot;
  }
  // Side jobs of the condensed CG (the p / x half of its update rides on the leg launches, Engine::XpRide): every leg of a
  // Legs level from `first` on takes a share of the pairs in proportion to its weight, the finest level's legs w0, the
  // others 1.  Each pair is computed independently by the same expression whichever launch takes it, so the weights move
  // work between launches and never a value; what no leg takes is done by a launch of its own.
  static double side_weight(int l, double w0) { return l == 0 ? w0 : 1.0; }
  double side_weight_sum(int first, double w0) const {
    double s = 0.0;
    for (int l = first; l < size(); l++)
      if (lev[l].form == VForm::Legs) s += 2.0 * side_weight(l, w0);
    return s;
  }
};

inline VertexPlan vertex_plan(int nx, bool periodic, const Options& o) {
  VertexPlan p;
  p.periodic = periodic;
  for (int n = nx;; n /= 2) {
    p.lev.push_back(VLevel{n, periodic ? (long)n * n : (long)(n + 1) * (n + 1), periodic ? n : n + 1, VForm::PerLevel});
    if (n % 2 != 0 || n <= 2 || (periodic && (n / 2) % 2 != 0)) break;  // periodic red-black sweeps need an even n
  }
  const int L = p.size();
  auto tail_from = [&](int l, VForm f) {
    for (int m = l; m < L; m++) p.lev[m].form = f;
    p.tail_nlev = L - l;
    if (f == VForm::DenseTail) p.dense_lev = l;
  };
  if (periodic) {
    int t = 0;  // the first level with n <= 32: the dense tail needs a level above it (something fused) and two levels
    while (t < L && p.lev[t].n > 32) t++;
    const bool dense = o.mg_dense_tail_periodic && t != 0 && L - t >= 2 && p.lev[t].n * p.lev[t].n <= 1024;
    for (int l = 0; l < L; l++) {
      VLevel& v = p.lev[l];
      if (dense && l == t) { tail_from(l, VForm::DenseTail); break; }
      if (o.mg_fuse && o.mg_sweeps == 2 && v.n > 32 && l + 1 < L) v.form = VForm::Legs;
      else v.form = l == L - 1 ? VForm::Coarsest : VForm::PerLevel;
    }
    return p;
  }
  for (int l = 0; l < L; l++) {
    VLevel& v = p.lev[l];
    long tot = 0;
    for (int m = l; m < L; m++) tot += p.lev[m].nv;
    if (o.mg_tail && v.n <= 32 && L - l <= 8 && tot <= HDG_P1_TAIL_MAX) {
      tail_from(l, o.mg_dense_tail && L - l >= 2 ? VForm::DenseTail : VForm::TailKernel);
      break;
    }
    if (l == L - 1) v.form = VForm::Coarsest;
    else if (o.mg_fuse && o.mg_sweeps >= 1 && o.mg_sweeps <= HDG_P1_MAXSW && (v.n & 1) == 0) v.form = VForm::Legs;
    else v.form = VForm::PerLevel;
  }
  return p;
}

}  // namespace hdg
