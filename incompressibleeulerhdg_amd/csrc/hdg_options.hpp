// Every HDG_* environment switch of the engine: one struct, one function that reads the environment, one lifetime.
// Host only (plain C++, no HIP): tests/host/options_check.cpp compiles it with g++.
//
// An Engine holds `const Options opt`, filled by options_from_env() when the engine is built; nothing else in csrc/ reads
// the environment.  A flag is set by the PRESENCE of its variable (any value, "0" included), a number by atoi / atof of it,
// a range by "lo:hi".  The default of every field is its member initialiser, the measured reason for it the comment beside
// it.  Variants that were measured and removed are recorded in DESIGN.md section 9, not here.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace hdg {

struct Options {
  // ---- general meshes
  bool general_csr_lift = false;      // assembled lift operators instead of the matrix-free k_g_lift
  bool general_block_jacobi = false;  // tentative velocity: element block-Jacobi alone instead of Pi + Dinv (I - Pi)
  bool general_gmres = false;         // tentative velocity: GMRES(30) instead of Chebyshev + s-step tail
  bool general_coarse = true;         // trace system: P1 coarse space with an algebraic V-cycle (off: edge block-Jacobi alone)
  // coarsening stops at <= 2000 vertices (round 3: 400), where the dense pseudo-inverse takes over: on the level-6 disk the
  // hierarchy is 16 641 -> 1 893 (dense) instead of -> 1 893 -> 149 (dense) -- one smoothed level (18 launches of ~5 us per
  // V-cycle) fewer for a 29 MB matrix-vector product
  int amg_max_coarse = 2000;
  bool amg_unfused = false;  // the six or seven launches of the algebraic smoother instead of the two of k_amg_cheb

  // ---- partition, layout, checks
  bool overlap = false;         // interior / boundary split of the stencil launches around the halo exchange
  bool force_rccl = false;      // the RCCL transport (and the gather buffers of a partition) on one rank as well
  int row_pad = -1;             // padding rows per dof plane (layout scans; 0 = none); < 0: by the memory-channel rule
  bool dbg_nonbr = false;       // Geo::dbg_nonbr (timing variant of the neighbour loads inside kernels)
  bool flow_check = false;      // verify the ghost-row depth bookkeeping against the data
  bool ext = true;              // operators compute on the ghost rows they can instead of exchanging their result
  bool direct_host = true;      // reductions land in pinned host memory directly (one rank)

  // ---- matrix-core kernels (k >= 3) and the kernel forms of lift and advection
  bool mfma_schur = true;       // off: the per-thread Schur kernels at every degree (A/B timing, parity of the two formulations)
  bool mfma_condense = false;   // the matrix-core form of the condensation as well
  bool mfma_lift = true;
  bool mfma_adv = true;
  bool lift_pair = true;        // k <= 2: both triangles of a square in one 128-thread workgroup
  // k = 3 without the matrix-core kernel: two lanes per cell, one velocity component each (k_adv_apply2).  Measured at
  // nx = 512, one-lane vs two-lane kernel: k=1 181 / 205 us (nx 1024), k=2 353 / 370 us (nx 1024), k=3 407 / 334 us,
  // k=4 719 / 1488 us (254 VGPRs, still 1 wave/SIMD, twice the waves)
  int adv_split_lo = 3, adv_split_hi = 3;

  // ---- tentative-velocity solver
  bool gmres_arnoldi = false;   // the Arnoldi form of GMRES for whole strict solves too (default: s-step cycles)
  bool tail_gmres = false;      // one GMRES(8) cycle as the tail of the Chebyshev iteration (default: s-step cycles)
  int sstep_max = 6;            // 28 inner products fit one reduction
  double sstep_per_decade = 1.7;  // iterations per decade + 1: GMRES's observed 5-6 for 3-4 decades
  // re-estimate period: 64 solves of a stage (round 3: 16).  The bounds of the preconditioned operator barely move between
  // time steps and a wrong interval is caught by the growth guard, which re-estimates at once; every estimate costs an
  // Arnoldi cycle and a re-learnt hand-over point (C3, 20 + 5 steps: 85.45 -> 82.71 ms/step, 15.55 -> 14.55 iterations)
  int cheb_every = 64;
  int cheb_m = 6;               // length of the opening Arnoldi cycle
  double cheb_flo = -1.0, cheb_fhi = -1.0;  // safety factors on the Ritz interval (< 0: by preconditioner and degree)
  double cheb_ell = -1.0;       // imaginary half-axis / real half-axis of the ellipse (< 0: by preconditioner and degree)
  int cheb_max_expected = 64;   // predicted Chebyshev iterations above which the solve goes to GMRES
  int cheb_fine_step = 2;       // distance of the convergence checks near the expected end
  double cheb_handover = -1.0;  // observed rate above which the tail takes over (< 0: by degree; 0: never)
  int cheb_min_k = 6;           // no hand-over before this iteration
  int cheb_hand_cycle = 8;      // the tail after a hand-over is 3-4 decades = 5-7 GMRES iterations: one cycle, no restart

  // ---- trace preconditioner
  bool trace_fuse = true;       // operator, edge block-Jacobi and Chebyshev update in one launch (k_trace_smooth)
  bool trace_fold = true;       // first smoother step and prolongation folded into the stencil launches that consume them
  int trace_smooth_its = 2;
  bool trace_tile = true;       // LDS-tiled form of the two smoother applications (off: five row-stencil launches)
  bool trace_tile_strips = true;    // ... on a strip partition too
  bool trace_tile_periodic = true;  // ... on the periodic square too
  // form of the tile kernels: one thread per edge (1) or one per corner (0); < 0: by degree.  Measured (pressure solve, ms;
  // corner form -> edge form): C3 6.24 -> 6.92, k = 3 at 512^2 3.16 -> 3.42, C2 1.03 -> 1.10 -- six instead of three waves
  // per SIMD buy nothing where the corner form fits; k = 4 at 512^2 (row-stencil kernels -> edge form) 5.32 -> 4.60.
  int trace_tile3 = -1;
  bool trace_fused_dots = true;  // the post tile kernel emits the partial inner products of the CG
  double trace_cheb_lo = 0.1;    // smoother interval [lo, 1.1] * lambda_max (PETSc's default)
  double trace_backward_tol = 0.0;  // > 0: normwise backward-error stop of the condensed solves (bench.py: alt_stop_rule)
  int mg_sweeps = 2;
  int mg_coarse = 2;            // coarsest-level sweeps: 6 -> 2 leaves every CG iteration count unchanged (C2: 15.57 -> 15.05 ms/step)
  bool mg_fuse = true;          // one kernel per V-cycle leg (LDS tiles) instead of the per-level launches
  bool mg_tail = true;          // levels with n <= 32 in one kernel
  bool mg_dense_tail = true;    // ... as one dense product; implied off by mg_tail off
  bool mg_dense_tail_periodic = true;  // periodic square: needs the fused legs above the tail as well
  bool mg_replicated = false;   // strips: every rank runs the whole V-cycle

  // ---- condensed CG
  bool cg_host_scalars = false;    // baseline forms of the iteration: scalars on the host,
  bool cg_two_reductions = false;  // device scalars with two reductions per iteration (default: one)
  bool cg_split_update = true;     // r, s first, then p, x on the legs of the V-cycle (off: one update launch)
  bool cg_fused_scalars = true;    // one rank: the CG scalars formed by the kernel that sums the tile partials
  // p / x updates applied in one pass, which is also the ring of z vectors and scalars they wait in (1: one per iteration; at
  // most 16).  C3 step, ms: 1: 77.1, 2: 75.7, 3: 75.3, 4: 74.4-75.2, 6: 73.9-74.8, 8: 74.6
  int cg_xp_batch = 6;
  double cg_xp_w0 = 1.6;           // share of the p / x update the finest level's legs carry (they run 18 us, the others 6-8)
  double cg_floor_c = 32.0;        // rounding floor |M r| <= c eps |x|: sqrt(75) ~ 10 with a factor three
  int cg_force_replace = 0;        // test hook: force a residual replacement at this iteration
  bool cg_mass_one_by_one = false;  // continuous-space mass solves one right-hand side at a time
  bool psi_jacobi = false;          // stream function: the diagonal alone as preconditioner, no vertex-grid cycle (the comparison test)

  // ---- stage bookkeeping of an IMEX step
  // the stage right-hand side formed inside the pressure-gradient kernel, pointer exchanges instead of copies (off: the
  // stand-alone k_lincomb launch and the copies; same bits either way -- tests/test_gpu_step_glue.py)
  bool glue_fusion = true;
};

inline Options options_from_env() {
  Options o;
  auto get = [](const char* name) { return std::getenv(name); };
  auto flag = [&](const char* name, bool& f) { if (get(name)) f = true; };
  auto unless = [&](const char* name, bool& f) { if (get(name)) f = false; };
  auto integer = [&](const char* name, int& v) { if (const char* e = get(name)) v = std::atoi(e); };
  auto real = [&](const char* name, double& v) { if (const char* e = get(name)) v = std::atof(e); };
  auto range = [&](const char* name, int& lo, int& hi) { if (const char* e = get(name)) std::sscanf(e, "%d:%d", &lo, &hi); };

  flag("HDG_GENERAL_CSR_LIFT", o.general_csr_lift);
  flag("HDG_GENERAL_BLOCK_JACOBI", o.general_block_jacobi);
  flag("HDG_GENERAL_GMRES", o.general_gmres);
  unless("HDG_GENERAL_NO_COARSE", o.general_coarse);
  integer("HDG_AMG_MAX_COARSE", o.amg_max_coarse);
  flag("HDG_AMG_UNFUSED", o.amg_unfused);

  bool no_overlap = false;
  flag("HDG_OVERLAP", o.overlap);
  flag("HDG_NO_OVERLAP", no_overlap);
  flag("HDG_FORCE_RCCL", o.force_rccl);
  integer("HDG_ROW_PAD", o.row_pad);
  flag("HDG_DBG_NONBR", o.dbg_nonbr);
  flag("HDG_FLOW_CHECK", o.flow_check);
  unless("HDG_NO_EXT", o.ext);
  unless("HDG_NO_DIRECT_HOST", o.direct_host);

  unless("HDG_NO_MFMA_SCHUR", o.mfma_schur);
  flag("HDG_MFMA_CONDENSE", o.mfma_condense);
  unless("HDG_NO_MFMA_LIFT", o.mfma_lift);
  unless("HDG_NO_MFMA_ADV", o.mfma_adv);
  unless("HDG_LIFT_NO_PAIR", o.lift_pair);
  range("HDG_ADV_SPLIT", o.adv_split_lo, o.adv_split_hi);

  flag("HDG_GMRES_ARNOLDI", o.gmres_arnoldi);
  flag("HDG_TAIL_GMRES", o.tail_gmres);
  integer("HDG_SSTEP_MAX", o.sstep_max);
  real("HDG_SSTEP_PER_DECADE", o.sstep_per_decade);
  integer("HDG_CHEB_EVERY", o.cheb_every);
  integer("HDG_CHEB_M", o.cheb_m);
  real("HDG_CHEB_FLO", o.cheb_flo);
  real("HDG_CHEB_FHI", o.cheb_fhi);
  real("HDG_CHEB_ELL", o.cheb_ell);
  integer("HDG_CHEB_MAX_EXPECTED", o.cheb_max_expected);
  integer("HDG_CHEB_FINE_STEP", o.cheb_fine_step);
  real("HDG_CHEB_HANDOVER", o.cheb_handover);
  integer("HDG_CHEB_MIN_K", o.cheb_min_k);
  integer("HDG_CHEB_HAND_CYCLE", o.cheb_hand_cycle);

  unless("HDG_TRACE_NO_FUSE", o.trace_fuse);
  unless("HDG_TRACE_NO_FOLD", o.trace_fold);
  integer("HDG_TRACE_SMOOTH_ITS", o.trace_smooth_its);
  unless("HDG_TRACE_NO_TILE", o.trace_tile);
  unless("HDG_TRACE_NO_TILE_STRIPS", o.trace_tile_strips);
  unless("HDG_TRACE_NO_TILE_PERIODIC", o.trace_tile_periodic);
  integer("HDG_TRACE_TILE3", o.trace_tile3);
  unless("HDG_TRACE_NO_FUSED_DOTS", o.trace_fused_dots);
  real("HDG_TRACE_CHEB_LO", o.trace_cheb_lo);
  real("HDG_TRACE_BACKWARD_TOL", o.trace_backward_tol);
  integer("HDG_MG_SWEEPS", o.mg_sweeps);
  integer("HDG_MG_COARSE", o.mg_coarse);
  unless("HDG_MG_NO_FUSE", o.mg_fuse);
  unless("HDG_MG_NO_TAIL", o.mg_tail);
  unless("HDG_MG_NO_DENSE_TAIL", o.mg_dense_tail);
  flag("HDG_MG_REPLICATED", o.mg_replicated);

  flag("HDG_CG_HOST_SCALARS", o.cg_host_scalars);
  flag("HDG_CG_TWO_REDUCTIONS", o.cg_two_reductions);
  unless("HDG_CG_NO_SPLIT_UPDATE", o.cg_split_update);
  unless("HDG_CG_NO_FUSED_SCALARS", o.cg_fused_scalars);
  integer("HDG_CG_XP_BATCH", o.cg_xp_batch);
  real("HDG_CG_XP_W0", o.cg_xp_w0);
  real("HDG_CG_FLOOR_C", o.cg_floor_c);
  integer("HDG_CG_FORCE_REPLACE", o.cg_force_replace);
  flag("HDG_CG_MASS_ONE_BY_ONE", o.cg_mass_one_by_one);
  flag("HDG_PSI_JACOBI", o.psi_jacobi);

  unless("HDG_NO_GLUE_FUSION", o.glue_fusion);

  // switches that imply others, resolved once
  o.overlap = o.overlap && !no_overlap;
  o.mg_dense_tail = o.mg_dense_tail && o.mg_tail;
  o.mg_dense_tail_periodic = o.mg_dense_tail && o.mg_fuse;
  o.cg_xp_batch = o.cg_xp_batch < 1 ? 1 : (o.cg_xp_batch > 16 ? 16 : o.cg_xp_batch);  // CG_XP_MAX_BATCH (hdg_cg_pending.hpp)
  return o;
}

// diagnostics switches of free functions, read once per process: HDG_DEBUG (solver decisions, communication census),
// HDG_DEBUG_CG (per-iteration residuals of the trace CG)
inline bool debug_on() { static const bool v = std::getenv("HDG_DEBUG") != nullptr; return v; }
inline bool debug_cg() { static const bool v = std::getenv("HDG_DEBUG_CG") != nullptr; return v; }

}  // namespace hdg
