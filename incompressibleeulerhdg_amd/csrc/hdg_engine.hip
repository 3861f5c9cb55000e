// MI355X-native HDG / HDG-IMEX timestep engine: device state, Krylov solvers, multigrid and the
// step orchestration behind the C-ABI of include/hdg_mi355x.h.
//
// Reference behaviour restated here (paths relative to the reference's src/):
//   timesteppers/hdg_imex.py:505-660   solve loop (stage loop, Richardson loop, final stage,
//                                      pressure reconstruction)            -> Engine::step
//   timesteppers/hdg_imex.py:257-281   pressure_solve / tentative_velocity_solve
//   timesteppers/hdg_imex.py:367-413   stage residuals r_i, r^{n+1}         -> residual_coeffs
//   timesteppers/hdg_implicit.py:92-190 first-order implicit projection step -> implicit_step
//   timesteppers/common.py:91-108      project_bdm
// The PETSc pieces are replaced by device-resident solvers:
//   KSPGMRES + PCILU (hdg_imex.py:224-228)  -> left-preconditioned GMRES(m), classical Gram-Schmidt,
//       preconditioner = element block-Jacobi + BDM-conforming subspace correction (Pi Pi^T)
//   SCPC + GMRES + GTMGPC (hdg_imex.py:128-170) -> static condensation with precomputed local
//       maps, preconditioned CG on the SPD condensed operator -S, preconditioner = Chebyshev(2)/
//       edge-block-Jacobi smoother + P1 coarse space solved by one geometric-multigrid V-cycle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hdg_mi355x.h"
#include "../../include/hdg_checkpoint.h"
#include "../../include/hdg_transfer.h"
#include "../../include/hdg_tracer_diffusion.h"
#include "../../include/hdg_tracer_walls.h"
#include "../../include/hdg_buoyancy.h"
#include "../../include/hdg_viscosity.h"
#include "../../include/hdg_coriolis.h"
#include "../../include/hdg_drag.h"
#include "../../include/hdg_moving_walls.h"
#include "../../include/hdg_adaptive_dt.h"
#include "../../include/hdg_streamfunction.h"
#include "../../include/hdg_tracer_implicit.h"
#include "hdg_options.hpp"
#include "hdg_cg_pending.hpp"
#include "hdg_dispatch.hpp"
#include "hdg_comm.hpp"
#include "hdg_kernels.hpp"
#include "hdg_vertex_levels.hpp"
#include "hdg_vertex_mg.hpp"
#include "hdg_schur_mfma.hpp"
#include "hdg_trace_tile.hpp"
#include "hdg_trace_tile3.hpp"
#include "hdg_cg.hpp"
#include "hdg_streamfunction.hpp"
#include "hdg_tables.hpp"
#include "hdg_mfma_pack.hpp"
#include "hdg_small_dense.hpp"
#include "hdg_krylov_host.hpp"
#include "hdg_tent_policy.hpp"
#include "hdg_stage_coeffs.hpp"
#include "hdg_step_control.hpp"
#include "hdg_general.hpp"
#include "hdg_general_kernels.hpp"
#include "hdg_buoyancy.hpp"
#include "hdg_viscosity.hpp"
#include "hdg_wall_force.hpp"
#include "hdg_coriolis.hpp"
#include "hdg_drag_host.hpp"
#include "hdg_drag.hpp"
#include "hdg_tracer_walls.hpp"
#include "hdg_tracer_implicit.hpp"
#include "hdg_amg.hpp"
#include "hdg_diagnostics.hpp"
#include "hdg_probes.hpp"
#include "hdg_particles.hpp"
#include "hdg_row_log.hpp"
#include "hdg_checkpoint.hpp"
#include "hdg_digest.hpp"
#include "hdg_transfer.hpp"
#include "hdg_transfer_kernels.hpp"

namespace hdg {

struct HipError {
  std::string msg;
};
#define HIPCHECK(expr)                                                                        \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      char _b[512];                                                                           \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      throw HipError{_b};                                                                     \
    }                                                                                         \
  } while (0)

struct NotConverged {
  std::string msg;
};

static constexpr int MAXV = 32;  // vectors per multi-dot launch

struct Engine {
  typedef std::vector<std::pair<const double*, double>> Terms;  // a linear combination of vectors: (vector, coefficient)
  const Options opt = options_from_env();  // every HDG_* switch, read when the engine is built (hdg_options.hpp)
  hdg_config cfg;
  Geo g;
  int K, NU, NP, NL, NE, NX, s;
  long NQ, NPv, NLv;  // vector lengths incl. ghost rows: velocity, pressure, trace (padded)
  long NQb, NPb, NLb;  // lengths of the nodal arrays at the C boundary (this rank's strip, no ghosts)
  Comm* comm = nullptr;
  bool periodic = false;  // doubly periodic square (hdg_config::periodic)
  double Ldom = 1.0;      // side of the square
  Geo g_all;           // same strip, but corner kernels visit every local row 0..ny (conversions)
  double* cg_s = nullptr;  // s = T p of the single-reduction CG
  double *hb_slo = nullptr, *hb_shi = nullptr, *hb_rlo = nullptr, *hb_rhi = nullptr;  // halo buffers
  size_t cap_halo = 0;
  double* mg_gather = nullptr;
  Tables* tab = nullptr;
  DevTables dt;
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  std::string err;

  // state (modal, device)
  double *curQ, *curP, *curL;
  std::vector<double*> stQ, stP, stL, Qstar, Qtent, brhs;  // brhs has s+1 slots (last = b_new)
  std::vector<double> bscale;                              // scale applied to brhs[slot]
  std::vector<int> bsep;                                   // slot uses the shared profile
  double* profile = nullptr;
  double *updU, *updP, *updL, *recP, *recL;
  // work
  double *wQ1, *wQ2, *wQ3, *wQ4, *wP1, *wL1, *wL2;
  double *cg_r, *cg_z, *cg_p, *cg_Ap, *ch_d, *ch_r, *tr_one;
  double *ones_c;
  const double** d_ones_ptr = nullptr;
  std::vector<double*> gm_V;  // GMRES basis (restart+1)
  const double** d_ptrs = nullptr;
  const double** d_gmV = nullptr;  // device array of the GMRES basis pointers
  double* d_part = nullptr;
  double* d_res = nullptr;
  double* h_res = nullptr;  // pinned host mirror of d_res
  double* cell_ss = nullptr;  // |z_K|^2 per cell (Chebyshev convergence checks)
  double* d_cgs = nullptr;  // device-resident CG scalars (k_cg_alpha / k_cg_beta)
  // ring of the deferred p / x updates of trace_cg_sr (XpRide, hdg_cg_pending.hpp): the z of iteration j in cg_zring[j mod M]
  // (slot 0 is cg_z; the others are allocated when a solve first asks for them), d_zring the same table on the device,
  // d_cgh (alpha, beta, c) per slot
  double* cg_zring[CG_XP_MAX_BATCH] = {nullptr};
  const double** d_zring = nullptr;
  double* d_cgh = nullptr;
  void ensure_zring(int M) {
    if (cg_zring[0] == cg_z && cg_zring[M - 1]) return;
    if (!d_cgh) { d_cgh = dalloc(3 * CG_XP_MAX_BATCH); d_zring = (const double**)dalloc(CG_XP_MAX_BATCH); }
    cg_zring[0] = cg_z;
    for (int k = 1; k < M; k++)
      if (!cg_zring[k]) cg_zring[k] = dalloc(NLv);
    HIPCHECK(hipMemcpyAsync(d_zring, cg_zring, sizeof(double*) * CG_XP_MAX_BATCH, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  double* h_cgs = nullptr;  // pinned snapshot of d_cgs for the lagged convergence check
  hipEvent_t cg_ev = nullptr;
  int dot_blocks = 0;
  // element block-Jacobi inverses per stage (depends on gamma = a_ii dt)
  std::vector<double*> dinv0, dinv1, hybg0, hybg1;
  std::vector<double> dinv_gamma;
  // trace Chebyshev bounds
  double cheb_lmin = 0, cheb_lmax = 0;
  double tr_one_nn = -1.0;
  // operator sets of the hybridised mixed Poisson problem, one per stabilisation parameter tau':
  // set 0 (tau) serves the projection method; the unsplit solves use tau/gamma (see mono_precond)
  struct PSet {
    DevTables dt; double lmin, lmax, tau;
    // the same local maps in A-operand lane order for the matrix-core kernels (k >= 3; built on first use)
    const double* bsm[2] = {nullptr, nullptr};  // back-substitution: [Ainv | -W], rows (u in memory order | phi)
    const double* cdm = nullptr;                // condensation: the four cell blocks of Y around a corner
  };
  std::vector<PSet> psets;
  int cur_pset = 0;
  const DevTables& pdt() const { return psets[cur_pset].dt; }
  void use_pset(int i) { cur_pset = i; cheb_lmin = psets[i].lmin; cheb_lmax = psets[i].lmax; }
  // multigrid levels (vertex grids)
  std::vector<double*> mg_x, mg_b, mg_r;
  // stats
  double it_sum[4] = {0, 0, 0, 0};
  long it_cnt[4] = {0, 0, 0, 0};
  // boundary staging buffers
  double *hQ_dev, *hP_dev, *hL_dev;

  // ------------------------------------------------------------------ section timers (hdg_get_timers)
  // Sections are bracketed by events on the stream; elapsed times are harvested once the stream has drained
  // (the end of every API call), so a fused step needs no synchronisation to report its per-solve breakdown.
  // T_KADV / T_KLIFT (hdg_set_kernel_timing): every launch of the two kernels of a tentative-velocity iteration -- the
  // advection operator in residual form and the hybrid lift with its Chebyshev / GMRES epilogue -- bracketed on its own,
  // in place (same operands, same cache state as in the solve): what bench.py's roofline block divides by.
  // Round 4: one label per FORM (the s-step tail makes the plain forms the more frequent ones at k >= 2): T_KADV = residual form
  // b - A x, T_KLIFT = lift with the fused Chebyshev step, T_KADV_PLAIN / T_KLIFT_PLAIN = the forms GMRES and the s-step cycles use.
  enum { T_STEP = 0, T_BDM = 1, T_TENT = 2, T_PRESS = 3, T_UNSPLIT = 4, T_KADV = 5, T_KLIFT = 6, T_KADV_PLAIN = 7, T_KLIFT_PLAIN = 8,
         T_DG = 9 /* the (u, phi) solve of the implicit DG step */ };
  double tm_total[HDG_N_TIMERS] = {0}, tm_sumsq[HDG_N_TIMERS] = {0};
  long tm_calls[HDG_N_TIMERS] = {0};
  struct Section { int label; hipEvent_t e0, e1; };
  std::vector<Section> tm_open;       // recorded, not yet harvested
  std::vector<hipEvent_t> tm_pool;    // idle events
  hipEvent_t tm_event() {
    if (!tm_pool.empty()) { hipEvent_t e = tm_pool.back(); tm_pool.pop_back(); return e; }
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    return e;
  }
  struct Timed {  // scope guard: records the closing event on every exit path
    Engine& E;
    Section sec;
    Timed(Engine& e, int label) : E(e) {
      sec.label = label;
      sec.e0 = E.tm_event();
      sec.e1 = E.tm_event();
      (void)hipEventRecord(sec.e0, E.stream);
    }
    ~Timed() {
      (void)hipEventRecord(sec.e1, E.stream);
      E.tm_open.push_back(sec);
    }
  };
  bool kernel_timing = false;
  struct KTimed {  // Timed, but only while kernel timing is switched on
    Engine& E; bool on; Section sec;
    KTimed(Engine& e, int label, bool cond) : E(e), on(e.kernel_timing && cond) {
      if (!on) return;
      sec.label = label; sec.e0 = E.tm_event(); sec.e1 = E.tm_event();
      (void)hipEventRecord(sec.e0, E.stream);
    }
    ~KTimed() { if (on) { (void)hipEventRecord(sec.e1, E.stream); E.tm_open.push_back(sec); } }
  };
  // inside a long fused run (hdg_run_separable): harvest the sections whose closing event has completed, so that the list
  // of live events stays bounded (two events per section, and with kernel timing two per bracketed launch)
  void harvest_completed() {
    size_t keep = 0;
    for (size_t q = 0; q < tm_open.size(); q++) {
      const Section sc = tm_open[q];
      float ms = 0.0f;
      if (hipEventQuery(sc.e1) == hipSuccess && hipEventElapsedTime(&ms, sc.e0, sc.e1) == hipSuccess) {
        tm_total[sc.label] += ms;
        tm_sumsq[sc.label] += (double)ms * ms;
        tm_calls[sc.label]++;
        tm_pool.push_back(sc.e0);
        tm_pool.push_back(sc.e1);
      } else {
        tm_open[keep++] = sc;
      }
    }
    tm_open.resize(keep);
  }
  void harvest_timers() {  // the stream must have been synchronised
    for (const Section& sc : tm_open) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, sc.e0, sc.e1) == hipSuccess) {
        tm_total[sc.label] += ms;
        tm_sumsq[sc.label] += (double)ms * ms;
        tm_calls[sc.label]++;
      }
      tm_pool.push_back(sc.e0);
      tm_pool.push_back(sc.e1);
    }
    tm_open.clear();
  }

  // ------------------------------------------------------------------ memory
  double* dalloc(long n) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, sizeof(double) * (size_t)std::max<long>(n, 1)));
    HIPCHECK(hipMemsetAsync(p, 0, sizeof(double) * (size_t)std::max<long>(n, 1), stream));
    allocs.push_back(p);
    return (double*)p;
  }
  void dfree(double*& p) {
    if (!p) return;
    auto it = std::find(allocs.begin(), allocs.end(), (void*)p);
    if (it != allocs.end()) allocs.erase(it);
    HIPCHECK(hipFree(p));
    p = nullptr;
  }
  // a device allocation of dalloc / upload / upload_ints that is replaced: freed and forgotten (null: nothing)
  void release_dev(const void* p) {
    if (!p) return;
    auto it = std::find(allocs.begin(), allocs.end(), const_cast<void*>(p));
    if (it != allocs.end()) allocs.erase(it);
    HIPCHECK(hipFree(const_cast<void*>(p)));
  }
  const double* upload(const dvec& v) {
    double* p = dalloc((long)v.size());
    HIPCHECK(hipMemcpyAsync(p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return p;
  }
  const double** upload_ptrs(const std::vector<const double*>& v) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, sizeof(double*) * v.size()));
    allocs.push_back(p);
    HIPCHECK(hipMemcpy(p, v.data(), sizeof(double*) * v.size(), hipMemcpyHostToDevice));
    return (const double**)p;
  }

  dim3 cell_grid() const { return dim3(8 * g.rows_xcd * 2 * g.nbx, 1, 1); }
  dim3 corner_grid() const { return dim3(8 * g.rows_xcdc * g.nbxc, 1, 1); }
  dim3 corner_grid_all() const { return dim3(8 * g_all.rows_xcdc * g_all.nbxc, 1, 1); }
  int bs() const { return g.nx <= 64 ? 64 : 128; }
  // vector kernels: one 16-byte pair per thread (no grid-stride trips: consecutive workgroups walk memory in order;
  // tools/probes/stream_probe: 3 reads + 1 write 5.1 TB/s with 2048 blocks, 5.85 with one pair per thread)
  int vec_blocks(long n) const { return (int)std::min<long>((n / 2 + 255) / 256 + 1, 1L << 22); }
  // streaming cache policy for vectors that exceed the Infinity Cache together with their partners
  bool big(long n) const { return n * 8L >= (96L << 20); }

  // ------------------------------------------------------------------ general affine triangulations
  // hdg_general.hpp builds topology, per-cell local matrices and the assembled solution-independent operators on the host;
  // here they are uploaded and every kernel wrapper below gets a `general` branch: one CSR kernel for the assembled
  // operators, k_g_adv / k_g_precon for the two solution-dependent forms.  The solvers (GMRES with element block-Jacobi,
  // condensation + CG with edge block-Jacobi + back-substitution) and the step orchestration are the structured engine's.
  bool general = false;
  GMesh* gm = nullptr;
  GeneralTables* gtab = nullptr;
  GeneralOps gops;
  std::vector<CellLocal> gloc;
  struct GDev {  // operators that do not depend on the stabilisation parameter
    DevCsr Pi, Wdiv, Bdiv, Gp, Gl, Rq, Rp, Rb, Cq, Cqi, Cp, Cpi, Cl, Cli, Psi_p, Psi_l, Mu_u, Mu_p, Mu_l;
  } gd;
  std::vector<DevCsr> gdinv;  // element block-Jacobi per stage
  // matrix-free lift on general meshes (k_g_lift, round 4): reference moment tables, per-cell lifting tables of the BDM
  // projection and (per stage) of the hybrid preconditioner; HDG_GENERAL_CSR_LIFT keeps the assembled operators
  const double* g_nref = nullptr;
  const double* g_lift = nullptr;
  std::vector<const double*> g_hyb;

  GGeo ggeo;
  const double *d_one_p = nullptr, *d_int_p = nullptr, *d_one_l = nullptr;
  const int* upload_ints(const std::vector<int>& v) {
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, sizeof(int) * std::max<size_t>(v.size(), 1)));
    allocs.push_back(p);
    HIPCHECK(hipMemcpy(p, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
    return (const int*)p;
  }
  DevCsr upload_csr(const Csr& m) {
    DevCsr d;
    d.nrows = m.nrows; d.ncols = m.ncols; d.nnz = (long)m.val.size();
    d.rowptr = upload_ints(m.rowptr);
    d.col = upload_ints(m.col);
    d.val = upload(m.val.empty() ? dvec(1, 0.0) : m.val);
    const double avg = m.nrows > 0 ? (double)m.val.size() / m.nrows : 0.0;
    d.tpr = avg <= 3.0 ? 1 : (avg <= 6.0 ? 2 : (avg <= 12.0 ? 4 : (avg <= 24.0 ? 8 : (avg <= 48.0 ? 16 : (avg <= 96.0 ? 32 : 64)))));
    return d;
  }
  // threads per row of a CSR kernel (DevCsr::tpr, chosen by upload_csr)
  template <class F> static void by_tpr(const DevCsr& A, F&& f) { with_int<1, 2, 4, 8, 16, 32, 64>(A.tpr, "CSR threads per row", f); }
  // y = beta y + alpha A x
  void csr(const DevCsr& A, const double* x, double alpha, double beta, double* y) {
    tally(LC_OTHER, 12.0 * A.nnz + 8.0 * (A.ncols + A.nrows * (beta != 0.0 ? 2 : 1)));
    const long nthr = (long)A.nrows * A.tpr;
    const int nblk = (int)((nthr + 255) / 256);
    by_tpr(A, [&](auto t) { k_csr_apply<t()><<<nblk, 256, 0, stream>>>(A, x, alpha, beta, y); });
    fl.set(y, 0);
  }
  // y = alpha A x + beta z
  void csr3(const DevCsr& A, const double* x, double alpha, double beta, const double* z, double* y) {
    tally(LC_OTHER, 12.0 * A.nnz + 8.0 * (A.ncols + 2.0 * A.nrows));
    const long nthr = (long)A.nrows * A.tpr;
    const int nblk = (int)((nthr + 255) / 256);
    by_tpr(A, [&](auto t) { k_csr_apply3<t()><<<nblk, 256, 0, stream>>>(A, x, alpha, beta, z, y); });
    fl.set(y, 0);
  }
  // P1 coarse space of the trace preconditioner on a general mesh and its algebraic hierarchy (hdg_amg.hpp)
  struct AmgDev {
    std::vector<const double*> dinv;     // inverse diagonals as vectors (fused smoother k_amg_cheb)
    DevCsr P0, R0;                       // vertices <-> trace space
    std::vector<DevCsr> A, P, R, Dinv;   // per level (Dinv: the inverse diagonal as a matrix for the CSR kernel)
    std::vector<double*> x, b, r, d;
    std::vector<double> lmax;
    std::vector<int> n;
    DevCsr Cinv;                         // dense pseudo-inverse of the coarsest operator (nrows = 0: smooth only)
  };
  // operators that depend on the stabilisation parameter tau: one set per PSet (psets[i] <-> gsets[i]; the second set,
  // tau' = tau / gamma, belongs to the block preconditioner of the monolithic solve, section 7 of DESIGN.md)
  struct GSet {
    DevCsr S, Dtr, Yw, Yp, Wu, Wp, Auu, Aup, Apu, App;
    AmgDev amg;
  };
  std::vector<GSet> gsets;
  GSet& gs() { return gsets[(size_t)cur_pset]; }
  void upload_gset(const GeneralOps& O, GSet& G) {
    G.S = upload_csr(O.S); G.Dtr = upload_csr(O.Dtr); G.Yw = upload_csr(O.Yw); G.Yp = upload_csr(O.Yp);
    G.Wu = upload_csr(O.Wu); G.Wp = upload_csr(O.Wp); G.Auu = upload_csr(O.Auu); G.Aup = upload_csr(O.Aup);
    G.Apu = upload_csr(O.Apu); G.App = upload_csr(O.App);
  }
  void setup_general_amg(const Csr& S_host, AmgDev& amg) {
    AmgHierarchy amg_host;
    const Csr P0 = p1_to_trace_matrix(*gtab, *gm);
    const Csr R0 = csr_transpose(P0);
    const Csr A0 = csr_multiply(R0, csr_multiply(S_host, P0));
    amg_build(A0, amg_host, opt.amg_max_coarse);
    amg.P0 = upload_csr(P0); amg.R0 = upload_csr(R0);
    for (size_t l = 0; l < amg_host.lev.size(); l++) {
      const AmgLevel& L = amg_host.lev[l];
      const int n = L.A.nrows;
      amg.n.push_back(n);
      amg.lmax.push_back(L.lmax);
      amg.A.push_back(upload_csr(L.A));
      amg.P.push_back(l + 1 < amg_host.lev.size() ? upload_csr(L.P) : DevCsr());
      amg.R.push_back(l + 1 < amg_host.lev.size() ? upload_csr(L.R) : DevCsr());
      Csr D;
      D.nrows = D.ncols = n;
      D.rowptr.resize((size_t)n + 1);
      D.col.resize((size_t)n);
      for (int i = 0; i <= n; i++) D.rowptr[(size_t)i] = i;
      for (int i = 0; i < n; i++) D.col[(size_t)i] = i;
      D.val = L.dinv;
      amg.Dinv.push_back(upload_csr(D));
      amg.dinv.push_back(upload(L.dinv));
      amg.x.push_back(dalloc(n)); amg.b.push_back(dalloc(n)); amg.r.push_back(dalloc(n)); amg.d.push_back(dalloc(n));
    }
    if (amg_host.coarse_pinv.nrows > 0) amg.Cinv = upload_csr(amg_host.coarse_pinv);
    if (debug_on()) {
      fprintf(stderr, "[amg] P1 coarse space %d vertices; levels:", amg.n.empty() ? 0 : amg.n[0]);
      for (size_t l = 0; l < amg.n.size(); l++) fprintf(stderr, " %d (nnz %ld, lmax %.2f)", amg.n[l], amg.A[l].nnz, amg.lmax[l]);
      fprintf(stderr, "%s\n", amg.Cinv.nrows ? "; dense coarsest solve" : "; coarsest level smoothed only");
    }
  }
  // Chebyshev(2) / Jacobi on level l: x (=, +=) p(D^{-1} A) D^{-1} (b - A x), interval [0.1, 1.1] lambda_max
  void amg_cheb(int l, bool zero_init) {
    AmgDev& amg = gs().amg;
    const int n = amg.n[l];
    const double lo = 0.1 * amg.lmax[l], hi = 1.1 * amg.lmax[l];
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma1 = theta / delta, rho = 1.0 / sigma1;
    const double rn = 1.0 / (2.0 * sigma1 - rho);
    double* r = amg.r[l];
    double* d = amg.d[l];
    if (!opt.amg_unfused) {  // two launches (k_amg_cheb) instead of six or seven
      const DevCsr& A = amg.A[l];
      const long nthr = (long)A.nrows * A.tpr;
      const int nblk = (int)((nthr + 255) / 256);
      const double* xin = zero_init ? nullptr : amg.x[l];
      tally(LC_OTHER, 2.0 * (12.0 * A.nnz + 8.0 * 5.0 * n));
      tally(LC_OTHER, 0.0);
      by_tpr(A, [&](auto t) {
        k_amg_cheb<t(), true><<<nblk, 256, 0, stream>>>(A, amg.dinv[l], amg.b[l], xin, r, d, nullptr, 1.0 / theta, 0.0, 0.0);
        k_amg_cheb<t(), false><<<nblk, 256, 0, stream>>>(A, amg.dinv[l], amg.b[l], xin, r, d, amg.x[l], 0.0, rn * rho, 2.0 * rn / delta);
      });
      return;
    }
    copy(r, amg.b[l], n);
    if (!zero_init) csr(amg.A[l], amg.x[l], -1.0, 1.0, r);        // r0 = b - A x
    csr(amg.Dinv[l], r, 1.0 / theta, 0.0, d);                     // d0 = Dinv r0 / theta
    if (zero_init) copy(amg.x[l], d, n); else axpby(n, 1.0, d, 1.0, amg.x[l]);
    csr(amg.A[l], d, -1.0, 1.0, r);                               // r1 = r0 - A d0
    csr(amg.Dinv[l], r, 2.0 * rn / delta, rn * rho, d);           // d1 = rn rho d0 + (2 rn / delta) Dinv r1
    axpby(n, 1.0, d, 1.0, amg.x[l]);
  }
  // V-cycle on b[l] -> x[l] (zero initial guess)
  void amg_vcycle(int l) {
    AmgDev& amg = gs().amg;
    const int last = (int)amg.n.size() - 1;
    if (l == last) {
      if (amg.Cinv.nrows > 0) csr(amg.Cinv, amg.b[l], 1.0, 0.0, amg.x[l]);
      else amg_cheb(l, true);
      return;
    }
    amg_cheb(l, true);
    csr3(amg.A[l], amg.x[l], -1.0, 1.0, amg.b[l], amg.r[l]);  // r = b - A x
    csr(amg.R[l], amg.r[l], 1.0, 0.0, amg.b[l + 1]);
    amg_vcycle(l + 1);
    csr(amg.P[l], amg.x[l + 1], 1.0, 1.0, amg.x[l]);
    amg_cheb(l, false);
  }
  Engine(const hdg_config& c, Comm* comm_, int nv, const double* coords, int nc, const int* cells) : cfg(c), comm(comm_) {
    if (c.degree < 1 || c.degree > 4) throw std::string("degree must be in 1..4");
    n_tr = checked_n_tracers(c);
    if (c.nstages < 1 || c.nstages > HDG_MAX_STAGES) throw std::string("nstages out of range");
    if (!(c.dt > 0)) throw std::string("dt must be positive");
    if (comm->size != 1) throw std::string("general meshes are implemented for a single rank");
    HIPCHECK(hipSetDevice(c.device));
    HIPCHECK(hipStreamCreate(&stream));
    try {
      construct_general(c, nv, coords, nc, cells);
    } catch (...) {
      release();
      throw;
    }
  }
  void construct_general(const hdg_config& c, int nv, const double* coords, int nc, const int* cells) {
    general = true;
    ck_mesh_nv = nv; ck_mesh_nc = nc;
    ck_mesh_coords = ckpt::digest_bytes(coords, sizeof(double) * 2 * (size_t)nv);
    ck_mesh_cells = ckpt::digest_bytes(cells, sizeof(int) * 3 * (size_t)nc);
    K = c.degree; s = c.nstages;
    NU = n_scalar(K + 1); NP = n_scalar(K); NL = K + 1; NE = K + 2; NX = 2 * NU + NP;
    // solvers of this path: GMRES(m) with the element block-Jacobi, CG with the edge block-Jacobi (the two-level
    // preconditioners of the structured engine lean on the two shared shapes / the vertex grid)
    // trace system: Chebyshev(2) / edge block-Jacobi + the P1 coarse space with an algebraic V-cycle (hdg_amg.hpp);
    // HDG_GENERAL_NO_COARSE: the edge block-Jacobi alone
    // tentative velocity: GMRES(30) with the hybrid preconditioner Pi + Dinv (I - Pi) (HDG_GENERAL_BLOCK_JACOBI: Dinv alone)
    // round 4: the Chebyshev iteration + s-step tail of the structured engine here as well (preconditioner and Chebyshev step as
    // separate launches: the assembled operators have no fused form); HDG_GENERAL_GMRES restores GMRES(30)
    cfg.tent_precond = opt.general_block_jacobi ? 0 : 2; cfg.periodic = 0;
    // (k = 1: GMRES -- with assembled operators an iteration is dear, and the Chebyshev iteration needs 41 where GMRES needs 33)
    cfg.tent_solver = (opt.general_gmres || cfg.tent_precond != 2 || K < 2) ? 0 : 1;
    cfg.trace_precond = opt.general_coarse ? 1 : 0;
    cfg.gmres_restart = std::max(cfg.gmres_restart, 30);
    gm = new GMesh();
    gm->build(nv, coords, nc, cells);
    gtab = new GeneralTables(K, c.tau, c.alpha_penalty, c.equispaced_nodes);
    assemble_general(*gtab, *gm, gops, gloc);
    // the structured-mesh descriptor only sizes scratch buffers and vector kernels here
    g = Geo{};
    g.nx = 1; g.ny = 1; g.P = 16; g.nyg = 1; g.joff = 0; g.nyc = 1; g.G = 16; g.R = 1; g.h = 1.0; g.nbx = 1; g.nbxc = 1;
    g.rows_xcd = 1; g.rows_xcdc = 1; g.wrows = 1; g.wrowsc = 1;
    g.Nc = gm->nc;
    g_all = g;
    Ldom = 1.0;
    NQ = (long)gm->nc * 2 * NU; NPv = (long)gm->nc * NP; NLv = (long)gm->ne * NL;
    NQb = NQ; NPb = NPv; NLb = NLv;
    tab = new Tables(K, 1.0, c.tau, c.alpha_penalty, c.equispaced_nodes);  // shared reference data only
    alloc_state();
    // device copies
    gd.Pi = upload_csr(gops.Pi); gd.Wdiv = upload_csr(gops.Wdiv); gd.Bdiv = upload_csr(gops.Bdiv); gd.Gp = upload_csr(gops.Gp);
    gd.Gl = upload_csr(gops.Gl); gd.Rq = upload_csr(gops.Rq);
    gsets.emplace_back();
    upload_gset(gops, gsets[0]);
    gd.Psi_p = upload_csr(gops.Psi_p); gd.Psi_l = upload_csr(gops.Psi_l); gd.Mu_u = upload_csr(gops.Mu_u);
    gd.Mu_p = upload_csr(gops.Mu_p); gd.Mu_l = upload_csr(gops.Mu_l);
    gd.Rp = upload_csr(gops.Rp); gd.Rb = upload_csr(gops.Rb); gd.Cq = upload_csr(gops.Cq); gd.Cqi = upload_csr(gops.Cqi);
    gd.Cp = upload_csr(gops.Cp); gd.Cpi = upload_csr(gops.Cpi); gd.Cl = upload_csr(gops.Cl); gd.Cli = upload_csr(gops.Cli);
    d_one_p = upload(gops.one_p); d_int_p = upload(gops.int_p); d_one_l = upload(gops.one_l);
    gdinv.assign((size_t)s, DevCsr());
    g_hyb.assign((size_t)s, nullptr);
    if (!opt.general_csr_lift) {
      dvec nr(gtab->Nref.size());
      for (size_t q = 0; q < nr.size(); q++) nr[q] = (double)gtab->Nref[q];
      g_nref = upload(nr);
      g_lift = upload(assemble_lift_tables(*gtab, *gm, gloc, -1.0));
    }
    {
      const GMesh& M = *gm;
      dvec isd((size_t)M.nc), celen((size_t)3 * M.nc), cenx((size_t)3 * M.nc), ceny((size_t)3 * M.nc);
      std::vector<int> cnbr((size_t)3 * M.nc), ctab((size_t)3 * M.nc), ntab((size_t)3 * M.nc, 0);
      for (int cc = 0; cc < M.nc; cc++) {
        isd[(size_t)cc] = 1.0 / std::sqrt(M.detJ[(size_t)cc]);
        for (int l = 0; l < 3; l++) {
          const int e = M.cedge[3 * (size_t)cc + l];
          const int side = M.ecell[2 * (size_t)e] == cc ? 0 : 1;
          const int cn = M.ecell[2 * (size_t)e + (1 - side)];
          cnbr[3 * (size_t)cc + l] = cn;
          ctab[3 * (size_t)cc + l] = l * 2 + M.cflip[3 * (size_t)cc + l];
          if (cn >= 0) {
            const int ln = M.elocal[2 * (size_t)e + (1 - side)];
            ntab[3 * (size_t)cc + l] = ln * 2 + M.cflip[3 * (size_t)cn + ln];
          }
          celen[3 * (size_t)cc + l] = M.elen[(size_t)e]; cenx[3 * (size_t)cc + l] = M.enx[(size_t)e]; ceny[3 * (size_t)cc + l] = M.eny[(size_t)e];
        }
      }
      ggeo.nc = M.nc;
      ggeo.inv_sdet = upload(isd); ggeo.detJ = upload(M.detJ); ggeo.Jinv = upload(M.Jinv);
      ggeo.cnbr = upload_ints(cnbr); ggeo.ctab = upload_ints(ctab); ggeo.ntab = upload_ints(ntab);
      ggeo.csig = upload(M.csig); ggeo.celen = upload(celen); ggeo.cenx = upload(cenx); ggeo.ceny = upload(ceny);
      ggeo.cw = upload(gtab->cw); ggeo.cPhi = upload(gtab->cPhi); ggeo.cGxi = upload(gtab->cGxi); ggeo.cGeta = upload(gtab->cGeta);
      ggeo.ew = upload(gtab->ew); ggeo.ePhi = upload(gtab->ePhi); ggeo.eGxi = upload(gtab->eGxi); ggeo.eGeta = upload(gtab->eGeta);
      ggeo.nqc = gtab->nqc; ggeo.nqe = gtab->nqe; ggeo.alpha = c.alpha_penalty;
    }
    setup_trace_solver();
    HIPCHECK(hipStreamSynchronize(stream));
  }
  [[noreturn]] void general_unsupported(const char* what) const {
    throw std::string("general meshes: ") + what + " is not implemented (structured meshes only)";
  }

  // ------------------------------------------------------------------ construction
  Engine(const hdg_config& c, Comm* comm_) : cfg(c), comm(comm_) {
    if (c.degree < 1 || c.degree > 4) throw std::string("degree must be in 1..4");
    n_tr = checked_n_tracers(c);
    if (c.nx < 1 || c.ny < 1) throw std::string("nx, ny must be positive");
    if (c.nx != c.ny) throw std::string("only square meshes nx == ny (UnitSquareMesh(nx, nx), driver.py:181)");
    if (c.nstages < 1 || c.nstages > HDG_MAX_STAGES) throw std::string("nstages out of range");
    if (!(c.dt > 0)) throw std::string("dt must be positive");
    HIPCHECK(hipSetDevice(c.device));
    HIPCHECK(hipStreamCreate(&stream));
    // no destructor runs for a half-built object: release what has been acquired so far and rethrow
    // (the communicator stays with the caller until construction has succeeded)
    try {
      construct(c);
    } catch (...) {
      release();
      throw;
    }
  }
  void release() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    if (h_res) { (void)hipHostFree(h_res); h_res = nullptr; }
    if (h_cgs) { (void)hipHostFree(h_cgs); h_cgs = nullptr; }
    if (cg_ev) { (void)hipEventDestroy(cg_ev); cg_ev = nullptr; }
    for (const Section& sc : tm_open) { (void)hipEventDestroy(sc.e0); (void)hipEventDestroy(sc.e1); }
    tm_open.clear();
    for (hipEvent_t e : tm_pool) (void)hipEventDestroy(e);
    tm_pool.clear();
    if (ev_in) { (void)hipEventDestroy(ev_in); ev_in = nullptr; }
    if (ev_halo) { (void)hipEventDestroy(ev_halo); ev_halo = nullptr; }
    if (cstream) { (void)hipStreamDestroy(cstream); cstream = nullptr; }
    if (h_cgm) { (void)hipHostFree(h_cgm); h_cgm = nullptr; }
    for (int q = 0; q < 2; q++) if (cgm_ev[q]) { (void)hipEventDestroy(cgm_ev[q]); cgm_ev[q] = nullptr; }
    if (psi_h) { (void)hipHostFree(psi_h); psi_h = nullptr; }
    for (int q = 0; q < 2; q++) if (psi_ev[q]) { (void)hipEventDestroy(psi_ev[q]); psi_ev[q] = nullptr; }
    if (tdi_h) { (void)hipHostFree(tdi_h); tdi_h = nullptr; }
    for (int q = 0; q < 2; q++) if (tdi_ev[q]) { (void)hipEventDestroy(tdi_ev[q]); tdi_ev[q] = nullptr; }
    if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    delete tab;
    tab = nullptr;
    delete gm; gm = nullptr;
    delete gtab; gtab = nullptr;
    delete gcg; gcg = nullptr;
    delete glocator; glocator = nullptr;
  }
  void construct(const hdg_config& c) {
    K = c.degree;
    s = c.nstages;
    NU = n_scalar(K + 1); NP = n_scalar(K); NL = K + 1; NE = K + 2; NX = 2 * NU + NP;
    if (c.ny % comm->size != 0) throw std::string("ny must be divisible by the number of ranks (strip partition)");
    g.nx = c.nx; g.nyg = c.ny;
    g.ny = c.ny / comm->size;
    g.joff = comm->rank * g.ny;
    g.nyc = g.ny + (comm->rank == comm->size - 1 ? 1 : 0);
    periodic = c.periodic != 0;
    Ldom = c.length > 0 ? c.length : 1.0;
    // interior / boundary split around halo exchanges on a second stream: OPT-IN (HDG_OVERLAP=1) since round 4 -- the logic is
    // tested on every multi-rank test over the shared-memory transport, but ncclSend / ncclRecv on a second stream beside
    // kernels has never run on two devices (round-3 advisor finding): the first multi-GPU run uses the plain single-stream order
    overlap_on = opt.overlap;
    if (periodic && (c.nx % 2 != 0)) throw std::string("the periodic mesh needs an even nx (red-black coarse-grid sweeps)");
    if (periodic && c.ny < 4) throw std::string("the periodic mesh needs at least 4 cell rows");
    if (periodic && comm->size > 1 && g.ny < PERIODIC_MIN_ROWS)
      throw std::string("periodic strips need at least ") + std::to_string(PERIODIC_MIN_ROWS) + " cell rows per rank (ny / ranks = " +
          std::to_string(g.ny) + ")";
    if (periodic) {
      // y-periodicity without touching a kernel: the strip pretends to lie in the middle of a taller mesh (no physical
      // boundary test in y fires, the top H row is a ghost copy of the bottom one like on a rank below another).  One rank:
      // its ghost rows are filled from its own opposite side (halo_rows -> k_wrap_rows).  P > 1 ranks (periodic strips): rank
      // r owns the cell / vertex / bottom H-edge rows r ny/P .. (r+1) ny/P - 1 of the global mesh, all strips sit in the SAME
      // taller mesh, and the ghost rows come from the ring neighbours (r -/+ 1) mod P (Comm::ring)
      g.joff = c.ny + comm->rank * g.ny; g.nyg = 3 * c.ny; g.nyc = g.ny;
      comm->ring = comm->size > 1;
    }
    g.px = periodic ? 1 : 0;
    g.pj0 = periodic ? comm->rank * g.ny : 0;
    g.P = ((c.nx + 1 + 15) / 16) * 16;
    g.G = (long)(g.ny + 2 * GH) * g.P;
    g.R = g.ny + 2 * GH;
    if (opt.row_pad >= 0) g.R += opt.row_pad;
    else {
      // Padding rows: the element kernels stream 2 (k+2)(k+3)/2 dof planes at once, and on MI355X planes whose stride is
      // close to a multiple of 2^15 B times 0, 1, 2, 4, 8 or 9 (mod 16) share memory channels.  Measured at C3, stride =
      // R * 2^15 B (tools/padscan.sh, ms/step): R mod 16 = 8: 153, 9: 139.5, 4: 139.0, 2: 140; 3 .. 7 and 11 .. 15: 134.5 - 137.
      for (int pad = 0; pad < 64; pad++) {
        const double t = std::fmod((double)(2L * c.nx * (g.R + pad) * 16L), 524288.0) / 32768.0;
        if ((t >= 2.5 && t <= 7.5) || (t >= 10.5 && t <= 15.5)) { g.R += pad; break; }
      }
    }
    g.Nc = 2L * c.nx * g.R;
    g.elo = g.ehi = 0;
    g.h = Ldom / c.nx;
    g.nbx = (g.nx + bs() - 1) / bs();
    g.nbxc = (g.nx + 1 + bs() - 1) / bs();
    g.rows_xcd = (g.ny + 7) / 8;
    g.rows_xcdc = (g.nyc + 7) / 8;
    g.wskip = 0; g.wgap0 = 0; g.wgapn = 0; g.wrows = g.ny; g.wrowsc = g.nyc;
    g.dbg_nonbr = opt.dbg_nonbr ? 1 : 0;
    g_all = g;
    g_all.nyc = g.ny + (periodic ? 0 : 1);
    g_all.rows_xcdc = (g_all.nyc + 7) / 8;
    g_all.wrowsc = g_all.nyc;
    NQ = 2L * NU * g.Nc; NPv = (long)NP * g.Nc; NLv = 3L * NL * g.G;
    // cell kernels address a vector with 32-bit byte offsets (buffer loads, hdg_kernels.hpp: CellBuf)
    if (NQ * 8L >= (1L << 32))
      throw std::string("mesh too large for one GPU: a velocity vector must stay below 4 GiB (32-bit buffer offsets); "
                        "use more ranks");
    NQb = 2L * NU * 2L * g.nx * g.ny; NPb = (long)NP * 2L * g.nx * g.ny;
    NLb = n_edges() * NL;
    tab = new Tables(K, g.h, c.tau, c.alpha_penalty, c.equispaced_nodes);
    if (periodic) cfg.trace_precond = cfg.trace_precond ? 1 : 0;
    build_dev_tables();
    alloc_state();
    setup_trace_solver();
    HIPCHECK(hipStreamSynchronize(stream));
  }
  ~Engine() {
    if (debug_on() && comm && comm->rank == 0)
      fprintf(stderr, "[comm] halo exchanges: velocity %ld, pressure %ld, trace %ld, vertex rows %ld (%ld of them beside an interior launch); all-reduces %ld; all-gathers %ld; tiled trace preconditioner applications %ld\n",
              n_halo[0], n_halo[1], n_halo[2], n_halo_mg, n_overlapped, n_reduce, n_gather, n_tile_precond);
    if (opt.flow_check && comm && comm->rank == 0)
      fprintf(stderr, "[flow check] %ld skipped exchanges verified, worst relative deviation %.3e\n", fc_count, fc_worst);
    release();
    delete comm;
  }

  void build_dev_tables() {
    const Tables& T = *tab;
    for (int sh = 0; sh < 2; sh++) {
      for (int e = 0; e < 3; e++) {
        dt.N[sh][e] = upload(T.N[sh][e]);
        dt.Nt[sh][e] = upload(transpose(T.N[sh][e], NE, 2 * NU));
        dt.Lift[sh][e] = upload(T.Lift[sh][e]);
        dt.LiftT[sh][e] = upload(transpose(T.Lift[sh][e], 2 * NU, NE));
        dt.Pt[sh][e] = upload(T.Pt[sh][e]);
        dt.ePhi[sh][e] = upload(T.ePhi[sh][e]);
        dt.eGx[sh][e] = upload(T.eGx[sh][e]);
        dt.eGy[sh][e] = upload(T.eGy[sh][e]);
      }
      dt.B[sh] = upload(T.B[sh]); dt.D0[sh] = upload(T.D0[sh]);
      dt.Ainv[sh] = upload(T.Ainv[sh]); dt.W[sh] = upload(T.W[sh]);
      dt.Y[sh] = upload(T.Y[sh]); dt.SK[sh] = upload(T.SK[sh]);
      dt.cPhi[sh] = upload(T.cPhi[sh]); dt.cGx[sh] = upload(T.cGx[sh]); dt.cGy[sh] = upload(T.cGy[sh]);
    }
    dt.cw = upload(T.cw);
    for (int e = 0; e < 3; e++) dt.ew[e] = upload(T.ew[e]);
    for (int t = 0; t < 3; t++)
      for (int v = 0; v < 3; v++) dt.trDinv[t][v] = upload(T.trDinv[t][v]);
    dt.Vu = upload(T.Vu); dt.Vuinv = upload(T.Vuinv); dt.Vp = upload(T.Vp); dt.Vpinv = upload(T.Vpinv);
    dt.Vl = upload(T.Vl); dt.Vlinv = upload(T.Vlinv);
    for (int e = 0; e < 3; e++) { dt.elen[e] = T.elen[e]; dt.enx[e] = T.enx[e]; dt.eny[e] = T.eny[e]; }
    for (int sh = 0; sh < 2; sh++) for (int e = 0; e < 3; e++) dt.sig[sh][e] = T.sig[sh][e];
    dt.h = T.h; dt.tau = T.tau; dt.alpha = T.alpha; dt.nqc = T.nqc; dt.nqe = T.nqe;
  }

  void alloc_state() {
    curQ = dalloc(NQ); curP = dalloc(NPv); curL = dalloc(NLv);
    for (int i = 0; i < s; i++) {
      stQ.push_back(dalloc(NQ)); stP.push_back(dalloc(NPv)); stL.push_back(dalloc(NLv));
      Qtent.push_back(dalloc(NQ));
      if (i < s - 1 || s == 1) Qstar.push_back(dalloc(NQ));
    }
    for (int i = 0; i <= s; i++) { brhs.push_back(dalloc(NQ)); bscale.push_back(1.0); bsep.push_back(0); }
    ch.assign((size_t)s + 1, ChebStage{});
    profile = dalloc(NQ);
    updU = dalloc(NQ); updP = dalloc(NPv); updL = dalloc(NLv); recP = dalloc(NPv); recL = dalloc(NLv);
    wQ1 = dalloc(NQ); wQ2 = dalloc(NQ); wQ3 = dalloc(NQ); wQ4 = dalloc(NQ);
    wP1 = dalloc(NPv); wL1 = dalloc(NLv); wL2 = dalloc(NLv);
    cg_r = dalloc(NLv); cg_z = dalloc(NLv); cg_p = dalloc(NLv); cg_Ap = dalloc(NLv);
    ch_d = dalloc(NLv); ch_r = dalloc(NLv); tr_one = dalloc(NLv);
    ones_c = dalloc(g.Nc);
    cell_ss = dalloc(g.Nc);
    k_fill<<<vec_blocks(g.Nc), 256, 0, stream>>>(g.Nc, ones_c, 1.0);
    d_ones_ptr = upload_ptrs({ones_c});
    int m = std::max(1, cfg.gmres_restart);
    m = std::min(m, MAXV - 1);
    for (int i = 0; i <= m; i++) gm_V.push_back(dalloc(NQ));
    {
      std::vector<const double*> pv(gm_V.begin(), gm_V.end());
      pv.push_back(nullptr);
      pv.push_back(nullptr);
      d_gmV = upload_ptrs(pv);
    }
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, sizeof(double*) * (std::max(m, MAXV) + 2)));
    allocs.push_back(p);
    d_ptrs = (const double**)p;
    dot_blocks = 8192;
    d_part = dalloc((long)dot_blocks * MAXV);
    d_res = dalloc(MAXV);
    HIPCHECK(hipHostMalloc((void**)&h_res, sizeof(double) * MAXV));
    d_cgs = dalloc(8);
    HIPCHECK(hipHostMalloc((void**)&h_cgs, sizeof(double) * 8));
    HIPCHECK(hipEventCreateWithFlags(&cg_ev, hipEventDisableTiming));
    hQ_dev = dalloc(NQb); hP_dev = dalloc(NPb);
    hL_dev = dalloc(NLb);
    {
      long cap = std::max<long>(GH * 2L * NU * 2L * g.nx, GH * 3L * NL * g.P);  // up to GH / GH rows per message
      cap_halo = (size_t)cap;
      hb_slo = dalloc(cap); hb_shi = dalloc(cap); hb_rlo = dalloc(cap); hb_rhi = dalloc(cap);
    }
    for (int i = 0; i < s; i++) { dinv0.push_back(nullptr); dinv1.push_back(nullptr); hybg0.push_back(nullptr); hybg1.push_back(nullptr); dinv_gamma.push_back(-1.0); }
  }

  // ------------------------------------------------------------------ kernel dispatch on K
  // (hdg_dispatch.hpp; f receives the degree as a type: k_name<k()>)
  template <class F> void by_degree(F&& f) const { with_int<1, 2, 3, 4>(K, "degree", f); }
  template <class F> void by_mfma_degree(F&& f) const { with_int<3, 4>(K, "degree of a matrix-core kernel", f); }
  template <class F> void by_pair_degree(F&& f) const { with_int<1, 2>(K, "degree of a pair kernel", f); }
  // condense / backsub <K, HAS_W, HAS_P>: which of the right-hand sides r_w, r_p is there.  Three instantiations, not four:
  // a call with neither runs the one for both (the kernels test the pointers they are given)
  enum { RHS_W = 0, RHS_P = 1, RHS_BOTH = 2 };
  template <class F> static void by_rhs(const double* rw, const double* rp, F&& f) {
    with_int<RHS_W, RHS_P, RHS_BOTH>((rw && !rp) ? RHS_W : ((!rw && rp) ? RHS_P : RHS_BOTH), "right-hand sides", f);
  }

  // ------------------------------------------------------------------ halo rows (strip partition)
  // Policy: every stencil operator refreshes the ghost rows of the vectors whose neighbour values it
  // reads; kernels write owned rows only.  (Pure vector updates act on ghosts too, which keeps
  // consistent copies consistent.)
  bool halo_on = true;  // switched off while timing bare kernel launches (hdg_time_kernel is not collective)
  long n_halo[3] = {0, 0, 0}, n_reduce = 0, n_gather = 0;  // communication census (HDG_DEBUG, printed at destruction)
  long n_halo_mg = 0;  // vertex-row exchanges of the distributed V-cycle level (their own counter: not pressure halos)
  long n_tile_precond = 0;  // applications of the LDS-tiled trace preconditioner (census; the multi-rank tests assert it ran)
  // ------------------------------------------------------------------ launch census (hdg_get_launch_stats)
  // Launches and ALGORITHMIC bytes per kernel class: every logical vector read or written once per launch, 8 B per OWNED
  // entry (no ghost / padding rows), shared operator tables free -- SURVEY.md section 8(d).  bench.py's whole-step roofline is
  // sum_k bytes_k / elapsed / peak with calls_k printed alongside.  Classes follow the kernel list K1..K9 of SURVEY 7.3.
  enum { LC_ADV = 0, LC_LIFT, LC_RHS, LC_WDIV, LC_CONDENSE, LC_TRACE_APPLY, LC_TRACE_SMOOTH, LC_BACKSUB, LC_MG, LC_VEC, LC_DOT,
         LC_COPY, LC_OTHER, LC_N };
  long lc_calls[HDG_N_LAUNCH_CLASSES] = {0};
  double lc_bytes[HDG_N_LAUNCH_CLASSES] = {0};
  static_assert(LC_N == HDG_N_LAUNCH_CLASSES, "launch classes out of step with the header");
  void tally(int c, double bytes) { lc_calls[c]++; lc_bytes[c] += bytes; }
  double bQ() const { return 8.0 * (double)NQb; }
  double bP() const { return 8.0 * (double)NPb; }
  double bL() const { return 8.0 * (double)NLb; }
  // bytes of one pass over a whole-array vector of allocated length n (owned entries only)
  double bvec(long n) const {
    if (n == NQ) return bQ();
    if (n == NPv) return bP();
    if (n == NLv) return bL();
    if (n == g.Nc) return 8.0 * 2.0 * g.nx * g.ny;
    return 8.0 * (double)n;
  }
  // The one place that decides whether this strip has a lower / upper neighbour: on the unit square every rank but the
  // bottom / top one; on the periodic square always -- the ring neighbours on P > 1 ranks, the strip's own opposite side on
  // one rank (k_wrap_rows; every use of the answer on one rank sits behind a comm->size > 1 test or is the tile kernels' wrap)
  bool has_lo() const { return periodic || (comm->size > 1 && comm->rank > 0); }
  bool has_hi() const { return periodic || (comm->size > 1 && comm->rank < comm->size - 1); }
  void halo_rows(double* v, long plane_stride, int row_len, int nplanes, int kind, int depth = 1, int gh = GH) {
    if (periodic && comm->size == 1 && halo_on) {  // ghost rows = the owned rows of the opposite side
      k_wrap_rows<<<std::min(vec_blocks((long)nplanes * row_len * gh), 512), 256, 0, stream>>>(v, plane_stride, row_len, nplanes, g.ny, gh);
      return;
    }
    if (comm->size == 1 || !halo_on) return;
    if (depth < 1 || depth > gh || depth > g.ny) throw std::string("halo depth out of range (a strip needs at least as many rows)");
    const long n = (long)nplanes * row_len * depth;
    if ((size_t)n > cap_halo) throw std::string("halo buffer too small");
    const int nb = vec_blocks(n);
    n_halo[kind]++;
    // 3 launches per exchange: pack both messages, neighbour send/recv, unpack both messages.  Array rows: owned rows are
    // gh .. gh+ny-1; the lowest `depth` owned rows go down into the lower neighbour's rows gh+ny .. gh+ny+depth-1, the
    // highest `depth` go up into the upper neighbour's rows gh-depth .. gh-1.
    const int nbh = std::min(nb, 256);
    k_pack_rows<<<dim3(nbh, 2), 256, 0, stream>>>(v, plane_stride, row_len, nplanes, depth, gh, gh + g.ny - depth, hb_slo, hb_shi);
    comm->exchange(hb_slo, hb_rlo, hb_shi, hb_rhi, (size_t)n, stream);
    k_unpack_rows<<<dim3(nbh, 2), 256, 0, stream>>>(v, plane_stride, row_len, nplanes, depth, has_lo() ? gh - depth : -1,
                                                    has_hi() ? gh + g.ny : -1, hb_rlo, hb_rhi);
  }
  // ---- self-check of the ghost-row bookkeeping (HDG_FLOW_CHECK=1, tests): whenever a stencil input is NOT exchanged because
  // the bookkeeping calls its ghost rows valid, exchange anyway into the receive buffers and compare with what is there.
  // The worst relative deviation of a solve is checked when its FlowScope closes (redundantly computed rows agree to
  // rounding); a stale validity shows up as an O(1) deviation and fails the call.
  unsigned long long* d_fc = nullptr;
  long fc_count = 0;
  double fc_worst = 0.0;
  void halo_rows_compare(const double* v, long plane_stride, int row_len, int nplanes, int depth, int gh = GH) {
    if (comm->size == 1 || !halo_on || depth < 1) return;
    const long n = (long)nplanes * row_len * depth;
    if ((size_t)n > cap_halo) throw std::string("halo buffer too small");
    if (!d_fc) d_fc = reinterpret_cast<unsigned long long*>(dalloc(2));
    const int nbh = std::min(vec_blocks(n), 256);
    k_pack_rows<<<dim3(nbh, 2), 256, 0, stream>>>(v, plane_stride, row_len, nplanes, depth, gh, gh + g.ny - depth, hb_slo, hb_shi);
    comm->exchange(hb_slo, hb_rlo, hb_shi, hb_rhi, (size_t)n, stream);
    k_compare_rows<<<dim3(nbh, 2), 256, 0, stream>>>(v, plane_stride, row_len, nplanes, depth, has_lo() ? gh - depth : -1,
                                                     has_hi() ? gh + g.ny : -1, hb_rlo, hb_rhi, d_fc);
    fc_count++;
  }
  void flow_check_input(const double* in, int kind, int depth) {
    if (kind == FQ_) halo_rows_compare(in, 2L * g.R * g.nx, 2 * g.nx, NU * 2, depth);
    else if (kind == FP_) halo_rows_compare(in, (long)g.R * g.nx, g.nx, NP * 2, depth);
    else halo_rows_compare(in, g.G, g.P, 3 * NL, depth);
  }
  void flow_check_close() {  // end of a solver scope: read the result back, fail on a stale ghost row
    if (!opt.flow_check || !d_fc || comm->size == 1) return;
    unsigned long long h[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(h, d_fc, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    HIPCHECK(hipMemsetAsync(d_fc, 0, sizeof(h), stream));
    double dmax, amax;
    std::memcpy(&dmax, &h[0], 8); std::memcpy(&amax, &h[1], 8);
    const double rel = amax > 0 ? dmax / amax : dmax;
    fc_worst = std::max(fc_worst, rel);
    if (rel > 1e-9) throw std::string("ghost-row bookkeeping: a vector was treated as valid on ghost rows that differ from the neighbour's rows");
  }
  enum { FQ_ = 0, FP_ = 1, FL_ = 2 };
  // velocity: component-pair layout -> a row of one (mode, shape) plane is 2 nx doubles
  void halo_Q(const double* v, int depth = 1) { halo_rows(const_cast<double*>(v), 2L * g.R * g.nx, 2 * g.nx, NU * 2, 0, depth); }
  void halo_P(const double* v) { halo_rows(const_cast<double*>(v), (long)g.R * g.nx, g.nx, NP * 2, 1); }
  void halo_L(const double* v, int depth = 1) { halo_rows(const_cast<double*>(v), g.G, g.P, 3 * NL, 2, depth); }

  // ------------------------------------------------------------------ ghost-row bookkeeping of the solvers (strip partition)
  // Inside a solver (FlowScope: tentative-velocity GMRES / Chebyshev, trace CG) every vector carries the number of ghost
  // rows on which it currently holds the right values.  A row stencil (advection operator, edge lift, trace operator,
  // fused smoother step) reads its input one row beyond the rows it computes: it is launched over as many ghost rows as
  // its inputs allow (Geo::elo / ehi) and its result is valid there; pointwise kernels and the whole-array vector
  // updates pass the validity of their inputs on.  Only a stencil input with NO valid ghost row triggers an exchange,
  // fl.Dx rows deep.  Dx = DX_DEFAULT = 4 (the arrays carry GH = 6 ghost rows: the tiled trace preconditioner exchanges 5):
  //   velocity: x_n exchanged -> b - A x_n on 3 ghost rows -> lift + Chebyshev step on 2 -> operator on 1 -> lift on 0:
  //             one exchange per TWO iterations (the odd iterates stay valid on 2 rows, which the three-term step needs);
  //   trace CG: z exchanged -> w = T z on 3 -> r on 3 -> pre-smoother 3 -> 2 -> coarse correction on 2 -> post-smoother
  //             1 -> 0: one exchange per iteration.
  // Redundant work: 6 row launches of operator + lift per two velocity iterations and side, 18 per CG iteration.
  // Strips of 2-3 rows use Dx = ny; Dx = 1 (HDG_NO_EXT, periodic wrap, outside a FlowScope) is the classic exchange
  // before every stencil.  A vector the bookkeeping has not seen counts as 0: the default is always the safe one.
  // an exchange stencil_in() has decided on but left to its caller (stencil_launch: beside the interior launch)
  struct Pending { bool on = false; const double* v = nullptr; int kind = 0, depth = 0; };
  struct Flow {
    int nest = 0, Dx = 1;
    std::vector<std::pair<const double*, int>> v;
    bool active() const { return nest > 0; }
    int get(const double* p) const {
      if (nest > 0) for (const auto& e : v) if (e.first == p) return e.second;
      return 0;
    }
    void set(const double* p, int d) {
      if (nest == 0 || !p) return;
      for (auto& e : v) if (e.first == p) { e.second = d; return; }
      v.emplace_back(p, d);
    }
  } fl;
  struct FlowScope {
    Engine& E;
    explicit FlowScope(Engine& e) : E(e) {
      if (E.fl.nest++ == 0) {
        E.fl.v.clear();
        E.fl.Dx = (!E.opt.ext || E.comm->size == 1 || !E.halo_on) ? 1 : std::min(DX_DEFAULT, E.g.ny);
      }
    }
    ~FlowScope() noexcept(false) {
      if (--E.fl.nest == 0) {
        E.fl.v.clear();
        if (E.opt.flow_check && !std::uncaught_exceptions()) E.flow_check_close();
      }
    }
  };
  enum { FQ = 0, FP = 1, FL = 2 };
  // input of a row stencil: at least one valid ghost row; returns the number of ghost rows the stencil may compute
  int stencil_in(const double* in, int kind, Pending* defer = nullptr) {
    const int depth = fl.active() ? fl.Dx : 1;
    if (!fl.active() || fl.get(in) < 1) {
      const bool real_exchange = comm->size > 1 && halo_on;
      if (defer && real_exchange && overlap_on && kind != FP) {
        defer->on = true; defer->v = in; defer->kind = kind; defer->depth = depth;  // the caller runs it (halo_run)
      } else {
        if (kind == FQ) halo_Q(in, depth); else if (kind == FP) halo_P(in); else halo_L(in, depth);
      }
      fl.set(in, kind == FP ? 1 : depth);
    } else if (opt.flow_check) {
      flow_check_input(in, kind, fl.get(in));  // no exchange needed, says the bookkeeping: verify
    }
    return fl.active() ? fl.get(in) - 1 : 0;
  }
  // further input read on the computed rows only
  int pw_in(const double* in, int ext) const { return in ? std::min(ext, fl.get(in)) : ext; }
  // a vector that stays fixed through a solve (right-hand side, advecting velocity): valid on every row a stencil can reach
  void flow_fixed_Q(const double* v) {
    if (fl.active() && fl.Dx > 1 && fl.get(v) < fl.Dx - 1) { halo_Q(v, fl.Dx - 1); fl.set(v, fl.Dx - 1); }
  }
  Geo g_ext(int ext) const {  // this launch's geometry: ext ghost rows towards every existing neighbour
    Geo c = g;
    if (comm->size > 1 && ext > 0) {
      c.elo = has_lo() ? ext : 0;
      c.ehi = has_hi() ? ext : 0;
      c.rows_xcd = (c.ny + c.elo + c.ehi + 7) / 8;
      c.rows_xcdc = (c.nyc + c.elo + c.ehi + 7) / 8;
      c.wrows = c.ny + c.elo + c.ehi;
      c.wrowsc = c.nyc + c.elo + c.ehi;
    }
    return c;
  }
  // ---- interior / boundary split of a stencil launch whose input is being exchanged (strip partition, SURVEY.md 5.8:
  // "interior elements computed while cut-edge data is in flight").  Rows whose stencil reads owned rows of the input only:
  // cells j in [lo, ny - hi), corners j in [lo, nyc - hi) with lo / hi = 1 where a neighbour exists.  The interior launch
  // runs on the compute stream while pack -> send/recv -> unpack run on the communication stream; the boundary launch
  // (ghost rows and the first / last owned row, ONE launch with a gap over the interior) waits for the unpack.
  bool can_split(const Geo& full) const {
    const int lo = has_lo() ? 1 : 0, hi = has_hi() ? 1 : 0;
    return overlap_on && comm->size > 1 && full.ny - lo - hi >= 2 && (full.elo + lo + full.ehi + hi) > 0;
  }
  Geo window_interior(const Geo& full) const {
    Geo c = full;
    const int lo = has_lo() ? 1 : 0, hi = has_hi() ? 1 : 0;
    c.wskip = full.elo + lo; c.wgap0 = 0; c.wgapn = 0;
    c.wrows = full.ny - lo - hi;
    c.wrowsc = full.nyc - lo - hi;
    c.rows_xcd = (c.wrows + 7) / 8;
    c.rows_xcdc = (c.wrowsc + 7) / 8;
    return c;
  }
  Geo window_boundary(const Geo& full) const {
    Geo c = full;
    const int lo = has_lo() ? 1 : 0, hi = has_hi() ? 1 : 0;
    c.wskip = 0;
    c.wgap0 = full.elo + lo;                    // the rows below the interior ...
    c.wgapn = full.ny - lo - hi;                // ... then skip it (cells)
    c.wrows = full.elo + lo + hi + full.ehi;
    c.wrowsc = c.wrows;                         // corners: the gap is nyc - lo - hi rows long (set by the corner launches)
    c.rows_xcd = (c.wrows + 7) / 8;
    c.rows_xcdc = (c.wrowsc + 7) / 8;
    return c;
  }
  static Geo corner_gap(Geo c, const Geo& full, int lo, int hi) { c.wgapn = full.nyc - lo - hi; return c; }
  hipStream_t cstream = nullptr;               // communication stream (exchanges that overlap with interior launches)
  hipEvent_t ev_in = nullptr, ev_halo = nullptr;
  // Opt-in (HDG_OVERLAP=1; every multi-rank test sets it): over RCCL it has never run on two devices; over the host-staged
  // shared-memory transport (ranks SHARING a device) the interior launch occupies the very GPU the peer needs for its pack
  // kernel (C3 rehearsal, 2 ranks on one MI355X: 226 ms/step with the split, 178 without).  HDG_NO_OVERLAP=1 forbids it.
  bool overlap_on = false;
  long n_overlapped = 0;                        // exchanges that ran beside an interior launch (census)
  // the deferred exchange of stencil_in(): runs on the communication stream after everything queued on the compute stream
  // so far (the producer of v); the compute stream continues and waits in halo_finish()
  void halo_run(const Pending& pd) {
    if (!pd.on) return;
    if (!cstream) {
      HIPCHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
      HIPCHECK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
      HIPCHECK(hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming));
    }
    HIPCHECK(hipStreamWaitEvent(cstream, ev_in, 0));
    hipStream_t saved = stream;
    stream = cstream;  // halo_rows packs / exchanges / unpacks on `stream`
    try {
      if (pd.kind == FQ) halo_Q(pd.v, pd.depth); else halo_L(pd.v, pd.depth);
    } catch (...) { stream = saved; throw; }
    stream = saved;
    HIPCHECK(hipEventRecord(ev_halo, cstream));
    HIPCHECK(hipStreamWaitEvent(stream, ev_halo, 0));
    n_overlapped++;
  }
  void halo_mark(const Pending& pd) {  // the producer of pd.v has been queued: everything before this point
    if (!pd.on) return;
    if (!cstream) {
      HIPCHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
      HIPCHECK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
      HIPCHECK(hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming));
    }
    HIPCHECK(hipEventRecord(ev_in, stream));
  }
  // a stencil launch with its input exchange overlapped: launch(const Geo&) is called once (no exchange needed, or no split)
  // or twice (interior, then boundary after the exchange)
  template <class L>
  void stencil_launch(const double* in, int kind, int max_ext, bool corner, const std::vector<const double*>& pw, L&& launch,
                      int* ext_out) {
    Pending pd;
    int ext = std::min(stencil_in(in, kind, &pd), max_ext);
    for (const double* q : pw) ext = pw_in(q, ext);
    const Geo full = g_ext(ext);
    if (ext_out) *ext_out = ext;
    if (pd.on && can_split(full)) {
      const int lo = has_lo() ? 1 : 0, hi = has_hi() ? 1 : 0;
      halo_mark(pd);
      launch(window_interior(full));
      halo_run(pd);
      launch(corner ? corner_gap(window_boundary(full), full, lo, hi) : window_boundary(full));
    } else {
      if (pd.on) { halo_mark(pd); halo_run(pd); }
      launch(full);
    }
  }
  dim3 cell_grid_of(const Geo& c) const { return dim3(8 * c.rows_xcd * 2 * c.nbx, 1, 1); }
  static dim3 corner_grid_of(const Geo& c) { return dim3(8 * c.rows_xcdc * c.nbxc, 1, 1); }

  // ---- matrix-core kernels (k >= 3): device copies of the tables hdg_mfma_pack.hpp packs, uploaded on first use
  const double *pgm[2] = {nullptr, nullptr}, *wdm[2] = {nullptr, nullptr}, *wdbm[2] = {nullptr, nullptr};
  // HDG_NO_MFMA_SCHUR: the per-thread kernels at every degree (A/B timing, parity of the two formulations)
  bool use_mfma_schur() const {
    return opt.mfma_schur && cfg.degree >= MFMA_MIN_DEGREE && !periodic && !general;  // the matrix-core kernels do not wrap column indices
  }
  void ensure_schur_tables(PSet& ps) {
    if (ps.bsm[0]) return;
    // the device tables of a set mirror host data that is recomputed here (the host side keeps only the default set)
    for (int sh = 0; sh < 2; sh++) {
      dvec Ai, W_, Y_, SK_;
      tab->poissonBlock(sh, ps.tau, Ai, W_, Y_, SK_);
      ps.bsm[sh] = upload(pack_backsub_mfma(*tab, Ai, W_));
      if (sh == 0) schur_Y0 = Y_; else ps.cdm = upload(pack_condense_mfma(*tab, schur_Y0, Y_));
    }
  }
  dvec schur_Y0;
  dim3 schur_cell_grid() const { return dim3(8 * g.rows_xcd * 2); }
  dim3 schur_corner_grid() const { return dim3(8 * g.rows_xcdc); }
  const double* advm[2] = {nullptr, nullptr};
  const double* liftm_plain[2] = {nullptr, nullptr};  // packed tables of the plain BDM projection
  std::vector<double*> liftm_hyb0, liftm_hyb1;         // per stage: hybrid preconditioner
  bool use_mfma_lift() const {
    return opt.mfma_lift && cfg.degree >= MFMA_MIN_DEGREE && !periodic && !general;  // the matrix-core kernels do not wrap column indices
  }
  static constexpr int MFMA_MIN_DEGREE = 3;  // the matrix-core kernels at k = 2 were 1.8-2 x slower
  // k >= 3: the whole operator on the matrix cores (k_adv_mfma); HDG_NO_MFMA_ADV falls back to the per-thread kernels
  bool use_mfma_adv() const { return opt.mfma_adv && cfg.degree >= MFMA_MIN_DEGREE && !periodic && !general; }
  bool lift_pair() const { return opt.lift_pair && K <= 2 && bs() == 128 && !general; }
  // Which form of the lift and of the advection operator runs: decided here, launched by bdm / bdm_hybrid / adv_apply and
  // reported by hdg_get_kernel_forms.  The enumerators of LiftForm are the integers of that call.  The two-lane advection
  // form (k_adv_apply2) has no code of its own yet and reports 0 like the per-thread form: ADVICE.md, fourth finding.
  enum class LiftForm { per_thread = 0, pair = 1, mfma = 2, general = 3 };
  enum class AdvForm { per_thread, two_lane, mfma, general };
  LiftForm lift_form() const {
    return general ? LiftForm::general : use_mfma_lift() ? LiftForm::mfma : lift_pair() ? LiftForm::pair : LiftForm::per_thread;
  }
  AdvForm adv_form() const {
    if (general) return AdvForm::general;
    if (use_mfma_adv()) return AdvForm::mfma;
    // without the matrix-core kernel: two lanes per cell, one velocity component each, at the degrees of opt.adv_split_*
    return (K >= opt.adv_split_lo && K <= opt.adv_split_hi) ? AdvForm::two_lane : AdvForm::per_thread;
  }
  static int form_code(AdvForm f) { return f == AdvForm::general ? 3 : (f == AdvForm::mfma ? 2 : 0); }
  void lift_mfma(const Geo& gx, const double* t0, const double* t1, const double* in, double* out, double* chd_ = nullptr,
                 const double* chx_ = nullptr, double c1 = 0.0, double c2 = 0.0) {
    const dim3 grid(8 * gx.rows_xcd * 2);
    by_mfma_degree([&](auto k) {
      if (chd_) k_edge_lift_mfma<k(), true><<<grid, 64 * HDG_LIFT_MFMA_WAVES, 0, stream>>>(gx, t0, t1, in, out, chd_, chx_, c1, c2);  // with the fused Chebyshev step
      else k_edge_lift_mfma<k()><<<grid, 64 * HDG_LIFT_MFMA_WAVES, 0, stream>>>(gx, t0, t1, in, out);
    });
  }
  void g_lift_apply(const double* Gt, const double* x, double* out) {
    tally(LC_LIFT, 2 * bQ() + 8.0 * (double)gm->nc * 2 * NU * 3 * NE);
    by_degree([&](auto k) { k_g_lift<k()><<<(gm->nc + 63) / 64, 64, 0, stream>>>(ggeo, g_nref, Gt, x, out); });
  }
  void bdm(const double* in, double* out) {
    const LiftForm form = lift_form();
    if (form == LiftForm::general) {
      if (g_lift) g_lift_apply(g_lift, in, out);
      else csr(gd.Pi, in, 1.0, 0.0, out);
      return;
    }
    const int ext = stencil_in(in, FQ);
    const Geo gx = g_ext(ext);
    fl.set(out, ext);
    tally(LC_LIFT, 2 * bQ());
    switch (form) {
      case LiftForm::mfma:
        if (!liftm_plain[0])
          for (int sh = 0; sh < 2; sh++) liftm_plain[sh] = upload(pack_lift_mfma(*tab, sh, tab->Lift[sh]));
        lift_mfma(gx, liftm_plain[0], liftm_plain[1], in, out);
        break;
      case LiftForm::pair:
        by_pair_degree([&](auto k) { k_edge_lift_pair<k(), false, 0, false><<<cell_grid_of(gx), 128, 0, stream>>>(gx, dt, in, out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, nullptr); });
        break;
      default:
        by_degree([&](auto k) { k_edge_lift<k(), false, 0, false><<<cell_grid_of(gx), bs(), 0, stream>>>(gx, dt, in, out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, nullptr); });
    }
  }
  // rows a lift with the optional Chebyshev epilogue may compute (chd_ = x_{n-1} -> x_{n+1}, chx_ = x_n)
  int lift_ext(const double* in, const double* r, const double* chd_, const double* chx_, double c1) {
    int ext = stencil_in(in, FQ);
    ext = pw_in(r, ext);
    if (chd_) { ext = pw_in(chx_, ext); if (c1 != 0.0) ext = pw_in(chd_, ext); }
    return ext;
  }
  // algorithmic bytes of a lift: reads in (+ r), writes out if given; Chebyshev epilogue: reads x_n (and x_{n-1} unless
  // c1 == 0), writes x_{n+1}
  double lift_bytes(bool has_r, bool has_out, bool cheb, double c1) const {
    return bQ() * (1 + (has_r ? 1 : 0) + (has_out ? 1 : 0) + (cheb ? (c1 != 0.0 ? 3 : 2) : 0));
  }
  // out = Pi(in) + Dinv r   (second half of the two-level preconditioner, block-Jacobi fused in)
  void bdm_plus_bj(const double* in, double* out, const double* r, const double* D0, const double* D1,
                   double* chd_ = nullptr, double* chx_ = nullptr, double c1 = 0.0, double c2 = 0.0) {
    const int ext = lift_ext(in, r, chd_, chx_, c1);
    const Geo gx = g_ext(ext);
    tally(LC_LIFT, lift_bytes(true, out != nullptr, chd_ != nullptr, c1));
    by_degree([&](auto k) { with_bool(chd_ != nullptr, [&](auto cheb) {
      k_edge_lift<k(), false, 1, cheb()><<<cell_grid_of(gx), bs(), 0, stream>>>(gx, dt, in, out, r, D0, D1, chd_, chx_, c1, c2, nullptr);
    }); });
    fl.set(out, ext); fl.set(chd_, ext);
  }
  // hybrid two-level preconditioner in ONE kernel: out = Pi(in) + Dinv (in - Pi(in)) = in + sum_e G_e d_e(in),
  // optionally fused with the Chebyshev step; G0 / G1: tables (I - Dinv_s) Lift_e of the stage (ensure_dinv)
  void bdm_hybrid(const double* in, double* out, const double* D0, const double* D1, double* chd_ = nullptr,
                  double* chx_ = nullptr, double c1 = 0.0, double c2 = 0.0, double* ss = nullptr) {
    // Chebyshev mode: the lift of an iteration carries the fused step (per-thread kernel) or is the matrix-core kernel
    // followed by the vector-kernel step; GMRES mode: the plain lift
    KTimed kt_(*this, chd_ != nullptr ? T_KLIFT : T_KLIFT_PLAIN, fl.active() && (chd_ != nullptr || (out && !ss)));
    tally(LC_LIFT, lift_bytes(false, out != nullptr, chd_ != nullptr, c1));
    std::vector<const double*> pw;
    if (chd_) { pw.push_back(chx_); if (c1 != 0.0) pw.push_back(chd_); }
    int ext = 0;
    const LiftForm form = lift_form();
    stencil_launch(in, FQ, GH, false, pw, [&](const Geo& gx) {
      if (form == LiftForm::mfma && !ss && (out || chd_)) {
        // k >= 3: matrix-core kernel with the packed G tables of this stage (GMRES path: plain; Chebyshev path: fused step)
        for (size_t q = 0; q < hybg0.size(); q++)
          if (hybg0[q] == D0) { lift_mfma(gx, liftm_hyb0[q], liftm_hyb1[q], in, out, chd_, chx_, c1, c2); return; }
      }
      if (form == LiftForm::pair) {  // k <= 2, 128-thread workgroups: both triangles of a square in one workgroup, moments through LDS
        by_pair_degree([&](auto k) { with_bool(chd_ != nullptr, [&](auto cheb) {
          k_edge_lift_pair<k(), false, 2, cheb()><<<cell_grid_of(gx), 128, 0, stream>>>(gx, dt, in, out, nullptr, D0, D1, chd_, chx_, c1, c2, ss);
        }); });
        return;
      }
      by_degree([&](auto k) { with_bool(chd_ != nullptr, [&](auto cheb) {
        k_edge_lift<k(), false, 2, cheb()><<<cell_grid_of(gx), bs(), 0, stream>>>(gx, dt, in, out, nullptr, D0, D1, chd_, chx_, c1, c2, ss);
      }); });
    }, &ext);
    fl.set(out, ext); fl.set(chd_, ext);
  }
  void bdm_T(const double* in, double* out) {
    if (general) general_unsupported("the transposed lift (additive preconditioner)");
    const int ext = stencil_in(in, FQ);
    const Geo gx = g_ext(ext);
    tally(LC_LIFT, 2 * bQ());
    by_degree([&](auto k) { k_edge_lift<k(), true, 0, false><<<cell_grid_of(gx), bs(), 0, stream>>>(gx, dt, in, out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, nullptr); });
    fl.set(out, ext);
  }
  void adv_apply(const double* x, const double* qstar, double* out, double gamma, const double* bsub = nullptr) {
    KTimed kt_(*this, bsub != nullptr ? T_KADV : T_KADV_PLAIN, fl.active());
    const double up = cfg.flux_upwind ? 1.0 : 0.0;
    tally(LC_ADV, bQ() * (bsub ? 4 : 3));
    const AdvForm form = adv_form();
    if (form == AdvForm::general) {
      by_degree([&](auto k) { k_g_adv<k()><<<(ggeo.nc + 63) / 64, 64, 0, stream>>>(ggeo, x, qstar, out, gamma, up, bsub); });
      fl.set(out, 0);
      return;
    }
    if (form == AdvForm::mfma && !advm[0]) {
      if (dt.nqc != (cfg.degree == 3 ? 36 : 64)) throw std::string("cell quadrature size does not match the matrix-core advection kernel");
      if (dt.nqe != (3 * cfg.degree + 5) / 2) throw std::string("edge quadrature size does not match the matrix-core advection kernel");
      for (int sh = 0; sh < 2; sh++) advm[sh] = upload(pack_adv_mfma(*tab, sh));
    }
    int ext = 0;
    // the launch of one row window (the whole extended strip, or interior / boundary rows around the exchange of x)
    stencil_launch(x, FQ, GH, false, {qstar, bsub}, [&](const Geo& g) {  // shadows the member on purpose
      switch (form) {
        case AdvForm::mfma: {
          const dim3 gridc(8 * g.rows_xcd * 2);
          by_mfma_degree([&](auto k) { with_bool(bsub != nullptr, [&](auto resid) {
            k_adv_mfma<k(), resid()><<<gridc, 512, 0, stream>>>(g, dt, advm[0], advm[1], x, qstar, out, gamma, up, bsub);
          }); });
          break;
        }
        case AdvForm::two_lane: {
          const int cpb = bs() / 2, nbx2 = (g.nx + cpb - 1) / cpb;
          by_degree([&](auto k) { k_adv_apply2<k()><<<dim3(8 * g.rows_xcd * 2 * nbx2), bs(), 0, stream>>>(g, dt, x, qstar, out, gamma, up, bsub); });
          break;
        }
        default:
          by_degree([&](auto k) { with_bool(bsub != nullptr, [&](auto resid) {
            k_adv_apply<k(), resid()><<<cell_grid_of(g), bs(), 0, stream>>>(g, dt, x, qstar, out, gamma, up, bsub);
          }); });
      }
    }, &ext);
    fl.set(out, ext);
  }
  void blockdiag(const double* D0, const double* D1, const double* r, const double* zin, double cz, double* out) {
    tally(LC_LIFT, bQ() * (zin ? 3 : 2));
    by_degree([&](auto k) { k_blockdiag<k()><<<cell_grid(), bs(), 0, stream>>>(g, D0, D1, r, zin, cz, out); });
    fl.set(out, 0);
  }
  void pgrad(const double* a, double ca, const double* b, double cb, const double* p, const double* l, double gamma,
             double* out) {
    if (general) {
      lincomb(NQ, {{a, a ? ca : 0.0}, {b, b ? cb : 0.0}}, out);
      csr(gd.Gp, p, gamma, 1.0, out);
      csr(gd.Gl, l, gamma, 1.0, out);
      return;
    }
    halo_L(l);
    tally(LC_RHS, bQ() * (1 + (a ? 1 : 0) + (b ? 1 : 0)) + bP() + bL());
    if (use_mfma_schur()) {
      if (!pgm[0]) for (int sh = 0; sh < 2; sh++) pgm[sh] = upload(pack_pgrad_mfma(*tab, sh));
      by_mfma_degree([&](auto k) { k_pgrad_mfma<k()><<<schur_cell_grid(), 64 * HDG_SCHUR_WAVES, 0, stream>>>(g, pgm[0], pgm[1], a, ca, b, cb, p, l, gamma, out); });
      return;
    }
    by_degree([&](auto k) { k_pgrad<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, a, ca, b, cb, p, l, gamma, out); });
  }
  // the pressure gradient that takes the neighbouring linear combination into its own launch exists in the per-thread form at
  // k <= 2 only (k_pgrad_terms)
  bool glue_kernels() const { return opt.glue_fusion && !general && K <= 2 && !use_mfma_schur(); }
  // out = (sum of terms) - b + gamma g(p, l) in one launch: the sum is formed in registers with the chain of k_lincomb, the
  // rest is pgrad(sum, 1, b, -1, ...).  False: not this form (glue_kernels(); empty or chunked list) -- nothing launched.
  bool pgrad_terms(const Terms& terms, const double* b, const double* p, const double* l, double gamma, double* out) {
    LinComb lc;
    if (!glue_kernels() || !b || !single_chain(lincomb_terms(terms), lc)) return false;
    halo_L(l);
    tally(LC_RHS, bQ() * (2 + lc.n) + bP() + bL());
    by_degree([&](auto k) {
      if constexpr (k() <= 2) k_pgrad_terms<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, lc, b, p, l, gamma, out);
    });
    return true;
  }
  void weak_div(const double* q, double sc, double* out, bool broken) {
    if (general) { csr(broken ? gd.Bdiv : gd.Wdiv, q, sc, 0.0, out); return; }
    if (!broken) halo_Q(q);
    tally(LC_WDIV, bQ() + bP());
    if (use_mfma_schur()) {
      const double** tb = broken ? wdbm : wdm;
      if (!tb[0]) for (int sh = 0; sh < 2; sh++) tb[sh] = upload(pack_weakdiv_mfma(*tab, sh, broken));
      by_mfma_degree([&](auto k) { with_bool(broken, [&](auto br) {
        k_weak_div_mfma<k(), br()><<<schur_cell_grid(), 64 * HDG_SCHUR_WAVES, 0, stream>>>(g, tb[0], tb[1], q, sc, out);
      }); });
      return;
    }
    by_degree([&](auto k) { with_bool(broken, [&](auto br) { k_weak_div<k(), br()><<<cell_grid(), bs(), 0, stream>>>(g, dt, q, sc, out); }); });
  }
  void trace_apply(const double* lam, const double* base, double cb, double ct, double* out, int max_ext = GH) {
    if (general) {
      if (base && cb != 0.0) { if (out != base) copy(out, base, NLv); if (cb != 1.0) axpby(NLv, 0.0, out, cb, out); csr(gs().S, lam, ct, 1.0, out); }
      else csr(gs().S, lam, ct, 0.0, out);
      return;
    }
    tally(LC_TRACE_APPLY, bL() * (2 + ((base && cb != 0.0) ? 1 : 0)));
    std::vector<const double*> pw;
    if (cb != 0.0) pw.push_back(base);
    int ext = 0;
    stencil_launch(lam, FL, max_ext, true, pw, [&](const Geo& c) {
      by_degree([&](auto k) { k_trace_apply<k()><<<corner_grid_of(c), bs(), 0, stream>>>(c, pdt(), lam, base, cb, ct, out); });
    }, &ext);
    fl.set(out, ext);
  }
  // fused smoother step (k_trace_smooth): r = cb*base + ct*(-S) v, z = Dinv r, dn = c1 v + c2 z, optional outputs
  // mode 1: v is used as c0 * Dinv v (first step of the zero-start pre-smoother on the fly); mode 2: v is used as
  // v + P xc (coarse correction on the fly) and x (= v) receives that sum -- k_trace_smooth / trace_stencil
  void trace_smooth(const double* v, const double* base, double cb, double ct, double c1, double c2, double* r_out,
                    double* d_out, double* x, bool xadd, double xv, int mode = 0, double c0 = 0.0, const double* xc = nullptr,
                    const double* xin = nullptr) {
    if (general) general_unsupported("the fused trace smoother (multigrid preconditioner)");
    if (!xin) xin = x;
    if (mode == 2 && x == v) throw std::string("trace_smooth: mode 2 must not write the vector its neighbours read");
    const bool same_base = base == v;  // mode 1: the right-hand side is also the stencil input
    tally(LC_TRACE_SMOOTH, bL() * (1 + ((base && !same_base) ? 1 : 0) + (r_out ? 1 : 0) + (d_out ? 1 : 0) + (x ? ((xadd && mode != 2 && x != v) ? 2 : 1) : 0))
                               + (mode == 2 ? 8.0 * (g.nx + 1.0) * (g.ny + 1.0) : 0.0));
    std::vector<const double*> pw;
    if (cb != 0.0) pw.push_back(base);
    if (x && xadd && mode != 2) pw.push_back(xin);
    int ext = 0;
    StencilAux aux{0, c0, xc, std::sqrt(dt.elen[0]), std::sqrt(dt.elen[2]), std::sqrt(dt.elen[1])};
    const int xa = mode == 2 ? 2 : (xadd ? 1 : 0);
    // mode 2: the vertex-grid correction is valid on the strip and 3 rows around it: results on at most 2 ghost rows
    stencil_launch(v, FL, mode == 2 ? 2 : GH, true, pw, [&](const Geo& c) {
      by_degree([&](auto k) { with_int<0, 1, 2>(mode, "smoother mode", [&](auto md) {
        k_trace_smooth<k(), md()><<<corner_grid_of(c), bs(), 0, stream>>>(c, pdt(), v, base, cb, ct, c1, c2, r_out, d_out, x, xa, xv, aux, xin);
      }); });
    }, &ext);
    fl.set(r_out, ext); fl.set(d_out, ext); fl.set(x, ext);
  }
  void trace_cheb(const double* r, double* d, double* x, double c1, double c2, bool assign = false) {
    if (general) {
      csr(gs().Dtr, r, c2, c1, d);  // d = c1 d + c2 Dinv r
      if (x) { if (assign) copy(x, d, NLv); else axpby(NLv, 1.0, d, 1.0, x); }
      return;
    }
    int ext = pw_in(r, GH - 1);
    if (c1 != 0.0) ext = pw_in(d, ext);
    if (x && !assign) ext = pw_in(x, ext);
    const Geo c = g_ext(ext);
    tally(LC_TRACE_SMOOTH, bL() * (2 + (c1 != 0.0 ? 1 : 0) + (x ? (assign ? 1 : 2) : 0)));
    by_degree([&](auto k) { k_trace_cheb<k()><<<corner_grid_of(c), bs(), 0, stream>>>(c, pdt(), r, d, x, c1, c2, assign ? 1 : 0); });
    fl.set(d, ext); fl.set(x, ext);
  }
  // z (+)= prolongation of the (replicated, global) vertex vector: pointwise, on every row on which z is valid
  void p1_to_trace(const double* xc, double* z, double accumulate) {
    const int ext = accumulate != 0.0 ? pw_in(z, GH - 1) : (fl.active() ? fl.Dx - 1 : 0);
    const Geo c = g_ext(ext);
    tally(LC_MG, bL() * (accumulate != 0.0 ? 2 : 1) + 8.0 * (g.nx + 1.0) * (g.ny + 1.0));
    k_p1_to_trace<<<corner_grid_of(c), bs(), 0, stream>>>(c, NL, xc, z, accumulate, dt.elen[0], dt.elen[2], dt.elen[1]);
    fl.set(z, ext);
  }
  void condense(const double* rw, const double* rp, const double* rl, double* out) {
    if (general) {
      if (rl) axpby(NLv, -1.0, rl, 0.0, out); else zero(out, NLv);
      if (rw) csr(gs().Yw, rw, 1.0, 1.0, out);
      if (rp) csr(gs().Yp, rp, 1.0, 1.0, out);
      return;
    }
    if (rw) halo_Q(rw);
    if (rp) halo_P(rp);
    tally(LC_CONDENSE, (rw ? bQ() : 0.0) + (rp ? bP() : 0.0) + bL() * (rl ? 2 : 1));
    // Condensation stays with the per-thread kernel by default: it is a gather over four cells per corner that already runs at
    // 3.4-4.5 TB/s (512^2, us per launch, per-thread | matrix-core: pressure-row form k = 3 / 4: 15 / 21 | 31 / 46, velocity-row
    // form 40 / 61 | 48 / 61).  HDG_MFMA_CONDENSE=1 (read when the engine is built) selects the matrix-core kernel.
    if (opt.mfma_condense && use_mfma_schur() && (rw || rp)) {
      PSet& ps = psets[cur_pset];
      ensure_schur_tables(ps);
      by_mfma_degree([&](auto k) { by_rhs(rw, rp, [&](auto f) {
        k_condense_mfma<k(), f() != RHS_P, f() != RHS_W><<<schur_corner_grid(), 64 * HDG_SCHUR_WAVES, 0, stream>>>(g, ps.cdm, rw, rp, rl, out);
      }); });
      return;
    }
    by_degree([&](auto k) { by_rhs(rw, rp, [&](auto f) {
      k_condense<k(), f() != RHS_P, f() != RHS_W><<<corner_grid(), bs(), 0, stream>>>(g, pdt(), rw, rp, rl, out);
    }); });
  }
  void backsub(const double* rw, const double* rp, const double* lam, double* u, double* phi) {
    if (general) {
      csr(gs().Wu, lam, 1.0, 0.0, u);    // Wu = -W
      csr(gs().Wp, lam, 1.0, 0.0, phi);
      if (rw) { csr(gs().Auu, rw, 1.0, 1.0, u); csr(gs().Apu, rw, 1.0, 1.0, phi); }
      if (rp) { csr(gs().Aup, rp, 1.0, 1.0, u); csr(gs().App, rp, 1.0, 1.0, phi); }
      return;
    }
    halo_L(lam);
    tally(LC_BACKSUB, (rw ? bQ() : 0.0) + (rp ? bP() : 0.0) + bL() + bQ() + bP());
    if (use_mfma_schur() && (rw || rp)) {
      PSet& ps = psets[cur_pset];
      ensure_schur_tables(ps);
      by_mfma_degree([&](auto k) { by_rhs(rw, rp, [&](auto f) {
        k_backsub_mfma<k(), f() != RHS_P, f() != RHS_W><<<schur_cell_grid(), 64 * HDG_BACKSUB_WAVES, 0, stream>>>(g, ps.bsm[0], ps.bsm[1], rw, rp, lam, u, phi);
      }); });
      return;
    }
    by_degree([&](auto k) { by_rhs(rw, rp, [&](auto f) {
      k_backsub<k(), f() != RHS_P, f() != RHS_W><<<cell_grid(), bs(), 0, stream>>>(g, pdt(), rw, rp, lam, u, phi);
    }); });
  }
  void gamma_psi(const double* u, const double* phi, const double* lam, double* out) {
    if (general) {
      double beta = 0.0;
      if (u) { csr(gd.Bdiv, u, 1.0, beta, out); beta = 1.0; }
      if (phi) { csr(gd.Psi_p, phi, 1.0, beta, out); beta = 1.0; }
      if (lam) { csr(gd.Psi_l, lam, 1.0, beta, out); beta = 1.0; }
      if (beta == 0.0) zero(out, NPv);
      return;
    }
    if (lam) halo_L(lam);
    tally(LC_OTHER, (u ? bQ() : 0.0) + (phi ? bP() : 0.0) + (lam ? bL() : 0.0) + bP());
    by_degree([&](auto k) { k_gamma_psi<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, u, phi, lam, out); });
  }
  void gamma_mu(const double* u, const double* phi, const double* lam, double* out) {
    if (general) {
      double beta = 0.0;
      if (u) { csr(gd.Mu_u, u, 1.0, beta, out); beta = 1.0; }
      if (phi) { csr(gd.Mu_p, phi, 1.0, beta, out); beta = 1.0; }
      if (lam) { csr(gd.Mu_l, lam, 1.0, beta, out); beta = 1.0; }
      if (beta == 0.0) zero(out, NLv);
      return;
    }
    if (u) halo_Q(u);
    if (phi) halo_P(phi);
    tally(LC_OTHER, (u ? bQ() : 0.0) + (phi ? bP() : 0.0) + bL() * (lam ? 2 : 1));
    by_degree([&](auto k) { k_gamma_mu<k()><<<corner_grid(), bs(), 0, stream>>>(g, dt, u, phi, lam, out); });
  }
  void trace_recon(const double* Q, const double* p, double* out) {
    if (general) { csr(gd.Rq, Q, 1.0, 0.0, out); csr(gd.Rp, p, 1.0, 1.0, out); return; }
    halo_Q(Q);
    halo_P(p);
    tally(LC_OTHER, bQ() + bP() + bL());
    by_degree([&](auto k) { k_trace_recon<k()><<<corner_grid(), bs(), 0, stream>>>(g, dt, Q, p, out); });
  }
  void precon_rhs(const double* Q, const double* b, double bsc, double* rp, double* rl) {
    if (general) {
      tally(LC_RHS, 2 * bQ() + bP() + bL());
      by_degree([&](auto k) { k_g_precon<k()><<<(ggeo.nc + 63) / 64, 64, 0, stream>>>(ggeo, Q, b, bsc, rp); });
      csr(gd.Rb, b, bsc, 0.0, rl);
      return;
    }
    halo_Q(Q);
    halo_Q(b);
    HIPCHECK(hipMemsetAsync(rl, 0, sizeof(double) * NLv, stream));
    tally(LC_COPY, bL());
    tally(LC_RHS, 2 * bQ() + bP() + bL());
    by_degree([&](auto k) { k_precon_rhs<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, Q, b, bsc, rp, rl); });
  }
  void q_to_modal(const double* nodal, double* modal) { if (general) { csr(gd.Cq, nodal, 1.0, 0.0, modal); return; } by_degree([&](auto k) { k_q_nodal_to_modal<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, nodal, modal); }); }
  void q_to_nodal(const double* modal, double* nodal) { if (general) { csr(gd.Cqi, modal, 1.0, 0.0, nodal); return; } by_degree([&](auto k) { k_q_modal_to_nodal<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, modal, nodal); }); }
  void p_to_modal(const double* nodal, double* modal) { if (general) { csr(gd.Cp, nodal, 1.0, 0.0, modal); return; } by_degree([&](auto k) { k_p_nodal_to_modal<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, nodal, modal); }); }
  void p_to_nodal(const double* modal, double* nodal) { if (general) { csr(gd.Cpi, modal, 1.0, 0.0, nodal); return; } by_degree([&](auto k) { k_p_modal_to_nodal<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, modal, nodal); }); }
  void l_to_modal(double* nodal, double* modal) {
    if (general) { csr(gd.Cl, nodal, 1.0, 0.0, modal); return; }
    HIPCHECK(hipMemsetAsync(modal, 0, sizeof(double) * NLv, stream));
    by_degree([&](auto k) { k_l_convert<k(), true><<<corner_grid_all(), bs(), 0, stream>>>(g_all, dt, nodal, modal); });
  }
  void l_to_nodal(double* modal, double* nodal) { if (general) { csr(gd.Cli, modal, 1.0, 0.0, nodal); return; } by_degree([&](auto k) { k_l_convert<k(), false><<<corner_grid_all(), bs(), 0, stream>>>(g_all, dt, nodal, modal); }); }

  // ------------------------------------------------------------------ vector helpers
  // (whole arrays, ghost rows included: a result is valid on the ghost rows all its inputs are valid on -- fl)
  void copy(double* dst, const double* src, long n) {
    if (dst != src) { HIPCHECK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, stream)); tally(LC_COPY, 2 * bvec(n)); }
    fl.set(dst, fl.get(src));
  }
  void zero(double* x, long n) { HIPCHECK(hipMemsetAsync(x, 0, sizeof(double) * n, stream)); tally(LC_COPY, bvec(n)); fl.set(x, GH); }
  void axpby(long n, double a, const double* x, double b, double* y) {
    tally(LC_VEC, bvec(n) * (b != 0.0 ? 3 : 2));
    if (big(n)) k_axpby<true><<<vec_blocks(n), 256, 0, stream>>>(n, a, x, b, y);
    else k_axpby<false><<<vec_blocks(n), 256, 0, stream>>>(n, a, x, b, y);
    fl.set(y, b == 0.0 ? fl.get(x) : std::min(fl.get(x), fl.get(y)));
  }
  void cheb_update(double* pn, const double* z, const double* x, double c1, double c2) {
    tally(LC_VEC, bQ() * (c1 != 0.0 ? 4 : 3));
    if (big(NQ)) k_cheb_update<true><<<vec_blocks(NQ), 256, 0, stream>>>(NQ, pn, z, x, c1, c2);
    else k_cheb_update<false><<<vec_blocks(NQ), 256, 0, stream>>>(NQ, pn, z, x, c1, c2);
    fl.set(pn, std::min(std::min(fl.get(z), fl.get(x)), c1 != 0.0 ? fl.get(pn) : GH));
  }
  // out = scale * (w - sum_{l < nv} h_l V_l)   (V_l: the GMRES basis gm_V)
  void gs_update(const double* w, const Coefs& h, int nv, double scale, double* out) {
    tally(LC_VEC, bQ() * (nv + 2));
    if (big(NQ)) k_gs_update<MAXV, true><<<vec_blocks(NQ), 256, 0, stream>>>(NQ, w, d_gmV, h, nv, scale, out);
    else k_gs_update<MAXV, false><<<vec_blocks(NQ), 256, 0, stream>>>(NQ, w, d_gmV, h, nv, scale, out);
    int d = fl.get(w);
    for (int l = 0; l < nv; l++) d = std::min(d, fl.get(gm_V[l]));
    fl.set(out, d);
  }
  // the list a linear combination runs over: duplicate pointers merged, zeros dropped, order of first appearance
  static Terms lincomb_terms(const Terms& terms) {
    Terms t;
    for (auto& pr : terms) {
      if (pr.second == 0.0) continue;
      bool found = false;
      for (auto& q : t)
        if (q.first == pr.first) { q.second += pr.second; found = true; }
      if (!found) t.push_back(pr);
    }
    return t;
  }
  // a merged list of 1 .. 8 terms as the kernel argument of a single k_lincomb-style chain
  static bool single_chain(const Terms& t, LinComb& lc) {
    if (t.empty() || t.size() > 8) return false;
    lc.n = 0;
    for (auto& q : t) { lc.v[lc.n] = q.first; lc.c[lc.n] = q.second; lc.n++; }
    for (int k = lc.n; k < 8; k++) { lc.v[k] = nullptr; lc.c[k] = 0.0; }
    return true;
  }
  void lincomb(long n, const Terms& terms, double* out) {
    // merged terms in chunks of 8
    const Terms t = lincomb_terms(terms);
    if (t.empty()) { zero(out, n); return; }
    bool first = true;
    for (size_t off = 0; off < t.size();) {
      LinComb lc;
      lc.n = 0;
      if (!first) { lc.v[0] = out; lc.c[0] = 1.0; lc.n = 1; }
      while (lc.n < 8 && off < t.size()) { lc.v[lc.n] = t[off].first; lc.c[lc.n] = t[off].second; lc.n++; off++; }
      tally(LC_VEC, bvec(n) * (lc.n + 1));
      if (big(n)) k_lincomb<true><<<vec_blocks(n), 256, 0, stream>>>(n, lc, out);
      else k_lincomb<false><<<vec_blocks(n), 256, 0, stream>>>(n, lc, out);
      first = false;
    }
    int d = GH;
    for (auto& q : t) d = std::min(d, fl.get(q.first));
    fl.set(out, d);
  }
  // ownership mask for a vector of length n (cell-type or trace-type row structure)
  // row structure of a vector: cell-type (pressure, per-cell scalars), trace-type, velocity (component-pair layout:
  // a row of a plane holds 2 nx doubles)
  enum { KC = 1, KL = 2, KQ = 3 };
  RowMask mask_for(int kind) const {
    if (general) return RowMask{0, 1, 0, 0};  // a single rank owns every entry
    if (kind == KL) return RowMask{g.P, g.ny + 2 * GH, GH, GH + g.nyc - 1};
    if (kind == KQ) return RowMask{2 * g.nx, g.R, GH, GH + g.ny - 1};
    return RowMask{g.nx, g.R, GH, GH + g.ny - 1};
  }
  // dots of w against nv vectors over the OWNED entries, summed over ranks (host result); one sync
  // cross: res[nv] additionally receives (V[0], V[1]) from the same pass (nv >= 2, single chunk)
  // res == nullptr: the results stay in d_res on the device (single chunk), no host copy, no synchronisation
  bool direct_host() const { return opt.direct_host; }
  void multidot(long n, const double* w, const std::vector<const double*>& V, double* res, int kind, bool cross = false) {
    int nv = (int)V.size();
    if (!res && nv > MAXV) throw std::string("multidot: device-resident result needs a single chunk");
    if (cross && (nv < 2 || nv >= MAXV)) throw std::string("multidot: cross product needs 2 <= nv < MAXV");
    for (int off = 0; off < nv; off += MAXV) {
      int cnt = std::min(MAXV, nv - off);
      const int nout = cnt + (cross ? 1 : 0);
      int nb = std::min(dot_blocks, vec_blocks(n));
      int self = -1;
      for (int q = 0; q < cnt && self < 0; q++) if (V[off + q] == w) self = q;
      const int cr = cross ? 1 : 0;
      const RowMask mk = mask_for(kind);
      tally(LC_DOT, bvec(n) * (cnt + (self >= 0 ? 0 : 1)));
      tally(LC_OTHER, 0.0);  // k_reduce_parts
      auto launch = [&](auto tag) {
        constexpr int MV = decltype(tag)::value;
        VecList<MV> vl;
        for (int q = 0; q < MV; q++) vl.p[q] = q < cnt ? V[off + q] : nullptr;
        if (big(n)) k_multidot<MV, true><<<nb, HDG_DOT_BLOCK, 0, stream>>>(n, w, vl, cnt, d_part, mk, cr, self);
        else k_multidot<MV, false><<<nb, HDG_DOT_BLOCK, 0, stream>>>(n, w, vl, cnt, d_part, mk, cr, self);
      };
      // lean instantiations by output count: <= 4 (norms, CG of round 1, early Gram-Schmidt passes), <= 6 (single-reduction
      // CG: 4 vectors + 1 cross product), <= 12 (the rest of a GMRES(8) cycle); the 32-wide one only beyond that
      with_int<4, 6, 12, MAXV>(nout <= 4 ? 4 : (nout <= 6 ? 6 : (nout <= 12 ? 12 : MAXV)), "multidot width", launch);
      // one rank: the reduction kernel writes the pinned host copy itself (no copy kernel on the stream)
      const bool direct = res && comm->size == 1 && direct_host();
      k_reduce_parts<<<nout, 256, 0, stream>>>(nb, nout, d_part, d_res, direct ? h_res : nullptr);
      comm->allreduce_sum(d_res, nout, stream);
      n_reduce++;
      if (!res) continue;
      if (!direct) HIPCHECK(hipMemcpyAsync(h_res, d_res, sizeof(double) * nout, hipMemcpyDeviceToHost, stream));  // pinned
      HIPCHECK(hipStreamSynchronize(stream));
      for (int q = 0; q < nout; q++) res[off + q] = h_res[q];
    }
  }
  // second stage of a reduction whose per-workgroup partials a kernel left in part[block * nout + q] (the tile kernels of the
  // trace preconditioner), summed over the ranks; the results stay in d_res
  void reduce_parts_allreduce(int nblocks, int nout, const double* part) {
    k_reduce_parts<<<nout, 256, 0, stream>>>(nblocks, nout, part, d_res, nullptr, 1);
    comm->allreduce_sum(d_res, nout, stream);
    n_reduce++;
  }
  double dot(long n, const double* a, const double* b, int kind) {
    double r;
    multidot(n, a, {b}, &r, kind);
    return r;
  }
  // Gram-Schmidt pass of the tentative-velocity GMRES: res[l] = (w, V_l), l < nb, and res[nb] = (w, w) in one pass over w
  // and the basis
  void multidot_basis(const double* w, int nb_, double* res) {
    std::vector<const double*> ptrs(gm_V.begin(), gm_V.begin() + nb_);
    ptrs.push_back(w);
    multidot(NQ, w, ptrs, res, KQ);
  }
  // ------------------------------------------------------------------ pressure mean shift
  void shift(double* p, double* l) {
    if (general) {  // p_mean = int p / vol (common.py:72-73, hdg_imex.py:471-478); the constant 1 in the modal bases
      const double pm = dot(NPv, p, d_int_p, KC) / gm->volume;
      axpby(NPv, -pm, d_one_p, 1.0, p);
      if (l) axpby(NLv, -pm, d_one_l, 1.0, l);
      return;
    }
    const double c0 = g.h / std::sqrt(2.0);  // integral of the mode-0 basis function = its "1" coefficient
    const double vol = Ldom * Ldom;          // domain_volume (common.py:72-73)
    int nb = std::min(dot_blocks, vec_blocks(g.Nc));
    VecList<4> vl{};
    vl.p[0] = ones_c;
    tally(LC_DOT, 2 * bvec(g.Nc));
    tally(LC_OTHER, 0.0);
    tally(LC_VEC, 2 * bvec(g.Nc) + (l ? 2 * bL() : 0.0));
    k_multidot<4, false><<<nb, HDG_DOT_BLOCK, 0, stream>>>(g.Nc, p, vl, 1, d_part, mask_for(KC), 0);
    k_reduce_parts<<<1, 256, 0, stream>>>(nb, 1, d_part, d_res);
    comm->allreduce_sum(d_res, 1, stream);
    k_shift_p<<<vec_blocks(g.Nc), 256, 0, stream>>>(g.Nc, p, d_res, c0 / vol, c0);
    if (l)
      k_shift_l<<<corner_grid(), bs(), 0, stream>>>(g, NL, l, d_res, c0 / vol, std::sqrt(dt.elen[0]),
                                                    std::sqrt(dt.elen[2]), std::sqrt(dt.elen[1]));
  }

  const double* bvec(int slot) const { return bsep[slot] ? profile : brhs[slot]; }
  Terms residual_terms(const std::vector<double>& cq, const std::vector<double>& cb) const {
    Terms terms;
    for (int j = 0; j < s; j++) terms.push_back({stQ[j], cq[j]});
    for (int j = 0; j < s; j++) terms.push_back({bvec(j), cb[j] * bscale[j]});
    if (buoyancy_on())  // b_rhs[j] + B(q^(j)): the buoyancy vectors stand beside the user's forcing
      for (int j = 0; j < s; j++) terms.push_back({buoy[(size_t)j], cb[j]});
    if (vel_linear_on())  // ... + nu M^-1 V Q^(j) + M^-1 C Q^(j): vectors of their own again (DESIGN.md sections 21, 22); filled by viscosity_slots
      for (int j = 0; j < s; j++) terms.push_back({visc[(size_t)j], cb[j]});
    return terms;
  }
  // the two implicit steppers: (Q, w) + dt (f(t_k) + B(q_n), w), slot 0
  Terms start_terms(double dtt) const {
    Terms terms{{curQ, 1.0}, {bvec(0), dtt * bscale[0]}};
    if (buoyancy_on()) terms.push_back({buoy[0], dtt});
    if (vel_linear_on()) terms.push_back({visc[0], dtt});
    return terms;
  }
  void residual_vector(const std::vector<double>& cq, const std::vector<double>& cb, double* out) {
    lincomb(NQ, residual_terms(cq, cb), out);
  }

  // ------------------------------------------------------------------ tentative velocity solve
  void ensure_dinv(int idx, double gamma) {
    if (general) {
      if (dinv_gamma[idx] == gamma && (gdinv[(size_t)idx].nrows || g_hyb[(size_t)idx])) return;
      // the tables of another gamma (hdg_set_dt) are freed, not kept
      if (!opt.general_csr_lift && cfg.tent_precond == 2) {
        release_dev(g_hyb[(size_t)idx]);
        g_hyb[(size_t)idx] = upload(assemble_lift_tables(*gtab, *gm, gloc, gamma));
      } else {
        DevCsr& D = gdinv[(size_t)idx];
        release_dev(D.rowptr); release_dev(D.col); release_dev(D.val);
        D = upload_csr(assemble_block_jacobi(*gtab, *gm, gloc, gamma));
      }
      dinv_gamma[idx] = gamma;
      return;
    }
    if (dinv_gamma[idx] == gamma && dinv0[idx]) return;
    dvec a = tab->blockJacobiInverse(0, gamma), b = tab->blockJacobiInverse(1, gamma);
    if (!dinv0[idx]) { dinv0[idx] = dalloc((long)a.size()); dinv1[idx] = dalloc((long)b.size()); }
    HIPCHECK(hipMemcpyAsync(dinv0[idx], a.data(), sizeof(double) * a.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(dinv1[idx], b.data(), sizeof(double) * b.size(), hipMemcpyHostToDevice, stream));
    // hybrid preconditioner tables G_e = (I - Dinv_s) Lift_e, 3 blocks of 2nu x ne per shape (k_edge_lift<.,.,2>)
    const int n2 = 2 * tab->nu, ne = tab->ne;
    dvec G[2];
    for (int sh = 0; sh < 2; sh++) {
      const dvec& Di = sh == 0 ? a : b;
      G[sh].assign((size_t)3 * n2 * ne, 0.0);
      for (int e = 0; e < 3; e++)
        for (int r = 0; r < n2; r++)
          for (int q = 0; q < ne; q++) {
            double acc = tab->Lift[sh][e][r * ne + q];
            for (int m = 0; m < n2; m++) acc -= Di[(size_t)r * n2 + m] * tab->Lift[sh][e][m * ne + q];
            G[sh][((size_t)e * n2 + r) * ne + q] = acc;
          }
    }
    if (use_mfma_lift()) {
      // the same tables in A-operand lane order for k_edge_lift_mfma (G[sh]: 3 blocks of 2nu x ne)
      if (liftm_hyb0.size() < hybg0.size()) { liftm_hyb0.resize(hybg0.size(), nullptr); liftm_hyb1.resize(hybg0.size(), nullptr); }
      for (int sh = 0; sh < 2; sh++) {
        dvec Ge[3];
        for (int e = 0; e < 3; e++) Ge[e].assign(G[sh].begin() + (size_t)e * n2 * ne, G[sh].begin() + (size_t)(e + 1) * n2 * ne);
        std::vector<double> pk = pack_lift_mfma(*tab, sh, Ge);
        double*& dstp = sh == 0 ? liftm_hyb0[idx] : liftm_hyb1[idx];
        if (!dstp) dstp = dalloc((long)pk.size());
        HIPCHECK(hipMemcpyAsync(dstp, pk.data(), sizeof(double) * pk.size(), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream));  // pk goes out of scope
      }
    }
    if (!hybg0[idx]) { hybg0[idx] = dalloc((long)G[0].size()); hybg1[idx] = dalloc((long)G[1].size()); }
    HIPCHECK(hipMemcpyAsync(hybg0[idx], G[0].data(), sizeof(double) * G[0].size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(hybg1[idx], G[1].data(), sizeof(double) * G[1].size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    dinv_gamma[idx] = gamma;
  }
  // one tentative-velocity system (I - gamma F(Q*)) x = b of stage didx (whose preconditioner tables ensure_dinv has built)
  struct TentSystem { const double* qstar; double gamma; int didx; const double* b; };
  // z = M r  (tentative-velocity preconditioner)
  void tent_precond(const TentSystem& S, const double* r, double* z) {
    const int didx = S.didx;
    if (general) {
      if (cfg.tent_precond == 2 && g_hyb[(size_t)didx]) {
        g_lift_apply(g_hyb[(size_t)didx], r, z);  // z = r + (I - Dinv) Lift d(r): one matrix-free kernel
      } else if (cfg.tent_precond == 2) {
        // hybrid two-level preconditioner Pi + Dinv (I - Pi): the H(div)-conforming part is left alone (mass matrix =
        // identity), the element block-Jacobi acts on the rest, which carries the normal-jump penalty
        csr(gd.Pi, r, 1.0, 0.0, wQ3);
        copy(wQ4, r, NQ);
        axpby(NQ, -1.0, wQ3, 1.0, wQ4);
        csr(gdinv[(size_t)didx], wQ4, 1.0, 0.0, z);
        axpby(NQ, 1.0, wQ3, 1.0, z);
      } else {
        csr(gdinv[(size_t)didx], r, 1.0, 0.0, z);
      }
      return;
    }
    if (cfg.tent_precond == 0) {
      blockdiag(dinv0[didx], dinv1[didx], r, nullptr, 0.0, z);
    } else if (cfg.tent_precond == 1) {
      bdm_T(r, wQ3);
      bdm_plus_bj(wQ3, z, r, dinv0[didx], dinv1[didx]);
    } else {
      bdm_hybrid(r, z, hybg0[didx], hybg1[didx]);
    }
  }
  // z = M r fused with the Chebyshev step x_{n+1} = x_n + c1 (x_n - x_{n-1}) + c2 z: d_ holds x_{n-1} on entry and
  // x_{n+1} on exit, x_ = x_n is only read (owned rows only: the ghost rows are refreshed by the next operator
  // application); z is written to `zout` only when it is needed
  // cell_norm (hybrid preconditioner only): instead of z the kernel writes |z_K|^2 per cell into cell_ss
  void tent_precond_cheb(const TentSystem& S, const double* r, double* zout, double* d_, double* x_, double c1, double c2,
                         bool cell_norm = false) {
    const int didx = S.didx;
    if (general) {  // assembled preconditioner, then the step as a vector kernel
      double* zz = zout ? zout : wQ1;  // (tent_precond uses wQ3 / wQ4 as its own scratch; wQ1 is the solver's z buffer)
      tent_precond(S, r, zz);
      cheb_update(d_, zz, x_, c1, c2);
      return;
    }
    if (cfg.tent_precond == 0) {
      blockdiag(dinv0[didx], dinv1[didx], r, nullptr, 0.0, wQ4);
      if (zout) copy(zout, wQ4, NQ);
      cheb_update(d_, wQ4, x_, c1, c2);
    } else if (cfg.tent_precond == 1) {
      bdm_T(r, wQ3);
      bdm_plus_bj(wQ3, zout, r, dinv0[didx], dinv1[didx], d_, x_, c1, c2);
    } else if (use_mfma_lift()) {
      // k >= 3: matrix-core lift with the Chebyshev step in its store epilogue (z is stored at check points only)
      bdm_hybrid(r, zout, hybg0[didx], hybg1[didx], d_, x_, c1, c2, nullptr);
    } else {
      bdm_hybrid(r, zout, hybg0[didx], hybg1[didx], d_, x_, c1, c2, cell_norm ? cell_ss : nullptr);
    }
  }
  // Krylov solvers of a tentative-velocity system S, left-preconditioned; x holds the initial guess.
  // Convergence: ||M r|| <= rtol * ||M r0||  (PETSc default for the SNES-ksponly linear solve the
  // reference performs: relative to the residual at the warm start); beta0 = ||M r0|| where the caller
  // has measured it, < 0: the norm of the first residual of the call.
  //
  // tent_krylov: where a solve, or the rest of one, that the Chebyshev iteration does not take goes.
  // Round 4: a WHOLE strict solve (the fully implicit stepper at k >= 2, wide-ellipse stages that the Chebyshev iteration
  // declines, general meshes at k = 1) runs as s-step minimal-residual cycles -- the same Krylov spaces as GMRES(6) without the
  // Gram-Schmidt passes, which cost more than the operator (sstep_mr; two weak cycles come back in Arnoldi form).  The
  // Arnoldi form stays for the Ritz estimate, the inexact inner solves of the monolithic preconditioner, the fall-backs after a
  // growing / stalled Chebyshev iteration (they call arnoldi_solve themselves); HDG_GMRES_ARNOLDI restores it everywhere.
  int tent_krylov(const TentSystem& S, double* x, double rtol, int maxit, bool strict, double beta0 = -1.0) {
    if (strict && !opt.gmres_arnoldi && gm_V.size() >= 4) return sstep_mr(S, x, rtol, beta0, -1.0);
    return arnoldi_solve(S, x, rtol, maxit, strict, beta0, 4);
  }
  // w = M(b - A x) in wQ1 (t = b - A x in wQ2): the norm of w
  double tent_residual(const TentSystem& S, const double* x) {
    adv_apply(x, S.qstar, wQ2, S.gamma, S.b);    // t = b - A x  (residual fused into the operator kernel)
    tent_precond(S, wQ2, wQ1);
    return std::sqrt(dot(NQ, wQ1, wQ1, KQ));
  }
  // GMRES(m): restarted Arnoldi cycles, the first of first_cycle iterations.  strict: throws at maxit.
  int arnoldi_solve(const TentSystem& S, double* x, double rtol, int maxit, bool strict, double beta0, int first_cycle) {
    FlowScope flow_(*this);
    flow_fixed_Q(S.qstar);
    flow_fixed_Q(S.b);
    const int m = std::min(std::max(1, cfg.gmres_restart), MAXV - 1);  // allocated basis / Hessenberg stride
    // adaptive cycle length: short cycles keep the Krylov-basis traffic low (the preconditioned operator
    // is benign: GMRES(4) needs 45.5 iterations where GMRES(30) needs 42.5 at C3); a cycle that reduces
    // the residual by less than 2x doubles the length, up to the configured restart
    int mcur = std::min(m, std::max(1, first_cycle));
    double beta_prev = -1.0;
    int its = 0;
    GivensLsq lsq(m);
    while (true) {
      const double beta = tent_residual(S, x);
      if (beta0 < 0) beta0 = beta;
      if (!(beta == beta)) throw NotConverged{"GMRES: NaN residual"};
      if (beta <= rtol * beta0 || beta == 0.0) return its;
      if (beta_prev > 0 && beta > 0.5 * beta_prev) mcur = std::min(m, 2 * mcur);
      beta_prev = beta;
      if (arnoldi_cycle(S, x, lsq, mcur, beta, beta0, rtol, maxit, its).done) return its;
      if (its >= maxit) {
        if (strict) throw NotConverged{"tentative-velocity GMRES reached max iterations"};
        return its;
      }
    }
  }
  // ONE Arnoldi cycle of at most m_cycle iterations from x: the eigenvalues of its Hessenberg matrix (Ritz values of the
  // preconditioned operator) and the initial / final preconditioned residual norms (beta_last is the Arnoldi estimate).
  // No Ritz values where x had converged already.
  struct RitzEstimate { int its = 0; double beta_first = 0.0, beta_last = 0.0; std::vector<std::complex<double>> ritz; };
  RitzEstimate ritz_cycle(const TentSystem& S, double* x, int m_cycle) {
    FlowScope flow_(*this);
    flow_fixed_Q(S.qstar);
    flow_fixed_Q(S.b);
    const int m = std::min(std::max(1, cfg.gmres_restart), MAXV - 1);
    RitzEstimate e;
    const double beta = e.beta_first = e.beta_last = tent_residual(S, x);
    if (!(beta == beta)) throw NotConverged{"GMRES: NaN residual"};
    if (beta <= cfg.tent_rtol * beta || beta == 0.0) return e;
    GivensLsq lsq(m, true);
    const ArnoldiCycle c = arnoldi_cycle(S, x, lsq, std::min(m, std::max(1, m_cycle)), beta, beta, cfg.tent_rtol, cfg.tent_maxit, e.its);
    e.beta_last = c.res;
    // Ritz values: eigenvalues of the leading j x j block of the (unrotated) Hessenberg matrix
    e.ritz = hessenberg_eig(lsq.unrotated(c.j), c.j);
    return e;
  }
  // One Arnoldi cycle of at most mcur iterations from the preconditioned residual tent_residual left in wQ1 (norm beta), and
  // the update of x at its end.  j: columns built; done: the estimate met the tolerance, or the Krylov space is exhausted;
  // res: the Arnoldi estimate of the new |M r|
  struct ArnoldiCycle { int j; bool done; double res; };
  ArnoldiCycle arnoldi_cycle(const TentSystem& S, double* x, GivensLsq& lsq, int mcur, double beta, double beta0, double rtol,
                             int maxit, int& its) {
    double* w = wQ1;
    double* t = wQ2;
    const int nvb = vec_blocks(NQ);
    gs_update(w, Coefs(), 0, 1.0 / beta, gm_V[0]);
    lsq.start(beta);
    int j = 0;
    bool done = false;
    double res = beta;
    for (; j < mcur; j++) {
      adv_apply(gm_V[j], S.qstar, t, S.gamma);
      tent_precond(S, t, w);
      // one pass: h_l = (w, V_l), l <= j, and (w, w); then ||w - V h||^2 = (w,w) - sum h_l^2
      std::vector<double> h(j + 2);
      multidot_basis(w, j + 1, h.data());
      double ww = h[j + 1], s2 = 0.0;
      for (int l = 0; l <= j; l++) s2 += h[l] * h[l];
      double hn2 = ww - s2;
      Coefs hc;
      for (int l = 0; l <= j; l++) hc.c[l] = h[l];
      double hn;
      if (hn2 > 1e-6 * ww) {
        hn = std::sqrt(hn2);
        gs_update(w, hc, j + 1, 1.0 / hn, gm_V[j + 1]);
      } else {
        // severe cancellation: orthogonalise explicitly and measure the norm (safe path)
        gs_update(w, hc, j + 1, 1.0, gm_V[j + 1]);
        hn = std::sqrt(dot(NQ, gm_V[j + 1], gm_V[j + 1], KQ));
        if (hn > 0) gs_update(w, hc, j + 1, 1.0 / hn, gm_V[j + 1]);  // once more with the norm (writes every copy of the vector)
      }
      res = lsq.add_column(j, h.data(), hn);
      its++;
      if (debug_on()) fprintf(stderr, "[gmres]   it %d (cycle start %.3e)  estimate %.3e  hn %.3e\n", its, beta / beta0, res / beta0, hn);
      if (res <= rtol * beta0 || hn == 0.0) { j++; done = true; break; }
      if (its >= maxit) { j++; done = false; break; }
    }
    const std::vector<double> y = lsq.solve(j);
    Coefs yc;
    for (int l = 0; l < j; l++) yc.c[l] = y[l];
    tally(LC_VEC, bQ() * (j + 2));
    if (big(NQ)) k_basis_axpy<MAXV, true><<<nvb, 256, 0, stream>>>(NQ, x, d_gmV, yc, j);
    else k_basis_axpy<MAXV, false><<<nvb, 256, 0, stream>>>(NQ, x, d_gmV, yc, j);
    {
      int d = fl.get(x);
      for (int l = 0; l < j; l++) d = std::min(d, fl.get(gm_V[l]));
      fl.set(x, d);
    }
    return ArnoldiCycle{j, done, res};
  }

  // s-step minimal-residual cycles on the left-preconditioned operator B = M (I - gamma F(Q*)) (hdg_kernels.hpp: k_gram,
  // k_sstep_update): the tail of the Chebyshev iteration (round 3: one GMRES(8) cycle, whose Gram-Schmidt passes cost more
  // than its operator applications).  Power basis K_0 = M(b - A x), K_i = B K_{i-1}, i <= s (s <= 6: 28 inner products fit one
  // reduction); the least-squares coefficients come from the Gram matrix by a Cholesky factorisation of its scaled trailing
  // block in long double, truncated at the first pivot below 1e-13 (a residual that a few eigenvectors dominate -- the very
  // situation at the hand-over -- spans a nearly invariant subspace: the basis then IS rank deficient and the truncated
  // problem is the right one).  Whatever y is, x += sum y_i K_{i-1} and r' = K_0 - sum y_i K_i stay consistent (r' is the
  // preconditioned residual of the new x up to rounding), so the accuracy of y decides the progress of a cycle only, never
  // the answer; the norm of r' is measured, not predicted.  Same stopping rule as GMRES and the Chebyshev iteration:
  // |M r| <= rtol |M r_0| (beta0).  cur0 > 0: the norm of the current preconditioned residual as the caller last measured it
  // (the cycle length is chosen from the reduction still needed: 1.7 iterations per decade + 1, GMRES's observed 5-6 for 3-4
  // decades).  Two cycles in a row that gain less than a factor 2 hand the solve to GMRES (which throws at its iteration limit).
  long n_sstep_cycles = 0, n_sstep_fallbacks = 0;
  double *d_gram = nullptr, *h_gram = nullptr;
  int sstep_mr(const TentSystem& S, double* x, double rtol, double beta0, double cur0) {
    FlowScope flow_(*this);
    flow_fixed_Q(S.qstar);
    flow_fixed_Q(S.b);
    const int smax = std::max(2, std::min(std::min(opt.sstep_max, HDG_SSTEP_MAXV - 1), (int)gm_V.size() - 1));
    if (!d_gram) {
      d_gram = dalloc(64);
      HIPCHECK(hipHostMalloc((void**)&h_gram, sizeof(double) * 64));
    }
    double* t = wQ2;
    const RowMask mk = mask_for(KQ);
    double target = rtol * beta0;  // beta0 <= 0: the norm of the first residual of this call (a whole solve by s-step cycles)
    const bool direct = comm->size == 1 && direct_host();
    int its = 0, weak = 0;
    double cur = cur0;
    bool have_r = false;
    while (true) {
      if (!have_r) {
        adv_apply(x, S.qstar, t, S.gamma, S.b);  // t = b - A x
        tent_precond(S, t, gm_V[0]);
      }
      int built = 0;
      int want = sstep_first_length(cur, target, opt.sstep_per_decade, smax);
      std::vector<long double> G, yv;
      int nv = 0, rank = 0;
      double k0n = 0.0, rho = 0.0;
      while (true) {
        for (int i = built + 1; i <= want; i++) {
          adv_apply(gm_V[i - 1], S.qstar, t, S.gamma);
          tent_precond(S, t, gm_V[i]);
          its++;
        }
        built = want;
        nv = built + 1;  // K_0 .. K_built
        const int npair = nv * (nv + 1) / 2;
        const int nb = std::min(std::min(dot_blocks, vec_blocks(NQ)), (dot_blocks * MAXV) / npair);
        tally(LC_DOT, bQ() * nv);
        tally(LC_OTHER, 0.0);
        // two instantiations: up to 7 vectors (28 accumulators, 3 waves / SIMD) and up to 9 (244 VGPRs)
        auto gram = [&](auto tag) {
          constexpr int NV = decltype(tag)::value;
          VecList<NV> vl;
          for (int q = 0; q < NV; q++) vl.p[q] = q <= built ? gm_V[q] : nullptr;
          if (big(NQ)) k_gram<NV, true><<<nb, HDG_DOT_BLOCK, 0, stream>>>(NQ, vl, nv, d_part, mk);
          else k_gram<NV, false><<<nb, HDG_DOT_BLOCK, 0, stream>>>(NQ, vl, nv, d_part, mk);
        };
        with_int<7, HDG_SSTEP_MAXV>(nv <= 7 ? 7 : HDG_SSTEP_MAXV, "Gram matrix width", gram);
        k_reduce_parts<<<npair, 256, 0, stream>>>(nb, npair, d_part, d_gram, direct ? h_gram : nullptr);
        comm->allreduce_sum(d_gram, npair, stream);
        n_reduce++;
        if (!direct) HIPCHECK(hipMemcpyAsync(h_gram, d_gram, sizeof(double) * npair, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        G.assign((size_t)nv * nv, 0.0L);
        {
          int p = 0;
          for (int a = 0; a < nv; a++) for (int c = a; c < nv; c++, p++) G[(size_t)a * nv + c] = G[(size_t)c * nv + a] = h_gram[p];
        }
        const double g00 = (double)G[0];
        if (!(g00 == g00)) throw NotConverged{"s-step cycle: NaN residual"};
        k0n = std::sqrt(std::max(g00, 0.0));
        if (beta0 <= 0.0) { beta0 = k0n; target = rtol * beta0; if (beta0 == 0.0) return its; }
        if (k0n <= target || k0n == 0.0) return its;  // the iterate the cycle started from had converged already
        rank = sstep_ls(G, nv, nv - 1, yv, rho);
        if (debug_on()) fprintf(stderr, "[sstep]   basis of %d (rank %d): |Mr|/|Mr0| %.3e, predicted %.3e\n", built, rank, k0n / beta0, rho / beta0);
        want = sstep_extend(rho, target, built, rank, smax, opt.sstep_per_decade);
        if (want == built) break;  // take the step
      }
      n_sstep_cycles++;
      const int nvu = built + 1;  // update list: K_0 .. K_built
      Coefs cx, cr;
      for (int i = 0; i < 32; i++) cx.c[i] = cr.c[i] = 0.0;
      cr.c[0] = 1.0;
      for (int i = 0; i < std::min(rank, built); i++) { cx.c[i] = (double)yv[i]; cr.c[i + 1] = -(double)yv[i]; }
      tally(LC_VEC, bQ() * (nvu + 3));
      tally(LC_OTHER, 0.0);
      {
        const int nb = std::min(dot_blocks, vec_blocks(NQ));
        VecList<HDG_SSTEP_MAXU> vl;
        for (int q = 0; q < HDG_SSTEP_MAXU; q++) vl.p[q] = q <= built ? gm_V[q] : nullptr;
        if (big(NQ)) k_sstep_update<HDG_SSTEP_MAXU, true><<<nb, HDG_DOT_BLOCK, 0, stream>>>(NQ, x, gm_V[0], vl, nvu, cx, cr, d_part, mk);
        else k_sstep_update<HDG_SSTEP_MAXU, false><<<nb, HDG_DOT_BLOCK, 0, stream>>>(NQ, x, gm_V[0], vl, nvu, cx, cr, d_part, mk);
        int dmin = fl.get(x);
        for (int l = 0; l <= built; l++) dmin = std::min(dmin, fl.get(gm_V[l]));
        fl.set(x, dmin);
        fl.set(gm_V[0], dmin);
        k_reduce_parts<<<1, 256, 0, stream>>>(nb, 1, d_part, d_gram, direct ? h_gram : nullptr);
      }
      comm->allreduce_sum(d_gram, 1, stream);
      n_reduce++;
      if (!direct) HIPCHECK(hipMemcpyAsync(h_gram, d_gram, sizeof(double), hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
      const double rn = std::sqrt(std::max(h_gram[0], 0.0));
      if (!(rn == rn)) throw NotConverged{"s-step cycle: NaN residual"};
      if (debug_on())
        fprintf(stderr, "[sstep] cycle of %d (rank %d): |Mr|/|Mr0| %.3e -> %.3e (predicted %.3e)\n", built, rank, k0n / beta0, rn / beta0, rho / beta0);
      if (rn <= target) return its;
      if (its >= cfg.tent_maxit) throw NotConverged{"tentative-velocity s-step iteration reached max iterations"};
      weak = (rn > 0.5 * k0n) ? weak + 1 : 0;
      if (weak >= 2 || rank == 0) {
        n_sstep_fallbacks++;
        if (debug_on()) fprintf(stderr, "[sstep] two weak cycles: GMRES takes over\n");
        return its + arnoldi_solve(S, x, rtol, cfg.tent_maxit, true, beta0, 4);
      }
      cur = rn;
      have_r = true;
    }
  }

  // Tentative-velocity solver (default): one short GMRES cycle, then Chebyshev iteration.
  // GMRES(4) needs as many iterations as GMRES(30) on this operator, i.e. the preconditioned iteration is
  // essentially stationary; a Chebyshev iteration reaches the same rate with NO inner products and no
  // Krylov basis (per iteration: operator + preconditioner + one fused update, one norm every 4th
  // iteration).  Spectral bounds come from the Ritz values of the opening GMRES cycle of THIS solve
  // (merged with the bounds seen so far for the stage), with safety factors; if the iteration stalls or
  // grows, the solve is finished by GMRES.  Same stopping rule as GMRES: ||M r|| <= rtol ||M r_0||.
  // The decisions -- interval, ellipse, method selection, check schedule, guards -- are hdg_tent_policy.hpp's; ch is what
  // each stage remembers between solves.
  std::vector<ChebStage> ch;
  double* chd = nullptr;
  // x: the engine's pointer to the iterate (Qtent[.]).  The solve may end with the iterate in the second buffer; the two
  // pointers are then exchanged instead of the vector copied, so x is a reference and every reader goes through the member.
  int cheb_gmres(const TentSystem& S, double*& x) {
    FlowScope flow_(*this);
    flow_fixed_Q(S.qstar);
    flow_fixed_Q(S.b);
    const double rtol = cfg.tent_rtol;
    const int didx = S.didx;
    const bool hyb = cfg.tent_precond == 2;
    ChebStage& st = ch[(size_t)didx];
    if (!chd) chd = dalloc(NQ);
    double beta0 = 0.0, beta = 0.0;
    int its = 0;
    // re-estimate period opt.cheb_every: a wrong interval is caught by the growth guard, which re-estimates at once
    const bool estimate = st.lmin <= 0 || (st.count % opt.cheb_every) == 0;
    st.count++;
    if (estimate) {
      st.hand = 0;  // the hand-over point is learnt anew with the bounds
      const RitzEstimate e = ritz_cycle(S, x, opt.cheb_m);
      its = e.its; beta0 = e.beta_first; beta = e.beta_last;
      if (beta <= rtol * beta0 || beta0 == 0.0) return its;
      if (!ritz_interval(e.ritz, st, opt, hyb, cfg.degree)) return its + tent_krylov(S, x, rtol, cfg.tent_maxit, true, beta0);
      if (debug_on()) {
        fprintf(stderr, "[cheb] stage %d ritz:", didx);
        for (auto v : e.ritz) fprintf(stderr, " %.3f%+.3fi", v.real(), v.imag());
        fprintf(stderr, "  -> interval [%.3f, %.3f], after GMRES cycle residual %.2e of %.2e\n", st.lmin, st.lmax, beta, beta0);
      }
    } else {
      // bounds of this stage are known (refreshed every opt.cheb_every-th solve): start the Chebyshev iteration at once
      beta0 = beta = tent_residual(S, x);
      if (!(beta0 == beta0)) throw NotConverged{"Chebyshev: NaN residual"};
      if (beta0 == 0.0) return 0;
    }
    const double lo = st.lmin, hi = st.lmax;
    const ChebEllipse el(lo, hi, cheb_ellipse_frac(opt, hyb, cfg.degree));
    const double theta = el.theta, delta = el.delta, sigma = el.sigma;
    double rho = 1.0 / sigma;

    double* t = wQ2;
    double* z = wQ1;
    const int expected = el.expected(rtol * beta0 / beta);
    // Method selection: a wide / fat ellipse (large implicit weight or CFL: ARS3(4,4,3), the implicit tableau,
    // dt > 0.25/nx) predicts a slow Chebyshev iteration; GMRES then needs 40-80 iterations where Chebyshev
    // needs 100-160 and is as fast or faster in wall time (tools/robustness_sweep.py) and has no parameters.
    if (expected > opt.cheb_max_expected || (!estimate && st.slow)) {
      if (debug_on()) fprintf(stderr, "[cheb] stage %d: %d iterations predicted on [%.3f, %.3f] -> GMRES\n", didx, expected, lo, hi);
      return its + tent_krylov(S, x, rtol, cfg.tent_maxit, true, beta0);
    }
    // Two iterate buffers, no direction vector: the step writes x_{n+1} over x_{n-1} (k_edge_lift epilogue /
    // k_cheb_update), then the roles swap.  `cur` holds the newest iterate; x receives it when the solve ends.
    double* cur = x;
    double* oth = chd;
    auto finish_in_x = [&]() {
      if (cur == x) return;
      if (opt.glue_fusion) std::swap(x, chd);  // the bookkeeping (fl) goes by address and follows
      else copy(x, cur, NQ);
    };
    if (estimate) {
      adv_apply(cur, S.qstar, t, S.gamma, S.b);
      tent_precond_cheb(S, t, nullptr, oth, cur, 0.0, 1.0 / theta);
    } else {
      // z = M(b - A x) of the unchanged iterate is already in wQ1 (= z) from the norm evaluation above
      cheb_update(oth, z, cur, 0.0, 1.0 / theta);
    }
    std::swap(cur, oth);
    // (its: the iterations of the opening GMRES cycle, 0 without an estimate)
    ChebMonitor mon(st, its, expected, opt, cheb_handover_rate(opt, hyb, cfg.degree), rtol * beta0, beta, cfg.tent_maxit);
    int k = 1;
    its++;
    while (true) {
      const bool check = mon.check_at(k);
      const double rn = 1.0 / (2.0 * sigma - rho);
      adv_apply(cur, S.qstar, t, S.gamma, S.b);
      // hybrid preconditioner: the lift kernel emits |z_K|^2 per cell (N_c doubles) instead of z (N_Q doubles)
      const bool cell_norm = check && hyb && !use_mfma_lift() && !general;
      tent_precond_cheb(S, t, (check && !cell_norm) ? z : nullptr, oth, cur, rn * rho, 2.0 * rn / delta, cell_norm);
      std::swap(cur, oth);
      rho = rn;
      k++;
      its++;
      if (!check) continue;
      double nz = cell_norm ? std::sqrt(dot(g.Nc, cell_ss, ones_c, KC)) : std::sqrt(dot(NQ, z, z, KQ));
      if (!(nz == nz)) throw NotConverged{"Chebyshev: NaN residual"};
      if (debug_on()) fprintf(stderr, "[cheb]   k=%d  |Mr|/|Mr0| = %.3e\n", k, nz / beta0);
      const ChebVerdict v = mon.observe(k, its, nz);
      if (v == ChebVerdict::Continue) continue;
      if (v != ChebVerdict::Converged && debug_on())
        fprintf(stderr, "[cheb]   falling back to GMRES at k=%d (%s; |Mr| %.2e, best %.2e)\n", k, verdict_name(v), nz, mon.last);
      finish_in_x();
      if (v == ChebVerdict::Converged) return its;
      // the tail after a hand-over is 3-4 decades = 5-7 GMRES iterations: one cycle of 8, no restart in between
      // round 4: the tail as s-step minimal-residual cycles (no Gram-Schmidt passes); HDG_TAIL_GMRES restores the GMRES cycle
      if (mon.tail && !opt.tail_gmres) return its + sstep_mr(S, x, rtol, beta0, nz);
      // robustness path after a growing / stalled iteration: the Arnoldi form
      return its + arnoldi_solve(S, x, rtol, cfg.tent_maxit, true, beta0, mon.tail ? opt.cheb_hand_cycle : 4);
    }
  }

  int tentative_solve(int i) {
    if (i < 1 || i >= s) throw std::string("stage out of range");
    Timed tm_(*this, T_TENT);
    const double gamma = cfg.a_impl[i * s + i] * cfg.dt;
    ensure_dinv(i, gamma);
    std::vector<double> cq, cb;
    residual_coeffs(cfg, i, cq, cb);
    // rhs = r_i - (I - gamma F) Q_i + gamma g(w, p_i, lambda_i)      (hdg_imex.py:239-247)
    double* rhs = updU;  // _update.u is overwritten by the following pressure solve anyway
    viscosity_slots(cb);
    const Terms ri = residual_terms(cq, cb);               // r_i
    adv_apply(stQ[i], Qstar[i - 1], wQ4, gamma);           // (I - gamma F) Q_i
    // r_i is formed inside the pressure-gradient kernel where that has a form for it; otherwise as a vector of its own (the
    // two launches commute: they write wQ3 and wQ4)
    if (!pgrad_terms(ri, wQ4, stP[i], stL[i], gamma, rhs)) {
      lincomb(NQ, ri, wQ3);
      pgrad(wQ3, 1.0, wQ4, -1.0, stP[i], stL[i], gamma, rhs);
    }
    const TentSystem S{Qstar[i - 1], gamma, i, rhs};
    int its = cfg.tent_solver == 0 ? tent_krylov(S, Qtent[i], cfg.tent_rtol, cfg.tent_maxit, true) : cheb_gmres(S, Qtent[i]);
    it_sum[0] += its; it_cnt[0]++;
    return its;
  }

  // ------------------------------------------------------------------ trace solver
  void project_const(double* x) {
    // x <- x - n (n.x)/(n.n), n = trace coefficients of the constant 1 (null space, hdg_imex.py:480-489)
    if (tr_one_nn < 0) tr_one_nn = dot(NLv, tr_one, tr_one, KL);  // = total skeleton length, constant
    const double nx_ = dot(NLv, tr_one, x, KL);
    axpby(NLv, -nx_ / tr_one_nn, tr_one, 1.0, x);
  }
  // xc != nullptr (second application of a preconditioner cycle): the iterate is x + P xc, the prolongation of the
  // vertex-grid correction xc, which the first step forms on the fly and stores in x (no separate k_p1_to_trace pass)
  void cheb_smooth(const double* b, double* x, bool zero_init, int its, const double* xc = nullptr) {
    const double theta = 0.5 * (cheb_lmax + cheb_lmin), delta = 0.5 * (cheb_lmax - cheb_lmin);
    const double sigma1 = theta / delta;
    double rho = 1.0 / sigma1;
    // round 3: the first step of the zero-start smoother and the prolongation folded into the stencil launches that consume
    // them (HDG_TRACE_NO_FOLD: the separate launches of round 2)
    const bool fuse = opt.trace_fuse, fold = opt.trace_fold;
    if (general) {
      if (xc) { csr(gs().amg.P0, xc, 1.0, 1.0, x); xc = nullptr; }
    } else if (xc && !(its == 2 && fuse && fold && !periodic)) { p1_to_trace(xc, x, 1.0); xc = nullptr; }
    if (its == 2 && fuse && !general) {
      // two Chebyshev steps in two launches: operator, edge block-Jacobi and update fused (k_trace_smooth)
      const double rn = 1.0 / (2.0 * sigma1 - rho), c2_0 = 1.0 / theta, c1_1 = rn * rho, c2_1 = 2.0 * rn / delta;
      if (zero_init && fold) {
        // ONE launch: d0 = Dinv b / theta at every edge of the stencil on the fly, x = d0 + d1
        trace_smooth(b, b, 1.0, -1.0, c1_1, c2_1, nullptr, nullptr, x, false, 1.0, 1, c2_0);
      } else if (zero_init) {
        trace_cheb(b, ch_d, nullptr, 0.0, c2_0);                                       // d0 = Dinv b / theta
        trace_smooth(ch_d, b, 1.0, -1.0, c1_1, c2_1, nullptr, nullptr, x, false, 1.0);  // x = d0 + d1
      } else {
        if (xc) {
          // x0 = x + P xc formed on the fly and stored in wL2 (not in x: the neighbouring threads still read x);
          // r0 = b - T x0, d0;  then x = x0 + d0 + d1
          trace_smooth(x, b, 1.0, -1.0, 0.0, c2_0, ch_r, ch_d, wL2, true, 0.0, 2, 0.0, xc);
          trace_smooth(ch_d, ch_r, 1.0, -1.0, c1_1, c2_1, nullptr, nullptr, x, true, 1.0, 0, 0.0, nullptr, wL2);
        } else {
          trace_smooth(x, b, 1.0, -1.0, 0.0, c2_0, ch_r, ch_d, nullptr, false, 0.0);      // r0 = b - T x, d0
          trace_smooth(ch_d, ch_r, 1.0, -1.0, c1_1, c2_1, nullptr, nullptr, x, true, 1.0);  // x += d0 + d1
        }
      }
      return;
    }
    // zero initial guess: the first residual is b itself and the first step assigns x (no copy, no fill)
    const double* r0 = b;
    if (!zero_init) { trace_apply(x, b, 1.0, -1.0, ch_r); r0 = ch_r; }
    trace_cheb(r0, ch_d, x, 0.0, 1.0 / theta, zero_init);
    for (int it = 1; it < its; it++) {
      trace_apply(ch_d, it == 1 ? r0 : ch_r, 1.0, -1.0, ch_r);
      double rn = 1.0 / (2.0 * sigma1 - rho);
      trace_cheb(ch_r, ch_d, x, rn * rho, 2.0 * rn / delta);
      rho = rn;
    }
  }
  // ---- vertex-grid V-cycle.  Which form a level runs as is decided in ONE place, the level plan (hdg_vertex_levels.hpp, built
  // in setup_trace_solver); the kernels of every form are in hdg_vertex_mg.hpp, each for both grids (PER: the periodic square).
  VertexPlan vplan;
  // trace_cg_sr with the tile preconditioner: the half of the update nothing reads before the next update (p, x) rides on the
  // leg launches of the V-cycle (k_p1_down / k_p1_up side jobs, hdg_vertex_mg.hpp: SideXP), a share of the pairs per leg by
  // weight (VertexPlan::side_weight_sum); what the legs did not take (no Legs level, rounding of the shares) is done by
  // finish() as a launch of its own.  (A second stream underneath the cycle was measured and removed: DESIGN.md section 9.)
  // The CG queues its updates and sets x, trace_precond brackets the cycle with begin / finish, the V-cycle takes its slices.
  // Up to opt.cg_xp_batch consecutive updates are queued (hdg_cg_pending.hpp) and applied in ONE pass over p and x, entry by
  // entry and in order -- the bits of one pass each, M + 5 vector passes instead of 6 M: the preconditioner writes the z of
  // iteration j to slot j mod M of a ring of trace vectors (cg_zring), the kernel that forms the CG scalars leaves (alpha, beta, c)
  // at the same slot of d_cgh, and the cycle that finds the ring full carries the batch.
  struct XpRide {
    Engine* e;
    CgPending q;          // the queued updates
    double* x = nullptr;  // the iterate they update
    bool due = false;     // the cycle between begin and finish has to apply the queue: its post kernel overwrites the oldest z
    long done = 0;        // pairs already handed to side jobs
    double wsum = 0.0;    // sum of the leg weights of one cycle
    bool riding = false;
    XpBatch batch(const CgBatch& b) const { return XpBatch{e->d_zring, e->d_cgh, q.slot(b.first), q.M, b.count}; }
    void begin(const VertexPlan& pl) {
      done = 0; riding = false;
      due = q.count() > 0 && q.full();
      if (!due) return;
      // strips: the finest level is distributed (vcycle_distributed_top launches its legs itself); the replicated levels carry the update
      wsum = pl.side_weight_sum(e->mg_distributed() ? 1 : 0, e->opt.cg_xp_w0);
      riding = wsum > 0.0;
    }
    SideXP slice(int lev, int nt, int& extra_rows) {
      extra_rows = 0;
      SideXP sj{};
      if (!riding) return sj;
      const long total = e->NLv >> 1;
      long cnt = (long)std::ceil((double)total * VertexPlan::side_weight(lev, e->opt.cg_xp_w0) / wsum);
      cnt = std::min(cnt, total - done);
      if (cnt <= 0) return sj;
      sj = SideXP{batch(q.all()), e->tr_one, e->cg_p, x, done, done + cnt};
      done += cnt;
      const long blocks = (cnt + HDG_P1_THREADS - 1) / HDG_P1_THREADS;
      extra_rows = (int)((blocks + nt - 1) / nt);
      return sj;
    }
    // the updates of b on the pairs from `taken` on, as a launch of its own; the census counts the passes of the whole batch here
    void apply(const CgBatch& b, long taken) {
      if (b.count <= 0) return;
      const long NLv = e->NLv;
      e->lc_bytes[LC_VEC] += e->bL() * (b.count + 5);  // reads p, x, n and count z, writes p, x (the launch: counted with the r / s half)
      if (taken < (NLv >> 1) || (NLv & 1))
        k_cg_sr_update_xp<<<e->vec_blocks(NLv - 2 * taken), 256, 0, e->stream>>>(NLv, batch(b), e->tr_one, e->cg_p, x, taken);
    }
    // everything queued, oldest first (what the legs of the cycle in flight did not take of it)
    void finish() {
      const long taken = riding ? done : 0;
      riding = false; done = 0; due = false;
      apply(q.all(), taken);
      q.applied();
    }
    // normal exit of the solve: everything but the newest update, which is the step beyond the tested iterate
    void finish_exit() {
      riding = false; done = 0; due = false;
      apply(q.all_but_newest(), 0);
      q.drop();
    }
  };
  XpRide xp{this};
  template <bool PER>
  void p1_smooth(int lev, int sweeps, bool reverse) {
    const VLevel& v = vplan.lev[lev];
    const dim3 grid((v.pitch + 63) / 64, v.pitch);
    for (int sw = 0; sw < sweeps; sw++) {
      k_p1_rbgs<PER><<<grid, 64, 0, stream>>>(v.n, mg_x[lev], mg_b[lev], reverse ? 1 : 0);
      k_p1_rbgs<PER><<<grid, 64, 0, stream>>>(v.n, mg_x[lev], mg_b[lev], reverse ? 0 : 1);
    }
  }
  static P1Tail tail_levels(const VertexPlan& pl) {
    P1Tail tl;
    tl.nlev = 0;
    for (int l = pl.size() - pl.tail_nlev; l < pl.size(); l++) tl.n[tl.nlev++] = pl.lev[l].n;
    return tl;
  }
  // one V(nsw,nsw) cycle from level `lev` down: right-hand side mg_b[lev], result mg_x[lev].  `pl` has the hierarchy of vplan
  // (the buffers are per level); `ride`: the side jobs the legs carry (null: none)
  void vcycle(const VertexPlan& pl, int lev, XpRide* ride) {
    with_bool(pl.periodic, [&](auto per) { vcycle_on<decltype(per)::value>(pl, lev, ride); });
  }
  template <bool PER>
  void vcycle_on(const VertexPlan& pl, int lev, XpRide* ride) {
    const VLevel& v = pl.lev[lev];
    const int n = v.n, nsw = opt.mg_sweeps, ncoarse = opt.mg_coarse;
    const dim3 grid((v.pitch + 63) / 64, v.pitch);
    switch (v.form) {
      case VForm::DenseTail: {  // the rest of the cycle as one dense matrix (build_dense_tail)
        if (!tail_M || lev != pl.dense_lev) throw std::string("vertex-grid V-cycle: dense tail entered at a level it was not built for");
        const int N = (int)v.nv;
        tally(LC_MG, 16.0 * (PER ? (long)N : pl.tail_vertices()));
        k_p1_dense_tail<<<(N + 3) / 4, 256, 0, stream>>>(N, tail_pitch, tail_M, mg_b[lev], mg_x[lev]);
        return;
      }
      case VForm::TailKernel: {  // all remaining levels fit one workgroup's LDS: the rest of the cycle in a single kernel
        if (PER || lev != pl.size() - pl.tail_nlev) throw std::string("vertex-grid V-cycle: one-workgroup tail entered at a level it does not start at");
        tally(LC_MG, 16.0 * pl.tail_vertices());
        k_p1_vcycle_tail<<<1, 1024, 0, stream>>>(tail_levels(pl), mg_b[lev], mg_x[lev], nsw, ncoarse);
        return;
      }
      case VForm::Coarsest:
        zero(mg_x[lev], v.nv);
        p1_smooth<PER>(lev, ncoarse, false);
        p1_smooth<PER>(lev, ncoarse, true);
        return;
      case VForm::Legs: {  // one kernel per leg (LDS tiles with recomputed halos), bit-identical to the per-level launches
        const int nt = (v.pitch + HDG_P1_TS - 1) / HDG_P1_TS;
        auto leg = [&](bool down) {
          // down: reads b, writes the pre-smoothed x and the coarse right-hand side; up: reads the coarse x, b, the pre-smoothed x, writes x
          tally(LC_MG, 8.0 * v.nv * (down ? 2.25 : 3.25));
          int extra = 0;
          const SideXP sj = ride ? ride->slice(lev, nt, extra) : SideXP{};
          const dim3 gl(nt, nt + extra);
          const int period = side_row_period(nt, extra);  // hdg_side_rows.hpp
          auto launch = [&](auto s) {
            constexpr int NSW = decltype(s)::value;
            if (down) k_p1_down<NSW, PER><<<gl, HDG_P1_THREADS, 0, stream>>>(n, mg_b[lev], mg_r[lev], mg_b[lev + 1], 0, extra, period, sj);
            else k_p1_up<NSW, PER><<<gl, HDG_P1_THREADS, 0, stream>>>(n, mg_x[lev + 1], mg_b[lev], mg_r[lev], mg_x[lev], 0, extra, period, sj);
          };
          if constexpr (PER) with_int<2>(nsw, "smoothing sweeps of a fused leg (periodic square)", launch);
          else with_int<1, 2, 3>(nsw, "smoothing sweeps of a fused leg", launch);
        };
        leg(true);
        vcycle_on<PER>(pl, lev + 1, ride);
        leg(false);
        return;
      }
      case VForm::PerLevel: {
        const VLevel& c = pl.lev[lev + 1];
        zero(mg_x[lev], v.nv);
        p1_smooth<PER>(lev, nsw, false);
        k_p1_residual<PER><<<grid, 64, 0, stream>>>(n, mg_x[lev], mg_b[lev], mg_r[lev]);
        k_p1_restrict<PER><<<dim3((c.pitch + 63) / 64, c.pitch), 64, 0, stream>>>(c.n, mg_r[lev], mg_b[lev + 1]);
        vcycle_on<PER>(pl, lev + 1, ride);
        k_p1_prolong_add<PER><<<grid, 64, 0, stream>>>(c.n, mg_x[lev + 1], mg_x[lev]);
        p1_smooth<PER>(lev, nsw, true);
        return;
      }
    }
  }
  // Dense form of the V-cycle tail (k_p1_dense_tail), built once per engine where the plan has one: column c of M = the tail
  // applied to the c-th unit vector.  Unit square: one launch of the tail kernel, a workgroup per unit vector.  Periodic
  // square: the per-level cycle from the tail's level applied to each unit vector in turn (n^2 <= 1024 columns of ~45 small
  // launches, a few tenths of a second), through a plan of the same hierarchy with the legs and the dense tail switched off.
  double* tail_M = nullptr;
  int tail_pitch = 0;
  void build_dense_tail() {
    const int lev = vplan.dense_lev;
    if (lev < 0) return;
    const int N = (int)vplan.lev[lev].nv, pitch = (N + 1) & ~1;
    double* MT = dalloc((long)N * pitch);
    double* M = dalloc((long)N * pitch);
    if (!periodic) k_p1_vcycle_tail<<<N, 1024, 0, stream>>>(tail_levels(vplan), nullptr, MT, opt.mg_sweeps, opt.mg_coarse, pitch);
    else {
      Options per_level = opt;
      per_level.mg_fuse = false; per_level.mg_dense_tail_periodic = false;
      const VertexPlan pl = vertex_plan(g.nx, true, per_level);
      const double one = 1.0;
      for (int c = 0; c < N; c++) {
        zero(mg_b[lev], N);
        HIPCHECK(hipMemcpyAsync(mg_b[lev] + c, &one, sizeof(double), hipMemcpyHostToDevice, stream));
        vcycle(pl, lev, nullptr);
        HIPCHECK(hipMemcpyAsync(MT + (long)c * pitch, mg_x[lev], sizeof(double) * N, hipMemcpyDeviceToDevice, stream));
      }
    }
    k_transpose_sq<<<dim3((N + 255) / 256, N), 256, 0, stream>>>(N, pitch, MT, M);
    HIPCHECK(hipStreamSynchronize(stream));
    HIPCHECK(hipFree(MT));
    allocs.erase(std::find(allocs.begin(), allocs.end(), (void*)MT));
    tail_M = M; tail_pitch = pitch;
  }
  // ---- strip partition: the finest vertex grid stays distributed, the rest of the V-cycle is replicated.
  // The replicated cycle (every rank gathers the whole (nx+1)^2 right-hand side, 8.4 MB at C3, and runs every level)
  // does not shrink with the number of ranks.  Here each rank keeps its ny+1 vertex rows of level 0:
  //   1 exchange of 40 vertex rows + the partial cut rows with the strip neighbours (contiguous rows, no packing),
  //   down leg (smoother, residual, restriction) on the tile rows that reach the strip -- the fused leg kernels work on
  //     32-row tiles with recomputed halos, so one extra tile row on either side makes x_pre and the coarse right-hand
  //     side right on everything the up leg and the neighbours' overlap need,
  //   all-gather of the LEVEL-1 right-hand side (a quarter of the bytes), levels >= 1 replicated as before,
  //   up leg on the same tile rows: x_0 on the strip and the 3 rows around it that the prolongation to the trace
  //   ghost rows reads.
  // Needs ny a multiple of 32 and >= 64 (C3 on 8 ranks: 128); otherwise the replicated cycle is used.
  static constexpr int MG_HALO = 40;
  bool mg_distributed() const {
    // (a Legs level 0 means: fused legs on, a coarser level exists, n even; the distributed legs are built for two sweeps)
    return !opt.mg_replicated && opt.mg_sweeps == 2 && mg_gather && comm->size > 1 && !periodic && halo_on && !vplan.lev.empty() &&
           vplan.lev[0].form == VForm::Legs && vplan.lev[0].n > 32 && (g.ny % HDG_P1_TS) == 0 && g.ny >= 2 * HDG_P1_TS &&
           (size_t)(MG_HALO + 1) * (g.nx + 1) <= cap_halo;
  }
  void vcycle_distributed_top() {
    const int n = vplan.lev[0].n, st = n + 1, J0 = g.joff, J1 = g.joff + g.ny;
    const bool has_lo = comm->rank > 0, has_hi = comm->rank < comm->size - 1;
    // halo of the level-0 right-hand side: lower message = rows J0 .. J0+40 (partial cut row first), upper = rows J1-40 .. J1
    const size_t nmsg = (size_t)(MG_HALO + 1) * st;
    comm->exchange(mg_b[0] + (long)J0 * st, hb_rlo, mg_b[0] + (long)(J1 - MG_HALO) * st, hb_rhi, nmsg, stream);
    n_halo_mg++;
    k_p1_merge_halo<<<std::min(vec_blocks((long)nmsg), 256), 256, 0, stream>>>(st, MG_HALO, J0, J1, has_lo ? 1 : 0, has_hi ? 1 : 0,
                                                                             hb_rlo, hb_rhi, mg_b[0]);
    // tile rows of this rank (+ one on either side where a neighbour exists)
    const int nt = (n + 1 + HDG_P1_TS - 1) / HDG_P1_TS;
    const int t0 = std::max(0, J0 / HDG_P1_TS - (has_lo ? 1 : 0));
    const int t1 = std::min(nt, J1 / HDG_P1_TS + 1);  // incl. the tile row that holds vertex row J1 (the top rank: row n)
    const dim3 gt(nt, t1 - t0);
    k_p1_down<2><<<gt, HDG_P1_THREADS, 0, stream>>>(n, mg_b[0], mg_r[0], mg_b[1], t0);
    // level-1 right-hand side: every rank contributes its ny/2 + 1 coarse rows (the cut rows are computed twice, identically)
    const int nc = vplan.lev[1].n, stc = nc + 1, nyc2 = g.ny / 2;
    comm->allgather(mg_b[1] + (long)(J0 / 2) * stc, mg_gather, (size_t)(nyc2 + 1) * stc, stream);
    n_gather++;
    k_p1_assemble<<<vec_blocks((long)stc * stc), 256, 0, stream>>>(comm->size, nyc2, stc, mg_gather, mg_b[1], 0);
    vcycle(vplan, 1, &xp);
    k_p1_up<2><<<gt, HDG_P1_THREADS, 0, stream>>>(n, mg_x[1], mg_b[0], mg_r[0], mg_x[0], t0);
  }
  // z = M r for the condensed system
  // LDS-tiled form of the two smoother applications (hdg_trace_tile.hpp): single rank, non-periodic structured mesh,
  // two Chebyshev steps.  HDG_TRACE_NO_TILE: the five row-stencil launches of before.
  // form of the tile kernels: one thread per edge (hdg_trace_tile3.hpp) or one per corner (hdg_trace_tile.hpp); default: the edge
  // form at k = 4 only (measurements beside Options::trace_tile3)
  bool tile3() const { return opt.trace_tile3 >= 0 ? opt.trace_tile3 != 0 : K >= 4; }
  static constexpr int TILE_HALO_R = 5;
  // Periodic strips: the shortest strip that is accepted.  Every exchange sends at most the strip's own rows (the solvers'
  // depth is Dx = min(DX_DEFAULT, ny), the tiled preconditioner's TILE_HALO_R only runs on strips of >= 8 rows), so one row
  // would be enough for the ghost depth; with one row, though, a rank's lower and upper messages are the same owned row,
  // a case nothing else exercises.  Two rows is the shortest strip the unit-square partition is tested at as well.
  static constexpr int PERIODIC_MIN_ROWS = 2;  // ghost rows of r the tiled preconditioner reads on a strip (pre: 3 computed + 2 halo)
  bool use_trace_tile() const {
    // k = 4: the post kernel needs 274 VGPRs (15 trace values per corner and stage): 5.88 instead of 5.65 ms per solve at 512^2
    // periodic square: the wrapped ghost rows play the neighbours' part (every tile reaches at most 3 columns / 5 rows beyond)
    if (periodic && !(opt.trace_tile_periodic && g.nx >= 16 && g.ny >= 8)) return false;
    return opt.trace_tile && opt.trace_fuse && opt.trace_smooth_its == 2 && cfg.trace_precond == 1 && !general && halo_on &&
           (K <= 3 || tile3()) && (comm->size == 1 || (opt.trace_tile_strips && g.ny >= TILE_HALO_R));
  }
  // periodic strips: the vertex grid has exactly ny rows and every rank restricts onto its own ny/P of them (k_trace_to_p1p at
  // rows pj0 ..), so the rank blocks are disjoint and lie in rank order: ONE all-gather, in place, assembles the global
  // right-hand side; the replicated V-cycle (fused legs, dense tail) then runs on every rank as on one rank
  void gather_periodic_rhs() {
    if (comm->size == 1) return;
    const long blk = (long)g.ny * g.nx;
    comm->allgather(mg_b[0] + (long)g.pj0 * g.nx, mg_b[0], (size_t)blk, stream);
    n_gather++;
  }
  // vertex-grid correction of the trace preconditioner: mg_b[0] <- restriction of `res` (owned edges), one V-cycle, result in
  // mg_x[0] (global vertex numbering; on a strip valid on the rank's vertex rows and the 3 rows around them)
  void coarse_correction(const double* res) {
    const int partial = mg_gather ? 1 : 0;
    tally(LC_MG, bL() + 8.0 * (g.nx + 1.0) * (g.ny + 1.0));
    if (periodic) {  // (row -1 of `res` comes from the pre kernel's ghost rows)
      k_trace_to_p1p<<<corner_grid(), bs(), 0, stream>>>(g, NL, res, mg_b[0], dt.elen[0], dt.elen[2], dt.elen[1]);
      gather_periodic_rhs();
      vcycle(vplan, 0, &xp);
      return;
    }
    k_trace_to_p1<<<corner_grid_all(), bs(), 0, stream>>>(g_all, NL, res, mg_b[0], dt.elen[0], dt.elen[2], dt.elen[1], partial);
    if (mg_distributed()) { vcycle_distributed_top(); return; }
    if (mg_gather) {
      // every rank contributes its (ny+1) vertex rows; one kernel assembles the global vector from the blocks
      const long blk = (long)(g.ny + 1) * (g.nx + 1);
      comm->allgather(mg_b[0] + (long)g.joff * (g.nx + 1), mg_gather, (size_t)blk, stream);
      n_gather++;
      const long nvtx = ((long)comm->size * g.ny + 1) * (g.nx + 1);
      k_p1_assemble<<<vec_blocks(nvtx), 256, 0, stream>>>(comm->size, g.ny, g.nx + 1, mg_gather, mg_b[0], partial);
    }
    vcycle(vplan, 0, &xp);
  }
  // returns true when w_out has received T z (the operator application the single-reduction CG needs next); with
  // dots_out set as well, d_res then holds (z,n), (z,r), (z,z), (z,w), (n,r) (the multi-dot of that CG: *dots_out = true)
  double* tile_part = nullptr;
  long tile_part_cap = 0;
  // trace_cg_sr on one rank: the post kernel's partial inner products are summed by k_cg_sr_reduce_scalars (one launch
  // instead of k_reduce_parts + k_cg_sr_scalars)
  bool defer_tile_reduce = false;
  int tile_nblk_deferred = 0;
  bool trace_precond(const double* r, double* z, double* w_out = nullptr, bool* dots_out = nullptr) {
    if (dots_out) *dots_out = false;
    if (cfg.trace_precond == 0) {
      zero(z, NLv);
      trace_cheb(r, ch_d, z, 0.0, 1.0);
      return false;
    }
    const int nsm = opt.trace_smooth_its;
    if (use_trace_tile()) {
      const double theta = 0.5 * (cheb_lmax + cheb_lmin), delta = 0.5 * (cheb_lmax - cheb_lmin), sigma1 = theta / delta;
      const double rho = 1.0 / sigma1, rn = 1.0 / (2.0 * sigma1 - rho), c0 = 1.0 / theta, c1 = rn * rho, c2 = 2.0 * rn / delta;
      const double nvtx = 8.0 * (g.nx + 1.0) * (g.ny + 1.0);
      // strip partition: the ONE exchange of a CG iteration -- r, 5 ghost rows deep (the pre kernel computes z on 3 ghost rows
      // towards every neighbour from r on 5; the post kernel then finds its halo of z and r locally)
      const bool has_lo = this->has_lo(), has_hi = this->has_hi();
      if (periodic && comm->size == 1) halo_L(r, TILE_HALO_R);  // (k_wrap_rows: every ghost row from the opposite side)
      else if (comm->size > 1) {
        if (fl.get(r) < TILE_HALO_R) { halo_L(r, TILE_HALO_R); fl.set(r, TILE_HALO_R); }
        else if (opt.flow_check) flow_check_input(r, FL, TILE_HALO_R);
      }
      auto launch = [&](auto kk) {
        constexpr int KK = decltype(kk)::value;
        typedef TraceTile<KK> TT;
        TileRows pre{has_lo ? -3 : 0, g.nyc + (has_hi ? 3 : 0), 0, 0}, post{0, g.nyc, -3, g.nyc + 3};
        pre.rlo = pre.jlo - 2; pre.rhi = pre.jhi + 2;
        const int ntx = (g.nx + (periodic ? 0 : 1) + TT::TW - 1) / TT::TW;
        const int nty_pre = (pre.jhi - pre.jlo + TT::TH - 1) / TT::TH, nty = (post.jhi - post.jlo + TT::TH - 1) / TT::TH;
        const int grid_pre = 8 * ((ntx * nty_pre + 7) / 8), grid = 8 * ((ntx * nty + 7) / 8);  // XCD-aware tile order (HDG_TILE_OF_BLOCK)
        tally(LC_TRACE_SMOOTH, 3 * bL());
        typedef TraceTile3<KK> T3;
        if (tile3()) k_trace_pre_tile3<KK><<<grid_pre, T3::NTHREADS, 0, stream>>>(ntx, nty_pre, g, pre, pdt(), r, c0, c1, c2, ch_d, wL2);
        else k_trace_pre_tile<KK><<<grid_pre, TT::NTHREADS, 0, stream>>>(ntx, nty_pre, g, pre, pdt(), r, c0, c1, c2, ch_d, wL2);
        xp.begin(vplan);  // a full batch of deferred CG updates: on the legs of the vertex-grid cycle ...
        if (xp.due && !xp.riding) xp.finish();  // ... or, where no leg can carry it, as a launch of its own
        coarse_correction(wL2);
        if (xp.due) xp.finish();  // what the legs did not take; the post kernel overwrites the oldest z of the batch
        tally(LC_TRACE_SMOOTH, (w_out ? 4 : 3) * bL() + nvtx);
        const long nblk = (long)ntx * nty;
        double* part = nullptr;
        if (w_out && dots_out && opt.trace_fused_dots) {
          if (tile_part_cap < nblk * 5) { tile_part = dalloc(nblk * 5); tile_part_cap = nblk * 5; }
          part = tile_part;
        }
        if (tile3() && part)
          k_trace_post_tile3<KK, true><<<grid, T3::NTHREADS, 0, stream>>>(ntx, nty, g, post, pdt(), ch_d, r, mg_x[0], std::sqrt(dt.elen[0]), std::sqrt(dt.elen[2]),
                                                                          std::sqrt(dt.elen[1]), c0, c1, c2, z, w_out, part);
        else if (tile3())
          k_trace_post_tile3<KK, false><<<grid, T3::NTHREADS, 0, stream>>>(ntx, nty, g, post, pdt(), ch_d, r, mg_x[0], std::sqrt(dt.elen[0]), std::sqrt(dt.elen[2]),
                                                                           std::sqrt(dt.elen[1]), c0, c1, c2, z, w_out, nullptr);
        else if (part)
          k_trace_post_tile<KK, true><<<grid, TT::NTHREADS, 0, stream>>>(ntx, nty, g, post, pdt(), ch_d, r, mg_x[0], std::sqrt(dt.elen[0]), std::sqrt(dt.elen[2]),
                                                                         std::sqrt(dt.elen[1]), c0, c1, c2, z, w_out, part);
        else
          k_trace_post_tile<KK, false><<<grid, TT::NTHREADS, 0, stream>>>(ntx, nty, g, post, pdt(), ch_d, r, mg_x[0], std::sqrt(dt.elen[0]), std::sqrt(dt.elen[2]),
                                                                          std::sqrt(dt.elen[1]), c0, c1, c2, z, w_out, nullptr);
        if (part) {
          if (defer_tile_reduce) tile_nblk_deferred = (int)nblk;  // one rank: summed by the kernel that forms the CG scalars
          else { tally(LC_OTHER, 0.0); reduce_parts_allreduce((int)nblk, 5, part); }  // second reduction stage (+ the all-reduce across ranks) -> d_res
          *dots_out = true;
        }
      };
      by_degree(launch);
      fl.set(z, 0); fl.set(w_out, 0);
      n_tile_precond++;
      return w_out != nullptr;
    }
    if (general) {
      cheb_smooth(r, z, true, nsm);
      trace_apply(z, r, 1.0, -1.0, wL2, 0);
      csr(gs().amg.R0, wL2, 1.0, 0.0, gs().amg.b[0]);
      amg_vcycle(0);
      cheb_smooth(r, z, false, nsm, gs().amg.x[0]);
      return false;
    }
    cheb_smooth(r, z, true, nsm);
    trace_apply(z, r, 1.0, -1.0, wL2, 0);  // restricted from owned rows only: no extension
    // restriction to the vertex grid from OWNED edges only (no halo of wL2): the cut rows are completed when the
    // gathered blocks are assembled
    const int partial = mg_gather ? 1 : 0;
    if (periodic) {
      halo_L(wL2);
      k_trace_to_p1p<<<corner_grid(), bs(), 0, stream>>>(g, NL, wL2, mg_b[0], dt.elen[0], dt.elen[2], dt.elen[1]);
      gather_periodic_rhs();
      vcycle(vplan, 0, &xp);
      k_p1p_to_trace<<<corner_grid(), bs(), 0, stream>>>(g, NL, mg_x[0], z, 1.0, dt.elen[0], dt.elen[2], dt.elen[1]);
      fl.set(z, 0);  // owned rows only: the wrapped ghost rows are stale
      cheb_smooth(r, z, false, nsm);
      return false;
    }
    coarse_correction(wL2);
    cheb_smooth(r, z, false, nsm, mg_x[0]);
    return false;
  }
  void setup_trace_solver() {
    // null-space vector
    {
      long ne = n_edges();
      std::vector<double> ones((size_t)ne * NL, 1.0);
      HIPCHECK(hipMemcpyAsync(hL_dev, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice, stream));
      l_to_modal(hL_dev, tr_one);
      HIPCHECK(hipStreamSynchronize(stream));
    }
    // multigrid hierarchy on the vertex grid (general meshes: algebraic hierarchy of the P1 space)
    if (cfg.trace_precond == 1 && general) setup_general_amg(gops.S, gsets[0].amg);
    else if (cfg.trace_precond == 1) {
      if (comm->size > 1 || opt.force_rccl) mg_gather = dalloc((long)comm->size * (g.ny + 1) * (g.nx + 1));
      vplan = vertex_plan(g.nx, periodic, opt);  // the hierarchy and the form of every level
      for (const VLevel& v : vplan.lev) { mg_x.push_back(dalloc(v.nv)); mg_b.push_back(dalloc(v.nv)); mg_r.push_back(dalloc(v.nv)); }
      build_dense_tail();
    }
    psets.push_back(PSet{dt, 0.0, 0.0, cfg.tau});
    estimate_cheb(0);
    use_pset(0);
    bwd_tol = opt.trace_backward_tol;
  }
  // largest eigenvalue of Dinv * (-S) by power iteration (PETSc estimates it with a few GMRES
  // steps and uses [0.1, 1.1] * lambda_max as Chebyshev interval)
  void estimate_cheb(int idx) {
    int saved = cur_pset;
    cur_pset = idx;
    long ne = n_edges();
    std::vector<double> rnd((size_t)ne * NL);
    unsigned long long st = 88172645463325252ULL;
    for (auto& v : rnd) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = (double)(st % 2000001ULL) / 1.0e6 - 1.0; }
    HIPCHECK(hipMemcpyAsync(hL_dev, rnd.data(), sizeof(double) * rnd.size(), hipMemcpyHostToDevice, stream));
    l_to_modal(hL_dev, cg_p);
    double lam = 1.0;
    for (int it = 0; it < 20; it++) {
      double nrm = std::sqrt(dot(NLv, cg_p, cg_p, KL));
      axpby(NLv, 0.0, cg_p, 1.0 / nrm, cg_p);
      trace_apply(cg_p, nullptr, 0.0, 1.0, cg_Ap);
      zero(cg_z, NLv);
      trace_cheb(cg_Ap, ch_d, cg_z, 0.0, 1.0);
      lam = std::sqrt(dot(NLv, cg_z, cg_z, KL));
      copy(cg_p, cg_z, NLv);
    }
    psets[idx].lmax = 1.1 * lam;
    psets[idx].lmin = opt.trace_cheb_lo * lam;
    cur_pset = saved;
  }
  // operator set for a stabilisation parameter tau' (created on first use)
  int get_pset(double tau_) {
    for (size_t i = 0; i < psets.size(); i++)
      if (std::fabs(psets[i].tau - tau_) <= 1e-14 * std::fabs(tau_)) return (int)i;
    if (general) {
      // a second set of the tau-dependent operators (and its own coarse hierarchy), assembled like the first
      GeneralTables t2(K, tau_, cfg.alpha_penalty, cfg.equispaced_nodes);
      GeneralOps o2;
      std::vector<CellLocal> l2;
      assemble_general(t2, *gm, o2, l2);
      gsets.emplace_back();
      upload_gset(o2, gsets.back());
      if (cfg.trace_precond == 1) setup_general_amg(o2.S, gsets.back().amg);
      psets.push_back(PSet{dt, 0.0, 0.0, tau_});
      estimate_cheb((int)psets.size() - 1);
      return (int)psets.size() - 1;
    }
    PSet ps{dt, 0.0, 0.0, tau_};
    dvec SKh[2];
    for (int sh = 0; sh < 2; sh++) {
      dvec Ai, W_, Y_;
      tab->poissonBlock(sh, tau_, Ai, W_, Y_, SKh[sh]);
      ps.dt.Ainv[sh] = upload(Ai); ps.dt.W[sh] = upload(W_); ps.dt.Y[sh] = upload(Y_); ps.dt.SK[sh] = upload(SKh[sh]);
    }
    dvec tri[3][3];
    tab->traceBlockInverses(SKh, tri);
    for (int t = 0; t < 3; t++) for (int v = 0; v < 3; v++) ps.dt.trDinv[t][v] = upload(tri[t][v]);
    ps.dt.tau = tau_;
    psets.push_back(ps);
    estimate_cheb((int)psets.size() - 1);
    return (int)psets.size() - 1;
  }
  // preconditioned CG on (-S) x = b from the initial guess in x; returns iterations.
  // Convergence on the preconditioned residual norm relative to its initial value (hdg_imex.py:136-137).
  // Same iteration with the scalars kept on the device: alpha, beta and the projection coefficient are produced
  // by one-thread kernels from the reduced dot products and read by the vector kernels, so the host never waits
  // inside an iteration.  Convergence is checked ONE launch group late: the next operator application and its
  // p.Ap reduction are queued first (they modify no state), then the host reads the snapshot of (z',z') taken
  // after the preconditioner -- by then it has long arrived.  2 blocking syncs per iteration become 0.
  int trace_cg_dev(double* b, double* x, double rtol, int maxit, bool strict) {
    project_const(b);
    FlowScope flow_(*this);
    if (fl.Dx > 1) { halo_L(b, fl.Dx - 1); fl.set(b, fl.Dx - 1); }  // r = b - T x on the ghost rows the operator reaches
    trace_apply(x, b, 1.0, -1.0, cg_r);  // r = b - T x
    trace_precond(cg_r, cg_z);
    if (tr_one_nn < 0) tr_one_nn = dot(NLv, tr_one, tr_one, KL);
    const int nvb = vec_blocks(NLv);
    HIPCHECK(hipMemsetAsync(d_cgs, 0, sizeof(double) * 8, stream));
    auto dots_and_snapshot = [&](int first) {
      multidot(NLv, cg_z, {tr_one, cg_r, cg_z}, nullptr, KL, true);  // (z,n), (z,r), (z,z), (n,r) -> d_res
      k_cg_beta<<<1, 1, 0, stream>>>(d_res, d_cgs, tr_one_nn, first);
      HIPCHECK(hipMemcpyAsync(h_cgs, d_cgs, sizeof(double) * 8, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipEventRecord(cg_ev, stream));
    };
    // (z',z') of the snapshot; on heavy cancellation (z almost parallel to the null vector) it is re-evaluated
    // with the projection applied explicitly (cg_z still holds the z of the snapshot)
    auto snapshot_norm2 = [&](bool direction_pending) {
      HIPCHECK(hipEventSynchronize(cg_ev));
      if (h_cgs[6] == 1.0) throw NotConverged{"trace CG: breakdown (p.Ap <= 0)"};
      double zz = h_cgs[4];
      if (h_cgs[6] == 2.0) {
        axpby(NLv, -h_cgs[3], tr_one, 1.0, cg_z);
        fl.set(cg_z, 0);
        zz = dot(NLv, cg_z, cg_z, KL);
        HIPCHECK(hipMemsetAsync(d_cgs + 6, 0, sizeof(double), stream));
        // the direction update that consumes this z has not been queued yet: it must not project a second time
        if (direction_pending) HIPCHECK(hipMemsetAsync(d_cgs + 3, 0, sizeof(double), stream));
      }
      if (!(zz == zz)) throw NotConverged{"trace CG: NaN residual"};
      return zz;
    };
    dots_and_snapshot(1);
    const double norm0 = std::sqrt(std::max(snapshot_norm2(true), 0.0));
    if (norm0 == 0.0) return 0;
    tally(LC_VEC, bL() * 3);
    k_cg_p_dev<<<nvb, 256, 0, stream>>>(NLv, cg_z, tr_one, d_cgs, cg_p);
    fl.set(cg_p, 0);
    int its = 0;
    while (true) {
      trace_apply(cg_p, nullptr, 0.0, 1.0, cg_Ap);
      multidot(NLv, cg_p, {cg_Ap}, nullptr, KL);
      k_cg_alpha<<<1, 1, 0, stream>>>(d_res, d_cgs);
      if (its > 0) {  // lagged check of the iterate x_its (the kernels queued above do not touch it)
        const double nrm = std::sqrt(std::max(snapshot_norm2(false), 0.0));
        if (debug_cg()) fprintf(stderr, "[cg] it %d |z|/|z0| %.3e  c %.3e rz %.3e\n", its, nrm / norm0, h_cgs[3], h_cgs[0]);
        if (nrm <= rtol * norm0) return its;
        if (its >= maxit) {
          if (strict) throw NotConverged{"trace CG reached max iterations"};
          return its;
        }
      }
      tally(LC_VEC, bL() * 6);
      k_cg_xr_dev<<<nvb, 256, 0, stream>>>(NLv, d_cgs, cg_p, cg_Ap, x, cg_r);  // whole arrays: ghost rows follow
      fl.set(cg_r, std::min(fl.get(cg_r), fl.get(cg_Ap)));
      fl.set(x, 0);
      trace_precond(cg_r, cg_z);
      dots_and_snapshot(0);
      its++;
      tally(LC_VEC, bL() * 4);
      k_cg_p_dev<<<nvb, 256, 0, stream>>>(NLv, cg_z, tr_one, d_cgs, cg_p);
      fl.set(cg_p, 0);
    }
  }
  // The same iteration with ONE reduction (and one all-reduce on several ranks) per iteration instead of two
  // (k_cg_sr_scalars): z = M r, w = T z, five inner products in one pass, then p, s = T p, x, r in one vector kernel.
  // The update is queued before the host looks at the snapshot of (z',z'): when r_k turns out to be converged, x has
  // already taken the step to x_{k+1}, which is harmless (a further CG step) and keeps the host off the critical path.
  // Returns the number of iterations the convergence test needed (the extra step is not counted).
  int trace_cg_sr(double* b, double* x, double rtol, int maxit, bool strict) {
    auto leave = [&]() {  // whatever is still queued is given up (an exception; after finish_exit: the step beyond the tested iterate)
      xp.q.drop(); xp.due = false; xp.riding = false;
      defer_tile_reduce = false; tile_nblk_deferred = 0;
    };
    try {
      defer_tile_reduce = comm->size == 1 && opt.cg_fused_scalars;
      const int its = trace_cg_sr_body(b, x, rtol, maxit, strict, opt.cg_split_update && use_trace_tile());
      xp.finish_exit();  // the queued updates up to the tested iterate
      leave();
      return its;
    } catch (...) {
      leave();
      throw;
    }
  }
  int trace_cg_sr_body(double* b, double* x, double rtol, int maxit, bool strict, bool split) {
    project_const(b);
    FlowScope flow_(*this);
    if (fl.Dx > 1) { halo_L(b, fl.Dx - 1); fl.set(b, fl.Dx - 1); }
    trace_apply(x, b, 1.0, -1.0, cg_r);  // r = b - T x
    if (tr_one_nn < 0) tr_one_nn = dot(NLv, tr_one, tr_one, KL);
    if (!cg_s) cg_s = dalloc(NLv);
    double *const r_cur = cg_r, *const s_cur = cg_s;
    const int nvb = vec_blocks(NLv);
    HIPCHECK(hipMemsetAsync(d_cgs, 0, sizeof(double) * 8, stream));
    // the ring of the deferred p / x updates.  One rank only: on strips the whole-array update carries the stale ghost rows of z
    // into those of x, and ring slots are work vectors a checkpoint does not hold
    xp.q.reset(split && comm->size == 1 ? opt.cg_xp_batch : 1);
    xp.x = x;
    if (split) ensure_zring(xp.q.M);
    double* zc = cg_z;  // z of the current iteration: its slot of the ring
    double norm0 = -1.0;
    int its = 0;
    // Residual replacement (round 4; replaces the "attainable accuracy" exit of round 3, which accepted a stalled
    // RECURRENCE residual within 1e3 rtol without looking at the true one).  A solve whose right-hand side is tiny against the
    // iterate it corrects (second Richardson pass, k = 4 on 2048^2: |z0| = 2e-4 against an O(1) trace) cannot always reduce the
    // recurrence residual by 1e-12: the single-reduction recurrences (s = w + beta s, p.Ap from inner products) drift from
    // the true residual, the norm stalls a few units above the target and p.Ap eventually turns non-positive.  On either
    // symptom -- no new best |z| for five iterations within three decades of the target, or p.Ap <= 0 -- the TRUE residual
    // r = b - T x is recomputed, the recurrences restart from it (beta = 0), and the solve ends only if the true
    // preconditioned residual meets rtol (hdg_imex.py:136-137) or lies at its rounding floor:
    //     |M r| <= cg_floor_c * eps * |x|
    // (r = b - T x cannot be evaluated more accurately than eps |T| |x| per entry, a sum of 3 n_lambda * 5 <= 75 products;
    // M T has its spectrum in (0, 1.1], so |M delta_r| ~ sqrt(75) eps |x| ~ 10 eps |x|; cg_floor_c = 32 leaves a factor
    // three; HDG_CG_FLOOR_C overrides).  |z| of a preconditioned CG is not monotone, so a slow but healthy solve (the one-level
    // edge block-Jacobi preconditioner: ~0.9 per iteration) can show five non-improving iterations as well: if the true
    // residual then agrees with the recurrence one (within a factor 4) it was a false alarm -- the restart is harmless, the
    // patience doubles (5, 10, 20, ... iterations) and the event does not count against the limit.  At most two CONFIRMED
    // drifts per solve; a third is HDG_ERR_NOT_CONVERGED (never silent).  Every replacement and every floor
    // exit is counted (hdg_get_solver_events, bench line).
    double best = 1e300, trigger_nrm = 0.0;
    int since_best = 0, replaced = 0, drifts = 0, patience = 5;
    bool trigger_breakdown = false;
    bool restart = true, true_residual = true;  // the first pass starts from r = b - T x as well
    const double floor_c = opt.cg_floor_c;
    auto replace_residual = [&](const char* why, double at, bool is_breakdown) {
      xp.finish();  // the true residual needs the current iterate
      if (drifts >= 2) throw NotConverged{std::string("trace CG: ") + why + " after two residual replacements that confirmed a drifted recurrence"};
      replaced++;
      trigger_nrm = at; trigger_breakdown = is_breakdown;
      ev_cg_replacements++;
      if (debug_cg()) fprintf(stderr, "[cg] it %d: %s at |z|/|z0| %.3e: residual replacement %d\n", its, why, at / norm0, replaced);
      HIPCHECK(hipMemsetAsync(d_cgs + 6, 0, sizeof(double), stream));
      trace_apply(x, b, 1.0, -1.0, r_cur);  // the true residual of the current iterate
      restart = true; true_residual = true;
      best = 1e300; since_best = 0;
    };
    while (true) {
      bool have_dots = false;
      const int slot = xp.q.write_slot();
      if (split) zc = cg_zring[slot];
      double* const hist = split ? d_cgh + 3 * slot : nullptr;  // (alpha, beta, c) for the deferred update of this iteration
      const bool have_w = trace_precond(r_cur, zc, cg_Ap, &have_dots);
      if (!have_w) trace_apply(zc, nullptr, 0.0, 1.0, cg_Ap);  // w = T z
      if (!have_dots) multidot(NLv, zc, {tr_one, r_cur, zc, cg_Ap}, nullptr, KL, true);  // (z,n), (z,r), (z,z), (z,w), (n,r) -> d_res
      tally(LC_OTHER, 0.0);
      // k_cg_sr_update: reads z, n, w, p, s, x, r; writes p, s, x, r.  Split: k_cg_sr_update_r reads w, s, r and writes s, r; the
      // p / x half is counted where a batch is applied (XpRide::apply)
      tally(LC_VEC, bL() * (split ? 5 : 11));
      if (have_dots && tile_nblk_deferred > 0) {
        k_cg_sr_reduce_scalars<<<1, 1024, 0, stream>>>(tile_nblk_deferred, tile_part, d_res, d_cgs, tr_one_nn, restart ? 1 : 0, direct_host() ? h_cgs : nullptr, hist);
        tile_nblk_deferred = 0;
        n_reduce++;
      } else
        k_cg_sr_scalars<<<1, 1, 0, stream>>>(d_res, d_cgs, tr_one_nn, restart ? 1 : 0, direct_host() ? h_cgs : nullptr, hist);  // + snapshot in pinned memory
      if (!direct_host()) HIPCHECK(hipMemcpyAsync(h_cgs, d_cgs, sizeof(double) * 8, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipEventRecord(cg_ev, stream));
      if (split) {
        // r first (the next preconditioner application waits for it); p and x with their batch, when the ring is full
        k_cg_sr_update_r<<<nvb, 256, 0, stream>>>(NLv, d_cgs, cg_Ap, s_cur, r_cur);
        xp.q.push();
      } else
        k_cg_sr_update<<<nvb, 256, 0, stream>>>(NLv, d_cgs, zc, tr_one, cg_Ap, cg_p, s_cur, x, r_cur);
      fl.set(s_cur, restart ? fl.get(cg_Ap) : std::min(fl.get(s_cur), fl.get(cg_Ap)));
      fl.set(r_cur, std::min(fl.get(r_cur), fl.get(s_cur)));
      fl.set(x, 0);
      const bool was_true = true_residual;
      restart = false; true_residual = false;
      // snapshot of iteration `its` (zc is intact: the next preconditioner application has not been queued)
      HIPCHECK(hipEventSynchronize(cg_ev));
      const bool breakdown = h_cgs[6] == 1.0;  // alpha was set to 0: the update just queued leaves x alone
      double zz = h_cgs[4];
      if (h_cgs[6] == 2.0) {  // z almost parallel to the null vector: measure the projected norm explicitly
        xp.finish();  // (the deferred updates read the unprojected z)
        axpby(NLv, -h_cgs[3], tr_one, 1.0, zc);
        fl.set(zc, 0);
        zz = dot(NLv, zc, zc, KL);
        HIPCHECK(hipMemsetAsync(d_cgs + 6, 0, sizeof(double), stream));
      }
      if (!(zz == zz)) throw NotConverged{"trace CG: NaN residual"};
      const double nrm = std::sqrt(std::max(zz, 0.0));
      if (its == 0) { norm0 = nrm; if (norm0 == 0.0) return 0; }
      if (debug_cg()) fprintf(stderr, "[cg] it %d |z|/|z0| %.3e  c %.3e rz %.3e%s\n", its, nrm / norm0, h_cgs[3], h_cgs[0], was_true ? "  (true residual)" : "");
      if (its > 0 && nrm <= rtol * norm0) return its;
      if (cg_floor > 0.0 && nrm <= cg_floor) return its;  // backward-error stop (experiment, see pressure_solve)
      if (was_true && replaced > 0) {
        // the true preconditioned residual after a replacement: at its rounding floor?
        xp.finish();
        const double xn = std::sqrt(std::max(dot(NLv, x, x, KL), 0.0));
        if (debug_cg()) fprintf(stderr, "[cg] it %d: true |z| %.3e, floor %.3e (|x| %.3e)\n", its, nrm, floor_c * 2.220446049250313e-16 * xn, xn);
        if (nrm <= floor_c * 2.220446049250313e-16 * xn) { ev_cg_floor_exits++; return its; }
        if (trigger_breakdown || nrm > 4.0 * trigger_nrm) drifts++;  // the recurrence residual had left the true one
        else patience *= 2;                                            // false alarm: a slow, non-monotone but healthy solve
      }
      if (breakdown) {
        if (was_true) throw NotConverged{"trace CG: breakdown (p.Ap <= 0) on a freshly computed residual"};
        replace_residual("p.Ap <= 0", nrm, true);
      } else {
        if (nrm < best) { best = nrm; since_best = 0; } else since_best++;
        const bool forced = opt.cg_force_replace > 0 && its == opt.cg_force_replace && replaced == 0;  // test hook
        if (forced || (its > 0 && since_best >= patience && nrm <= 1e3 * rtol * norm0)) replace_residual(forced ? "forced (test hook)" : "stall", nrm, false);
      }
      if (its >= maxit) {
        if (strict) throw NotConverged{"trace CG reached max iterations"};
        return its;
      }
      its++;
    }
  }
  // residual replacements / floor exits of the condensed solves since the last reset (hdg_get_solver_events)
  long ev_cg_replacements = 0, ev_cg_floor_exits = 0;
  int trace_cg(double* b, double* x, double rtol = -1.0, int maxit = -1, bool strict = true) {
    if (rtol < 0) rtol = cfg.trace_rtol;
    if (maxit < 0) maxit = cfg.trace_maxit;
    const bool host_scalars = opt.cg_host_scalars, two_red = opt.cg_two_reductions;
    if (!host_scalars && !two_red) return trace_cg_sr(b, x, rtol, maxit, strict);
    if (!host_scalars) return trace_cg_dev(b, x, rtol, maxit, strict);
    project_const(b);
    trace_apply(x, b, 1.0, -1.0, cg_r);  // r = b - T x
    trace_precond(cg_r, cg_z);
    double rz, zz, c;
    cg_dots(rz, zz, c);
    double norm0 = std::sqrt(zz);
    if (!(norm0 == norm0)) throw NotConverged{"trace CG: NaN residual"};
    if (norm0 == 0.0) return 0;
    const int nvb = vec_blocks(NLv);
    k_cg_p<<<nvb, 256, 0, stream>>>(NLv, cg_z, tr_one, c, 0.0, cg_p);
    int its = 0;
    while (true) {
      trace_apply(cg_p, nullptr, 0.0, 1.0, cg_Ap);
      double pAp = dot(NLv, cg_p, cg_Ap, KL);
      if (!(pAp > 0)) throw NotConverged{"trace CG: breakdown (p.Ap <= 0)"};
      double alpha = rz / pAp;
      k_cg_xr<<<nvb, 256, 0, stream>>>(NLv, alpha, cg_p, cg_Ap, x, cg_r);
      trace_precond(cg_r, cg_z);
      double rz_new;
      cg_dots(rz_new, zz, c);
      its++;
      double nrm = std::sqrt(zz);
      if (debug_cg()) fprintf(stderr, "[cg] it %d |z|/|z0| %.3e  c %.3e rz %.3e pAp %.3e\n", its, nrm / norm0, c, rz_new, pAp);
      if (nrm <= rtol * norm0) return its;
      if (its >= maxit) {
        if (strict) throw NotConverged{"trace CG reached max iterations"};
        return its;
      }
      double beta = rz_new / rz;
      rz = rz_new;
      k_cg_p<<<nvb, 256, 0, stream>>>(NLv, cg_z, tr_one, c, beta, cg_p);
    }
  }
  // inner products of the PROJECTED preconditioned residual z' = z - c n (n = null-space vector, c = (n,z)/(n,n))
  // from one pass over z, r, n:  (z', r) = (z, r) - c (n, r),  (z', z') = (z, z) - c (n, z).  (n, r) vanishes
  // only up to rounding, and that remainder matters once the residual has dropped by 1e-10: without the term the
  // iteration loses orthogonality and diverges.  The projection itself is applied where z' is consumed (k_cg_p).
  // If the subtraction in (z', z') cancels more than 6 digits the projection is done explicitly instead.
  void cg_dots(double& rz, double& zz, double& c) {
    if (tr_one_nn < 0) tr_one_nn = dot(NLv, tr_one, tr_one, KL);
    double d3[4];
    multidot(NLv, cg_z, {tr_one, cg_r, cg_z}, d3, KL, true);  // (z,n), (z,r), (z,z), (n,r)
    c = d3[0] / tr_one_nn;
    rz = d3[1] - c * d3[3];
    zz = d3[2] - c * d3[0];
    if (!(zz > 1e-6 * d3[2])) {
      axpby(NLv, -c, tr_one, 1.0, cg_z);
      double d2[2];
      multidot(NLv, cg_z, {cg_r, cg_z}, d2, KL);
      rz = d2[0]; zz = d2[1]; c = 0.0;
    }
  }

  // ------------------------------------------------------------------ unsplit (monolithic) solve
  // System (hdg_imex.py:602-620; hdg_implicit.py:153-185), gamma = a_ii dt (or dt):
  //     [ A    -gamma G ] [u]   [r]        A = I - gamma F(Q*),  G y = g(w; phi, lambda)
  //     [ D_u    D_y    ] [y] = [0]        (D_u, D_y) = rows of Gamma(psi, mu; u, phi, lambda)
  // The reference factorises the assembled matrix with MUMPS.  Here: flexible GMRES on the full
  // system, right-preconditioned by the block factorisation with A^{-1} ~ inexact tentative-velocity
  // solve and the pressure Schur complement ~ hybridised mixed Poisson operator with
  // stabilisation tau' = tau/gamma acting on y' = gamma y  (D_y is linear in tau):
  //     u~ = A^{-1} r_u ;  K_mp(tau') (du, y') = (0, r_y - D_u u~) ;  u = u~ + du ;  y = y'/gamma
  struct V3 { double *u, *p, *l; };
  std::vector<V3> fg_V, fg_Z;
  V3 fg_r{nullptr, nullptr, nullptr}, fg_w{nullptr, nullptr, nullptr}, fg_b{nullptr, nullptr, nullptr};
  V3 alloc3() { return V3{dalloc(NQ), dalloc(NPv), dalloc(NLv)}; }
  double dot3(const V3& a, const V3& b) { return dot(NQ, a.u, b.u, KQ) + dot(NPv, a.p, b.p, KC) + dot(NLv, a.l, b.l, KL); }
  void axpby3(double a, const V3& x, double b, V3& y) { axpby(NQ, a, x.u, b, y.u); axpby(NPv, a, x.p, b, y.p); axpby(NLv, a, x.l, b, y.l); }
  void copy3(V3& d, const V3& s_) { copy(d.u, s_.u, NQ); copy(d.p, s_.p, NPv); copy(d.l, s_.l, NLv); }
  void mono_apply(const V3& x, const double* qstar, double gamma, V3& out) {
    adv_apply(x.u, qstar, wQ1, gamma);
    pgrad(wQ1, 1.0, nullptr, 0.0, x.p, x.l, -gamma, out.u);
    gamma_psi(x.u, x.p, x.l, out.p);
    gamma_mu(x.u, x.p, x.l, out.l);
  }
  void mono_precond(const V3& r, const double* qstar, double gamma, int didx, int psidx, V3& z) {
    zero(z.u, NQ);
    tent_krylov(TentSystem{qstar, gamma, didx, r.u}, z.u, cfg.unsplit_inner_rtol, 200, false);
    gamma_psi(z.u, nullptr, nullptr, wP1);
    axpby(NPv, 1.0, r.p, -1.0, wP1);
    gamma_mu(z.u, nullptr, nullptr, wL2);
    axpby(NLv, 1.0, r.l, -1.0, wL2);
    use_pset(psidx);
    condense(nullptr, wP1, wL2, wL1);
    zero(z.l, NLv);
    trace_cg(wL1, z.l, cfg.unsplit_inner_rtol, 200, false);
    backsub(nullptr, wP1, z.l, wQ3, z.p);
    use_pset(0);
    axpby(NQ, 1.0, wQ3, 1.0, z.u);
    axpby(NPv, 0.0, z.p, 1.0 / gamma, z.p);
    axpby(NLv, 0.0, z.l, 1.0 / gamma, z.l);
  }
  // flexible GMRES(m) of the unsplit solves; x holds the initial guess
  int fgmres(const double* qstar, double gamma, int didx, int psidx, const V3& b, V3& x) {
    return fgmres_blocks(
        [&](const V3& in, V3& out) { mono_apply(in, qstar, gamma, out); },
        [&](const V3& in, V3& out) { mono_precond(in, qstar, gamma, didx, psidx, out); }, b, x, fg_V, fg_Z, fg_r, fg_w,
        std::max(1, cfg.unsplit_restart), cfg.unsplit_rtol, cfg.unsplit_maxit, "unsplit FGMRES");
  }
  // block-vector operations of fgmres_blocks: (u, phi, lambda) of the HDG systems, (u, phi) of the DG system
  void alloc_block(V3& v) { v = alloc3(); }
  double dot_block(const V3& a, const V3& b) { return dot3(a, b); }
  void axpby_block(double a, const V3& x, double b, V3& y) { axpby3(a, x, b, y); }
  void copy_block(V3& d, const V3& s_) { copy3(d, s_); }
  // right-preconditioned flexible GMRES(m) on block vectors V, restarted; x holds the initial guess; convergence on
  // ||b - K x|| relative to its initial value, confirmed with the true residual (the preconditioner's inner solves are
  // inexact).  apply(x, out): out = K x;  precond(r, z): z ~ K^-1 r.  Vb / Zb / r / w: the caller's basis and work vectors.
  template <class V, class Apply, class Precond>
  int fgmres_blocks(Apply&& apply, Precond&& precond, const V& b, V& x, std::vector<V>& Vb, std::vector<V>& Zb, V& r, V& w,
                    int m, double rtol, int maxit, const char* name) {
    if ((int)Vb.size() < m + 1) {
      while ((int)Vb.size() < m + 1) { Vb.emplace_back(); alloc_block(Vb.back()); }
      while ((int)Zb.size() < m) { Zb.emplace_back(); alloc_block(Zb.back()); }
      alloc_block(r); alloc_block(w);
    }
    GivensLsq lsq(m);
    std::vector<double> h((size_t)m);
    int its = 0;
    double beta0 = -1.0;
    while (true) {
      apply(x, r);
      axpby_block(1.0, b, -1.0, r);
      double beta = std::sqrt(dot_block(r, r));
      if (beta0 < 0) beta0 = beta;
      if (!(beta == beta)) throw NotConverged{std::string(name) + ": NaN residual"};
      if (beta <= rtol * beta0 || beta == 0.0) return its;
      copy_block(Vb[0], r);
      axpby_block(0.0, r, 1.0 / beta, Vb[0]);
      lsq.start(beta);
      int j = 0;
      bool done = false;
      for (; j < m; j++) {
        precond(Vb[j], Zb[j]);
        apply(Zb[j], w);
        for (int l = 0; l <= j; l++) {  // modified Gram-Schmidt
          h[l] = dot_block(w, Vb[l]);
          axpby_block(-h[l], Vb[l], 1.0, w);
        }
        double hn = std::sqrt(dot_block(w, w));
        if (hn > 0) { copy_block(Vb[j + 1], w); axpby_block(0.0, w, 1.0 / hn, Vb[j + 1]); }
        const double res = lsq.add_column(j, h.data(), hn);
        its++;
        if (res <= rtol * beta0 || hn == 0.0) { j++; done = true; break; }
        if (its >= maxit) { j++; break; }
      }
      const std::vector<double> y = lsq.solve(j);
      for (int l = 0; l < j; l++) axpby_block(y[l], Zb[l], 1.0, x);
      if (done) {
        // confirm with the true residual (the inner solves are inexact)
        apply(x, r);
        axpby_block(1.0, b, -1.0, r);
        if (std::sqrt(dot_block(r, r)) <= 10.0 * rtol * beta0) return its;
      }
      if (its >= maxit) throw NotConverged{std::string(name) + " reached max iterations"};
    }
  }
  // stage i of the IMEX scheme without the projection method (hdg_imex.py:600-620)
  int unsplit_solve(int i) {
    if (i < 1 || i >= s) throw std::string("stage out of range");
    Timed tm_(*this, T_UNSPLIT);
    const double gamma = cfg.a_impl[i * s + i] * cfg.dt;
    ensure_dinv(i, gamma);
    const int ps = get_pset(cfg.tau / gamma);
    if (!fg_b.u) fg_b = alloc3();
    std::vector<double> cq, cb;
    residual_coeffs(cfg, i, cq, cb);
    viscosity_slots(cb);
    residual_vector(cq, cb, fg_b.u);
    zero(fg_b.p, NPv);
    zero(fg_b.l, NLv);
    V3 x{stQ[i], stP[i], stL[i]};
    int its = fgmres(Qstar[i - 1], gamma, i, ps, fg_b, x);
    it_sum[0] += its; it_cnt[0]++;
    return its;
  }

  // EXPERIMENT (HDG_TRACE_BACKWARD_TOL = t > 0, read when an engine is built; default off = the reference's rule only): a
  // normwise backward-error stop for the condensed solves of the projection method.  The solves of a step correct ONE field, the
  // pressure trace (|lambda| = S, taken from the last reconstruction solve): an update whose preconditioned residual -- a proxy of
  // its error, M ~ T^-1 -- is below t S (t = 1e-15: ten units in the last place of the field it is added to) cannot change that
  // field any more.  With it the update solves start from zero (the warm start from the PREVIOUS update is a residual 1e4 times
  // the right-hand side in the second Richardson pass), the second pass stops after 6-7 instead of 11 iterations, and the
  // final-stage solve, whose right-hand side vanishes analytically (5e-14 at C3), ends at once.  bench.py reports the step time
  // with it as a secondary number (`alt_stop_rule`); the headline runs without.
  double bwd_tol = 0.0, trace_scale = 0.0, cg_floor = 0.0;
  int pressure_solve(int key) {
    Timed tm_(*this, T_PRESS);
    int its;
    cg_floor = bwd_tol > 0.0 ? bwd_tol * trace_scale : 0.0;
    struct FloorOff { double& f; ~FloorOff() { f = 0.0; } } floor_off_{cg_floor};
    if (key >= 1) {
      if (key >= s) throw std::string("stage out of range");
      const double gamma = cfg.a_impl[key * s + key] * cfg.dt;
      weak_div(Qtent[key], -1.0 / gamma, wP1, false);   // hdg_imex.py:177-179
      condense(nullptr, wP1, nullptr, wL1);
      if (bwd_tol > 0.0) zero(updL, NLv);
      its = trace_cg(wL1, updL);
      backsub(nullptr, wP1, updL, updU, updP);
      it_sum[1] += its; it_cnt[1]++;
    } else if (key == HDG_KEY_FINAL_STAGE) {
      std::vector<double> cq, cb;
      final_residual_coeffs(cfg, cq, cb);
      viscosity_slots(cb);
      residual_vector(cq, cb, wQ3);                     // r^{n+1}  (hdg_imex.py:190-192)
      condense(wQ3, nullptr, nullptr, wL1);
      if (bwd_tol > 0.0) zero(curL, NLv);
      its = trace_cg(wL1, curL);
      backsub(wQ3, nullptr, curL, curQ, curP);
      it_sum[2] += its; it_cnt[2]++;
    } else if (key == HDG_KEY_PRESSURE_RECONSTRUCTION) {
      if (vel_linear_on()) viscosity_slot(s, curQ);  // slot s: Q_{n+1}, complete since the final-stage back-substitution
      if (buoyancy_on() || vel_linear_on()) {  // the kernels take one forcing vector and read the neighbour's too: b_new + B(q^{n+1}) + nu M^-1 V Q_{n+1} summed first
        Terms bnew{{bvec(s), bscale[s]}};
        if (buoyancy_on()) bnew.push_back({buoy[(size_t)s], 1.0});
        if (vel_linear_on()) bnew.push_back({visc[(size_t)s], 1.0});
        lincomb(NQ, bnew, wQ3);
        precon_rhs(curQ, wQ3, 1.0, wP1, wL2);
      } else {
        precon_rhs(curQ, bvec(s), bscale[s], wP1, wL2);   // hdg_imex.py:201-207
      }
      condense(nullptr, wP1, wL2, wL1);
      its = trace_cg(wL1, recL);
      if (bwd_tol > 0.0) trace_scale = std::sqrt(dot(NLv, recL, recL, KL));
      backsub(nullptr, wP1, recL, wQ3, recP);
      it_sum[3] += its; it_cnt[3]++;
    } else
      throw std::string("unknown pressure_solve key");
    return its;
  }

  void state_ptrs(int which, double*& Q, double*& p, double*& l) {
    Q = p = l = nullptr;
    if (which == HDG_STATE_CURRENT) { Q = curQ; p = curP; l = curL; }
    else if (which == HDG_STATE_UPDATE) { Q = updU; p = updP; l = updL; }
    else if (which == HDG_STATE_RECON) { p = recP; l = recL; }
    else if (which >= 1 && which < s) { Q = stQ[which]; p = stP[which]; l = stL[which]; }
    else if (which >= 100 && which < 100 + s) { Q = Qtent[which - 100]; }
    else if (which >= 200 && which < 200 + (int)Qstar.size()) { Q = Qstar[which - 200]; }
    else throw std::string("unknown state selector");
  }

  // Stage slot 0 is the state at the start of the step.  Nothing reads its pressure or trace (state_ptrs does not even expose
  // slot 0), and the velocity of the current state is read by nothing between here and the final-stage back-substitution,
  // which writes all of it after the last reader of slot 0 (the final residual) has run: the recorders (end_of_step), the
  // tracer (stQ[0]) and hdg_get_field all come after that or go through the members.  So a whole step (whole_step: step(),
  // which reaches that back-substitution or fails and undoes the exchange) exchanges the velocity pointers and drops the
  // other two copies.
  // hdg_begin_step keeps the copies: its caller may read the current state, or begin again, before the step is complete.
  // curL and recL keep their copies too (finish_step): the final-stage and reconstruction solves warm-start from the values
  // at those addresses, and HDG_STATE_RECON is readable.
  void begin_step(bool whole_step = false) {
    visc_valid = 0; visc_step = true;  // the viscous slots of the last step are stale
    if (whole_step && opt.glue_fusion) { std::swap(stQ[0], curQ); return; }
    copy(stQ[0], curQ, NQ); copy(stP[0], curP, NPv); copy(stL[0], curL, NLv);
  }
  void stage_update(int i) {
    const double gamma = cfg.a_impl[i * s + i] * cfg.dt;
    lincomb(NQ, {{stQ[i], 1.0}, {Qtent[i], 1.0}, {updU, gamma}}, stQ[i]);
    axpby(NPv, 1.0, updP, 1.0, stP[i]);
    axpby(NLv, 1.0, updL, 1.0, stL[i]);
  }
  void finish_step() {
    visc_step = false;
    copy(curP, recP, NPv);
    copy(curL, recL, NLv);
    shift(curP, curL);
  }
  void step() {
    Timed tm_(*this, T_STEP);
    begin_step(true);
    // a step that fails (a Krylov solve that does not converge) before the final-stage back-substitution has written the new
    // velocity leaves the current state where it was, as the copy did: the exchange is undone
    struct Undo {
      Engine& e;
      bool armed;
      ~Undo() { if (armed) std::swap(e.stQ[0], e.curQ); }
    } undo{*this, opt.glue_fusion};
    tracer_begin_step();
    for (int i = 1; i < s; i++) {
      { Timed tb_(*this, T_BDM); bdm(stQ[i - 1], Qstar[i - 1]); }
      if (cfg.use_projection) {
        for (int r = 0; r < cfg.n_richardson; r++) {
          tentative_solve(i);
          pressure_solve(i);
          shift(updP, updL);
          stage_update(i);
        }
      } else {
        unsplit_solve(i);
      }
      shift(stP[i], stL[i]);
      tracer_stage(i);
    }
    pressure_solve(HDG_KEY_FINAL_STAGE);
    undo.armed = false;
    pressure_solve(HDG_KEY_PRESSURE_RECONSTRUCTION);
    finish_step();
    tracer_finish_step();
  }
  // hdg_implicit.py:92-190 with use_projection_method=True.  Uses stage slot 0 for Q, slot 0 forcing.
  void implicit_step(int* its_t, int* its_p) {
    Timed tm_(*this, T_STEP);
    const double dtt = cfg.dt;
    if (tracer_on) {  // hdg_implicit.py:93-96: b_tracer is built from the fields at the START of the step
      cg_project(curQ, uproj);
      tracer_tendency(q_cur, uproj, q_t);
      if (buoyancy_on()) buoyancy(q_cur, buoy[0]);  // slot 0: the tracer at the start of the step, next to f(t_k)
    }
    // hdg_implicit.py:192-193: the tracer is advanced only after a SUCCESSFUL step (a failed Krylov solve must leave it
    // where Q and p stay), so the update sits before each of the two normal returns, not in a scope guard
    auto tracer_end = [&]() { if (tracer_on) { axpby(NTv(), dtt, q_t, 1.0, q_cur); tracer_implicit_diffusion(); } };
    if (vel_linear_on()) vel_linear_apply(curQ, visc[0]);  // slot 0: Q_n, forward Euler, beside f(t_k)
    ensure_dinv(0, dtt);
    { Timed tb_(*this, T_BDM); bdm(curQ, Qstar[0]); }             // hdg_implicit.py:98
    if (!cfg.use_projection) {
      // monolithic (u, phi, lambda) solve, hdg_implicit.py:153-186; fresh Function -> zero guess
      const int ps = get_pset(cfg.tau / dtt);
      if (!fg_b.u) fg_b = alloc3();
      lincomb(NQ, start_terms(dtt), fg_b.u);
      zero(fg_b.p, NPv); zero(fg_b.l, NLv);
      V3 x{updU, updP, updL};
      zero(updU, NQ); zero(updP, NPv); zero(updL, NLv);
      int it;
      { Timed tu_(*this, T_UNSPLIT); it = fgmres(Qstar[0], dtt, 0, ps, fg_b, x); }
      copy(curQ, updU, NQ); copy(curP, updP, NPv); copy(curL, updL, NLv);
      shift(curP, curL);
      if (its_t) *its_t = it;
      if (its_p) *its_p = 0;
      tracer_end();
      return;
    }
    // rhs lives in updU: wQ1..wQ4 are scratch of GMRES and its preconditioner
    lincomb(NQ, start_terms(dtt), updU);  // (Q,w) + dt (f,w)
    zero(Qtent[0], NQ);
    int it1, it2;
    {
      Timed tt_(*this, T_TENT);
      const TentSystem S{Qstar[0], dtt, 0, updU};  // hdg_implicit.py:103-129
      it1 = cfg.tent_solver == 0 ? tent_krylov(S, Qtent[0], cfg.tent_rtol, cfg.tent_maxit, true) : cheb_gmres(S, Qtent[0]);
    }
    {
      Timed tp_(*this, T_PRESS);
      weak_div(Qtent[0], -1.0 / dtt, wP1, true);                 // hdg_implicit.py:145
      condense(nullptr, wP1, nullptr, wL1);
      zero(updL, NLv);
      it2 = trace_cg(wL1, updL);
      backsub(nullptr, wP1, updL, updU, updP);
    }
    lincomb(NQ, {{Qtent[0], 1.0}, {updU, dtt}}, curQ);           // hdg_implicit.py:150
    copy(curP, updP, NPv);
    copy(curL, updL, NLv);
    shift(curP, curL);                                           // hdg_implicit.py:189-190
    if (its_t) *its_t = it1;
    if (its_p) *its_p = it2;
    tracer_end();
  }

  // ================================================================== implicit DG discretisation (dg_implicit.py:10-136)
  // Spaces [DG_{k+1}]^2 x DG_k (the HDG spaces without the trace).  With A = I - dt F(Q*) (F: the HDG f_impl, alpha = 1)
  // the system of dg_implicit.py:48-75 is
  //     [ A      -dt B^T ] [u  ]   [ Q + dt f ]          B = weak_div(., broken = false)  (hdg_imex.py:353-365)
  //     [ dt B    0      ] [phi] = [ 0        ]          B^T phi = g(w; phi, avg(phi))  (pgrad with lambda = avg(phi))
  // Solved with the continuity rows scaled by 1/dt for y = dt phi:  K_dg (u, y) = (A u - g(y, avg y), B u).
  // K_dg is singular and consistent (phi = const: B^T 1 = 0; the continuity rows sum to zero): GMRES on the consistent
  // system, then phi is shifted to zero mean like the reference does after MUMPS (dg_implicit.py:130).
  // Preconditioner (block triangular, right): u~ = A^-1 r_u (inexact GMRES), then the Schur complement B A^-1 B^T is
  // replaced by the hybridised mixed Poisson operator at tau' = tau / dt (condense / trace CG / back-substitution, as in
  // mono_precond without the trace rows): K_mp (du, y, lambda) = (0, r_p - B u~, 0), u = u~ + du.
  struct V2 { double *u, *p; };
  std::vector<V2> dg_V, dg_Z;
  V2 dg_r{nullptr, nullptr}, dg_w{nullptr, nullptr}, dg_b{nullptr, nullptr}, dg_x{nullptr, nullptr};
  double *dg_lam = nullptr, *dg_lam2 = nullptr, *dg_rp = nullptr, *dg_du = nullptr;
  const int* dg_ecl = nullptr;  // general meshes: (3 c + l) of the cells of every edge (k_g_dg_avg_trace)
  void alloc_block(V2& v) { v = V2{dalloc(NQ), dalloc(NPv)}; }
  double dot_block(const V2& a, const V2& b) { return dot(NQ, a.u, b.u, KQ) + dot(NPv, a.p, b.p, KC); }
  void axpby_block(double a, const V2& x, double b, V2& y) { axpby(NQ, a, x.u, b, y.u); axpby(NPv, a, x.p, b, y.p); }
  void copy_block(V2& d, const V2& s_) { copy(d.u, s_.u, NQ); copy(d.p, s_.p, NPv); }
  void dg_alloc() {
    if (dg_lam) return;
    if (comm->size > 1) throw std::string("DG discretisation: single rank only");
    dg_lam = dalloc(NLv); dg_lam2 = dalloc(NLv); dg_rp = dalloc(NPv); dg_du = dalloc(NQ);
    alloc_block(dg_b); alloc_block(dg_x);
    if (general) {
      std::vector<int> ecl((size_t)2 * gm->ne, -1);
      for (int e = 0; e < gm->ne; e++)
        for (int sd = 0; sd < 2; sd++) {
          const int c = gm->ecell[2 * (size_t)e + sd];
          if (c >= 0) ecl[2 * (size_t)e + sd] = 3 * c + gm->elocal[2 * (size_t)e + sd];
        }
      dg_ecl = upload_ints(ecl);
    }
  }
  // lam = avg(p) in DGT_k (k_dg_avg_trace / k_g_dg_avg_trace)
  void avg_trace(const double* p, double* lam) {
    tally(LC_OTHER, bP() + bL());
    if (general) {
      if (!g_nref) { csr(gd.Rp, p, 1.0, 0.0, lam); return; }  // HDG_GENERAL_CSR_LIFT: the assembled form of the same map
      dg_alloc();
      by_degree([&](auto k) { k_g_dg_avg_trace<k()><<<(gm->ne + 63) / 64, 64, 0, stream>>>(ggeo, gm->ne, dg_ecl, g_nref, p, lam); });
      return;
    }
    halo_P(p);
    by_degree([&](auto k) { k_dg_avg_trace<k()><<<corner_grid(), bs(), 0, stream>>>(g, dt, p, lam); });
  }
  void dg_apply(const V2& x, const double* qstar, double dtt, V2& out) {
    adv_apply(x.u, qstar, wQ1, dtt);
    avg_trace(x.p, dg_lam);
    pgrad(wQ1, 1.0, nullptr, 0.0, x.p, dg_lam, -1.0, out.u);
    weak_div(x.u, 1.0, out.p, false);
  }
  void dg_precond(const V2& r, const double* qstar, double dtt, int psidx, V2& z) {
    zero(z.u, NQ);
    tent_krylov(TentSystem{qstar, dtt, 0, r.u}, z.u, cfg.unsplit_inner_rtol, 200, false);
    weak_div(z.u, 1.0, dg_rp, false);
    axpby(NPv, 1.0, r.p, -1.0, dg_rp);  // r_p - B u~
    use_pset(psidx);
    condense(nullptr, dg_rp, nullptr, wL1);
    zero(dg_lam2, NLv);
    trace_cg(wL1, dg_lam2, cfg.unsplit_inner_rtol, 200, false);
    backsub(nullptr, dg_rp, dg_lam2, dg_du, z.p);
    use_pset(0);
    axpby(NQ, 1.0, dg_du, 1.0, z.u);
  }
  // K_dg (u, y) = b; x holds the initial guess
  int dg_solve(const double* qstar, double dtt, const V2& b, V2& x) {
    dg_alloc();
    ensure_dinv(0, dtt);
    const int ps = get_pset(cfg.tau / dtt);
    const int m = cfg.dg_restart > 0 ? cfg.dg_restart : 30;
    return fgmres_blocks(
        [&](const V2& in, V2& out) { dg_apply(in, qstar, dtt, out); },
        [&](const V2& in, V2& out) { dg_precond(in, qstar, dtt, ps, out); }, b, x, dg_V, dg_Z, dg_r, dg_w, m,
        cfg.dg_rtol > 0.0 ? cfg.dg_rtol : 1e-10, cfg.dg_maxit > 0 ? cfg.dg_maxit : 2000, "DG FGMRES");
  }
  // one step of dg_implicit.py:116-134 (slot-0 forcing at the start of the step, as implicit_step)
  void dg_implicit_step(int* its) {
    dg_alloc();
    Timed tm_(*this, T_STEP);
    const double dtt = cfg.dt;
    if (tracer_on) {  // dg_implicit.py:117-120: b_tracer is built from the fields at the START of the step
      cg_project(curQ, uproj);
      tracer_tendency(q_cur, uproj, q_t);
      if (buoyancy_on()) buoyancy(q_cur, buoy[0]);  // slot 0: the tracer at the start of the step, next to f(t_k)
    }
    if (vel_linear_on()) vel_linear_apply(curQ, visc[0]);  // slot 0: Q_n, forward Euler, beside f(t_k)
    { Timed tb_(*this, T_BDM); bdm(curQ, Qstar[0]); }              // dg_implicit.py:122
    lincomb(NQ, start_terms(dtt), dg_b.u);  // (Q, w) + dt (f, w)   dg_implicit.py:73
    zero(dg_b.p, NPv);
    zero(dg_x.u, NQ); zero(dg_x.p, NPv);                             // fresh Function: zero guess
    int it;
    { Timed td_(*this, T_DG); it = dg_solve(Qstar[0], dtt, dg_b, dg_x); }  // dg_implicit.py:126
    copy(curQ, dg_x.u, NQ);                                          // dg_implicit.py:128-130
    axpby(NPv, 1.0 / dtt, dg_x.p, 0.0, curP);
    shift(curP, nullptr);
    it_sum[0] += it; it_cnt[0]++;
    if (its) *its = it;
    if (tracer_on) { axpby(NTv(), dtt, q_t, 1.0, q_cur); tracer_implicit_diffusion(); }  // dg_implicit.py:131-132, after a successful solve only
  }
  // operator-level access (hdg_apply_dg_operator): out = K x of dg_implicit.py:48-71 (unscaled rows, phi not y)
  void dg_operator(const double* qstar, const double* u, const double* p, double dtt, double* out_u, double* out_p) {
    dg_alloc();
    adv_apply(u, qstar, wQ4, dtt);
    avg_trace(p, dg_lam);
    pgrad(wQ4, 1.0, nullptr, 0.0, p, dg_lam, -dtt, out_u);
    weak_div(u, dtt, out_p, false);
  }


  // ================================================================== continuous space CG_{k+1}, tracer, vorticity
  // (hdg_cg.hpp; reference: common.py:110-129, hdg_imex.py:415-448,560,622-623,638-639, hdg_implicit.py:93-96,192-193,
  //  callbacks.py:43-69).  Built on first use; single rank only.
  CgTabs cgt;
  bool cg_ready = false;
  const double *cg_Mloc = nullptr, *cg_Wx[2] = {nullptr, nullptr}, *cg_Wy[2] = {nullptr, nullptr}, *cg_Eb = nullptr;
  double *cg_y = nullptr, *cg_b = nullptr, *cg_x = nullptr, *cg_rr = nullptr, *cg_zz = nullptr, *cg_pp = nullptr, *cg_Ap2 = nullptr,
         *cg_dinv = nullptr, *uproj = nullptr;
  int cg_its_last = 0;
  GeneralCG* gcg = nullptr;
  struct { DevCsr M, Bp[2], Ep[2], Vort, R; } gcgd;
  void cg_setup() {
    if (cg_ready) return;
    if (general) {  // host-assembled operators of the continuous space (hdg_general.hpp: assemble_cg)
      gcg = new GeneralCG();
      assemble_cg(*gtab, *gm, gops, *gcg);
      std::memset(&cgt, 0, sizeof(cgt));
      cgt.p = K + 1; cgt.ncg = gcg->ncg;
      gcgd.M = upload_csr(gcg->M); gcgd.Vort = upload_csr(gcg->Vort); gcgd.R = upload_csr(gcg->R);
      for (int d = 0; d < 2; d++) { gcgd.Bp[d] = upload_csr(gcg->Bp[d]); gcgd.Ep[d] = upload_csr(gcg->Ep[d]); }
      for (double** v : {&cg_b, &cg_x, &cg_rr, &cg_zz, &cg_pp, &cg_Ap2}) *v = dalloc(cgt.ncg);
      cg_dinv = const_cast<double*>(upload(gcg->diag));  // the diagonal itself (k_pointwise_div divides by it)
      uproj = dalloc(NQ);
      cg_ready = true;
      return;
    }
    if (comm->size > 1) throw std::string("the continuous space (tracer, vorticity) is implemented for a single rank");
    const int p = K + 1;
    std::vector<real> xi, eta;
    triangleNodes(p, cfg.equispaced_nodes, xi, eta);
    if ((int)xi.size() != NU) throw std::string("node count mismatch");
    std::memset(&cgt, 0, sizeof(cgt));
    cgt.p = p; cgt.nint = (p - 1) * (p - 2) / 2; cgt.nx = g.nx; cgt.ny = g.ny;
    cgt.per = periodic ? 1 : 0;
    cgt.vs = periodic ? g.nx : g.nx + 1;
    const long nrows = periodic ? g.ny : g.ny + 1;  // corner rows that carry vertices / horizontal edges
    const long nvt = (long)cgt.vs * nrows;
    cgt.baseH = nvt;
    cgt.baseV = cgt.baseH + (long)g.nx * nrows * (p - 1);
    cgt.baseD = cgt.baseV + (long)cgt.vs * g.ny * (p - 1);
    cgt.baseI = cgt.baseD + (long)g.nx * g.ny * (p - 1);
    cgt.ncg = cgt.baseI + 2L * g.nx * g.ny * cgt.nint;
    // forward table from the lattice index (a, b) of each node (order: for b: for a), checked against coordinates below
    int nv = 0, ne_cnt[3][4] = {{0}}, ni[2] = {0, 0};
    for (int sh = 0; sh < 2; sh++) {
      int n = 0;
      for (int b = 0; b <= p; b++)
        for (int a = 0; a <= p - b; a++, n++) {
          const int c = p - a - b;
          short* f = cgt.fwd[sh][n];
          auto set = [&](int ty, int di, int dj, int t) { f[0] = (short)ty; f[1] = (short)di; f[2] = (short)dj; f[3] = (short)t; };
          if (a == 0 && b == 0) sh == 0 ? set(0, 0, 0, 0) : set(0, 1, 1, 0);
          else if (a == p) sh == 0 ? set(0, 1, 0, 0) : set(0, 0, 1, 0);
          else if (b == p) sh == 0 ? set(0, 0, 1, 0) : set(0, 1, 0, 0);
          else if (b == 0) sh == 0 ? set(1, 0, 0, a - 1) : set(1, 0, 1, p - a - 1);
          else if (a == 0) sh == 0 ? set(2, 0, 0, b - 1) : set(2, 1, 0, p - b - 1);
          else if (c == 0) sh == 0 ? set(3, 0, 0, b - 1) : set(3, 0, 0, a - 1);
          else { set(4, 0, 0, ni[sh]); cgt.intr[sh][ni[sh]++] = (short)n; }
          // inverse tables: the entity at corner (i + di, j + dj) receives cell (sh, i, j) node n
          if (f[0] == 0) { short* v = cgt.vtx[nv++]; v[0] = (short)sh; v[1] = (short)-f[1]; v[2] = (short)-f[2]; v[3] = (short)n; }
          else if (f[0] <= 3) {
            int& k2 = ne_cnt[f[0] - 1][f[3]];
            short* v = cgt.edg[f[0] - 1][f[3]][k2++];
            v[0] = (short)sh; v[1] = (short)-f[1]; v[2] = (short)-f[2]; v[3] = (short)n;
          }
        }
    }
    if (nv != 6 || ni[0] != cgt.nint || ni[1] != cgt.nint) throw std::string("continuous-space tables inconsistent");
    // cross-check: physical position of every local node of cell (sh, 0, 0) on the unit-h square against its entity
    {
      std::vector<real> gl = gllPoints(p);
      if (cfg.equispaced_nodes) { gl.clear(); for (int q = 0; q <= p; q++) gl.push_back((real)q / p); }
      for (int sh = 0; sh < 2; sh++)
        for (int n = 0; n < NU; n++) {
          const short* f = cgt.fwd[sh][n];
          const double x = sh == 0 ? (double)xi[n] : 1.0 - (double)xi[n], y = sh == 0 ? (double)eta[n] : 1.0 - (double)eta[n];
          double ex, ey;
          const double t = f[0] >= 1 && f[0] <= 3 ? (double)gl[f[3] + 1] : 0.0;
          if (f[0] == 0) { ex = f[1]; ey = f[2]; }
          else if (f[0] == 1) { ex = f[1] + t; ey = f[2]; }
          else if (f[0] == 2) { ex = f[1]; ey = f[2] + t; }
          else if (f[0] == 3) { ex = f[1] + 1.0 - t; ey = f[2] + t; }
          else continue;
          if (std::fabs(x - ex) > 1e-12 || std::fabs(y - ey) > 1e-12) throw std::string("continuous-space node classification failed");
        }
    }
    // local matrices: nodal mass Vinv^T Vinv; curl blocks W[m][l] = int d psi_m psi_l; boundary edge mass
    dvec Ml((size_t)NU * NU, 0.0);
    for (int a = 0; a < NU; a++)
      for (int b = 0; b < NU; b++) {
        long double acc = 0;
        for (int m = 0; m < NU; m++) acc += (long double)tab->Vuinv[m * NU + a] * tab->Vuinv[m * NU + b];
        Ml[(size_t)a * NU + b] = (double)acc;
      }
    cg_Mloc = upload(Ml);
    dvec Eb((size_t)2 * 3 * NU * NU, 0.0);
    for (int sh = 0; sh < 2; sh++) {
      dvec Wx((size_t)NU * NU, 0.0), Wy((size_t)NU * NU, 0.0);
      for (int q = 0; q < tab->nqc; q++)
        for (int m = 0; m < NU; m++)
          for (int l = 0; l < NU; l++) {
            Wx[(size_t)m * NU + l] += tab->cw[q] * tab->cGx[sh][q * NU + m] * tab->cPhi[sh][q * NU + l];
            Wy[(size_t)m * NU + l] += tab->cw[q] * tab->cGy[sh][q * NU + m] * tab->cPhi[sh][q * NU + l];
          }
      cg_Wx[sh] = upload(Wx); cg_Wy[sh] = upload(Wy);
      for (int e = 0; e < 3; e++)
        for (int q = 0; q < tab->nqe; q++)
          for (int m = 0; m < NU; m++)
            for (int l = 0; l < NU; l++)
              Eb[(((size_t)sh * 3 + e) * NU + m) * NU + l] += tab->ew[e][q] * tab->ePhi[sh][e][q * NU + m] * tab->ePhi[sh][e][q * NU + l];
    }
    cg_Eb = upload(Eb);
    cg_y = dalloc((long)NU * g.Nc);
    for (double** v : {&cg_b, &cg_x, &cg_rr, &cg_zz, &cg_pp, &cg_Ap2, &cg_dinv}) *v = dalloc(cgt.ncg);
    uproj = dalloc(NQ);
    cg_ready = true;
    // Jacobi preconditioner: diagonal of the mass matrix = M applied dof by dof is too dear; use the row sums of |M| instead?
    // The diagonal itself: gather of diag(Mloc): y_K[n] = Mloc[n][n]
    {
      dvec dg((size_t)NU * g.Nc, 0.0);
      for (int n = 0; n < NU; n++)
        for (long cc = 0; cc < g.Nc; cc++) dg[(size_t)n * g.Nc + cc] = Ml[(size_t)n * NU + n];
      HIPCHECK(hipMemcpyAsync(cg_y, dg.data(), sizeof(double) * dg.size(), hipMemcpyHostToDevice, stream));
      by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, cg_dinv); });
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
  void cg_mass(const double* c_in, double* out) {  // out = M_CG c_in
    if (general) { csr(gcgd.M, c_in, 1.0, 0.0, out); return; }
    by_degree([&](auto k) { k_cg_cell<k(), 0><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, nullptr, nullptr, nullptr, nullptr,
                                                                     nullptr, c_in, nullptr, 0, cg_y); });
    by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, out); });
  }
  double dot_plain(long n, const double* a, const double* b) {
    VecList<4> vl{};
    vl.p[0] = b;
    const int nb = std::min(dot_blocks, vec_blocks(n));
    k_multidot<4, false><<<nb, HDG_DOT_BLOCK, 0, stream>>>(n, a, vl, 1, d_part, RowMask{0, 1, 0, 0}, 0);
    k_reduce_parts<<<1, 256, 0, stream>>>(nb, 1, d_part, d_res);
    HIPCHECK(hipMemcpyAsync(h_res, d_res, sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return h_res[0];
  }
  // solve M_CG x = b (b in cg_b) by Jacobi-preconditioned CG to rtol 1e-13 on the preconditioned residual; result in cg_x
  void cg_solve() {
    const long n = cgt.ncg;
    zero(cg_x, n);
    copy(cg_rr, cg_b, n);
    auto precond = [&]() {  // z = r / diag
      k_pointwise_div<<<vec_blocks(n), 256, 0, stream>>>(n, cg_rr, cg_dinv, cg_zz);
    };
    precond();
    double rz = dot_plain(n, cg_rr, cg_zz);
    const double rz0 = rz;
    if (!(rz0 > 0.0)) { cg_its_last = 0; return; }
    copy(cg_pp, cg_zz, n);
    for (int it = 1; it <= 500; it++) {
      cg_mass(cg_pp, cg_Ap2);
      const double alpha = rz / dot_plain(n, cg_pp, cg_Ap2);
      axpby(n, alpha, cg_pp, 1.0, cg_x);
      axpby(n, -alpha, cg_Ap2, 1.0, cg_rr);
      precond();
      const double rzn = dot_plain(n, cg_rr, cg_zz);
      cg_its_last = it;
      if (rzn <= 1e-26 * rz0) return;
      axpby(n, 1.0, cg_zz, rzn / rz, cg_pp);
      rz = rzn;
    }
    throw NotConverged{"continuous-space mass solve did not converge"};
  }
  // The same solve for TWO right-hand sides at once (structured meshes: the two components of cg_project), scalars on the device,
  // no host synchronisation inside an iteration (hdg_cg.hpp: k_cgm_*): r0 / r1 hold the right-hand sides on entry and the
  // residuals afterwards, the solutions come out in x0 / x1.  Convergence as in cg_solve (1e-13 on the preconditioned residual
  // of EACH component), read by the host one iteration late.  HDG_CG_MASS_ONE_BY_ONE: the one-vector loop.
  double *cg_b2 = nullptr, *cg_x2 = nullptr, *cg_pp2 = nullptr, *cg_Ap3 = nullptr, *d_cgm = nullptr, *h_cgm = nullptr;
  hipEvent_t cgm_ev[2] = {nullptr, nullptr};
  void cg_solve2(double* r0, double* r1, double* x0, double* x1) {
    const long n = cgt.ncg;
    if (!d_cgm) {
      d_cgm = dalloc(24);
      HIPCHECK(hipHostMalloc((void**)&h_cgm, sizeof(double) * 8));
      for (int q = 0; q < 2; q++) HIPCHECK(hipEventCreateWithFlags(&cgm_ev[q], hipEventDisableTiming));
    }
    const int nb = std::min(std::min(dot_blocks, vec_blocks(n)), 1024);
    const double tol2 = 1e-26;
    zero(x0, n); zero(x1, n);
    k_cgm_update2<<<nb, HDG_CGM_BLOCK, 0, stream>>>(n, 1, d_cgm, cg_dinv, cg_pp, cg_Ap2, x0, r0, cg_pp2, cg_Ap3, x1, r1, d_part);
    k_cgm_scalars<<<1, HDG_CGM_BLOCK, 0, stream>>>(nb, 2, tol2, d_part, d_cgm, h_cgm);
    HIPCHECK(hipStreamSynchronize(stream));
    cg_its_last = 0;
    if (h_cgm[0] == 1.0) return;  // both right-hand sides vanish
    k_cgm_dir2<<<vec_blocks(n), 256, 0, stream>>>(n, d_cgm, cg_dinv, r0, cg_pp, r1, cg_pp2);
    for (int it = 1; it <= 500; it++) {
      cg_mass(cg_pp, cg_Ap2);
      cg_mass(cg_pp2, cg_Ap3);
      k_cgm_pap2<<<nb, HDG_CGM_BLOCK, 0, stream>>>(n, cg_pp, cg_Ap2, cg_pp2, cg_Ap3, d_part);
      k_cgm_scalars<<<1, HDG_CGM_BLOCK, 0, stream>>>(nb, 0, tol2, d_part, d_cgm, nullptr);
      k_cgm_update2<<<nb, HDG_CGM_BLOCK, 0, stream>>>(n, 0, d_cgm, cg_dinv, cg_pp, cg_Ap2, x0, r0, cg_pp2, cg_Ap3, x1, r1, d_part);
      k_cgm_scalars<<<1, HDG_CGM_BLOCK, 0, stream>>>(nb, 1, tol2, d_part, d_cgm, h_cgm + 4 * (it & 1));
      HIPCHECK(hipEventRecord(cgm_ev[it & 1], stream));
      k_cgm_dir2<<<vec_blocks(n), 256, 0, stream>>>(n, d_cgm, cg_dinv, r0, cg_pp, r1, cg_pp2);
      if (it >= 2) {  // the flag of the previous iteration has long arrived; x has taken one more (harmless) step by now
        HIPCHECK(hipEventSynchronize(cgm_ev[(it - 1) & 1]));
        const double* f = h_cgm + 4 * ((it - 1) & 1);
        if (!(f[1] == f[1]) || !(f[2] == f[2])) throw NotConverged{"continuous-space mass solve: NaN residual"};
        if (f[0] == 1.0) { cg_its_last = it - 1; return; }
      }
    }
    throw NotConverged{"continuous-space mass solve did not converge"};
  }
  // L2 projection of a broken velocity onto [CG_{k+1}]^2 (common.py:119-122); result as a broken modal vector
  void cg_project(const double* vel_in, double* vel_out) {
    cg_setup();
    if (general) {
      for (int d = 0; d < 2; d++) {
        csr(gcgd.Bp[d], vel_in, 1.0, 0.0, cg_b);
        cg_solve();
        csr(gcgd.Ep[d], cg_x, 1.0, d == 0 ? 0.0 : 1.0, vel_out);  // component 0 clears the rows of component 1, which then adds
      }
      return;
    }
    if (!opt.cg_mass_one_by_one) {  // both components in one solve
      if (!cg_b2) for (double** v : {&cg_b2, &cg_x2, &cg_pp2, &cg_Ap3}) *v = dalloc(cgt.ncg);
      for (int d = 0; d < 2; d++) {
        by_degree([&](auto k) { k_cg_cell<k(), 1><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, nullptr, nullptr, nullptr, nullptr,
                                                                         nullptr, nullptr, const_cast<double*>(vel_in), d, cg_y); });
        by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, d == 0 ? cg_b : cg_b2); });
      }
      cg_solve2(cg_b, cg_b2, cg_x, cg_x2);
      for (int d = 0; d < 2; d++)
        by_degree([&](auto k) { k_cg_cell<k(), 2><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, nullptr, nullptr, nullptr, nullptr,
                                                                         nullptr, d == 0 ? cg_x : cg_x2, vel_out, d, nullptr); });
      return;
    }
    for (int d = 0; d < 2; d++) {
      by_degree([&](auto k) { k_cg_cell<k(), 1><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, nullptr, nullptr, nullptr, nullptr,
                                                                       nullptr, nullptr, const_cast<double*>(vel_in), d, cg_y); });
      by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, cg_b); });
      cg_solve();
      by_degree([&](auto k) { k_cg_cell<k(), 2><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, nullptr, nullptr, nullptr, nullptr,
                                                                       nullptr, cg_x, vel_out, d, nullptr); });
    }
  }
  // vorticity of a broken velocity in CG_{k+1} (callbacks.py:43-69); result in cg_x (ncg values)
  void vorticity(const double* vel_in) {
    cg_setup();
    if (general) { csr(gcgd.Vort, vel_in, 1.0, 0.0, cg_b); cg_solve(); return; }
    by_degree([&](auto k) { k_cg_cell<k(), 3><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, cg_Wx[0], cg_Wy[0], cg_Wx[1], cg_Wy[1],
                                                                     cg_Eb, nullptr, const_cast<double*>(vel_in), 0, cg_y); });
    by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, cg_b); });
    cg_solve();
  }
  // ================================================================== stream function (hdg_streamfunction.hpp)
  // psi in CG_{k+1} with (grad psi, grad tau) = int (u_x d_y tau - u_y d_x tau) dx: conjugate gradients on the stiffness matrix,
  // preconditioned by the diagonal plus one V-cycle of the P1 vertex grid.  Structured meshes on one rank.  Built on first use; the
  // vectors are the scratch vectors of the mass solves (cg_rr, cg_zz, cg_pp, cg_Ap2; result in cg_x), the vertex grid is vplan's.
  PsiTabs psit;
  bool psi_ready = false;
  const double *psi_Kloc = nullptr, *psi_Iphi = nullptr, *psi_Dxy = nullptr;
  double *psi_dg = nullptr, *psi_part = nullptr, *psi_sc = nullptr, *psi_h = nullptr;
  hipEvent_t psi_ev[2] = {nullptr, nullptr};
  int psi_nb = 0;
  // the launch tallies as they were: the V-cycle and the fills count themselves, and a diagnostic between two steps must not
  // show in the census of the step path
  struct TallyGuard {
    Engine& e;
    long calls[HDG_N_LAUNCH_CLASSES];
    double bytes[HDG_N_LAUNCH_CLASSES];
    explicit TallyGuard(Engine& e_) : e(e_) { std::memcpy(calls, e.lc_calls, sizeof(calls)); std::memcpy(bytes, e.lc_bytes, sizeof(bytes)); }
    ~TallyGuard() { std::memcpy(e.lc_calls, calls, sizeof(calls)); std::memcpy(e.lc_bytes, bytes, sizeof(bytes)); }
  };
  void psi_setup() {
    cg_setup();
    if (psi_ready) return;
    if (general || comm->size > 1) throw std::string("the stream function is implemented for structured meshes on a single rank");
    const int p = K + 1;
    std::vector<real> xi, eta;
    triangleNodes(p, cfg.equispaced_nodes, xi, eta);
    std::vector<real> gl = cfg.equispaced_nodes ? std::vector<real>() : gllPoints(p);
    if (cfg.equispaced_nodes) for (int q = 0; q <= p; q++) gl.push_back((real)q / p);
    std::memset(&psit, 0, sizeof(psit));
    for (int t = 0; t < p - 1; t++) psit.et[t] = (double)gl[t + 1];
    for (int sh = 0; sh < 2; sh++)
      for (int q = 0; q < cgt.nint; q++) {
        const int n = cgt.intr[sh][q];
        psit.plam[sh][q][0] = (double)((real)1 - xi[n] - eta[n]);
        psit.plam[sh][q][1] = (double)xi[n];
        psit.plam[sh][q][2] = (double)eta[n];
      }
    for (int e = 0; e < 6; e++) {  // the vertex an entry of CgTabs::vtx stands for is local node vtx[e][3] of its cell
      const short* f = cgt.vtx[e];
      const int slot = xi[f[3]] > 0.5 ? 1 : eta[f[3]] > 0.5 ? 2 : 0;
      for (int q = 0; q < cgt.nint; q++) psit.vlam[e][q] = psit.plam[f[0]][q][slot];
    }
    // element stiffness matrices in the nodal basis (phi_a = sum_m Vinv[m][a] psi_m) and the integrals of the modal basis
    dvec Kl((size_t)2 * NU * NU, 0.0), Ip((size_t)2 * NU, 0.0), Dn((size_t)4 * NU * NU, 0.0);
    for (int sh = 0; sh < 2; sh++) {
      std::vector<real> gx((size_t)tab->nqc * NU, 0), gy((size_t)tab->nqc * NU, 0);
      for (int q = 0; q < tab->nqc; q++)
        for (int a = 0; a < NU; a++)
          for (int m = 0; m < NU; m++) {
            gx[(size_t)q * NU + a] += (real)tab->Vuinv[m * NU + a] * tab->cGx[sh][q * NU + m];
            gy[(size_t)q * NU + a] += (real)tab->Vuinv[m * NU + a] * tab->cGy[sh][q * NU + m];
          }
      for (int a = 0; a < NU; a++)
        for (int b = 0; b < NU; b++) {
          real acc = 0;
          for (int q = 0; q < tab->nqc; q++)
            acc += (real)tab->cw[q] * (gx[(size_t)q * NU + a] * gx[(size_t)q * NU + b] + gy[(size_t)q * NU + a] * gy[(size_t)q * NU + b]);
          Kl[((size_t)sh * NU + a) * NU + b] = (double)acc;
        }
      for (int l = 0; l < NU; l++) {
        real acc = 0;
        for (int q = 0; q < tab->nqc; q++) acc += (real)tab->cw[q] * tab->cPhi[sh][q * NU + l];
        Ip[(size_t)sh * NU + l] = (double)acc;
        for (int n = 0; n < NU; n++) {  // mode l of d_x phi_n, d_y phi_n (the basis is orthonormal)
          real ax = 0, ay = 0;
          for (int q = 0; q < tab->nqc; q++) {
            ax += (real)tab->cw[q] * gx[(size_t)q * NU + n] * tab->cPhi[sh][q * NU + l];
            ay += (real)tab->cw[q] * gy[(size_t)q * NU + n] * tab->cPhi[sh][q * NU + l];
          }
          Dn[((size_t)(2 * sh) * NU + l) * NU + n] = (double)ax;
          Dn[((size_t)(2 * sh + 1) * NU + l) * NU + n] = (double)ay;
        }
      }
    }
    psi_Kloc = upload(Kl);
    psi_Iphi = upload(Ip);
    psi_Dxy = upload(Dn);
    psi_dg = dalloc(cgt.ncg);
    psi_nb = std::min(std::min(dot_blocks, vec_blocks(cgt.ncg)), 1024);
    psi_part = dalloc(std::max<long>(4L * cell_grid().x, 2L * psi_nb));
    psi_sc = dalloc(32);
    HIPCHECK(hipHostMalloc((void**)&psi_h, sizeof(double) * 8));
    for (int q = 0; q < 2; q++) HIPCHECK(hipEventCreateWithFlags(&psi_ev[q], hipEventDisableTiming));
    {  // diag(K): the gather of the diagonals of the element matrices
      dvec dgv((size_t)NU * g.Nc, 0.0);
      const long plane = (long)g.R * g.nx;  // cells of one shape (rowbase)
      for (int n = 0; n < NU; n++)
        for (long cc = 0; cc < g.Nc; cc++) dgv[(size_t)n * g.Nc + cc] = Kl[((size_t)(cc / plane) * NU + n) * NU + n];
      HIPCHECK(hipMemcpyAsync(cg_y, dgv.data(), sizeof(double) * dgv.size(), hipMemcpyHostToDevice, stream));
      by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, psi_dg); });
      HIPCHECK(hipStreamSynchronize(stream));
    }
    if (vplan.lev.empty()) {  // a configuration whose trace preconditioner has no vertex grid: the same plan, built here
      vplan = vertex_plan(g.nx, periodic, opt);
      for (const VLevel& v : vplan.lev) { mg_x.push_back(dalloc(v.nv)); mg_b.push_back(dalloc(v.nv)); mg_r.push_back(dalloc(v.nv)); }
      build_dense_tail();
    }
    psi_ready = true;
  }
  long psi_vertices() const { return vplan.lev[0].nv; }
  void psi_stiff(const double* x, double* y) {  // y = K x
    by_degree([&](auto k) { k_psi_stiff<k()><<<cell_grid(), bs(), 0, stream>>>(g, cgt, psi_Kloc, x, cg_y); });
    by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, y); });
  }
  void psi_restrict(const double* r, double* rc) {  // rc = P^T r on the vertex grid
    by_degree([&](auto k) { k_psi_restrict<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, psit, r, rc); });
  }
  void psi_prolong(const double* xc, const double* r, double* out) {  // out = r / diag(K) + P xc (either part may be absent)
    by_degree([&](auto k) { k_psi_prolong<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, psit, xc, r, psi_dg, out); });
  }
  // z = B r.  Default: r / diag(K) + P V(P^T r), V one cycle of the vertex grid; jacobi: the first term alone
  void psi_precond(bool jacobi, const double* r, double* z) {
    if (jacobi) { psi_prolong(nullptr, r, z); return; }
    psi_restrict(r, mg_b[0]);
    vcycle(vplan, 0, nullptr);
    psi_prolong(mg_x[0], r, z);
  }
  void psi_dot(const double* a, const double* b, int mode, double tol2, double* hflag) {
    k_psi_dot<<<psi_nb, HDG_PSI_BLOCK, 0, stream>>>(cgt.ncg, a, b, psi_part);
    k_psi_scalars<<<1, HDG_PSI_BLOCK, 0, stream>>>(psi_nb, mode, tol2, psi_part, psi_sc, hflag);
  }
  // the stream function of a broken velocity (modal, device); gauged result in cg_x, info as in include/hdg_streamfunction.h
  void streamfunction(const double* vel_in, double rtol, double* info) {
    psi_setup();
    const long n = cgt.ncg;
    const bool jacobi = opt.psi_jacobi;
    const double tol2 = rtol * rtol;
    const int nvb = vec_blocks(n);
    by_degree([&](auto k) { k_cg_cell<k(), 4><<<cell_grid(), bs(), 0, stream>>>(g, cgt, dt, cg_Mloc, dt.Vuinv, cg_Wx[0], cg_Wy[0], cg_Wx[1], cg_Wy[1],
                                                                     cg_Eb, nullptr, const_cast<double*>(vel_in), 0, cg_y); });
    by_degree([&](auto k) { k_cg_gather<k()><<<corner_grid_all(), bs(), 0, stream>>>(g_all, cgt, cg_y, cg_rr); });
    // the right-hand side sums to zero up to rounding; what is left would be an inconsistent part no iteration removes
    k_psi_dot<<<psi_nb, HDG_PSI_BLOCK, 0, stream>>>(n, cg_rr, nullptr, psi_part);
    k_psi_finish<1><<<1, HDG_PSI_BLOCK, 0, stream>>>(psi_nb, psi_part, psi_sc + 8);
    k_psi_shift_mean<<<nvb, 256, 0, stream>>>(n, psi_sc + 8, cg_rr);
    HIPCHECK(hipMemsetAsync(cg_x, 0, sizeof(double) * n, stream));
    psi_precond(jacobi, cg_rr, cg_zz);
    psi_dot(cg_rr, cg_zz, 2, tol2, psi_h);
    HIPCHECK(hipStreamSynchronize(stream));
    int its = 0;
    double rel2 = 0.0;
    if (!(psi_h[1] == psi_h[1])) throw NotConverged{"stream function: the right-hand side is not finite"};
    if (psi_h[0] != 1.0) {
      bool done = false;
      k_psi_dir<<<nvb, 256, 0, stream>>>(n, psi_sc, cg_zz, cg_pp);
      for (int it = 1; it <= 2001 && !done; it++) {
        psi_stiff(cg_pp, cg_Ap2);
        psi_dot(cg_pp, cg_Ap2, 0, tol2, nullptr);
        k_psi_update<<<nvb, 256, 0, stream>>>(n, psi_sc, cg_pp, cg_Ap2, cg_x, cg_rr);
        psi_precond(jacobi, cg_rr, cg_zz);
        psi_dot(cg_rr, cg_zz, 1, tol2, psi_h + 4 * (it & 1));
        HIPCHECK(hipEventRecord(psi_ev[it & 1], stream));
        k_psi_dir<<<nvb, 256, 0, stream>>>(n, psi_sc, cg_zz, cg_pp);
        if (it >= 2) {  // the flag of the previous iteration has arrived by now; x has taken one more (harmless) step
          HIPCHECK(hipEventSynchronize(psi_ev[(it - 1) & 1]));
          const double* f = psi_h + 4 * ((it - 1) & 1);
          if (!(f[1] == f[1])) throw NotConverged{"stream function: NaN residual"};
          if (f[0] == 1.0) { its = it - 1; rel2 = f[2] > 0.0 ? f[1] / f[2] : 0.0; done = true; }
        }
      }
      if (!done) throw NotConverged{"stream function: the conjugate gradient iteration did not converge in 2000 iterations"};
    }
    // gauge (mean over the boundary vertices | over all vertices of the periodic square), extrema, defect and mean flow
    k_psi_gauge_mean<<<1, HDG_PSI_BLOCK, 0, stream>>>(g.nx, periodic ? 0 : 1, cg_x, psi_sc + 8);
    k_psi_shift<<<psi_nb, HDG_PSI_BLOCK, 0, stream>>>(n, psi_sc + 8, cg_x, psi_part);
    k_psi_minmax<<<1, HDG_PSI_BLOCK, 0, stream>>>(psi_nb, psi_part, psi_sc + 10);
    const int ncb = (int)cell_grid().x;
    for (int d = 0; d < 2; d++)  // curl psi as a broken velocity in the scratch vector of the test hooks
      by_degree([&](auto k) { k_psi_curl<k()><<<cell_grid(), bs(), 0, stream>>>(g, cgt, psi_Dxy, cg_x, d, wQ2); });
    auto defect = [&](const double* ub, double* res) {
      by_degree([&](auto k) { k_psi_defect<k()><<<cell_grid(), bs(), 0, stream>>>(g, psi_Iphi, wQ2, vel_in, ub, psi_part); });
      k_psi_finish<4><<<1, HDG_PSI_BLOCK, 0, stream>>>(ncb, psi_part, res);
    };
    defect(nullptr, psi_sc + 12);
    if (periodic) {
      k_psi_mean_flow<<<1, 64, 0, stream>>>(psi_sc + 12, (double)g.h * g.nx * (double)g.h * g.ny, psi_sc + 16);
      defect(psi_sc + 16, psi_sc + 12);
    }
    double hs[24];
    HIPCHECK(hipMemcpyAsync(hs, psi_sc, sizeof(hs), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    info[0] = its; info[1] = std::sqrt(rel2); info[2] = std::sqrt(std::max(hs[15], 0.0)); info[3] = std::sqrt(hs[14]);
    info[4] = periodic ? hs[16] : 0.0; info[5] = periodic ? hs[17] : 0.0; info[6] = hs[10]; info[7] = hs[11];
  }
  void cg_coordinates(double* xy) const {  // physical position of every continuous dof
    if (general) { std::memcpy(xy, gcg->xy.data(), sizeof(double) * gcg->xy.size()); return; }
    const int p = cgt.p;
    std::vector<real> gl = cfg.equispaced_nodes ? std::vector<real>() : gllPoints(p);
    if (cfg.equispaced_nodes) for (int q = 0; q <= p; q++) gl.push_back((real)q / p);
    std::vector<real> xi, eta;
    triangleNodes(p, cfg.equispaced_nodes, xi, eta);
    const double h = g.h;
    auto put = [&](long id, double x, double y) { xy[2 * id] = x; xy[2 * id + 1] = y; };
    const int jmax = periodic ? g.ny - 1 : g.ny, imax = periodic ? g.nx - 1 : g.nx;  // periodic: nx x ny corners
    for (int j = 0; j <= jmax; j++)
      for (int i = 0; i <= imax; i++) {
        put((long)j * cgt.vs + i, i * h, j * h);
        for (int t = 0; t < p - 1; t++) {
          const double tt = (double)gl[t + 1];
          if (i < g.nx) put(cgt.baseH + ((long)j * g.nx + i) * (p - 1) + t, (i + tt) * h, j * h);
          if (j < g.ny) put(cgt.baseV + ((long)j * cgt.vs + i) * (p - 1) + t, i * h, (j + tt) * h);
          if (i < g.nx && j < g.ny) put(cgt.baseD + ((long)j * g.nx + i) * (p - 1) + t, (i + 1 - tt) * h, (j + tt) * h);
        }
        if (i < g.nx && j < g.ny)
          for (int sh = 0; sh < 2; sh++)
            for (int q = 0; q < cgt.nint; q++) {
              const int n = cgt.intr[sh][q];
              const double x = sh == 0 ? (double)xi[n] : 1.0 - (double)xi[n], y = sh == 0 ? (double)eta[n] : 1.0 - (double)eta[n];
              put(cgt.baseI + (((long)j * g.nx + i) * 2 + sh) * cgt.nint + q, (i + x) * h, (j + y) * h);
            }
      }
  }

  // ------------------------------------------------------------------ passive tracers (explicit DG transport)
  // n_tr tracers (hdg_config::n_tracers, 0 means 1) ride one flow: every tracer vector holds them tracer-major and contiguous,
  // [t][NPv], so the copies and updates below are the single-tracer calls over n_tr * NPv entries, the projection of the
  // stage velocity runs once per stage and one launch of the transport kernel covers all tracers.
  bool tracer_on = false;
  int n_tr = 1;
  // hdg_config::n_tracers: 0 means 1; anything outside 0 .. HDG_MAX_TRACERS is refused (the three constructors call this
  // before they touch the device or the transport)
  static int checked_n_tracers(const hdg_config& c) {
    if (c.n_tracers < 0 || c.n_tracers > HDG_MAX_TRACERS)
      throw std::string("n_tracers must be in 0 .. " + std::to_string(HDG_MAX_TRACERS) + " (got " + std::to_string(c.n_tracers) + ")");
    return c.n_tracers == 0 ? 1 : c.n_tracers;
  }
  long NTv() const { return (long)n_tr * NPv; }
  double *q_cur = nullptr, *q_fin = nullptr, *q_t = nullptr;
  std::vector<double*> q_st;
  void tracer_alloc() {
    if (q_cur) return;
    q_cur = dalloc(NTv()); q_fin = dalloc(NTv()); q_t = dalloc(NTv());
    for (int i = 0; i < s; i++) q_st.push_back(dalloc(NTv()));
  }
  // tracers per thread of the transport kernels: the largest power of two within the degree's register budget
  // (TracerBlock<K>) and within n, so one tracer runs the TB = 1 instantiation and a short block only follows a full one
  template <int TBMAX, class F> static void by_tracer_block(int n, F&& f) {
    const int tb = std::min(TBMAX, n >= 4 ? 4 : (n >= 2 ? 2 : 1));
    if constexpr (TBMAX >= 4) { if (tb == 4) { f(std::integral_constant<int, 4>()); return; } }
    if constexpr (TBMAX >= 2) { if (tb == 2) { f(std::integral_constant<int, 2>()); return; } }
    f(std::integral_constant<int, 1>());
  }
  // out = M^-1 T(.; q, u) for a continuous velocity u given as a broken modal vector; q, out: n tracers, tracer-major
  void tracer_adv(const double* q, const double* u, double* out, int n) {
    if (n < 1 || n > HDG_MAX_TRACERS) throw std::string("tracer count out of range");
    if (!general) halo_rows(const_cast<double*>(q), (long)g.R * g.nx, g.nx, NP * 2 * n, 1);  // halo_P of every tracer: contiguous planes
    by_degree([&](auto k) {
      constexpr int KK = decltype(k)::value;
      by_tracer_block<TracerBlock<KK>::TB>(n, [&](auto tb) {
        constexpr int TB = decltype(tb)::value;
        const unsigned nblk = (unsigned)((n + TB - 1) / TB);
        if (general) { k_g_tracer<KK, TB><<<dim3((gm->nc + 63) / 64, nblk), 64, 0, stream>>>(ggeo, n, NPv, q, u, out); return; }
        dim3 grid = cell_grid();
        grid.y = nblk;
        k_tracer_adv<KK, TB><<<grid, bs(), 0, stream>>>(g, dt, n, NPv, q, u, out);
      });
    });
  }
  // ---- tracer diffusion: every tracer tendency gains kappa_t M^-1 D q_t, the symmetric interior-penalty
  // form with no-flux walls.  Structured meshes: seven NP x NP blocks per element shape, built once on the host
  // (hdg_tables.hpp: TracerDiffusionTables) and applied by k_tracer_diff right after k_tracer_adv on the same q; general
  // meshes: M^-1 D assembled once (hdg_general.hpp: assemble_tracer_diffusion) and applied per tracer by the CSR kernel.
  // Both are built on the first use.  kappa is configuration like dt: it stays when the tracers are switched off and on.
  std::vector<double> tr_kappa;  // n_tr values while the feature is on (some kappa_t != 0), empty while it is off
  double* d_kappa = nullptr;     // n_tr values, then a 1.0 (hdg_apply_tracer_diffusion)
  const double* d_difftab = nullptr;
  DevCsr gdiff;
  double diff_lambda = -1.0;  // upper bound of rho(M^-1 D); < 0: not built
  void diff_setup() {
    if (diff_lambda >= 0.0) return;
    if (comm->size > 1) cg_setup();  // a strip: the tracer error of hdg_set_tracer
    d_kappa = dalloc(HDG_MAX_TRACERS + 1);
    std::vector<double> k0(HDG_MAX_TRACERS + 1, 0.0);
    k0[HDG_MAX_TRACERS] = 1.0;
    HIPCHECK(hipMemcpy(d_kappa, k0.data(), sizeof(double) * k0.size(), hipMemcpyHostToDevice));
    if (general) {
      double lam = 0.0;
      gdiff = upload_csr(assemble_tracer_diffusion(*gtab, *gm, lam));
      diff_lambda = lam;
    } else {
      const TracerDiffusionTables D(K, g.h);
      d_difftab = upload(D.packed());
      diff_lambda = D.lambda;
    }
  }
  void set_tracer_diffusivity(int n, const double* kappa) {
    if (comm->size > 1) cg_setup();  // a strip: the tracer error of hdg_set_tracer
    if (step_open) throw std::string("hdg_set_tracer_diffusivity: a step is open (between hdg_begin_step and the end of the step)");
    bool any = false;
    if (kappa) {
      if (n != n_tr) throw std::string("hdg_set_tracer_diffusivity: " + std::to_string(n) + " value(s) for " + std::to_string(n_tr) + " tracer(s)");
      for (int t = 0; t < n; t++) {
        if (!(kappa[t] >= 0.0) || !std::isfinite(kappa[t]))
          throw std::string("hdg_set_tracer_diffusivity: kappa[" + std::to_string(t) + "] = " + std::to_string(kappa[t]) + " is not a finite value >= 0");
        any = any || kappa[t] != 0.0;
      }
    }
    if (!any) { tr_kappa.clear(); return; }
    diff_setup();
    tr_kappa.assign(kappa, kappa + n);
    HIPCHECK(hipMemcpyAsync(d_kappa, tr_kappa.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // out_t += kap_t M^-1 D q_t for n tracers, tracer-major (kap: device values for the kernel, host values for the CSR path);
  // structured meshes read the ghost rows of q, which the caller has filled (tracer_adv on the same q, or halo_rows)
  // slot: the first tracer's row of the wall arrays (0: the engine's setting, HDG_MAX_TRACERS: the hook's); < 0: no walls
  void tracer_diff(const double* q, const double* kap_dev, const double* kap_host, double* out, int n, int slot = -1) {
    if (general) {
      for (int t = 0; t < n; t++) {
        if (kap_host[t] == 0.0) continue;
        const bool fixed = slot >= 0 && tw_kind_all[(size_t)(slot + t) * 4] != 0;  // the whole boundary: index 0
        csr(fixed ? gdiffw : gdiff, q + t * NPv, kap_host[t], 1.0, out + t * NPv);
        if (fixed) axpby(NPv, kap_host[t] * tw_val_all[(size_t)(slot + t) * 4], d_gwload, 1.0, out + t * NPv);
      }
      return;
    }
    tally(LC_OTHER, 3.0 * n * bP());
    by_degree([&](auto k) {
      constexpr int KK = decltype(k)::value;
      by_tracer_block<TracerBlock<KK>::TB>(n, [&](auto tb) {
        constexpr int TB = decltype(tb)::value;
        dim3 grid = cell_grid();
        grid.y = (unsigned)((n + TB - 1) / TB);
        if (slot >= 0)  // instead of the plain form, not after it: no launch more and no second pass over out
          k_tracer_diff<KK, TB, true><<<grid, bs(), 0, stream>>>(g, d_difftab, kap_dev, n, NPv, q, out, d_walltab, d_wkind + 4 * slot, d_wval + 4 * slot);
        else
          k_tracer_diff<KK, TB, false><<<grid, bs(), 0, stream>>>(g, d_difftab, kap_dev, n, NPv, q, out, nullptr, nullptr, nullptr);
      });
    });
  }
  // the tendency of every tracer: transport, plus diffusion when some kappa_t != 0 (with the wall terms when some side is fixed)
  void tracer_tendency(const double* q, const double* u, double* out) {
    tracer_adv(q, u, out, n_tr);
    if (!tr_kappa.empty() && !tdi_mode) tracer_diff(q, d_kappa, tr_kappa.data(), out, n_tr, tw_kind.empty() ? -1 : 0);
  }
  // ---- fixed-value walls and the wall flux (include/hdg_tracer_walls.h).  Per tracer and side (structured:
  // bottom, right, top, left; general: the whole boundary at index 0) a kind (0 no flux, 1 fixed value) and a value; a fixed side
  // adds the Nitsche terms D_w q + l_w(g) to the diffusion form.  Structured meshes: k_tracer_diff<K, TB, true> runs instead of
  // the plain form; general meshes: a second assembled operator M^-1 (D + D_w) and one axpy with the load vector per tracer.
  // Configuration like kappa, and independent of it: with every kappa_t = 0 the walls do nothing.
  std::vector<int> tw_kind;     // n_tr x 4 while some side is fixed, empty while the feature is off
  std::vector<double> tw_val;   // n_tr x 4 (0 on a no-flux side)
  std::vector<int> tw_kind_all = std::vector<int>((HDG_MAX_TRACERS + 1) * 4, 0);       // host mirror of d_wkind, the hook's row last
  std::vector<double> tw_val_all = std::vector<double>((HDG_MAX_TRACERS + 1) * 4, 0.0);  // host mirror of d_wval
  int* d_wkind = nullptr;
  double *d_wval = nullptr, *d_wflux = nullptr, *d_wpart = nullptr, *d_gwload = nullptr;
  const double* d_walltab = nullptr;
  DevCsr gdiffw;
  double wall_wone = 0.0;         // structured: eta_b h; general: the sum of eta_b |e| over the boundary
  double diff_lambda_gw = -1.0;   // general: the infinity norm of M^-1 (D + D_w)
  static const char* wall_side_name(bool gen, int w) {
    static const char* names[4] = {"bottom", "right", "top", "left"};
    return gen ? "boundary" : names[w];
  }
  int wall_flux_blocks() const { return (std::max(g.nx, g.ny) + HDG_WALL_FLUX_BLOCK - 1) / HDG_WALL_FLUX_BLOCK; }
  // the wall tables, on the first fixed side
  void walls_setup() {
    diff_setup();
    if (d_wkind) return;
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, sizeof(int) * tw_kind_all.size()));
    allocs.push_back(p);
    HIPCHECK(hipMemset(p, 0, sizeof(int) * tw_kind_all.size()));
    d_wval = dalloc((long)tw_val_all.size());
    d_wflux = dalloc(HDG_MAX_TRACERS * 4);
    if (general) {
      double lam = 0.0;
      std::vector<double> load;
      gdiffw = upload_csr(assemble_tracer_diffusion(*gtab, *gm, lam, &load, &wall_wone));
      d_gwload = const_cast<double*>(upload(load));
      diff_lambda_gw = lam;
    } else {
      const TracerDiffusionTables D(K, g.h);
      d_walltab = upload(D.packed_walls());
      wall_wone = D.wone;
      d_wpart = dalloc((long)HDG_MAX_TRACERS * 4 * wall_flux_blocks());
    }
    d_wkind = (int*)p;
  }
  // throws unless kind / value (rows x 4) are an admissible setting of this mesh; what: the entry point's name
  void check_walls(const char* what, int rows, const int* kind, const double* value) const {
    for (int t = 0; t < rows; t++)
      for (int w = 0; w < 4; w++) {
        const int kd = kind[t * 4 + w];
        const std::string where = std::string(what) + ": tracer " + std::to_string(t) + ", side " + std::to_string(w) +
            " (" + wall_side_name(general && w == 0, w) + ")";
        if (kd != 0 && kd != 1) throw where + ": kind " + std::to_string(kd) + " is neither 0 (no flux) nor 1 (fixed value)";
        if (kd == 0) continue;
        if (!value || !std::isfinite(value[t * 4 + w])) throw where + ": the fixed value " + (value ? std::to_string(value[t * 4 + w]) : std::string("(null)")) + " is not finite";
        if (!general && periodic) throw where + ": the doubly periodic square has no walls";
        if (general && w != 0) throw where + ": a general mesh has one side, the whole boundary, at index 0";
      }
  }
  void upload_walls(int row0, int rows) {
    HIPCHECK(hipMemcpyAsync(d_wkind + 4 * row0, tw_kind_all.data() + 4 * row0, sizeof(int) * 4 * rows, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(d_wval + 4 * row0, tw_val_all.data() + 4 * row0, sizeof(double) * 4 * rows, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void set_tracer_walls(int n, const int* kind, const double* value) {
    if (comm->size > 1) cg_setup();  // a strip: the tracer error of hdg_set_tracer
    if (step_open) throw std::string("hdg_set_tracer_walls: a step is open (between hdg_begin_step and the end of the step)");
    bool any = false;
    if (kind) {
      if (n != n_tr) throw std::string("hdg_set_tracer_walls: " + std::to_string(n) + " row(s) for " + std::to_string(n_tr) + " tracer(s)");
      check_walls("hdg_set_tracer_walls", n, kind, value);
      for (int m = 0; m < 4 * n; m++) any = any || kind[m] != 0;
    }
    if (!any) { tw_kind.clear(); tw_val.clear(); return; }
    walls_setup();
    tw_kind.assign(kind, kind + 4 * n);
    tw_val.assign((size_t)4 * n, 0.0);
    for (int m = 0; m < 4 * n; m++) if (kind[m]) tw_val[(size_t)m] = value[m];
    std::copy(tw_kind.begin(), tw_kind.end(), tw_kind_all.begin());
    std::copy(tw_val.begin(), tw_val.end(), tw_val_all.begin());
    upload_walls(0, n);
  }
  // test hook: out = M^-1 (D + sum_w D_w) q + M^-1 sum_w l_w for one field (device layout), without kappa; sets nothing
  void apply_tracer_wall_diffusion(const int* kind, const double* value, double* q, double* out) {
    bool any = false;
    check_walls("hdg_apply_tracer_wall_diffusion", 1, kind, value);
    for (int w = 0; w < 4; w++) any = any || kind[w] != 0;
    if (!any) { apply_tracer_diffusion(q, out); return; }  // the plain form: bit for bit
    walls_setup();
    for (int w = 0; w < 4; w++) {
      tw_kind_all[(size_t)HDG_MAX_TRACERS * 4 + w] = kind[w];
      tw_val_all[(size_t)HDG_MAX_TRACERS * 4 + w] = kind[w] ? value[w] : 0.0;
    }
    upload_walls(HDG_MAX_TRACERS, 1);
    if (!general) halo_rows(q, (long)g.R * g.nx, g.nx, NP * 2, 1);
    zero(out, NPv);
    const double one = 1.0;
    tracer_diff(q, d_kappa + HDG_MAX_TRACERS, &one, out, 1, HDG_MAX_TRACERS);
  }
  // flux[n_tr x 4] of the current tracers q_cur
  void tracer_wall_flux(double* flux) {
    std::fill(flux, flux + 4 * n_tr, 0.0);
    if (tw_kind.empty() || tr_kappa.empty()) return;  // no fixed side, or no diffusivity: no flux through any wall
    if (general) {
      for (int t = 0; t < n_tr; t++) {
        if (!tw_kind[(size_t)t * 4] || tr_kappa[(size_t)t] == 0.0) continue;
        flux[t * 4] = tr_kappa[(size_t)t] * (tw_val[(size_t)t * 4] * wall_wone - dot(NPv, d_gwload, q_cur + t * NPv, KC));
      }
      return;
    }
    const int nblk = wall_flux_blocks();
    tally(LC_OTHER, 0.0);
    tally(LC_OTHER, 0.0);
    by_degree([&](auto k) { k_tracer_wall_flux<k()><<<dim3(nblk, 4), HDG_WALL_FLUX_BLOCK, 0, stream>>>(g, d_walltab, n_tr, NPv, q_cur, d_wpart); });
    k_tracer_wall_flux_finish<<<1, 64, 0, stream>>>(n_tr, nblk, g.nx, g.ny, wall_wone, d_kappa, d_wkind, d_wval, d_wpart, d_wflux);
    HIPCHECK(hipMemcpyAsync(flux, d_wflux, sizeof(double) * 4 * n_tr, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // test hook: out = M^-1 D q for one field (q, out in the device layout), without kappa
  void apply_tracer_diffusion(double* q, double* out) {
    diff_setup();
    if (!general) halo_rows(q, (long)g.R * g.nx, g.nx, NP * 2, 1);
    zero(out, NPv);
    const double one = 1.0;
    tracer_diff(q, d_kappa + HDG_MAX_TRACERS, &one, out, 1);
  }
  void tracer_diffusion_number(double* out2) {
    diff_setup();
    double kmax = 0.0;
    for (double x : tr_kappa) kmax = std::max(kmax, x);
    double lam = diff_lambda;
    if (!tw_kind.empty()) {  // with the wall blocks of every side that is fixed for some tracer
      if (general) lam = std::max(lam, diff_lambda_gw);
      else {
        bool fixed[4] = {false, false, false, false};
        for (size_t m = 0; m < tw_kind.size(); m++) fixed[m & 3] = fixed[m & 3] || tw_kind[m] != 0;
        lam = TracerDiffusionTables(K, g.h).lambda_walls(fixed);
      }
    }
    out2[0] = lam;
    out2[1] = kmax * cfg.dt * lam;
  }
  // ---- implicit tracer diffusion (include/hdg_tracer_implicit.h, hdg_tracer_implicit.hpp).  In implicit
  // mode the tendencies carry transport alone (tracer_tendency), and where a step forms its new tracers every tracer with
  // kappa_t != 0 becomes the solution of (I - dt kappa_t M^-1 D_w) q = q~ + dt kappa_t l_w: a Lie splitting, first order in dt.
  // Structured meshes on one rank.  The five work vectors are scratch, written from their start in every solve: no state.
  int tdi_mode = 0;  // 0 explicit, 1 implicit
  double tdi_rtol = 1e-10;
  int tdi_maxit = 2000;
  double *tdi_x = nullptr, *tdi_r = nullptr, *tdi_p = nullptr, *tdi_y = nullptr, *tdi_w = nullptr, *tdi_part = nullptr, *tdi_sc = nullptr,
         *tdi_tau = nullptr, *tdi_h = nullptr;
  hipEvent_t tdi_ev[2] = {nullptr, nullptr};
  std::vector<int> tdi_its = std::vector<int>(HDG_MAX_TRACERS, 0);        // the last solve, per tracer
  std::vector<double> tdi_res = std::vector<double>(HDG_MAX_TRACERS, 0.0);
  std::string tdi_failure;                                                 // the last solve's, until tdi_raise reports it
  long tdi_solves = 0, tdi_iterations = 0;                                 // solves and operator passes since the engine exists
  void tdi_alloc() {
    if (tdi_x) return;
    tracer_alloc();
    for (double** v : {&tdi_x, &tdi_r, &tdi_p, &tdi_y, &tdi_w}) *v = dalloc(NTv());
    tdi_part = dalloc(3L * HDG_MAX_TRACERS * cell_grid().x);
    tdi_sc = dalloc((long)HDG_MAX_TRACERS * TDI_NSC);
    tdi_tau = dalloc(HDG_MAX_TRACERS);
    HIPCHECK(hipHostMalloc((void**)&tdi_h, sizeof(double) * 2));
    for (int q = 0; q < 2; q++) HIPCHECK(hipEventCreateWithFlags(&tdi_ev[q], hipEventDisableTiming));
  }
  void set_tracer_diffusion_mode(int mode, double rtol, int max_iterations) {
    if (step_open) throw std::string("hdg_set_tracer_diffusion_mode: a step is open (between hdg_begin_step and the end of the step)");
    if (mode != 0 && mode != 1) throw std::string("hdg_set_tracer_diffusion_mode: mode " + std::to_string(mode) + " is neither 0 (explicit) nor 1 (implicit)");
    if (!(rtol > 0.0) || !std::isfinite(rtol)) throw std::string("hdg_set_tracer_diffusion_mode: rtol = " + std::to_string(rtol) + " is not a finite value > 0");
    if (max_iterations < 1) throw std::string("hdg_set_tracer_diffusion_mode: max_iterations = " + std::to_string(max_iterations) + " is not positive");
    tdi_mode = mode; tdi_rtol = rtol; tdi_maxit = max_iterations;
  }
  // the ghost rows of the tracers still in the solve (the periodic square reads them): one call per run of neighbours in t
  void tdi_halo(double* v, const std::vector<char>& on) {
    if (!periodic) return;
    const int n = (int)on.size();
    for (int t = 0; t < n;) {
      if (!on[(size_t)t]) { t++; continue; }
      int e = t;
      while (e < n && on[(size_t)e]) e++;
      halo_rows(v + t * NPv, (long)g.R * g.nx, g.nx, NP * 2 * (e - t), 1);
      t = e;
    }
  }
  // q_t <- the solution of (I - tau_t M^-1 D_w) x = q_t + tau_t l_w for the n tracer-major fields at q; tau[n]: host values, copied
  // to the small device array tdi_tau the kernels read, and the choice of the tracers that take part.  slot: the wall rows, as in
  // tracer_diff.  A tracer that does not converge keeps its values, and tdi_failure says so.
  void tdi_solve(double* q, int n, const double* tau_host, int slot) {
    tdi_alloc();
    diff_setup();
    std::vector<char> on((size_t)n);
    std::vector<double> sc0((size_t)n * TDI_NSC, 0.0);
    int nact = 0;
    for (int t = 0; t < n; t++) {
      on[(size_t)t] = tau_host[t] != 0.0;
      nact += on[(size_t)t];
      sc0[(size_t)t * TDI_NSC + TDI_STATE] = on[(size_t)t] ? (double)TDI_ITERATING : (double)TDI_IDLE;
    }
    std::fill(tdi_its.begin(), tdi_its.end(), 0);
    std::fill(tdi_res.begin(), tdi_res.end(), 0.0);
    tdi_failure.clear();
    if (nact == 0) return;
    tdi_solves++;
    HIPCHECK(hipMemcpyAsync(tdi_sc, sc0.data(), sizeof(double) * sc0.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(tdi_tau, tau_host, sizeof(double) * n, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));  // sc0 and tau_host leave scope
    const int nblk = (int)cell_grid().x;
    double *part_rr = tdi_part, *part_rw = tdi_part + (long)HDG_MAX_TRACERS * nblk, *part_bb = tdi_part + 2L * HDG_MAX_TRACERS * nblk;
    const double rtol2 = tdi_rtol * tdi_rtol;
    auto helm = [&](auto init, const double* in, double* out, double* p0, double* p1) {
      tally(LC_OTHER, 3.0 * nact * bP());
      by_degree([&](auto k) {
        constexpr int KK = decltype(k)::value;
        by_tracer_block<TracerBlock<KK>::TB>(n, [&](auto tb) {
          constexpr int TB = decltype(tb)::value;
          constexpr bool INIT = decltype(init)::value;
          dim3 grid = cell_grid();
          grid.y = (unsigned)((n + TB - 1) / TB);
          if (slot >= 0)
            k_tracer_helm<KK, TB, true, INIT><<<grid, bs(), 0, stream>>>(g, d_difftab, tdi_tau, tdi_sc, n, NPv, in, out, tdi_x, p0, p1, d_walltab,
                                                                         d_wkind + 4 * slot, d_wval + 4 * slot);
          else
            k_tracer_helm<KK, TB, false, INIT><<<grid, bs(), 0, stream>>>(g, d_difftab, tdi_tau, tdi_sc, n, NPv, in, out, tdi_x, p0, p1, nullptr,
                                                                          nullptr, nullptr);
        });
      });
    };
    auto scalars = [&](int first, int last, double* hflag) {
      tally(LC_OTHER, 0.0);
      k_tdi_scalars<<<1, HDG_TDI_SC_BLOCK, 0, stream>>>(n, nblk, first, last, rtol2, part_rr, part_rw, part_bb, tdi_sc, hflag);
    };
    tdi_halo(q, on);
    helm(std::true_type{}, q, tdi_r, part_rr, part_bb);  // x_0 = q~, r_0, (r_0, r_0), (b, b)
    bool seen_done = false;
    for (int it = 0; it < tdi_maxit; it++) {
      tdi_halo(tdi_r, on);
      helm(std::false_type{}, tdi_r, tdi_w, part_rw, nullptr);
      scalars(it == 0, 0, tdi_h + (it & 1));
      HIPCHECK(hipEventRecord(tdi_ev[it & 1], stream));
      tally(LC_OTHER, 9.0 * nact * bP());
      dim3 grid = cell_grid();
      grid.y = (unsigned)n;
      by_degree([&](auto k) { k_tdi_update<k()><<<grid, bs(), 0, stream>>>(g, tdi_sc, NPv, tdi_w, tdi_p, tdi_y, tdi_x, tdi_r, part_rr); });
      tdi_iterations++;
      if (it >= 1) {  // the flag word of the previous iteration: every tracer frozen means the launches since did nothing
        HIPCHECK(hipEventSynchronize(tdi_ev[(it - 1) & 1]));
        if (tdi_h[(it - 1) & 1] == 0.0) { seen_done = true; break; }
      }
    }
    if (!seen_done) scalars(0, 1, tdi_h);  // the residual of the last update is still unjudged
    {
      tally(LC_OTHER, 2.0 * nact * bP());
      dim3 grid = cell_grid();
      grid.y = (unsigned)n;
      by_degree([&](auto k) { k_tdi_accept<k()><<<grid, bs(), 0, stream>>>(g, tdi_sc, NPv, tdi_x, q); });
    }
    std::vector<double> sc1((size_t)n * TDI_NSC);
    HIPCHECK(hipMemcpyAsync(sc1.data(), tdi_sc, sizeof(double) * sc1.size(), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    for (int t = 0; t < n; t++) {
      const double* st = sc1.data() + (size_t)t * TDI_NSC;
      if (!on[(size_t)t]) continue;
      tdi_its[(size_t)t] = (int)st[TDI_ITS];
      tdi_res[(size_t)t] = st[TDI_RES];
      if (st[TDI_STATE] == (double)TDI_CONVERGED || !tdi_failure.empty()) continue;
      char buf[200];
      snprintf(buf, sizeof(buf), "implicit tracer diffusion: tracer %d %s after %d iteration(s), relative residual %.3e (rtol %.3e)", t,
               st[TDI_STATE] == (double)TDI_BROKE_DOWN ? "broke down" : "did not converge", (int)st[TDI_ITS], st[TDI_RES], tdi_rtol);
      tdi_failure = buf;
    }
  }
  // the split step: called where a step has formed its transported tracers q_cur
  void tracer_implicit_diffusion() {
    if (!tdi_mode || tr_kappa.empty()) return;
    std::vector<double> tau((size_t)n_tr);
    for (int t = 0; t < n_tr; t++) tau[(size_t)t] = cfg.dt * tr_kappa[(size_t)t];
    tdi_solve(q_cur, n_tr, tau.data(), tw_kind.empty() ? -1 : 0);
  }
  // a solve that failed inside a step is reported once the step is complete: the flow has advanced, the tracer is the transported one
  void tdi_raise() {
    if (tdi_failure.empty()) return;
    const std::string m = tdi_failure;
    tdi_failure.clear();
    throw NotConverged{m};
  }
  // test hook: n fields (device layout, tracer-major at q_t), tau[n] on the host; the walls that are set (row t for field t)
  void solve_tracer_diffusion(int n, const double* tau) {
    if (!tw_kind.empty()) walls_setup();
    tdi_solve(q_t, n, tau, tw_kind.empty() ? -1 : 0);
  }
  // ---- Boussinesq buoyancy: the forcing slot j of a step becomes b_rhs[j] + B(q^(j)),
  // B(q) = sum_t beta_t q_t g embedded in the velocity space (hdg_buoyancy.hpp).  The s + 1 vectors buoy[j] stand beside brhs and
  // profile, whose meaning stays; they are allocated (zeroed: the kernels write the first NP modes only) on the first non-zero
  // beta and rebuilt inside every step, so they are no state.  beta, g are configuration like kappa.  Without a tracer
  // (hdg_set_tracer(NULL)) nothing forces the flow.
  std::vector<double> by_beta;  // n_tr values while the term is on (some beta_t != 0), empty while it is off
  double by_g[2] = {0.0, -1.0};
  std::vector<double*> buoy;    // s + 1 slots, the last one for the pressure reconstruction
  bool buoyancy_on() const { return tracer_on && !by_beta.empty(); }
  BuoyCoef buoyancy_coef() const {
    BuoyCoef B{};
    for (size_t t = 0; t < by_beta.size(); t++) B.beta[t] = by_beta[t];
    B.gx = by_g[0]; B.gy = by_g[1];
    return B;
  }
  void set_buoyancy(int n, const double* beta, const double* grav) {
    if (comm->size > 1) cg_setup();  // a strip: the tracer error of hdg_set_tracer
    if (step_open) throw std::string("hdg_set_buoyancy: a step is open (between hdg_begin_step and the end of the step)");
    if (!tracer_on) throw std::string("hdg_set_buoyancy: no tracer is set (hdg_set_tracer)");
    bool any = false;
    if (beta) {
      if (n != n_tr) throw std::string("hdg_set_buoyancy: " + std::to_string(n) + " value(s) for " + std::to_string(n_tr) + " tracer(s)");
      for (int t = 0; t < n; t++) {
        if (!std::isfinite(beta[t])) throw std::string("hdg_set_buoyancy: beta[" + std::to_string(t) + "] = " + std::to_string(beta[t]) + " is not finite");
        any = any || beta[t] != 0.0;
      }
    }
    if (grav)
      for (int d = 0; d < 2; d++)
        if (!std::isfinite(grav[d])) throw std::string("hdg_set_buoyancy: g[" + std::to_string(d) + "] = " + std::to_string(grav[d]) + " is not finite");
    by_g[0] = grav ? grav[0] : 0.0; by_g[1] = grav ? grav[1] : -1.0;
    if (!any) { by_beta.clear(); return; }  // off: the vectors stay allocated, nothing reads them
    if (buoy.empty())
      for (int j = 0; j <= s; j++) {
        buoy.push_back(dalloc(NQ));
        HIPCHECK(hipMemsetAsync(buoy.back(), 0, sizeof(double) * NQ, stream));
      }
    by_beta.assign(beta, beta + n);
  }
  // f = B(q): q the n_tr tracers tracer-major, f a velocity vector whose modes NP .. NU-1 are zero (owned rows only)
  void buoyancy(const double* q, double* f) {
    int live = 0;
    for (double b : by_beta) live += b != 0.0;
    tally(LC_OTHER, live * bP() + 2.0 * bP());
    const BuoyCoef B = buoyancy_coef();
    if (general) by_degree([&](auto k) { k_g_buoyancy<k()><<<(gm->nc + 63) / 64, 64, 0, stream>>>(gm->nc, B, NPv, q, f); });
    else by_degree([&](auto k) { k_buoyancy<k()><<<cell_grid(), bs(), 0, stream>>>(g, B, NPv, q, f); });
    fl.set(f, 0);
  }
  // slot i of an IMEX step takes the stage tracer q_st[i], complete at the end of tracer_begin_step (i = 0) / tracer_stage(i);
  // behind the last stage q_fin = q_{n+1} is complete too: slot s, the pressure reconstruction
  void buoyancy_slot(int i) {
    if (!buoyancy_on()) return;
    buoyancy(q_st[(size_t)i], buoy[(size_t)i]);
    if (i == s - 1) buoyancy(q_fin, buoy[(size_t)s]);
  }
  // ---- viscous term: the forcing slot j of a step becomes b_rhs[j] + B(q^(j)) + nu M^-1 V Q^(j), V the
  // symmetric interior-penalty form on [DG_{k+1}]^2 with free-slip or no-slip Nitsche walls.  Structured meshes: nine scalar
  // NU x NU blocks per element shape (hdg_tables.hpp: ViscosityTables) applied by k_viscosity; general meshes: M^-1 V assembled
  // once per wall mode (hdg_general.hpp: assemble_viscosity) and applied by the CSR kernel.  The s + 1 vectors visc[j] stand
  // beside brhs, profile and buoy; they are allocated (zeroed: the kernel writes owned rows only) on the first nu != 0 and
  // rebuilt inside every step, so they are no state.  Slot j < s is filled from stQ[j] the first time a residual of the open
  // step reads it (visc_valid, cleared by begin_step; stQ[j] is final once stage j + 1 begins, so the Richardson passes of a
  // stage reuse it); outside a step a read recomputes.  nu and the wall mode are configuration like kappa.
  double visc_nu = 0.0;
  int visc_wall = 0;  // 0 free slip, 1 no slip
  std::vector<double*> visc;
  unsigned visc_valid = 0;   // bit j: slot j holds nu M^-1 V Q^(j) of the open step
  bool visc_step = false;    // between begin_step and finish_step
  const double* d_visctab = nullptr;
  DevCsr gvisc[2];
  double visc_lambda[2] = {-1.0, -1.0};  // upper bound of rho(M^-1 V) per wall mode; < 0: not built
  bool viscosity_on() const { return visc_nu != 0.0; }
  void visc_setup(int wall) {
    if (visc_lambda[wall] >= 0.0) return;
    if (general) {
      if (comm->size > 1) throw std::string("viscosity on a general mesh: single rank only");
      double lam = 0.0;
      gvisc[wall] = upload_csr(assemble_viscosity(*gtab, *gm, wall == 1, lam));
      visc_lambda[wall] = lam;
    } else {
      const ViscosityTables V(K, g.h);
      if (!d_visctab) d_visctab = upload(V.packed_moving());  // packed(), then the load vectors of moving walls (section 24)
      visc_wone = V.wone;
      visc_lambda[0] = visc_lambda[1] = V.lambda;
    }
  }
  static void visc_check_wall(const char* who, int wall) {
    if (wall != 0 && wall != 1) throw std::string(who) + ": wall = " + std::to_string(wall) + " (0: free slip, 1: no slip)";
  }
  void visc_alloc() {
    if (!visc.empty()) return;
    for (int j = 0; j <= s; j++) {
      visc.push_back(dalloc(NQ));
      HIPCHECK(hipMemsetAsync(visc.back(), 0, sizeof(double) * NQ, stream));
    }
  }
  void set_viscosity(double nu, int wall) {
    if (step_open) throw std::string("hdg_set_viscosity: a step is open (between hdg_begin_step and the end of the step)");
    if (!(nu >= 0.0) || !std::isfinite(nu)) throw std::string("hdg_set_viscosity: nu = " + std::to_string(nu) + " is not a finite value >= 0");
    visc_check_wall("hdg_set_viscosity", wall);
    if (wall != 1 && moving_on()) throw std::string("hdg_set_viscosity: a wall velocity is set (hdg_set_wall_velocity), which needs no-slip walls");
    if (nu != 0.0) {
      visc_setup(wall);
      visc_alloc();
    }
    visc_nu = nu; visc_wall = wall;  // off: the vectors stay allocated, nothing reads them
    visc_valid = 0;
  }
  // out = sc M^-1 V Q (owned rows); Q's ghost rows are filled here: wrapped on the periodic square, one exchange on a strip
  // U (may be NULL): the four wall speeds of section 24; with one of them != 0 the kernel that adds sc M^-1 l(U) runs instead
  void viscosity_apply(const double* Q, double sc, int wall, double* out, const double* U = nullptr) {
    if (general) { csr(gvisc[wall], Q, sc, 0.0, out); return; }  // tallied in 'other' by csr()
    tally(LC_OTHER, 2.0 * bQ());
    stencil_in(Q, FQ);
    const WallSpeed W = wall_speed(U);
    if (U && wall_moving(U)) by_degree([&](auto k) { k_viscosity<k(), true><<<cell_grid(), bs(), 0, stream>>>(g, d_visctab, sc, wall, Q, out, W); });
    else by_degree([&](auto k) { k_viscosity<k(), false><<<cell_grid(), bs(), 0, stream>>>(g, d_visctab, sc, wall, Q, out, W); });
    fl.set(out, 0);
  }
  // ---- moving no-slip walls and the wall force: the tangential Nitsche term of the viscous form acts on
  // u.t - U_w, U_w the constant Cartesian tangential speed of side w (bottom, right, top, left) of the structured unit square,
  // which adds nu M^-1 l(U) to every viscous slot: k_viscosity<K, true> runs instead of the plain kernel, no launch more.
  // Configuration like nu; on a strip every rank has to be given the same speeds (not checked).
  double wall_u[4] = {0.0, 0.0, 0.0, 0.0};
  double visc_wone = 0.0;  // eta_b h of the viscous form
  double *d_wforce = nullptr, *d_wfpart = nullptr;
  static bool wall_moving(const double* U) { return U[0] != 0.0 || U[1] != 0.0 || U[2] != 0.0 || U[3] != 0.0; }
  static WallSpeed wall_speed(const double* U) { return U ? WallSpeed{U[0], U[1], U[2], U[3]} : WallSpeed{0.0, 0.0, 0.0, 0.0}; }
  bool moving_on() const { return wall_moving(wall_u); }
  // throws unless the speeds U (NULL: none) are admissible on this mesh in the wall mode `wall`; general meshes are refused by
  // the entry points before (HDG_ERR_UNSUPPORTED)
  void check_wall_velocity(const char* who, const double* U, int wall) const {
    if (step_open) throw std::string(who) + ": a step is open (between hdg_begin_step and the end of the step)";
    if (!U) return;
    for (int w = 0; w < 4; w++)
      if (!std::isfinite(U[w])) throw std::string(who) + ": side " + std::to_string(w) + " (" + wall_side_name(false, w) + "): the speed " + std::to_string(U[w]) + " is not finite";
    if (!wall_moving(U)) return;
    if (periodic) throw std::string(who) + ": the doubly periodic square has no walls";
    if (wall != 1) throw std::string(who) + ": a wall velocity needs no-slip walls (HDG_WALL_NO_SLIP)";
  }
  void set_wall_velocity(const double* U) {
    check_wall_velocity("hdg_set_wall_velocity", U, visc_wall);
    for (int w = 0; w < 4; w++) wall_u[w] = U ? U[w] : 0.0;
    visc_valid = 0;
  }
  int wall_force_blocks() const { return (std::max(g.nx, g.ny) + HDG_WALL_FORCE_BLOCK - 1) / HDG_WALL_FORCE_BLOCK; }
  // F[2 w + c] = sc * (the force functional of section 24) of the modal field Q in the wall mode `wall` with the speeds U;
  // on a strip the eight values are added over the ranks, so every rank returns the same
  void wall_force(const double* Q, double sc, int wall, const double* U, double* F) {
    std::fill(F, F + 8, 0.0);
    if (periodic) return;  // no walls
    visc_setup(wall);
    const int nblk = wall_force_blocks();
    if (!d_wforce) { d_wforce = dalloc(8); d_wfpart = dalloc(8L * nblk); }
    const WallSpeed W = wall_speed(U);
    tally(LC_OTHER, 0.0);
    tally(LC_OTHER, 0.0);
    by_degree([&](auto k) { k_wall_force<k()><<<dim3(nblk, 4), HDG_WALL_FORCE_BLOCK, 0, stream>>>(g, d_visctab, wall, visc_wone, W, Q, d_wfpart); });
    k_wall_force_finish<<<1, 64, 0, stream>>>(nblk, g.nx, g.ny, sc, d_wfpart, d_wforce);
    if (comm->size > 1) comm->allreduce_sum(d_wforce, 8, stream);
    HIPCHECK(hipMemcpyAsync(F, d_wforce, sizeof(double) * 8, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void viscosity_slot(int j, const double* Q) {
    if (visc_step && (visc_valid >> j & 1u)) return;
    vel_linear_apply(Q, visc[(size_t)j]);
    visc_valid |= 1u << j;
  }
  // the slots a residual with the forcing coefficients cb reads
  void viscosity_slots(const std::vector<double>& cb) {
    if (!vel_linear_on()) return;
    for (int j = 0; j < s; j++)
      if (cb[(size_t)j] != 0.0) viscosity_slot(j, stQ[j]);
  }
  void viscosity_number(double nu, int wall, double* out2) {
    if (!(nu >= 0.0) || !std::isfinite(nu)) throw std::string("hdg_get_viscosity: nu = " + std::to_string(nu) + " is not a finite value >= 0");
    visc_check_wall("hdg_get_viscosity", wall);
    visc_setup(wall);
    out2[0] = visc_lambda[wall];
    out2[1] = nu * cfg.dt * visc_lambda[wall];
  }
  // ---- Coriolis term: - f_c k x u, f_c = f0 + beta y.  M^-1 C is block diagonal per cell, so the term
  // rides in the vectors of the viscous term: visc[j] is the velocity-linear part of slot j, nu M^-1 V Q^(j) + M^-1 C Q^(j).
  // With both terms on k_viscosity writes the slot and k_coriolis adds to it in place; with rotation alone k_coriolis writes
  // it.  No ghost rows, no exchange; general meshes run matrix-free on one rank.  f0 and beta are configuration like nu.
  double cor_f0 = 0.0, cor_beta = 0.0;
  const double* d_cortab = nullptr;  // structured: Y_0, Y_1 transposed; general: L_1, L_2
  const double* d_coryv = nullptr;   // general: the ordinates of a cell's three vertices, nc x 3
  bool coriolis_on() const { return cor_f0 != 0.0 || cor_beta != 0.0; }
  void coriolis_check(const char* who, double f0, double beta) const {
    if (step_open) throw std::string(who) + ": a step is open (between hdg_begin_step and the end of the step)";
    if (!std::isfinite(f0) || !std::isfinite(beta))
      throw std::string(who) + ": f0 = " + std::to_string(f0) + ", beta = " + std::to_string(beta) + " are not both finite";
    if (beta != 0.0 && cfg.periodic)
      throw std::string(who) + ": beta != 0 on the doubly periodic square (f0 + beta y jumps at the wrap)";
  }
  void coriolis_setup() {
    if (d_cortab) return;
    const CoriolisTables T(K);
    if (general) {
      if (comm->size > 1) throw std::string("rotation on a general mesh: single rank only");
      dvec yv((size_t)3 * gm->nc);
      for (size_t n = 0; n < yv.size(); n++) yv[n] = gm->X[2 * (size_t)gm->C[n] + 1];
      d_coryv = upload(yv);
      d_cortab = upload(T.general());
    } else
      d_cortab = upload(T.packed());
  }
  void set_coriolis(double f0, double beta) {
    coriolis_check("hdg_set_coriolis", f0, beta);
    if (f0 != 0.0 || beta != 0.0) {
      coriolis_setup();
      visc_alloc();
    }
    cor_f0 = f0; cor_beta = beta;  // off: the vectors stay allocated, nothing reads them
    visc_valid = 0;
  }
  // out = M^-1 C Q, or out += M^-1 C Q (acc), on the owned rows
  void coriolis_apply(const double* Q, double f0, double beta, bool acc, double* out) {
    tally(LC_OTHER, (acc ? 3.0 : 2.0) * bQ());
    by_degree([&](auto k) {
      if (general) {
        const dim3 gr((gm->nc + 63) / 64);
        if (acc) k_g_coriolis<k(), true><<<gr, 64, 0, stream>>>(gm->nc, d_cortab, d_coryv, f0, beta, Q, out);
        else k_g_coriolis<k(), false><<<gr, 64, 0, stream>>>(gm->nc, d_cortab, d_coryv, f0, beta, Q, out);
      } else {
        if (acc) k_coriolis<k(), true><<<cell_grid(), bs(), 0, stream>>>(g, d_cortab, f0, beta, g.h, Q, out);
        else k_coriolis<k(), false><<<cell_grid(), bs(), 0, stream>>>(g, d_cortab, f0, beta, g.h, Q, out);
      }
    });
    fl.set(out, 0);
  }
  // the velocity-linear part of a slot: out = nu M^-1 V Q + M^-1 C Q - M^-1 D (Q - u_s), whichever of the three are on; the
  // first one that runs writes the slot, the others add to it in place (the drag kernel last, section 26)
  void vel_linear_apply(const double* Q, double* out) {
    if (viscosity_on()) viscosity_apply(Q, visc_nu, visc_wall, out, wall_u);
    if (coriolis_on()) coriolis_apply(Q, cor_f0, cor_beta, viscosity_on(), out);
    if (drag_on()) drag_apply(drag_set, Q, -1.0, drag_set.load, viscosity_on() || coriolis_on(), out);
  }
  // F = max over the mesh vertices of |f0 + beta y|, an upper bound of rho(M^-1 C); f_c is linear, so on the structured meshes
  // the two ends of the ordinate decide
  double coriolis_bound(double f0, double beta) const {
    if (general) {
      double F = 0.0;
      for (int v = 0; v < gm->nv; v++) F = std::max(F, std::fabs(f0 + beta * gm->X[2 * (size_t)v + 1]));
      return F;
    }
    if (cfg.periodic) return std::fabs(f0);
    return std::max(std::fabs(f0), std::fabs(f0 + beta * g.h * g.nyg));
  }
  // ---- linear drag and volume penalisation: - sigma (u - u_s), sigma >= 0 linear per cell.  M^-1 D is
  // block diagonal per cell like M^-1 C, so the term rides in the same vectors: visc[j] is the velocity-linear part of slot j,
  // nu M^-1 V Q^(j) + M^-1 C Q^(j) - M^-1 D (Q^(j) - u_s).  k_drag runs last: it accumulates when viscosity or rotation wrote
  // the slot and writes otherwise.  The target enters as one vector M^-1 D u_s built at set time by the same kernel, so the
  // slot stays affine in Q.  No ghost rows, no exchange; general meshes run on one rank.  Host packing: hdg_drag_host.hpp.
  struct DragSet {
    double* coef = nullptr;  // structured: three planes of Nc in the kernels' cell order; general: nc x 3
    int* region = nullptr;   // structured: Nc tags in the kernels' cell order; general: nc
    double* load = nullptr;  // M^-1 D u_s (NQ), or null: u_s = 0
    double S = 0.0;          // the largest vertex value of this rank
  };
  DragSet drag_set;
  double drag_S = 0.0;  // the largest vertex value over all ranks; 0: off
  std::vector<double> drag_sigma;  // the setting as given (public numbering): what hdg_get_drag returns
  ckpt::Digest drag_dig[3];        // the coefficient planes, the target and the tags, as a checkpoint's fingerprint names them
  bool drag_has_target = false;
  const double* d_dragtab = nullptr;  // L_1, L_2
  double *d_dforce = nullptr, *d_dfpart = nullptr;
  double* d_dragS = nullptr;  // strips: 1 + size words for the collective maximum
  bool drag_on() const { return drag_S > 0.0; }
  bool vel_linear_on() const { return viscosity_on() || coriolis_on() || drag_on(); }
  long drag_cells() const { return general ? (long)gm->nc : 2L * g.nx * g.ny; }
  void drag_setup() {
    if (d_dragtab) return;
    if (general && comm->size > 1) throw std::string("drag on a general mesh: single rank only");
    d_dragtab = upload(CoriolisTables(K).general());
  }
  void drag_release(DragSet& D) {
    release_dev(D.coef); release_dev(D.region); release_dev(D.load);
    D = DragSet{};
  }
  // out = sgn M^-1 D Q + load (null: none), or out += that (acc), on the owned rows
  void drag_apply(const DragSet& D, const double* Q, double sgn, const double* load, bool acc, double* out) {
    tally(LC_OTHER, ((acc ? 3.0 : 2.0) + (load ? 1.0 : 0.0)) * bQ() + 24.0 * (double)drag_cells());
    auto go = [&](auto k, auto a, auto l) {
      if (general) k_g_drag<k(), a(), l()><<<dim3((gm->nc + 63) / 64), 64, 0, stream>>>(gm->nc, d_dragtab, D.coef, sgn, Q, load, out);
      else k_drag<k(), a(), l()><<<cell_grid(), bs(), 0, stream>>>(g, d_dragtab, D.coef, sgn, Q, load, out);
    };
    by_degree([&](auto k) {
      if (acc) { if (load) go(k, std::true_type{}, std::true_type{}); else go(k, std::true_type{}, std::false_type{}); }
      else { if (load) go(k, std::false_type{}, std::true_type{}); else go(k, std::false_type{}, std::false_type{}); }
    });
    fl.set(out, 0);
  }
  // the device form of a setting that drag_validate has passed; sigma not null.  Uses wQ1.
  DragSet drag_build(const double* sigma, const double* target, const int* region) {
    drag_setup();
    DragSet D;
    const long nc = drag_cells();
    D.S = drag_bound(sigma, nc);
    D.coef = const_cast<double*>(upload(general ? drag_pack_general(sigma, nc) : drag_pack_planes(sigma, g.nx, g.ny, g.R, GH)));
    D.region = const_cast<int*>(upload_ints(general ? (region ? std::vector<int>(region, region + nc) : std::vector<int>((size_t)nc, 0))
                                                    : drag_pack_regions(region, g.nx, g.ny, g.R, GH)));
    bool any = false;
    if (target)
      for (long n = 0; n < NQb && !any; n++) any = target[n] != 0.0;
    if (any) {
      D.load = dalloc(NQ);
      put_Q(target, wQ1);
      drag_apply(D, wQ1, 1.0, nullptr, false, D.load);
    }
    return D;
  }
  void drag_check(const char* who, const double* sigma, const double* target, const int* region) const {
    if (step_open) throw std::string(who) + ": a step is open (between hdg_begin_step and the end of the step)";
    const std::string bad = drag_validate(sigma, drag_cells(), target, NQb, region);
    if (!bad.empty()) throw std::string(who) + ": " + bad;
  }
  void set_drag(const double* sigma, const double* target, const int* region) {
    if (step_open) throw std::string("hdg_set_drag: a step is open (between hdg_begin_step and the end of the step)");
    if (general && comm->size > 1) throw std::string("drag on a general mesh: single rank only");
    const long nc = drag_cells();
    const std::string bad = drag_validate(sigma, nc, target, NQb, region);
    double S = bad.empty() ? drag_bound(sigma, nc) : -1.0;
    bool other = false;
    if (comm->size > 1) {  // collective: the bound is a global maximum, and a fault anywhere refuses the call everywhere
      if (!d_dragS) d_dragS = dalloc(1L + comm->size);
      HIPCHECK(hipMemcpyAsync(d_dragS, &S, sizeof(double), hipMemcpyHostToDevice, stream));
      comm->allgather(d_dragS, d_dragS + 1, 1, stream);
      n_gather++;
      std::vector<double> all((size_t)comm->size);
      HIPCHECK(hipMemcpyAsync(all.data(), d_dragS + 1, sizeof(double) * all.size(), hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
      for (double x : all) { if (x < 0.0) other = true; else S = S < 0.0 ? S : std::max(S, x); }
    }
    if (!bad.empty()) throw "hdg_set_drag: " + bad;
    if (other) throw std::string("hdg_set_drag: another rank refused its arrays");
    std::vector<double> zeros;
    if (!sigma && S > 0.0) { zeros.assign((size_t)(3 * nc), 0.0); sigma = zeros.data(); }  // a rank of a strip whose cells carry none
    drag_release(drag_set);
    drag_sigma.clear();
    drag_has_target = false;
    drag_S = S;
    visc_valid = 0;
    if (S == 0.0) return;  // off: the slot vectors stay allocated, nothing reads them
    drag_set = drag_build(sigma, target, region);
    visc_alloc();
    drag_sigma.assign(sigma, sigma + 3 * nc);
    drag_has_target = drag_set.load != nullptr;
    drag_dig[0] = ckpt::digest_bytes(sigma, sizeof(double) * 3 * (size_t)nc);
    if (drag_has_target) drag_dig[1] = ckpt::digest_bytes(target, sizeof(double) * (size_t)NQb);
    const std::vector<int> tags = region ? std::vector<int>(region, region + nc) : std::vector<int>((size_t)nc, 0);
    drag_dig[2] = ckpt::digest_bytes(tags.data(), sizeof(int) * tags.size());
  }
  // F[3 r + 0 .. 2] = (F_x, F_y, P) of region r for the modal field Q and the setting D; added over the ranks of a strip
  void drag_force(const DragSet& D, const double* Q, double* F) {
    const int nb = general ? (gm->nc + 127) / 128 : (int)cell_grid().x;
    if (!d_dforce) { d_dforce = dalloc(HDG_DRAG_FORCE_NVAL); d_dfpart = dalloc((long)HDG_DRAG_FORCE_NVAL * nb); }
    tally(LC_OTHER, ((D.load ? 2.0 : 1.0)) * bQ() + 28.0 * (double)drag_cells());
    auto go = [&](auto k, auto l) {
      if (general) k_g_drag_force<k(), l()><<<nb, 128, 0, stream>>>(gm->nc, ggeo.detJ, d_dragtab, D.coef, D.region, Q, D.load, d_dfpart);
      else k_drag_force<k(), l()><<<cell_grid(), bs(), 0, stream>>>(g, d_dragtab, D.coef, D.region, Q, D.load, d_dfpart);
    };
    by_degree([&](auto k) { if (D.load) go(k, std::true_type{}); else go(k, std::false_type{}); });
    tally(LC_OTHER, 0.0);
    k_drag_force_finish<<<1, 256, 0, stream>>>(nb, d_dfpart, d_dforce);
    if (comm->size > 1) comm->allreduce_sum(d_dforce, HDG_DRAG_FORCE_NVAL, stream);
    HIPCHECK(hipMemcpyAsync(F, d_dforce, sizeof(double) * HDG_DRAG_FORCE_NVAL, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // hdg_imex.py:560 and the i = 0 term of _tracer_final_residual
  void tracer_begin_step() {
    if (!tracer_on) return;
    copy(q_st[0], q_cur, NTv());
    copy(q_fin, q_cur, NTv());
    if (cfg.b_expl[0] != 0.0) {
      cg_project(stQ[0], uproj);
      tracer_tendency(q_st[0], uproj, q_t);
      axpby(NTv(), cfg.dt * cfg.b_expl[0], q_t, 1.0, q_fin);
    }
    buoyancy_slot(0);
  }
  // hdg_imex.py:622-623: q_i = q_0 + dt sum_{j<i} a_expl[i,j] T(q_j, P(Q_i)); plus the i-th term of the final residual
  void tracer_stage(int i) {
    if (!tracer_on) return;
    if (i < 1 || i >= s) throw std::string("stage out of range");
    cg_project(stQ[i], uproj);
    copy(q_st[i], q_st[0], NTv());
    for (int j = 0; j < i; j++)
      if (cfg.a_expl[i * s + j] != 0.0) {
        tracer_tendency(q_st[j], uproj, q_t);
        axpby(NTv(), cfg.dt * cfg.a_expl[i * s + j], q_t, 1.0, q_st[i]);
      }
    if (cfg.b_expl[i] != 0.0) {
      tracer_tendency(q_st[i], uproj, q_t);
      axpby(NTv(), cfg.dt * cfg.b_expl[i], q_t, 1.0, q_fin);
    }
    buoyancy_slot(i);
  }
  void tracer_finish_step() {  // hdg_imex.py:638-639
    if (tracer_on) { copy(q_cur, q_fin, NTv()); tracer_implicit_diffusion(); }
  }

  // ------------------------------------------------------------------ per-step outputs (hdg_row_log.hpp)
  // The three recorders below (diagnostics, probes, particles) each append one row per completed step to a device buffer on
  // the stream, no host synchronisation; the RowLog counts rows and drops, the buffer follows its lifetime rule.  Switched
  // off, no step issues a single launch more.
  void log_size(RowLog& L, double*& buf, long width, long cap) {
    L.reset(width, cap);
    if (width * cap > L.alloc) { dfree(buf); L.alloc = 0; buf = dalloc(width * cap); L.alloc = width * cap; }
  }
  double* log_next(RowLog& L, double* buf) {
    const long off = L.next();
    return off == RowLog::DROPPED ? nullptr : buf + off;
  }
  void log_fetch(const RowLog& L, const double* buf, double* rows, long nrows) {
    if (nrows > 0) HIPCHECK(hipMemcpyAsync(rows, buf, sizeof(double) * (size_t)(L.width * nrows), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // what hdg_get_diagnostics / hdg_get_probes / hdg_get_particles do: the row count, the first min(n, max_rows) rows, the
  // optional reset of the counts, and the error for rows dropped since the last reset
  void log_get(const char* label, RowLog& L, const double* buf, double* rows, int max_rows, int* n_rows, int reset,
               long* pa_counts = nullptr) {
    if (max_rows < 0 || (max_rows > 0 && !rows)) throw std::string("bad arguments");
    if (pa_counts) particles_counts(pa_counts);  // hdg_get_particles: the dropped-rows error below leaves them filled
    const long n = L.n, dropped = L.dropped;
    log_fetch(L, buf, rows, std::min<long>(n, max_rows));
    if (n_rows) *n_rows = (int)n;
    if (reset) L.clear_counts();
    if (dropped > 0)
      throw std::string(label) + ": " + std::to_string(dropped) + " row(s) dropped beyond the capacity of " +
          std::to_string(L.cap) + " rows";
  }
  // every entry has one non-zero contributor: the sum is the owner's value on every rank
  void allreduce_chunked(double* v, int total) {
    const int chunk = comm->allreduce_max();  // the shared-memory transport: 64 per call
    for (int off = 0; off < total; off += chunk) {
      comm->allreduce_sum(v + off, std::min(chunk, total - off), stream);
      n_reduce++;
    }
  }
  // modal copies of nodal host fields (hdg_compute_diagnostics, hdg_evaluate_points): one set, allocated on first use
  double *nodal_Qw = nullptr, *nodal_pw = nullptr, *nodal_qw = nullptr;
  const double* stage_Q(const double* host) {
    if (!host) return nullptr;
    if (!nodal_Qw) nodal_Qw = dalloc(NQ);
    put_Q(host, nodal_Qw);
    return nodal_Qw;
  }
  const double* stage_P(const double* host, double*& w) {
    if (!host) return nullptr;
    if (!w) w = dalloc(NPv);
    put_P(host, w);
    return w;
  }

  // ------------------------------------------------------------------ flow diagnostics (hdg_diagnostics.hpp)
  RowLog diag_log;
  double *diag_part = nullptr, *diag_acc = nullptr, *diag_gat = nullptr, *diag_out = nullptr, *diag_rows = nullptr;
  const double *diag_hmin = nullptr, *diag_gVu = nullptr;  // general meshes: shortest edge per cell, unscaled modal -> nodal
  const int* diag_ecl = nullptr;                            // general meshes: (3 c + l) of the cells of every edge
  int diag_ncb = 0, diag_neb = 0;
  // general meshes: the shortest edge of every cell and the unscaled modal -> nodal matrix (the diagnostics and the step rate)
  void diag_general_geo() {
    if (diag_hmin) return;
    const GMesh& M = *gm;
    dvec hm((size_t)M.nc);
    for (int c = 0; c < M.nc; c++) {
      double h = M.elen[(size_t)M.cedge[3 * (size_t)c]];
      for (int l = 1; l < 3; l++) h = std::min(h, M.elen[(size_t)M.cedge[3 * (size_t)c + l]]);
      hm[(size_t)c] = h;
    }
    diag_hmin = upload(hm);
    diag_gVu = upload(gtab->Vu);
  }
  void diag_alloc() {
    if (diag_part) return;
    if (general) {
      const GMesh& M = *gm;
      diag_ncb = (M.nc + DIAG_BLOCK - 1) / DIAG_BLOCK;
      diag_neb = (M.ne + DIAG_BLOCK - 1) / DIAG_BLOCK;
      std::vector<int> ecl((size_t)2 * M.ne, -1);
      for (int e = 0; e < M.ne; e++)
        for (int sd = 0; sd < 2; sd++) {
          const int c = M.ecell[2 * (size_t)e + sd];
          if (c >= 0) ecl[2 * (size_t)e + sd] = 3 * c + M.elocal[2 * (size_t)e + sd];
        }
      diag_ecl = upload_ints(ecl);
      diag_general_geo();
    } else {
      diag_ncb = (int)cell_grid().x;
      diag_neb = (int)corner_grid().x;
    }
    diag_part = dalloc((long)diag_ncb * DIAG_NPART + 2L * diag_neb);
    diag_acc = dalloc(DIAG_NACC);
    diag_gat = dalloc(2L * comm->size);
    diag_out = dalloc(DIAG_NCOL);
  }
  // the nine columns of (Q, p, q) (modal, device; q may be null) into the device row `row`; Qn: nodal copy of Q in the
  // boundary layout for the maxima (null: from Q)
  void diag_pass(const double* Q, const double* p, const double* q, double* row, const double* Qn = nullptr) {
    diag_alloc();
    if (!row) throw std::string("diagnostics: no row buffer");
    double* cpart = diag_part;
    double* epart = diag_part + (long)diag_ncb * DIAG_NPART;
    tally(LC_OTHER, bQ() + bP() * (q ? 2.0 : 1.0));
    if (general) {
      by_degree([&](auto k) { k_g_diag_cell<k()><<<diag_ncb, DIAG_BLOCK, 0, stream>>>(ggeo, diag_gVu, diag_hmin, Q, p, q, Qn, cpart); });
      tally(LC_OTHER, 2.0 * bQ());
      by_degree([&](auto k) { k_g_diag_edge<k()><<<diag_neb, DIAG_BLOCK, 0, stream>>>(ggeo, gm->ne, diag_ecl, Q, epart); });
    } else {
      by_degree([&](auto k) { k_diag_cell<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt, Q, p, q, Qn, cpart); });
      halo_Q(Q);  // the edges of the strip's bottom row (and the periodic wrap) read the neighbour's cells
      tally(LC_OTHER, 3.0 * bQ());
      by_degree([&](auto k) { k_diag_edge<k()><<<corner_grid(), bs(), 0, stream>>>(g, dt, Q, epart); });
    }
    tally(LC_OTHER, 0.0);
    k_diag_reduce<<<1, 1024, 0, stream>>>(diag_ncb, cpart, diag_neb, epart, diag_acc);
    const double* mxs = diag_acc + 7;
    if (comm->size > 1) {  // sums over the owned cells and edges of every rank; maxima gathered, taken by k_diag_row
      comm->allreduce_sum(diag_acc, 7, stream);
      comm->allgather(diag_acc + 7, diag_gat, 2, stream);
      n_reduce++; n_gather++;
      mxs = diag_gat;
    }
    tally(LC_OTHER, 0.0);
    k_diag_row<<<1, 64, 0, stream>>>(diag_acc, mxs, comm->size, cfg.dt, q ? 1 : 0, row);
  }
  // end of a completed step: one row of the current state
  void diag_record() {
    if (double* row = log_next(diag_log, diag_rows)) diag_pass(curQ, curP, tracer_on ? q_cur : nullptr, row);
  }
  void diag_set(int cap) {
    if (cap < 0) throw std::string("diagnostics capacity must be >= 0");
    log_size(diag_log, diag_rows, DIAG_NCOL, cap);
    diag_record();  // row 0: the state as it is now
  }
  void diag_compute(const double* Q, const double* p, const double* q, double* out) {
    diag_alloc();  // before diag_out is read below
    const double* qw = stage_P(q, nodal_qw);
    const double* pw = stage_P(p, nodal_pw);
    const double* Qw = stage_Q(Q);  // last: the staging buffer hQ_dev keeps the nodal velocity for the maxima
    diag_pass(Qw, pw, qw, diag_out, hQ_dev);
    HIPCHECK(hipMemcpyAsync(out, diag_out, sizeof(double) * DIAG_NCOL, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }

  // ------------------------------------------------------------------ point values (hdg_points.hpp, hdg_probes.hpp)
  // A point set is located on the host once (every rank locates every point, the same way) into a device table; one launch
  // per row evaluates it (strip partitions: one all-reduce sum of the row).  Probe recording appends one row per completed
  // step at end_of_step, next to the diagnostics row.
  struct PointSet {
    int n = 0, alloc = 0;
    PointLoc* dev = nullptr;
  };
  PointSet pt_eval, pt_probe;
  GLocator* glocator = nullptr;
  RowLog probe_log;
  std::vector<double> pt_probe_xy;
  double *pt_out = nullptr, *pt_rows = nullptr;
  long pt_out_alloc = 0;
  // located[i] = 1 / 0; throws nothing for an outside point (PT_OUTSIDE)
  void points_locate(int n, const double* xy, PointSet& ps, int* located) {
    if (n < 0 || (n > 0 && !xy)) throw std::string("points: bad arguments");
    std::vector<PointLoc> loc((size_t)n);
    if (general && !glocator) { glocator = new GLocator(); glocator->build(*gm); }
    for (int t = 0; t < n; t++) {
      PointLoc& L = loc[(size_t)t];
      L.xi = L.eta = 0.0; L.c = 0; L.s = PT_OUTSIDE; L.pad = 0;
      const double x = xy[2 * (size_t)t], y = xy[2 * (size_t)t + 1];
      if (general) {
        const int c = glocator->locate(*gm, x, y, POINT_TOL, L.xi, L.eta);
        if (c >= 0) { L.c = c; L.s = 0; }
      } else {
        int i, j, s;
        if (square_locate(x, y, g.nx, cfg.ny, Ldom, periodic, i, j, s, L.xi, L.eta)) {
          const int r = j / g.ny;  // the rank that owns cell row j
          if (r == comm->rank) { L.c = ((long)s * g.R + (j - r * g.ny + GH)) * g.nx + i; L.s = s; }
          else L.s = PT_OTHER_RANK;
        }
      }
      if (located) located[t] = L.s == PT_OUTSIDE ? 0 : 1;
    }
    if (n > ps.alloc) {
      ps.dev = (PointLoc*)dalloc(((long)n * sizeof(PointLoc) + 7) / 8);
      ps.alloc = n;
    }
    ps.n = n;
    if (n > 0) {
      HIPCHECK(hipMemcpyAsync(ps.dev, loc.data(), sizeof(PointLoc) * (size_t)n, hipMemcpyHostToDevice, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
  // one row (ps.n x POINT_NCOL) of the modal device fields Q, p, q (any may be null: NaN columns) into the device row `row`
  void points_pass(const PointSet& ps, const double* Q, const double* p, const double* q, double* row) {
    if (ps.n == 0) return;
    const int nb = (ps.n + POINT_BLOCK - 1) / POINT_BLOCK;
    tally(LC_OTHER, 0.0);
    if (general) {
      by_degree([&](auto k) { k_g_point_eval<k()><<<nb, POINT_BLOCK, 0, stream>>>(ggeo, ps.n, ps.dev, Q, p, q, row); });
    } else {
      by_degree([&](auto k) { k_point_eval<k()><<<nb, POINT_BLOCK, 0, stream>>>(ps.n, ps.dev, g.Nc, g.h, Q, p, q, row); });
    }
    if (comm->size > 1) allreduce_chunked(row, POINT_NCOL * ps.n);
  }
  void points_evaluate(const double* Q, const double* p, const double* q, int n, const double* xy, double* out, int* located) {
    points_locate(n, xy, pt_eval, located);
    if ((long)n * POINT_NCOL > pt_out_alloc) { pt_out = dalloc((long)n * POINT_NCOL); pt_out_alloc = (long)n * POINT_NCOL; }
    const double* Qw = stage_Q(Q);
    const double* pw = stage_P(p, nodal_pw);
    const double* qw = stage_P(q, nodal_qw);
    points_pass(pt_eval, Qw, pw, qw, pt_out);
    if (n > 0) HIPCHECK(hipMemcpyAsync(out, pt_out, sizeof(double) * POINT_NCOL * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void probe_record() {
    if (double* row = log_next(probe_log, pt_rows)) points_pass(pt_probe, curQ, curP, tracer_on ? q_cur : nullptr, row);
  }
  void probe_set(int n, const double* xy, int cap) {
    if (n < 0 || cap < 0) throw std::string("probes: n and capacity must be >= 0");
    probe_log.reset(0, 0);
    pt_probe_xy.clear();
    if (n == 0 || cap == 0) { pt_probe.n = 0; return; }
    if ((double)n * cap * POINT_NCOL > (double)HDG_MAX_PROBE_VALUES)
      throw std::string("probes: ") + std::to_string(n) + " points x " + std::to_string(cap) + " rows x " +
          std::to_string(POINT_NCOL) + " values exceed the limit of " + std::to_string((long)HDG_MAX_PROBE_VALUES) + " values";
    std::vector<int> located((size_t)n);
    points_locate(n, xy, pt_probe, located.data());
    for (int t = 0; t < n; t++)
      if (!located[(size_t)t]) {
        pt_probe.n = 0;
        throw std::string("probes: point ") + std::to_string(t) + " (" + std::to_string(xy[2 * (size_t)t]) + ", " +
            std::to_string(xy[2 * (size_t)t + 1]) + ") lies outside the domain";
      }
    log_size(probe_log, pt_rows, (long)POINT_NCOL * n, cap);
    pt_probe_xy.assign(xy, xy + 2 * (size_t)n);  // a checkpoint stores the points; a load locates them again
    probe_record();  // row 0: the state as it is now
  }

  // ------------------------------------------------------------------ Lagrangian particles (hdg_particles.hpp)
  // Positions X, predictor X*, k1 (and, on strips, the k2 of the sum) live on the device beside the probe state; one launch
  // per completed step at end_of_step advances them (strips: three launches around two all-reduce sums of 2 n values,
  // every rank holding all positions and doing the same update).  Switched off: pa_n == 0, and the work vectors X, X*,
  // k1, k2 and the counters are freed (the row buffer follows the rule of hdg_row_log.hpp).
  RowLog pa_log;
  int pa_n = 0, pa_every = 1;
  long pa_steps = 0;
  double *pa_X = nullptr, *pa_Xs = nullptr, *pa_k1 = nullptr, *pa_k2 = nullptr, *pa_rows = nullptr, *pa_cnt = nullptr;
  ParticleGeo particle_geo() const {
    ParticleGeo G;
    G.nx = g.nx; G.ny = cfg.ny; G.j0 = comm->rank * g.ny; G.nyl = g.ny; G.periodic = periodic ? 1 : 0;
    G.R = g.R; G.Nc = g.Nc; G.L = Ldom; G.h = g.h;
    return G;
  }
  void particles_launch(int phase, int nsteps, double dt, double* row) {
    const int nb = (pa_n + PARTICLE_BLOCK - 1) / PARTICLE_BLOCK;
    const ParticleGeo G = particle_geo();
    unsigned long long* cnt = (unsigned long long*)pa_cnt;
    tally(LC_OTHER, 0.0);
    by_degree([&](auto k) {
      k_particles_step<k()><<<nb, PARTICLE_BLOCK, 0, stream>>>(G, pa_n, phase, nsteps, dt, curQ, pa_X, pa_Xs, pa_k1, pa_k2, row, cnt);
    });
  }
  // k1 = u(X) of the current velocity and X* = X + dt k1
  void particles_predict(double dt) {
    if (pa_n == 0) return;
    if (comm->size == 1) { particles_launch(PF_EVAL_X | PF_PREDICT, 1, dt, nullptr); return; }
    particles_launch(PF_EVAL_X, 1, dt, nullptr);
    allreduce_chunked(pa_k1, 2 * pa_n);
    particles_launch(PF_PREDICT, 1, dt, nullptr);
  }
  // nsteps Heun steps of size dt through the current velocity (k1 and X* of the same dt are in place); row: where the last
  // position goes (null: nowhere).  nsteps > 1: the field is frozen, k2 of a step and k1 of the next use the same one
  void particles_advance(double dt, int nsteps, double* row) {
    if (pa_n == 0 || nsteps <= 0) return;
    if (comm->size == 1) { particles_launch(PF_STEP, nsteps, dt, row); return; }
    for (int it = 0; it < nsteps; it++) {
      particles_launch(PF_EVAL_STAR, 1, dt, nullptr);
      allreduce_chunked(pa_k2, 2 * pa_n);
      particles_launch(PF_CORRECT | PF_EVAL_X, 1, dt, it == nsteps - 1 ? row : nullptr);
      allreduce_chunked(pa_k1, 2 * pa_n);
      particles_launch(PF_PREDICT, 1, dt, nullptr);
    }
  }
  double* particles_next_row() { return log_next(pa_log, pa_rows); }
  // end of a completed step: X^{n+1} from k1, X* and the new velocity; then k1 and X* of the next step
  void particles_step() {
    if (pa_n == 0) return;
    pa_steps++;
    particles_advance(cfg.dt, 1, pa_steps % pa_every == 0 ? particles_next_row() : nullptr);
  }
  void particles_off() {
    pa_n = 0; pa_steps = 0; pa_every = 1;
    pa_log.reset(0, 0);
    dfree(pa_X); dfree(pa_Xs); dfree(pa_k1); dfree(pa_k2); dfree(pa_cnt);
  }
  void particles_set(int n, const double* xy, int cap, int every) {
    if (n < 0 || cap < 0) throw std::string("particles: n and capacity must be >= 0");
    if (every < 1) throw std::string("particles: record_every must be >= 1");
    particles_off();
    if (n == 0 || cap == 0) return;
    if (2.0 * n * cap > (double)HDG_MAX_PROBE_VALUES)
      throw std::string("particles: ") + std::to_string(n) + " particles x " + std::to_string(cap) + " rows x 2 values exceed " +
          "the limit of " + std::to_string((long)HDG_MAX_PROBE_VALUES) + " values";
    for (int t = 0; t < n; t++) {
      int i, j, sh;
      double xi, eta;
      if (!square_locate(xy[2 * (size_t)t], xy[2 * (size_t)t + 1], g.nx, cfg.ny, Ldom, periodic, i, j, sh, xi, eta))
        throw std::string("particles: seed ") + std::to_string(t) + " (" + std::to_string(xy[2 * (size_t)t]) + ", " +
            std::to_string(xy[2 * (size_t)t + 1]) + ") lies outside the domain";
    }
    pa_X = dalloc(2L * n); pa_Xs = dalloc(2L * n); pa_k1 = dalloc(2L * n);
    if (comm->size > 1) pa_k2 = dalloc(2L * n);
    log_size(pa_log, pa_rows, 2L * n, cap);
    pa_cnt = dalloc(PARTICLE_NCOUNT);  // two 64-bit counters, zeroed
    pa_n = n; pa_every = every;
    // seeds within the location tolerance of the unit square are clamped onto it like every later position
    std::vector<double> seeds(xy, xy + 2 * (size_t)n);
    if (!periodic)
      for (double& v : seeds) v = std::fmin(std::fmax(v, 0.0), Ldom);
    HIPCHECK(hipMemcpyAsync(pa_X, seeds.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(particles_next_row(), seeds.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));  // seeds is a host temporary
    particles_predict(cfg.dt);
  }
  // the velocity changed under the particles (hdg_set_state): a stale k1 is never used
  void particles_refresh() { particles_predict(cfg.dt); }
  void particles_frozen(double dt, int nsteps) {
    if (pa_n == 0) throw std::string("particles: none set (hdg_set_particles)");
    if (!std::isfinite(dt) || nsteps < 0) throw std::string("particles: dt must be finite and nsteps >= 0");
    if (nsteps == 0) return;
    particles_launch(PF_PREDICT, 1, dt, nullptr);  // X* of this dt from the k1 in place
    particles_advance(dt, nsteps, particles_next_row());
    particles_predict(cfg.dt);  // back to the predictor of the flow's own step
  }
  // clamped updates, lost particles, dropped rows
  void particles_counts(long* counts) {
    unsigned long long c[PARTICLE_NCOUNT] = {0, 0};
    if (pa_n > 0) HIPCHECK(hipMemcpyAsync(c, pa_cnt, sizeof(c), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    counts[0] = (long)c[0]; counts[1] = (long)c[1]; counts[2] = pa_log.dropped;
  }
  // end of a completed step: the diagnostics row and the probe row of the same state, then the particles
  void end_of_step() {
    diag_record();
    probe_record();
    particles_step();
  }

  // ------------------------------------------------------------------ adaptive time step (hdg_step_rate.hpp, hdg_step_control.hpp;
  // DESIGN.md section 25).  cfg.dt is read where it is used -- gamma = a_ii dt at the solve sites, the stage coefficients of
  // hdg_stage_coeffs.hpp, the three stability reports -- and ensure_dinv follows gamma, so a new dt is a new cfg.dt and what
  // remembers the old one: the Chebyshev history of the stages and the predictor of the particles.
  double* d_rate = nullptr;  // word 0: this rank's maximum as a bit pattern; words 1 .. size: the gathered ones (strips);
                             // behind them one word per workgroup of the rate kernel
  // The monolithic and the DG step key a preconditioner set by tau / dt (get_pset): the sets of the step sizes left behind are
  // freed, so an adaptive run holds the set of the construction and that of the dt in use.  Structured meshes only: on a
  // general mesh a set is an assembled operator set with its algebraic hierarchy, which is kept.
  void drop_other_psets() {
    if (general || psets.size() <= 1) return;
    for (size_t i = 1; i < psets.size(); i++) {
      PSet& ps = psets[i];
      for (int sh = 0; sh < 2; sh++) {
        release_dev(ps.dt.Ainv[sh]); release_dev(ps.dt.W[sh]); release_dev(ps.dt.Y[sh]); release_dev(ps.dt.SK[sh]);
        release_dev(ps.bsm[sh]);
      }
      for (int t = 0; t < 3; t++) for (int vv = 0; vv < 3; vv++) release_dev(ps.dt.trDinv[t][vv]);
      release_dev(ps.cdm);
    }
    psets.resize(1);
    use_pset(0);
  }
  void set_dt(double v) {
    if (!std::isfinite(v) || !(v > 0.0)) throw std::string("hdg_set_dt: dt = " + std::to_string(v) + " is not a finite value > 0");
    if (step_open) throw std::string("hdg_set_dt: a step is open (between hdg_begin_step and the end of the step)");
    if (v == cfg.dt) return;  // nothing at all: the steps after it are those of a run without the call
    cfg.dt = v;
    ch.assign((size_t)s + 1, ChebStage{});
    drop_other_psets();
    if (pa_n > 0) particles_launch(PF_PREDICT, 1, v, nullptr);  // X* of this dt from the k1 in place
  }
  // A = max_K (max nodal |u| in K) / h_K of the modal device velocity Q: NaN when it is not finite anywhere
  double advective_rate(const double* Q) {
    const int nb = general ? (gm->nc + STEP_RATE_BLOCK - 1) / STEP_RATE_BLOCK : (int)cell_grid().x;
    if (!d_rate) d_rate = dalloc(1L + comm->size + nb);
    unsigned long long* word = (unsigned long long*)d_rate;
    unsigned long long* part = word + 1 + comm->size;
    tally(LC_OTHER, bQ());
    if (general) {
      diag_general_geo();
      by_degree([&](auto k) { k_g_step_rate<k()><<<nb, STEP_RATE_BLOCK, 0, stream>>>(gm->nc, ggeo.inv_sdet, diag_gVu, diag_hmin, Q, part); });
    } else {
      by_degree([&](auto k) { k_step_rate<k()><<<cell_grid(), bs(), 0, stream>>>(g, dt.Vu, Q, part); });
    }
    tally(LC_OTHER, 0.0);
    k_step_rate_reduce<<<1, 1024, 0, stream>>>(nb, part, word);
    const double* src = d_rate;
    if (comm->size > 1) {  // the maxima of every rank, gathered as the diagnostics gather theirs; taken below
      comm->allgather(d_rate, d_rate + 1, 1, stream);
      n_gather++;
      src = d_rate + 1;
    }
    std::vector<unsigned long long> bits((size_t)comm->size);
    HIPCHECK(hipMemcpyAsync(bits.data(), src, sizeof(unsigned long long) * bits.size(), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    const unsigned long long top = *std::max_element(bits.begin(), bits.end());
    if (top > 0x7ff0000000000000ull) return std::numeric_limits<double>::quiet_NaN();  // a NaN pattern, of either sign
    double A;
    std::memcpy(&A, &top, sizeof(A));
    return A;
  }
  // the four rates whose product with dt has to stay bounded; [1..3] are what the three reports multiply by dt
  void step_rates(double* rates) {
    if (step_open) throw std::string("hdg_get_step_rates: a step is open (between hdg_begin_step and the end of the step)");
    rates[0] = advective_rate(curQ);
    rates[1] = rates[2] = rates[3] = 0.0;
    double kmax = 0.0;
    for (double x : tr_kappa) kmax = std::max(kmax, x);
    double out2[2];
    if (kmax > 0.0 && !tdi_mode) { tracer_diffusion_number(out2); rates[1] = kmax * out2[0]; }  // implicit: no limit (section 28)
    if (visc_nu > 0.0) { viscosity_number(visc_nu, visc_wall, out2); rates[2] = visc_nu * out2[0]; }
    if (drag_on()) rates[2] += drag_S;  // both spectra are real and non-positive: the rates add (section 26)
    if (cor_f0 != 0.0 || cor_beta != 0.0) rates[3] = coriolis_bound(cor_f0, cor_beta);
  }
  double propose_dt(const hdg_step_control& control, double t, double t_final) {
    if (!step_control_valid(control))
      throw std::string("hdg_propose_dt: cfl must be > 0 and no field of the control may be negative or NaN");
    if (!std::isfinite(t) || !std::isfinite(t_final)) throw std::string("hdg_propose_dt: t and t_final must be finite");
    double rates[4], p;
    step_rates(rates);
    switch (step_proposal(control, rates[0], cfg.dt, t, t_final, p)) {
      case StepVerdict::Ok: break;
      case StepVerdict::NotFinite: throw NotConverged{"hdg_propose_dt: velocity is not finite"};
      case StepVerdict::BelowMin: {
        char buf[160];
        snprintf(buf, sizeof(buf), "hdg_propose_dt: the proposal dt = %.17g is below dt_min = %.17g", p, control.dt_min);
        throw std::string(buf);
      }
      case StepVerdict::BadControl: throw std::string("hdg_propose_dt: bad control");
    }
    return p;
  }

  // ------------------------------------------------------------------ checkpoint and restart (hdg_checkpoint.hpp)
  // After checkpoint_load the engine is the engine that was saved: every vector a later step or getter reads before it is
  // written, stored raw (ghost and padding rows included) BY ROLE -- begin_step exchanges stQ[0] and curQ, the Chebyshev
  // iteration Qtent[i] and chd -- plus the host history of the solvers and the three row logs.  Timers and the launch census are
  // not state: they start at zero.  Tables built from the configuration alone (ensure_dinv, get_pset, the dense V-cycle tails,
  // the matrix-core packs, estimate_cheb with its fixed seed) are set-up: a restored engine builds them again on first use.
  bool step_open = false;  // between hdg_begin_step and the end of the step: no save
  int ck_mesh_nv = 0, ck_mesh_nc = 0;
  ckpt::Digest ck_mesh_coords, ck_mesh_cells;
  unsigned long long *dig_part = nullptr, *dig_out = nullptr;
  static constexpr int DIG_SLOTS = 256;  // results of one batch of digests (one per section)
  // digest of the n doubles at v (device) into result slot `slot`: two launches on the stream, no synchronisation
  void digest_launch(const double* v, long n, int slot) {
    if (n < 0 || slot < 0 || slot >= DIG_SLOTS) throw std::string("digest: bad arguments");
    if (n > 0 && (!v || (reinterpret_cast<uintptr_t>(v) & 15))) throw std::string("digest: the vector must be 16-byte aligned");
    if (!dig_part) {
      dig_part = reinterpret_cast<unsigned long long*>(dalloc(2L * HDG_DIGEST_MAX_BLOCKS));
      dig_out = reinterpret_cast<unsigned long long*>(dalloc(2L * DIG_SLOTS));
    }
    const int nb = (int)std::min<long>(vec_blocks(n), HDG_DIGEST_MAX_BLOCKS);
    tally(LC_OTHER, 8.0 * (double)n);
    k_digest<<<nb, HDG_DIGEST_BLOCK, 0, stream>>>(n, reinterpret_cast<const unsigned long long*>(v), dig_part);
    tally(LC_OTHER, 0.0);
    k_digest_final<<<1, HDG_DIGEST_BLOCK, 0, stream>>>(nb, dig_part, dig_out + 2 * slot);
  }
  void digest_fetch(int nslots, std::vector<ckpt::Digest>& out) {
    std::vector<unsigned long long> h(2 * (size_t)std::max(nslots, 1), 0ULL);
    if (nslots > 0) HIPCHECK(hipMemcpyAsync(h.data(), dig_out, sizeof(unsigned long long) * 2 * (size_t)nslots, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    out.resize((size_t)nslots);
    for (int q = 0; q < nslots; q++) { out[(size_t)q].d0 = h[2 * (size_t)q]; out[(size_t)q].d1 = h[2 * (size_t)q + 1]; }
  }
  // hdg_digest_vector: a host vector through the device kernel (operator hook)
  void digest_host_vector(const double* v, long n, unsigned long long* out) {
    if (n < 0 || (n > 0 && !v) || !out) throw std::string("digest: bad arguments");
    double* d = dalloc(n);
    if (n > 0) HIPCHECK(hipMemcpyAsync(d, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
    digest_launch(d, n, 0);
    std::vector<ckpt::Digest> r;
    digest_fetch(1, r);
    dfree(d);
    out[0] = r[0].d0; out[1] = r[0].d1;
  }

  // the host part of the state
  struct CkHost {
    std::vector<ChebStage> ch;  // empty before the first Chebyshev solve
    std::vector<double> bscale;
    std::vector<int> bsep;
    double it_sum[4] = {0, 0, 0, 0};
    long it_cnt[4] = {0, 0, 0, 0}, ev[4] = {0, 0, 0, 0};
    double trace_scale = 0.0;
    int tracer_on = 0, tracer_vecs = 0, has_chd = 0;
    long log[3][4] = {{0}};  // width, cap, n, dropped of the diagnostics, probe and particle logs
    std::vector<double> probe_xy;
    int pa_n = 0, pa_every = 1;
    long pa_steps = 0;
  };
  CkHost ck_capture() const {
    CkHost h;
    if (!cheb_history_empty(ch)) h.ch = ch;
    h.bscale = bscale; h.bsep = bsep;
    for (int q = 0; q < 4; q++) { h.it_sum[q] = it_sum[q]; h.it_cnt[q] = it_cnt[q]; }
    h.ev[0] = ev_cg_replacements; h.ev[1] = ev_cg_floor_exits; h.ev[2] = n_sstep_cycles; h.ev[3] = n_sstep_fallbacks;
    h.trace_scale = trace_scale;
    // Only what can be observed is state: the tracer vectors while a tracer is on (switched off, nothing reads them before
    // hdg_set_tracer has written them again), a row log while it records (switched off, its width is what the last user left).
    // So a run that recorded diagnostics and a run that did not end in the same state, with the same digest.
    h.tracer_on = tracer_on ? 1 : 0; h.tracer_vecs = tracer_on ? 1 : 0; h.has_chd = chd ? 1 : 0;
    const RowLog* L[3] = {&diag_log, &probe_log, &pa_log};
    for (int q = 0; q < 3; q++)
      if (L[q]->cap > 0) { h.log[q][0] = L[q]->width; h.log[q][1] = L[q]->cap; h.log[q][2] = L[q]->n; h.log[q][3] = L[q]->dropped; }
    if (pt_probe.n > 0) h.probe_xy = pt_probe_xy;
    h.pa_n = pa_n; h.pa_every = pa_every; h.pa_steps = pa_steps;
    return h;
  }
  static void ck_write_host(const CkHost& h, ckpt::ByteWriter& solver, ckpt::ByteWriter& outputs) {
    write_cheb_stages(solver, h.ch); solver.vec(h.bscale); solver.vec(h.bsep);
    solver.raw(h.it_sum, sizeof(h.it_sum)); solver.raw(h.it_cnt, sizeof(h.it_cnt)); solver.raw(h.ev, sizeof(h.ev));
    solver.put(h.trace_scale); solver.put(h.tracer_on); solver.put(h.tracer_vecs); solver.put(h.has_chd);
    outputs.raw(h.log, sizeof(h.log)); outputs.vec(h.probe_xy); outputs.put(h.pa_n); outputs.put(h.pa_every); outputs.put(h.pa_steps);
  }
  // empty return: read; otherwise what is wrong with the record
  std::string ck_read_host(CkHost& h, const void* solver, size_t ns, const void* outputs, size_t no) const {
    ckpt::ByteReader a(solver, ns), b(outputs, no);
    const std::string cheb_err = read_cheb_stages(a, (size_t)s + 1, h.ch);
    a.vec(h.bscale); a.vec(h.bsep);
    a.raw(h.it_sum, sizeof(h.it_sum)); a.raw(h.it_cnt, sizeof(h.it_cnt)); a.raw(h.ev, sizeof(h.ev));
    h.trace_scale = a.get<double>(); h.tracer_on = a.get<int>(); h.tracer_vecs = a.get<int>(); h.has_chd = a.get<int>();
    if (!a.done()) return "section 'solver': the record does not have the length its fields need";
    b.raw(h.log, sizeof(h.log)); b.vec(h.probe_xy); h.pa_n = b.get<int>(); h.pa_every = b.get<int>(); h.pa_steps = b.get<long>();
    if (!b.done()) return "section 'outputs': the record does not have the length its fields need";
    if (!cheb_err.empty()) return cheb_err;
    if (h.bscale.size() != (size_t)s + 1 || h.bsep.size() != (size_t)s + 1) return "section 'solver': forcing scales of another stage count";
    for (int q = 0; q < 3; q++)
      if (h.log[q][0] < 0 || h.log[q][1] < 0 || h.log[q][2] < 0 || h.log[q][2] > h.log[q][1] || h.log[q][3] < 0 ||
          (double)h.log[q][0] * (double)h.log[q][1] > 4.0 * (double)HDG_MAX_PROBE_VALUES)
        return "section 'outputs': row log " + std::to_string(q) + " has impossible counts";
    if (h.pa_n < 0 || h.pa_every < 1 || h.pa_steps < 0 || (h.pa_n > 0 && h.log[2][0] != 2L * h.pa_n)) return "section 'outputs': particle counts";
    if (h.pa_n > 0 && general) return "section 'outputs': particles on a general mesh";
    if (h.probe_xy.size() % 2 != 0 || (!h.probe_xy.empty() && h.log[1][0] != (long)POINT_NCOL * (long)(h.probe_xy.size() / 2)))
      return "section 'outputs': probe points do not match the width of the probe log";
    if (h.tracer_vecs && comm->size > 1) return "section 'solver': a tracer on a strip partition";
    return "";
  }
  // the device sections of a state whose host part is hs, in blob order; ptr() is called once the vectors exist
  struct CkDev { std::string id; long n; std::function<double*()> ptr; };
  std::vector<CkDev> ck_device_sections(const CkHost& hs) {
    std::vector<CkDev> v;
    auto add = [&](const std::string& id, long n, std::function<double*()> f) { v.push_back(CkDev{id, n, std::move(f)}); };
    auto idx = [](const char* base, int i) { return std::string(base) + std::to_string(i); };
    add("curQ", NQ, [this] { return curQ; }); add("curP", NPv, [this] { return curP; }); add("curL", NLv, [this] { return curL; });
    for (int i = 0; i < s; i++) {
      add(idx("stQ", i), NQ, [this, i] { return stQ[(size_t)i]; });
      add(idx("stP", i), NPv, [this, i] { return stP[(size_t)i]; });
      add(idx("stL", i), NLv, [this, i] { return stL[(size_t)i]; });
      add(idx("Qtent", i), NQ, [this, i] { return Qtent[(size_t)i]; });
    }
    for (int i = 0; i < (int)Qstar.size(); i++) add(idx("Qstar", i), NQ, [this, i] { return Qstar[(size_t)i]; });
    for (int i = 0; i <= s; i++) add(idx("brhs", i), NQ, [this, i] { return brhs[(size_t)i]; });
    add("profile", NQ, [this] { return profile; });
    add("updU", NQ, [this] { return updU; }); add("updP", NPv, [this] { return updP; }); add("updL", NLv, [this] { return updL; });
    add("recP", NPv, [this] { return recP; }); add("recL", NLv, [this] { return recL; });
    if (hs.has_chd) add("chd", NQ, [this] { return chd; });
    if (comm->size > 1) {
      // Strips: the work vectors of the solvers are state as well.  A stencil writes as many ghost rows as its inputs allow and
      // leaves the rest of a work vector as earlier solves left it; the whole-array updates (x += V y, the s-step update)
      // carry those stale rows into the ghost rows of Qtent[i] and from there into stQ[i].  No owned value ever depends on
      // them (the bookkeeping exchanges before a stencil reads), but the raw vectors, and with them the state digest, do.
      // On one rank there is nothing to carry: ghost rows are never written (unit square) or rewritten by the wrap before
      // every use (periodic square).
      add("wQ1", NQ, [this] { return wQ1; }); add("wQ2", NQ, [this] { return wQ2; });
      add("wQ3", NQ, [this] { return wQ3; }); add("wQ4", NQ, [this] { return wQ4; });
      for (int i = 0; i < (int)gm_V.size(); i++) add(idx("gm_V", i), NQ, [this, i] { return gm_V[(size_t)i]; });
      add("wP1", NPv, [this] { return wP1; }); add("wL1", NLv, [this] { return wL1; }); add("wL2", NLv, [this] { return wL2; });
      add("cg_r", NLv, [this] { return cg_r; }); add("cg_z", NLv, [this] { return cg_z; }); add("cg_p", NLv, [this] { return cg_p; });
      add("cg_Ap", NLv, [this] { return cg_Ap; }); add("ch_d", NLv, [this] { return ch_d; }); add("ch_r", NLv, [this] { return ch_r; });
    }
    if (hs.tracer_vecs) {
      add("q_cur", NTv(), [this] { return q_cur; }); add("q_fin", NTv(), [this] { return q_fin; });
      for (int i = 0; i < s; i++) add(idx("q_st", i), NTv(), [this, i] { return q_st[(size_t)i]; });
    }
    if (hs.pa_n > 0) {
      add("pa_X", 2L * hs.pa_n, [this] { return pa_X; }); add("pa_Xs", 2L * hs.pa_n, [this] { return pa_Xs; });
      add("pa_k1", 2L * hs.pa_n, [this] { return pa_k1; });
      if (comm->size > 1) add("pa_k2", 2L * hs.pa_n, [this] { return pa_k2; });
      add("pa_cnt", PARTICLE_NCOUNT, [this] { return pa_cnt; });
    }
    // the rows written so far
    if (hs.log[0][2] > 0) add("diag_rows", hs.log[0][0] * hs.log[0][2], [this] { return diag_rows; });
    if (hs.log[1][2] > 0) add("probe_rows", hs.log[1][0] * hs.log[1][2], [this] { return pt_rows; });
    if (hs.log[2][2] > 0) add("particle_rows", hs.log[2][0] * hs.log[2][2], [this] { return pa_rows; });
    if ((int)v.size() > DIG_SLOTS) throw std::string("checkpoint: too many sections");
    return v;
  }
  // what a checkpoint is bound to.  hdg_config::device is left out: where a run is computed is not part of what it computes
  ckpt::Fingerprint ck_fingerprint() const {
    ckpt::Fingerprint f;
    f.add("engine_kind", (long)(general ? 2 : (comm->size > 1 ? 1 : 0)));  // hdg_create / hdg_create_distributed / hdg_create_general
    f.add("mesh_kind", (long)(general ? 2 : (periodic ? 1 : 0)));
    f.add("nx", (long)cfg.nx); f.add("ny", (long)cfg.ny); f.add("degree", (long)cfg.degree); f.add("dt", cfg.dt);
    f.add("flux_upwind", (long)cfg.flux_upwind); f.add("use_projection", (long)cfg.use_projection);
    f.add("n_richardson", (long)cfg.n_richardson); f.add("tau", cfg.tau); f.add("alpha_penalty", cfg.alpha_penalty);
    f.add("nstages", (long)cfg.nstages);
    auto arr = [&](const char* name, const double* a, int n) { for (int q = 0; q < n; q++) f.add(std::string(name) + "[" + std::to_string(q) + "]", a[q]); };
    arr("a_expl", cfg.a_expl, HDG_MAX_STAGES * HDG_MAX_STAGES); arr("a_impl", cfg.a_impl, HDG_MAX_STAGES * HDG_MAX_STAGES);
    arr("b_expl", cfg.b_expl, HDG_MAX_STAGES); arr("b_impl", cfg.b_impl, HDG_MAX_STAGES + 1); arr("c_expl", cfg.c_expl, HDG_MAX_STAGES);
    f.add("equispaced_nodes", (long)cfg.equispaced_nodes); f.add("tent_rtol", cfg.tent_rtol); f.add("tent_maxit", (long)cfg.tent_maxit);
    f.add("gmres_restart", (long)cfg.gmres_restart); f.add("tent_precond", (long)cfg.tent_precond); f.add("tent_solver", (long)cfg.tent_solver);
    f.add("trace_rtol", cfg.trace_rtol); f.add("trace_maxit", (long)cfg.trace_maxit); f.add("trace_precond", (long)cfg.trace_precond);
    f.add("unsplit_rtol", cfg.unsplit_rtol); f.add("unsplit_inner_rtol", cfg.unsplit_inner_rtol);
    f.add("unsplit_restart", (long)cfg.unsplit_restart); f.add("unsplit_maxit", (long)cfg.unsplit_maxit);
    f.add("periodic", (long)cfg.periodic); f.add("length", cfg.length);
    f.add("dg_rtol", cfg.dg_rtol); f.add("dg_restart", (long)cfg.dg_restart); f.add("dg_maxit", (long)cfg.dg_maxit);
    f.add("n_tracers", (long)cfg.n_tracers);
    for (size_t t = 0; t < tr_kappa.size(); t++) f.add("tracer_kappa[" + std::to_string(t) + "]", tr_kappa[t]);  // only with some kappa != 0
    for (size_t m = 0; m < tw_kind.size(); m++)  // one line per (tracer, side) with a fixed value, and only then
      if (tw_kind[m]) f.add("tracer_wall[" + std::to_string(m / 4) + "][" + std::to_string(m % 4) + "]", tw_val[m]);
    if (tdi_mode) f.add("tracer_diffusion_mode", (long)tdi_mode);  // only in implicit mode (section 28)
    for (size_t t = 0; t < by_beta.size(); t++) f.add("buoyancy_beta[" + std::to_string(t) + "]", by_beta[t]);  // only with some beta != 0
    if (!by_beta.empty()) { f.add("gravity[0]", by_g[0]); f.add("gravity[1]", by_g[1]); }
    if (viscosity_on()) { f.add("viscosity", visc_nu); f.add("viscosity_wall", (long)visc_wall); }  // only with nu != 0
    if (coriolis_on()) { f.add("coriolis_f0", cor_f0); f.add("coriolis_beta", cor_beta); }  // only with one of them != 0
    if (drag_on()) {  // only while the term is on: the setting as it was given, by its digests (section 26)
      f.add_u64("drag_sigma_d0", drag_dig[0].d0); f.add_u64("drag_sigma_d1", drag_dig[0].d1);
      if (drag_has_target) { f.add_u64("drag_target_d0", drag_dig[1].d0); f.add_u64("drag_target_d1", drag_dig[1].d1); }
      f.add_u64("drag_region_d0", drag_dig[2].d0); f.add_u64("drag_region_d1", drag_dig[2].d1);
    }
    for (int w = 0; w < 4; w++)  // one line per side with a wall speed, and only then
      if (wall_u[w] != 0.0) f.add("wall_velocity[" + std::to_string(w) + "]", wall_u[w]);
    if (general) {
      f.add("n_vertices", (long)ck_mesh_nv); f.add("n_cells", (long)ck_mesh_nc);
      f.add_u64("coords_d0", ck_mesh_coords.d0); f.add_u64("coords_d1", ck_mesh_coords.d1);
      f.add_u64("cells_d0", ck_mesh_cells.d0); f.add_u64("cells_d1", ck_mesh_cells.d1);
    }
    f.add("rank", (long)comm->rank); f.add("nranks", (long)comm->size);
    f.add("NQ", NQ); f.add("NPv", NPv); f.add("NLv", NLv);
    f.add("rows", (long)g.R); f.add("row_pitch", (long)g.P);  // the row padding (HDG_ROW_PAD or the channel rule)
    return f;
  }
  struct CkPlan {
    CkHost hs;
    std::vector<CkDev> dev;
    ckpt::ByteWriter hb[2];
    std::vector<ckpt::Section> secs;  // device sections, then 'solver' and 'outputs'
    std::string fp;
    uint64_t total = 0;
  };
  CkPlan ck_plan() {
    CkPlan P;
    P.hs = ck_capture();
    P.dev = ck_device_sections(P.hs);
    ck_write_host(P.hs, P.hb[0], P.hb[1]);
    for (const CkDev& d : P.dev) {
      ckpt::Section sc;
      sc.id = d.id; sc.kind = ckpt::DEVICE_DOUBLES; sc.length = (uint64_t)d.n;
      P.secs.push_back(sc);
    }
    const char* names[2] = {"solver", "outputs"};
    for (int q = 0; q < 2; q++) {
      ckpt::Section sc;
      sc.id = names[q]; sc.kind = ckpt::HOST_BYTES; sc.length = P.hb[q].b.size();
      sc.digest = ckpt::digest_bytes(P.hb[q].b.data(), P.hb[q].b.size());
      P.secs.push_back(sc);
    }
    P.fp = ck_fingerprint().text();
    P.total = ckpt::layout(P.fp, P.secs);
    return P;
  }
  void ck_refuse_open_step() const {
    if (step_open)
      throw std::string("checkpoint: a step is open (between hdg_begin_step and the end of the step); a save is valid between steps only");
  }
  long checkpoint_size() {
    ck_refuse_open_step();
    return (long)ck_plan().total;
  }
  void checkpoint_save(long step, double t, void* buf, long nbytes) {
    ck_refuse_open_step();
    if (!buf) throw std::string("checkpoint: no buffer");
    CkPlan P = ck_plan();
    if ((uint64_t)nbytes != P.total)
      throw std::string("checkpoint: byte count: the buffer has ") + std::to_string(nbytes) + " bytes, the state needs " +
          std::to_string(P.total) + " (hdg_checkpoint_size)";
    unsigned char* c = static_cast<unsigned char*>(buf);
    // every device section: digest on the device, download, check the downloaded bytes against that digest
    for (size_t q = 0; q < P.dev.size(); q++) {
      const double* p = P.dev[q].ptr();
      digest_launch(p, P.dev[q].n, (int)q);
      if (P.dev[q].n > 0) HIPCHECK(hipMemcpyAsync(c + P.secs[q].offset, p, sizeof(double) * (size_t)P.dev[q].n, hipMemcpyDeviceToHost, stream));
    }
    std::vector<ckpt::Digest> dd;
    digest_fetch((int)P.dev.size(), dd);
    for (size_t q = 0; q < P.dev.size(); q++) {
      if (ckpt::digest_words(c + P.secs[q].offset, (uint64_t)P.dev[q].n) != dd[q])
        throw std::string("checkpoint: section '") + P.dev[q].id + "': the downloaded bytes do not match the digest taken on the device";
      P.secs[q].digest = dd[q];
    }
    for (int q = 0; q < 2; q++)
      if (!P.hb[q].b.empty()) std::memcpy(c + P.secs[P.dev.size() + (size_t)q].offset, P.hb[q].b.data(), P.hb[q].b.size());
    const uint64_t flags = (P.hs.tracer_on ? ckpt::FLAG_TRACER : 0) | (P.hs.log[0][1] > 0 ? ckpt::FLAG_DIAGNOSTICS : 0) |
                           (P.hs.log[1][1] > 0 ? ckpt::FLAG_PROBES : 0) | (P.hs.pa_n > 0 ? ckpt::FLAG_PARTICLES : 0);
    ckpt::write_front(buf, P.total, step, t, (int)(P.hs.probe_xy.size() / 2), P.hs.pa_n, flags, P.fp, P.secs);
  }
  void state_digest(unsigned long long* out) {
    if (!out) throw std::string("null argument");
    ck_refuse_open_step();
    CkPlan P = ck_plan();
    for (size_t q = 0; q < P.dev.size(); q++) digest_launch(P.dev[q].ptr(), P.dev[q].n, (int)q);
    std::vector<ckpt::Digest> dd;
    digest_fetch((int)P.dev.size(), dd);
    for (int q = 0; q < 2; q++) dd.push_back(P.secs[P.dev.size() + (size_t)q].digest);
    const ckpt::Digest d = ckpt::digest_of_digests(dd);
    out[0] = d.d0; out[1] = d.d1;
  }
  void ck_restore_log(RowLog& L, double*& rows, const long* rec) {
    log_size(L, rows, rec[0], rec[1]);
    L.n = rec[2]; L.dropped = rec[3];
  }
  void checkpoint_load(const void* buf, long nbytes, long* step, double* t) {
    // ---- everything is validated before the engine is touched
    if (nbytes < 0) throw std::string("checkpoint: negative byte count");
    ckpt::Parsed B;
    const std::string perr = ckpt::parse(buf, (uint64_t)nbytes, B);
    if (!perr.empty()) throw "checkpoint: " + perr;
    const std::string fdiff = ck_fingerprint().difference(ckpt::Fingerprint::parse(B.fingerprint));
    if (!fdiff.empty()) throw "checkpoint: " + fdiff;
    const unsigned char* c = static_cast<const unsigned char*>(buf);
    const ckpt::Section *hsolver = nullptr, *houtputs = nullptr;
    for (const ckpt::Section& sc : B.sections) {
      if (sc.kind == ckpt::HOST_BYTES && sc.id == "solver") hsolver = &sc;
      if (sc.kind == ckpt::HOST_BYTES && sc.id == "outputs") houtputs = &sc;
    }
    if (!hsolver) throw std::string("checkpoint: section 'solver' is missing");
    if (!houtputs) throw std::string("checkpoint: section 'outputs' is missing");
    CkHost hs;
    const std::string herr = ck_read_host(hs, c + hsolver->offset, (size_t)hsolver->length, c + houtputs->offset, (size_t)houtputs->length);
    if (!herr.empty()) throw "checkpoint: " + herr;
    std::vector<CkDev> dev = ck_device_sections(hs);
    if (B.sections.size() != dev.size() + 2)
      throw std::string("checkpoint: ") + std::to_string(B.sections.size()) + " sections in the table, this state has " + std::to_string(dev.size() + 2);
    for (size_t q = 0; q < dev.size(); q++) {
      const ckpt::Section& sc = B.sections[q];
      if (sc.id != dev[q].id || sc.kind != ckpt::DEVICE_DOUBLES)
        throw std::string("checkpoint: section ") + std::to_string(q) + " is '" + sc.id + "' where this engine expects '" + dev[q].id + "'";
      if (sc.length != (uint64_t)dev[q].n)
        throw std::string("checkpoint: section '") + sc.id + "' holds " + std::to_string(sc.length) + " values, this engine's has " + std::to_string(dev[q].n);
    }
    // ---- the engine becomes the saved one
    if (hs.tracer_vecs) { cg_setup(); tracer_alloc(); }
    if (hs.has_chd && !chd) chd = dalloc(NQ);
    ch = hs.ch.empty() ? std::vector<ChebStage>((size_t)s + 1) : hs.ch;
    bscale = hs.bscale; bsep = hs.bsep;
    for (int q = 0; q < 4; q++) { it_sum[q] = hs.it_sum[q]; it_cnt[q] = hs.it_cnt[q]; }
    ev_cg_replacements = hs.ev[0]; ev_cg_floor_exits = hs.ev[1]; n_sstep_cycles = hs.ev[2]; n_sstep_fallbacks = hs.ev[3];
    trace_scale = hs.trace_scale;
    tracer_on = hs.tracer_on != 0;
    ck_restore_log(diag_log, diag_rows, hs.log[0]);
    if (!hs.probe_xy.empty()) {  // located again, by the code hdg_set_probes uses
      points_locate((int)(hs.probe_xy.size() / 2), hs.probe_xy.data(), pt_probe, nullptr);
      pt_probe_xy = hs.probe_xy;
    } else { pt_probe.n = 0; pt_probe_xy.clear(); }
    ck_restore_log(probe_log, pt_rows, hs.log[1]);
    particles_off();
    if (hs.pa_n > 0) {
      pa_X = dalloc(2L * hs.pa_n); pa_Xs = dalloc(2L * hs.pa_n); pa_k1 = dalloc(2L * hs.pa_n);
      if (comm->size > 1) pa_k2 = dalloc(2L * hs.pa_n);
      pa_cnt = dalloc(PARTICLE_NCOUNT);
      pa_n = hs.pa_n; pa_every = hs.pa_every; pa_steps = hs.pa_steps;
    }
    ck_restore_log(pa_log, pa_rows, hs.log[2]);
    // upload, digest again on the device, compare with the table
    for (size_t q = 0; q < dev.size(); q++) {
      double* p = dev[q].ptr();
      if (dev[q].n > 0) HIPCHECK(hipMemcpyAsync(p, c + B.sections[q].offset, sizeof(double) * (size_t)dev[q].n, hipMemcpyHostToDevice, stream));
      digest_launch(p, dev[q].n, (int)q);
    }
    std::vector<ckpt::Digest> dd;
    digest_fetch((int)dev.size(), dd);
    for (size_t q = 0; q < dev.size(); q++)
      if (dd[q] != B.sections[q].digest)
        throw std::string("checkpoint: section '") + dev[q].id + "': the uploaded vector does not match the digest in the table";
    step_open = false;
    // timers and the launch census are not state
    for (int q = 0; q < HDG_N_TIMERS; q++) { tm_total[q] = 0; tm_sumsq[q] = 0; tm_calls[q] = 0; }
    for (int q = 0; q < HDG_N_LAUNCH_CLASSES; q++) { lc_calls[q] = 0; lc_bytes[q] = 0.0; }
    if (step) *step = (long)B.header.step;
    if (t) *t = B.header.t;
  }

  // ------------------------------------------------------------------ transfer between engines
  // L2 projection of another engine's state onto this engine's spaces on a nested structured mesh, and the L2 norm of the
  // difference of two engines' states (hdg_transfer.hpp: tables, hdg_transfer_kernels.hpp: kernels).  Used once per run: the
  // table of the pair is built and uploaded per call and freed again, and no step ever sees any of this.
  //
  // Stream ordering: every engine owns a stream.  The other engine's stream is drained (hipStreamSynchronize) before the
  // first kernel that reads its vectors is put on the stream the call works on -- a transfer happens between steps, where
  // that stream is idle anyway, so an event would save nothing.
  template <class F> static void by_degree_pair(int k1, int k2, F&& f) {
    with_int<1, 2, 3, 4>(k1, "degree", [&](auto a) { with_int<1, 2, 3, 4>(k2, "degree", [&](auto b) { f(a, b); }); });
  }
  // what a pair must satisfy, each refusal naming its cause; HDG_ERR_UNSUPPORTED cases come back as false with `unsupported`
  // set, the others throw (HDG_ERR_ARG).  Returns the ratio through r (always >= 1).
  static void transfer_pair_check(const Engine& A, const Engine& B, const char* call, std::string& unsupported, int& r) {
    unsupported.clear();
    r = 1;
    const std::string c(call);
    if (A.general || B.general) { unsupported = c + ": general meshes are not supported (nested structured meshes only)"; return; }
    if (A.comm->size > 1 || B.comm->size > 1) { unsupported = c + ": engines with more than one rank are not supported"; return; }
    if (A.periodic != B.periodic) throw c + ": different mesh kind (unit square and doubly periodic square)";
    if (A.Ldom != B.Ldom) throw c + ": different L (" + std::to_string(A.Ldom) + " and " + std::to_string(B.Ldom) + ")";
    if (A.cfg.device != B.cfg.device) throw c + ": different device (" + std::to_string(A.cfg.device) + " and " + std::to_string(B.cfg.device) + ")";
    if (A.g.ny != A.g.nx || B.g.ny != B.g.nx) throw c + ": ny = nx is required";
    const int hi = std::max(A.g.nx, B.g.nx), lo = std::min(A.g.nx, B.g.nx);
    if (hi % lo != 0) throw c + ": the meshes are not nested (non-integer ratio " + std::to_string(hi) + " / " + std::to_string(lo) + ")";
    r = hi / lo;
    if (r > transfer::MAX_RATIO) throw c + ": ratio r = " + std::to_string(r) + " > " + std::to_string(transfer::MAX_RATIO);
    if (A.step_open || B.step_open) throw c + ": a step is open (between hdg_begin_step and the end of the step) on " +
        (A.step_open ? (B.step_open ? "both engines" : "the first engine") : "the second engine");
  }
  // the velocity table of (coarse degree kc, fine degree kf) on the device; the caller frees it
  double* transfer_table(int kc, int kf, int r) { return const_cast<double*>(upload(transfer::child_tables(kc + 1, kf + 1, r))); }
  void transfer_from(Engine& S, int r, bool with_tracers) {
    if (with_tracers && (!S.tracer_on || S.n_tr != n_tr))
      throw std::string("hdg_transfer_state: tracer mismatch: the source ") +
          (S.tracer_on ? "carries " + std::to_string(S.n_tr) + " tracer(s), this engine " + std::to_string(n_tr) : "has no tracer switched on");
    HIPCHECK(hipStreamSynchronize(S.stream));  // stream ordering: see above
    const bool prolong = g.nx >= S.g.nx;
    double* T = prolong ? transfer_table(S.K, K, r) : transfer_table(K, S.K, r);
    if (with_tracers) { cg_setup(); tracer_alloc(); }
    auto launch = [&](auto vel, const double* src, long sstride, double* dst, long dstride, int nfields) {
      dim3 grid = cell_grid();
      grid.y = (unsigned)nfields;
      tally(LC_OTHER, (vel() ? 16.0 : 8.0) * nfields * (2.0 * g.nx * g.ny * (vel() ? NU : NP) + 2.0 * S.g.nx * S.g.ny * (vel() ? S.NU : S.NP)));
      by_degree_pair(S.K, K, [&](auto ks, auto kd) {
        if (prolong) k_xfer_prolong<ks(), kd(), vel()><<<grid, bs(), 0, stream>>>(g, S.g, r, T, src, sstride, dst, dstride);
        else k_xfer_restrict<ks(), kd(), vel()><<<grid, bs(), 0, stream>>>(g, S.g, r, T, src, sstride, dst, dstride);
      });
    };
    // velocity and scalars are separate launches (pair planes / scalar planes); the tracers are one launch, grid.y apart
    launch(std::true_type{}, S.curQ, 0, curQ, 0, 1);
    launch(std::false_type{}, S.curP, 0, curP, 0, 1);
    if (with_tracers) { launch(std::false_type{}, S.q_cur, S.NPv, q_cur, NPv, n_tr); tracer_on = true; }
    shift(curP, nullptr);  // as hdg_set_state: p_0 -= mean
    particles_refresh();
    HIPCHECK(hipStreamSynchronize(stream));
    dfree(T);
  }
  // norms of the differences of the current states of A and B (n_q: tracer norms wanted, needs the same tracers on both)
  static void transfer_difference(Engine& A, Engine& B, int r, double* norm_Q, double* norm_p, double* norm_q) {
    if (norm_q && (!A.tracer_on || !B.tracer_on || A.n_tr != B.n_tr))
      throw std::string("hdg_transfer_difference: tracer mismatch: tracer norms need the same tracers switched on in both engines");
    Engine& F = A.g.nx >= B.g.nx ? A : B;  // the work runs on the finer mesh's engine and stream
    Engine& C = &F == &A ? B : A;
    HIPCHECK(hipStreamSynchronize(C.stream));  // stream ordering: see above
    HIPCHECK(hipStreamSynchronize(F.stream));
    const int km = std::max(C.K, F.K);
    double* T = F.transfer_table(C.K, km, r);
    auto norm = [&](auto vel, const double* coarse, const double* fine) {
      F.tally(LC_OTHER, 0.0);
      by_degree_pair(C.K, F.K, [&](auto kc, auto kf) {
        k_xfer_diff<kc(), kf(), vel()><<<F.cell_grid(), F.bs(), 0, F.stream>>>(F.g, C.g, r, T, coarse, fine, F.wP1);
      });
      return std::sqrt(F.dot(F.g.Nc, F.wP1, F.ones_c, KC));  // the two-stage deterministic reduction over the owned cells
    };
    if (norm_Q) *norm_Q = norm(std::true_type{}, C.curQ, F.curQ);
    if (norm_p) *norm_p = norm(std::false_type{}, C.curP, F.curP);
    if (norm_q)
      for (int t = 0; t < A.n_tr; t++) norm_q[t] = norm(std::false_type{}, C.q_cur + t * C.NPv, F.q_cur + t * F.NPv);
    F.dfree(T);
  }

  // ------------------------------------------------------------------ host <-> device fields
  long n_edges() const {
    if (general) return gm->ne;
    if (periodic) return 3L * g.nx * g.ny;
    return (long)g.nx * (g.ny + 1) + (long)(g.nx + 1) * g.ny + (long)g.nx * g.ny;
  }
  void put_Q(const double* host, double* modal) {
    HIPCHECK(hipMemcpyAsync(hQ_dev, host, sizeof(double) * NQb, hipMemcpyHostToDevice, stream));
    q_to_modal(hQ_dev, modal);
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void put_P(const double* host, double* modal) {
    HIPCHECK(hipMemcpyAsync(hP_dev, host, sizeof(double) * NPb, hipMemcpyHostToDevice, stream));
    p_to_modal(hP_dev, modal);
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void put_L(const double* host, double* modal) {
    HIPCHECK(hipMemcpyAsync(hL_dev, host, sizeof(double) * n_edges() * NL, hipMemcpyHostToDevice, stream));
    l_to_modal(hL_dev, modal);
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void get_Q(const double* modal, double* host) {
    q_to_nodal(modal, hQ_dev);
    HIPCHECK(hipMemcpyAsync(host, hQ_dev, sizeof(double) * NQb, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void get_P(const double* modal, double* host) {
    p_to_nodal(modal, hP_dev);
    HIPCHECK(hipMemcpyAsync(host, hP_dev, sizeof(double) * NPb, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
  void get_L(double* modal, double* host) {
    halo_L(modal);  // the strip's top row is a ghost copy on every rank but the topmost
    l_to_nodal(modal, hL_dev);
    HIPCHECK(hipMemcpyAsync(host, hL_dev, sizeof(double) * n_edges() * NL, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }


  // physical coordinates of the velocity / pressure nodes in boundary (reference) numbering
  void node_coords(double* xq, double* xp) const {
    if (general) {
      if (xq) std::copy(gops.xq.begin(), gops.xq.end(), xq);
      if (xp) std::copy(gops.xp.begin(), gops.xp.end(), xp);
      return;
    }
    for (int which = 0; which < 2; which++) {
      double* out = which == 0 ? xq : xp;
      if (!out) continue;
      std::vector<real> xi, eta;
      triangleNodes(which == 0 ? K + 1 : K, cfg.equispaced_nodes, xi, eta);
      const long nn = (long)xi.size();
      for (int j = 0; j < g.ny; j++)
        for (int i = 0; i < g.nx; i++)
          for (int sh = 0; sh < 2; sh++) {
            const long c = 2 * ((long)j * g.nx + i) + sh;
            const int joff_true = periodic ? g.pj0 : g.joff;
            const double x0 = (sh == 0 ? i : i + 1) * g.h, y0 = (joff_true + (sh == 0 ? j : j + 1)) * g.h;
            const double sg = sh == 0 ? 1.0 : -1.0;
            for (long n = 0; n < nn; n++) {
              out[(c * nn + n) * 2 + 0] = x0 + sg * g.h * (double)xi[n];
              out[(c * nn + n) * 2 + 1] = y0 + sg * g.h * (double)eta[n];
            }
          }
    }
  }

  // Micro-benchmark of one kernel launch (bench.py's roofline probe).  Ids: 0 advection operator, 1 trace operator,
  // 2 BDM projection, 3 back-substitution, 4 additive preconditioner + Chebyshev step, 5 transposed lift,
  // 6 hybrid preconditioner + Chebyshev step (per-thread lift kernel), 7 advection operator in residual form,
  // 8 stream triad on velocity vectors, 9 hybrid preconditioner alone (the GMRES path: matrix-core lift at k >= 3)
  // 10 condensation (pressure-row form), 11 pressure-gradient combination, 12 weak divergence, 13 reconstruction rhs
  // 14 condensation (velocity-row form of the final stage)
  static constexpr int N_TIME_KERNELS = 15;
  double time_kernel(int kernel, int reps) {
    if (kernel < 0 || kernel >= N_TIME_KERNELS) throw std::string("unknown kernel id");  // before any state is touched
    if (general) general_unsupported("hdg_time_kernel");
    // halo exchanges are switched off for the bare launches (the call is not collective); restored on EVERY exit path
    struct Guard {
      Engine& e;
      hipEvent_t e0 = nullptr, e1 = nullptr;
      explicit Guard(Engine& e_) : e(e_) { e.halo_on = false; }
      ~Guard() {
        e.halo_on = true;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
      }
    } gd(*this);
    HIPCHECK(hipEventCreate(&gd.e0));
    HIPCHECK(hipEventCreate(&gd.e1));
    auto launch = [&]() {
      switch (kernel) {
        case 0: adv_apply(curQ, Qstar[0], wQ1, 0.25 * cfg.dt); break;
        case 1: trace_apply(curL, nullptr, 0.0, 1.0, wL1); break;
        case 2: bdm(curQ, wQ1); break;
        case 3: backsub(curQ, curP, curL, wQ1, wP1); break;
        case 4:  // second half of the two-level preconditioner fused with the Chebyshev step
          ensure_dinv(1 % s, 0.25 * cfg.dt);
          if (!chd) chd = dalloc(NQ);
          bdm_plus_bj(wQ3, nullptr, wQ2, dinv0[1 % s], dinv1[1 % s], chd, wQ4, 0.5, 0.1);
          break;
        case 5: bdm_T(curQ, wQ1); break;
        case 6:  // hybrid two-level preconditioner (one lift + block-Jacobi of the remainder) + Chebyshev step
          ensure_dinv(1 % s, 0.25 * cfg.dt);
          if (!chd) chd = dalloc(NQ);
          bdm_hybrid(wQ2, nullptr, hybg0[1 % s], hybg1[1 % s], chd, wQ4, 0.5, 0.1);
          break;
        case 7: adv_apply(curQ, Qstar[0], wQ1, 0.25 * cfg.dt, wQ2); break;  // residual form b - A x
        case 8: axpby(NQ, 0.5, wQ2, 0.25, wQ1); break;  // stream triad y = a x + b y on velocity vectors: 3 passes of 8 N_Q bytes
        case 9:  // hybrid preconditioner without the Chebyshev epilogue (what GMRES applies; k >= 3: k_edge_lift_mfma)
          ensure_dinv(1 % s, 0.25 * cfg.dt);
          bdm_hybrid(wQ2, wQ1, hybg0[1 % s], hybg1[1 % s]);
          break;
        case 10: condense(nullptr, curP, nullptr, wL1); break;
        case 11: pgrad(wQ3, 1.0, wQ4, -1.0, curP, curL, 0.25 * cfg.dt, wQ1); break;
        case 12: weak_div(curQ, 1.0, wP1, false); break;
        case 13: precon_rhs(curQ, wQ2, 1.0, wP1, wL2); break;
        case 14: condense(curQ, nullptr, nullptr, wL1); break;
        default: throw std::string("unknown kernel id");
      }
    };
    for (int i = 0; i < 3; i++) launch();
    HIPCHECK(hipEventRecord(gd.e0, stream));
    for (int i = 0; i < reps; i++) launch();
    HIPCHECK(hipEventRecord(gd.e1, stream));
    HIPCHECK(hipEventSynchronize(gd.e1));
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, gd.e0, gd.e1));
    return (double)ms / reps;
  }
};

}  // namespace hdg

// =============================================================================================
// C-ABI
// =============================================================================================
struct hdg_handle {
  hdg::Engine* eng;
  std::string err;
};
static std::string g_create_error;

#define HDG_API_BEGIN(h)                      \
  if (!(h) || !(h)->eng) return HDG_ERR_ARG;  \
  hdg::Engine& E = *(h)->eng;                 \
  (void)E;                                    \
  try {
#define HDG_API_END(h)                                                        \
    hipError_t _le = hipStreamSynchronize(E.stream);                          \
    if (_le != hipSuccess) { (h)->err = std::string("HIP: ") + hipGetErrorString(_le); if (E.comm) E.comm->failed = true; return HDG_ERR_HIP; } \
    if (E.comm) E.comm->check_async();  /* a failed collective must not pass as a finished call */ \
    _le = hipGetLastError();                                                  \
    if (_le != hipSuccess) { (h)->err = std::string("HIP launch: ") + hipGetErrorString(_le); return HDG_ERR_HIP; } \
    E.harvest_timers();                                                       \
    return HDG_OK;                                                            \
  } catch (const hdg::HipError& e) { (h)->err = e.msg; if (E.comm) E.comm->failed = true; return HDG_ERR_HIP; \
  } catch (const hdg::NotConverged& e) { (h)->err = e.msg; return HDG_ERR_NOT_CONVERGED; \
  } catch (const hdg::CommError& e) { (h)->err = e.msg; if (E.comm) E.comm->failed = true; return HDG_ERR_COMM; \
  } catch (const std::string& e) { (h)->err = e; return HDG_ERR_ARG;          \
  } catch (const std::exception& e) { (h)->err = e.what(); return HDG_ERR_ARG; \
  } catch (...) { (h)->err = "unknown error"; return HDG_ERR_ARG; }

extern "C" {

static int create_impl(const hdg_config* cfg, int rank, int nranks, int backend, const char* token, hdg_handle** out);
int hdg_create(const hdg_config* cfg, hdg_handle** out) { return create_impl(cfg, 0, 1, 0, nullptr, out); }
int hdg_create_distributed(const hdg_config* cfg, int rank, int nranks, int backend, const char* token, hdg_handle** out) {
  return create_impl(cfg, rank, nranks, backend, token, out);
}
int hdg_rccl_unique_id(char* out128) {
  if (!out128) return HDG_ERR_ARG;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return HDG_ERR_HIP;
  std::memcpy(out128, &id, sizeof(id) < 128 ? sizeof(id) : 128);
  return HDG_OK;
}
// One-GPU self-test of the RCCL transport (the multi-rank send / recv path cannot run on a box with one GPU: RCCL refuses two
// ranks on one device): a 1-rank communicator runs the grouped ncclSend / ncclRecv pattern of Comm::exchange with itself as
// both neighbours, an all-reduce and an all-gather on the given stream-ordered buffers of n doubles; *max_err = largest
// deviation from the expected contents.
int hdg_rccl_selftest(int device, int n, double* max_err) {
  if (n < 1 || !max_err) return HDG_ERR_ARG;
  *max_err = -1.0;
  try {
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed (no GPU?)"; return HDG_ERR_HIP; }
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return HDG_ERR_COMM; }
    hdg::CommRccl comm(0, 1, reinterpret_cast<const char*>(&id));
    hipStream_t st;
    if (hipStreamCreate(&st) != hipSuccess) throw hdg::HipError{"hipStreamCreate failed"};
    std::vector<double> a(n), b(n), out(4 * (size_t)n);
    for (int i = 0; i < n; i++) { a[i] = 1.0 + i; b[i] = -2.0 * i - 0.5; }
    double* d = nullptr;
    if (hipMalloc((void**)&d, sizeof(double) * 6 * (size_t)n) != hipSuccess) throw hdg::HipError{"hipMalloc failed"};
    double *slo = d, *shi = d + n, *rlo = d + 2 * (size_t)n, *rhi = d + 3 * (size_t)n, *red = d + 4 * (size_t)n, *gat = d + 5 * (size_t)n;
    (void)hipMemcpyAsync(slo, a.data(), sizeof(double) * n, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(shi, b.data(), sizeof(double) * n, hipMemcpyHostToDevice, st);
    (void)hipMemsetAsync(rlo, 0, sizeof(double) * 4 * (size_t)n, st);
    comm.exchange_loopback(slo, rlo, shi, rhi, (size_t)n, st);
    (void)hipMemcpyAsync(red, slo, sizeof(double) * n, hipMemcpyDeviceToDevice, st);
    comm.allreduce_sum(red, n, st);
    comm.allgather(shi, gat, (size_t)n, st);
    (void)hipMemcpyAsync(out.data(), rlo, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) throw hdg::HipError{"hipStreamSynchronize failed"};
    double err = 0.0;
    for (int i = 0; i < n; i++) {
      err = std::max(err, std::fabs(out[i] - a[i]));                        // rlo <- slo
      err = std::max(err, std::fabs(out[(size_t)n + i] - b[i]));            // rhi <- shi
      err = std::max(err, std::fabs(out[2 * (size_t)n + i] - a[i]));        // all-reduce over one rank
      err = std::max(err, std::fabs(out[3 * (size_t)n + i] - b[i]));        // all-gather of one block
    }
    *max_err = err;
    (void)hipFree(d);
    (void)hipStreamDestroy(st);
    return HDG_OK;
  } catch (const hdg::HipError& e) { g_create_error = e.msg; return HDG_ERR_HIP;
  } catch (const hdg::CommError& e) { g_create_error = e.msg; return HDG_ERR_COMM;
  } catch (...) { g_create_error = "unknown error"; return HDG_ERR_ARG; }
}
static int create_impl(const hdg_config* cfg, int rank, int nranks, int backend, const char* token, hdg_handle** out) {
  if (!cfg || !out || nranks < 1 || rank < 0 || rank >= nranks) return HDG_ERR_ARG;
  *out = nullptr;
  try {
    hdg::Engine::checked_n_tracers(*cfg);
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed (no GPU?)"; return HDG_ERR_HIP; }
    std::unique_ptr<hdg::Comm> comm;  // owned here until the engine has been built
    if (nranks == 1 && hdg::options_from_env().force_rccl) {
      // smoke path: exercise RCCL initialisation, all-reduce and all-gather with a 1-rank communicator
      ncclUniqueId id;
      if (ncclGetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return HDG_ERR_COMM; }
      comm.reset(new hdg::CommRccl(0, 1, reinterpret_cast<const char*>(&id)));
    } else if (nranks == 1) comm.reset(new hdg::Comm());
    else if (backend == HDG_COMM_RCCL) { if (!token) return HDG_ERR_ARG; comm.reset(new hdg::CommRccl(rank, nranks, token)); }
    else if (backend == HDG_COMM_SHM) {
      if (!token) return HDG_ERR_ARG;
      const int k = cfg->degree;
      const size_t nu = (size_t)(k + 2) * (k + 3) / 2;
      const size_t P = ((size_t)cfg->nx + 1 + 15) / 16 * 16;
      const size_t cap_halo = std::max<size_t>(hdg::GH * 2 * nu * 2 * cfg->nx, hdg::GH * 3 * (size_t)(k + 1) * P);
      const size_t cap_gather = ((size_t)cfg->ny / nranks + 1) * ((size_t)cfg->nx + 1);
      comm.reset(new hdg::CommShm(rank, nranks, token, cap_halo, cap_gather));
    } else return HDG_ERR_ARG;
    hdg::Engine* e = new hdg::Engine(*cfg, comm.get());
    comm.release();  // the engine owns it from here (~Engine)
    *out = new hdg_handle{e, ""};
    return HDG_OK;
  } catch (const hdg::HipError& e) { g_create_error = e.msg; return HDG_ERR_HIP;
  } catch (const hdg::CommError& e) { g_create_error = e.msg; return HDG_ERR_COMM;
  } catch (const std::string& e) { g_create_error = e; return HDG_ERR_ARG;
  } catch (const std::runtime_error& e) { g_create_error = e.what(); return HDG_ERR_SINGULAR;
  } catch (const std::exception& e) { g_create_error = e.what(); return HDG_ERR_ARG;
  } catch (...) { g_create_error = "unknown error"; return HDG_ERR_ARG; }
}
int hdg_create_general(const hdg_config* cfg, int n_vertices, const double* coords, int n_cells, const int* cells, hdg_handle** out) {
  if (!cfg || !out || !coords || !cells) return HDG_ERR_ARG;
  *out = nullptr;
  try {
    hdg::Engine::checked_n_tracers(*cfg);
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed (no GPU?)"; return HDG_ERR_HIP; }
    std::unique_ptr<hdg::Comm> comm(new hdg::Comm());
    hdg::Engine* e = new hdg::Engine(*cfg, comm.get(), n_vertices, coords, n_cells, cells);
    comm.release();
    *out = new hdg_handle{e, ""};
    return HDG_OK;
  } catch (const hdg::HipError& e) { g_create_error = e.msg; return HDG_ERR_HIP;
  } catch (const hdg::CommError& e) { g_create_error = e.msg; return HDG_ERR_COMM;
  } catch (const std::string& e) { g_create_error = e; return HDG_ERR_ARG;
  } catch (const std::runtime_error& e) { g_create_error = e.what(); return HDG_ERR_SINGULAR;
  } catch (const std::exception& e) { g_create_error = e.what(); return HDG_ERR_ARG;
  } catch (...) { g_create_error = "unknown error"; return HDG_ERR_ARG; }
}
int hdg_general_topology(const hdg_handle* h, int* edge_vertices, int* edge_cells) {
  if (!h || !h->eng || !h->eng->general) return HDG_ERR_ARG;
  const hdg::GMesh& M = *h->eng->gm;
  if (edge_vertices) std::copy(M.ev.begin(), M.ev.end(), edge_vertices);
  if (edge_cells) std::copy(M.ecell.begin(), M.ecell.end(), edge_cells);
  return HDG_OK;
}
int hdg_destroy(hdg_handle* h) {
  if (!h) return HDG_ERR_ARG;
  delete h->eng;
  delete h;
  return HDG_OK;
}
const char* hdg_last_error(const hdg_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int hdg_get_sizes(const hdg_handle* h, long* n_cells, long* n_edges, int* n_u, int* n_p, int* n_l) {
  if (!h || !h->eng) return HDG_ERR_ARG;
  const hdg::Engine& E = *h->eng;
  if (n_cells) *n_cells = E.general ? (long)E.gm->nc : 2L * E.g.nx * E.g.ny;
  if (n_edges) *n_edges = E.n_edges();
  if (n_u) *n_u = E.NU;
  if (n_p) *n_p = E.NP;
  if (n_l) *n_l = E.NL;
  return HDG_OK;
}

int hdg_set_state(hdg_handle* h, const double* Q, const double* p) {
  HDG_API_BEGIN(h)
  if (!Q || !p) throw std::string("null state");
  E.put_Q(Q, E.curQ);
  E.put_P(p, E.curP);
  E.shift(E.curP, nullptr);  // p_0 -= mean (hdg_imex.py:522)
  E.particles_refresh();
  HDG_API_END(h)
}
int hdg_get_field(hdg_handle* h, int which, double* Q, double* p, double* lam) {
  HDG_API_BEGIN(h)
  double *dQ, *dP, *dL;
  E.state_ptrs(which, dQ, dP, dL);
  if (Q) { if (!dQ) throw std::string("field has no velocity part"); E.get_Q(dQ, Q); }
  if (p) { if (!dP) throw std::string("field has no pressure part"); E.get_P(dP, p); }
  if (lam) { if (!dL) throw std::string("field has no trace part"); E.get_L(dL, lam); }
  HDG_API_END(h)
}
int hdg_set_field(hdg_handle* h, int which, const double* Q, const double* p, const double* lam) {
  HDG_API_BEGIN(h)
  double *dQ, *dP, *dL;
  E.state_ptrs(which, dQ, dP, dL);
  if (Q) { if (!dQ) throw std::string("field has no velocity part"); E.put_Q(Q, dQ); }
  if (p) { if (!dP) throw std::string("field has no pressure part"); E.put_P(p, dP); }
  if (lam) { if (!dL) throw std::string("field has no trace part"); E.put_L(lam, dL); }
  if (Q && which == HDG_STATE_CURRENT) E.particles_refresh();
  HDG_API_END(h)
}
int hdg_set_forcing_nodal(hdg_handle* h, int slot, const double* f) {
  HDG_API_BEGIN(h)
  if (slot < 0 || slot > E.s || !f) throw std::string("bad forcing slot");
  E.put_Q(f, E.brhs[slot]);
  E.bscale[slot] = 1.0;
  E.bsep[slot] = 0;
  HDG_API_END(h)
}
int hdg_set_forcing_profile(hdg_handle* h, const double* profile) {
  HDG_API_BEGIN(h)
  if (!profile) throw std::string("null profile");
  E.put_Q(profile, E.profile);
  HDG_API_END(h)
}
int hdg_set_forcing_scale(hdg_handle* h, int slot, double scale) {
  HDG_API_BEGIN(h)
  if (slot < 0 || slot > E.s) throw std::string("bad forcing slot");
  E.bscale[slot] = scale;
  E.bsep[slot] = 1;
  HDG_API_END(h)
}
int hdg_reconstruct_trace(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.trace_recon(E.curQ, E.curP, E.curL);
  HDG_API_END(h)
}
int hdg_project_bdm(hdg_handle* h, int src_stage, int dst) {
  HDG_API_BEGIN(h)
  if (src_stage < 0 || src_stage >= E.s || dst < 0 || dst >= (int)E.Qstar.size()) throw std::string("bad stage index");
  { hdg::Engine::Timed tb_(E, hdg::Engine::T_BDM); E.bdm(E.stQ[src_stage], E.Qstar[dst]); }
  HDG_API_END(h)
}
int hdg_project_bdm_nodal(hdg_handle* h, const double* Qin, double* Qout) {
  HDG_API_BEGIN(h)
  if (!Qin || !Qout) throw std::string("null argument");
  E.put_Q(Qin, E.wQ1);
  E.bdm(E.wQ1, E.wQ2);
  E.get_Q(E.wQ2, Qout);
  HDG_API_END(h)
}
int hdg_begin_step(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.step_open = true;  // no checkpoint until the step is complete
  E.begin_step();
  HDG_API_END(h)
}
int hdg_tentative_solve(hdg_handle* h, int stage, int* its) {
  HDG_API_BEGIN(h)
  int n = E.tentative_solve(stage);
  if (its) *its = n;
  HDG_API_END(h)
}
int hdg_unsplit_solve(hdg_handle* h, int stage, int* its) {
  HDG_API_BEGIN(h)
  int n = E.unsplit_solve(stage);
  if (its) *its = n;
  HDG_API_END(h)
}
int hdg_pressure_solve(hdg_handle* h, int key, int* its) {
  HDG_API_BEGIN(h)
  int n = E.pressure_solve(key);
  if (its) *its = n;
  HDG_API_END(h)
}
int hdg_shift_pressure(hdg_handle* h, int which) {
  HDG_API_BEGIN(h)
  double *dQ, *dP, *dL;
  E.state_ptrs(which, dQ, dP, dL);
  if (!dP) throw std::string("state has no pressure");
  E.shift(dP, dL);
  HDG_API_END(h)
}
int hdg_stage_update(hdg_handle* h, int stage) {
  HDG_API_BEGIN(h)
  if (stage < 1 || stage >= E.s) throw std::string("stage out of range");
  E.stage_update(stage);
  HDG_API_END(h)
}
int hdg_finish_step(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.finish_step();
  if (!E.tracer_on) { E.end_of_step(); E.step_open = false; }  // with a tracer the rows are taken after hdg_tracer_finish_step
  HDG_API_END(h)
}
int hdg_step(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.step();
  E.end_of_step();
  E.step_open = false;  // a whole step: complete
  E.tdi_raise();
  HDG_API_END(h)
}
int hdg_run_separable(hdg_handle* h, int nsteps, const double* scales) {
  HDG_API_BEGIN(h)
  if (nsteps < 0 || !scales) throw std::string("bad arguments");
  for (int n = 0; n < nsteps; n++) {
    for (int sl = 0; sl <= E.s; sl++) { E.bscale[sl] = scales[(long)n * (E.s + 1) + sl]; E.bsep[sl] = 1; }
    E.step();
    E.end_of_step();
    E.step_open = false;
    E.tdi_raise();
    E.harvest_completed();  // keeps the number of live timer events bounded over a long run
  }
  HDG_API_END(h)
}
int hdg_implicit_step(hdg_handle* h, int* its_tentative, int* its_pressure) {
  HDG_API_BEGIN(h)
  E.implicit_step(its_tentative, its_pressure);
  E.end_of_step();
  E.step_open = false;  // a whole step: complete
  E.tdi_raise();
  HDG_API_END(h)
}
// ---- implicit DG discretisation (dg_implicit.py:10-136), single rank
static int dg_single_rank(hdg_handle* h) {
  if (h && h->eng && h->eng->comm && h->eng->comm->size > 1) {
    h->err = "the DG discretisation runs on one rank only (strip partitions are not supported)";
    return HDG_ERR_UNSUPPORTED;
  }
  return HDG_OK;
}
int hdg_dg_implicit_step(hdg_handle* h, int* its) {
  if (int rc = dg_single_rank(h)) return rc;
  HDG_API_BEGIN(h)
  E.dg_implicit_step(its);
  E.end_of_step();
  E.step_open = false;  // a whole step: complete
  E.tdi_raise();
  HDG_API_END(h)
}
int hdg_apply_dg_operator(hdg_handle* h, const double* Qstar, const double* u, const double* p, double dt, double* out_u,
                          double* out_p) {
  if (int rc = dg_single_rank(h)) return rc;
  HDG_API_BEGIN(h)
  if (!Qstar || !u || !p || !out_u || !out_p) throw std::string("null argument");
  E.dg_alloc();
  E.put_Q(Qstar, E.wQ1);
  E.put_Q(u, E.wQ2);
  E.put_P(p, E.wP1);
  E.dg_operator(E.wQ1, E.wQ2, E.wP1, dt, E.wQ3, E.dg_b.p);
  E.get_Q(E.wQ3, out_u);
  E.get_P(E.dg_b.p, out_p);
  HDG_API_END(h)
}
int hdg_dg_avg_trace(hdg_handle* h, const double* p, double* lam) {
  if (int rc = dg_single_rank(h)) return rc;
  HDG_API_BEGIN(h)
  if (!p || !lam) throw std::string("null argument");
  E.dg_alloc();
  E.put_P(p, E.wP1);
  E.avg_trace(E.wP1, E.wL1);
  E.get_L(E.wL1, lam);
  HDG_API_END(h)
}
int hdg_get_iteration_stats(hdg_handle* h, double* sums, long* counts, int reset) {
  HDG_API_BEGIN(h)
  for (int i = 0; i < 4; i++) {
    if (sums) sums[i] = E.it_sum[i];
    if (counts) counts[i] = E.it_cnt[i];
    if (reset) { E.it_sum[i] = 0; E.it_cnt[i] = 0; }
  }
  HDG_API_END(h)
}
int hdg_get_solver_events(hdg_handle* h, long* events, int reset) {
  HDG_API_BEGIN(h)
  if (events) { events[0] = E.ev_cg_replacements; events[1] = E.ev_cg_floor_exits; events[2] = E.n_sstep_cycles; events[3] = E.n_sstep_fallbacks; }
  if (reset) { E.ev_cg_replacements = 0; E.ev_cg_floor_exits = 0; E.n_sstep_cycles = 0; E.n_sstep_fallbacks = 0; }
  HDG_API_END(h)
}
int hdg_get_kernel_forms(hdg_handle* h, int* forms) {
  HDG_API_BEGIN(h)
  if (!forms) throw std::string("forms is NULL");
  forms[0] = (int)E.lift_form();
  forms[1] = hdg::Engine::form_code(E.adv_form());
  forms[2] = E.general ? 3 : (E.use_trace_tile() ? (E.tile3() ? 2 : 1) : 0);
  forms[3] = E.general ? 3 : (E.use_mfma_schur() ? 2 : 0);
  HDG_API_END(h)
}
int hdg_get_timers(hdg_handle* h, double* total_ms, double* sumsq_ms, long* ncalls, int reset) {
  HDG_API_BEGIN(h)
  if (hipStreamSynchronize(E.stream) != hipSuccess) throw hdg::HipError{"hipStreamSynchronize failed"};
  E.harvest_timers();
  for (int i = 0; i < HDG_N_TIMERS; i++) {
    if (total_ms) total_ms[i] = E.tm_total[i];
    if (sumsq_ms) sumsq_ms[i] = E.tm_sumsq[i];
    if (ncalls) ncalls[i] = E.tm_calls[i];
    if (reset) { E.tm_total[i] = 0; E.tm_sumsq[i] = 0; E.tm_calls[i] = 0; }
  }
  HDG_API_END(h)
}
int hdg_get_comm_info(const hdg_handle* h, int* rank, int* nranks, int* transport_ranks, char* name16) {
  if (!h || !h->eng || !h->eng->comm) return HDG_ERR_ARG;
  const hdg::Comm& c = *h->eng->comm;
  if (rank) *rank = c.rank;
  if (nranks) *nranks = c.size;
  if (transport_ranks) *transport_ranks = c.transport_size();
  if (name16) { std::strncpy(name16, c.name(), 15); name16[15] = 0; }
  return HDG_OK;
}
int hdg_get_launch_stats(hdg_handle* h, long* calls, double* bytes, int reset) {
  if (!h || !h->eng) return HDG_ERR_ARG;
  hdg::Engine& E = *h->eng;
  for (int i = 0; i < HDG_N_LAUNCH_CLASSES; i++) {
    if (calls) calls[i] = E.lc_calls[i];
    if (bytes) bytes[i] = E.lc_bytes[i];
    if (reset) { E.lc_calls[i] = 0; E.lc_bytes[i] = 0.0; }
  }
  return HDG_OK;
}
int hdg_set_kernel_timing(hdg_handle* h, int on) {
  HDG_API_BEGIN(h)
  E.kernel_timing = on != 0;
  HDG_API_END(h)
}
// ---- passive tracer and continuous-space diagnostics
int hdg_set_tracer(hdg_handle* h, const double* q) {
  HDG_API_BEGIN(h)
  if (!q) { E.tracer_on = false; }
  else {
    E.cg_setup();
    E.tracer_alloc();
    for (int t = 0; t < E.n_tr; t++) E.put_P(q + t * E.NPb, E.q_cur + t * E.NPv);
    E.tracer_on = true;
  }
  HDG_API_END(h)
}
int hdg_get_tracer(hdg_handle* h, double* q) {
  HDG_API_BEGIN(h)
  if (!E.tracer_on || !q) throw std::string("no tracer field");
  for (int t = 0; t < E.n_tr; t++) E.get_P(E.q_cur + t * E.NPv, q + t * E.NPb);
  HDG_API_END(h)
}
int hdg_tracer_begin_step(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.step_open = true;
  E.tracer_begin_step();
  HDG_API_END(h)
}
int hdg_tracer_stage(hdg_handle* h, int stage) {
  HDG_API_BEGIN(h)
  E.tracer_stage(stage);
  HDG_API_END(h)
}
int hdg_tracer_finish_step(hdg_handle* h) {
  HDG_API_BEGIN(h)
  E.tracer_finish_step();
  if (E.tracer_on) { E.end_of_step(); E.step_open = false; }
  E.tdi_raise();
  HDG_API_END(h)
}
int hdg_cg_size(hdg_handle* h, long* n_cg) {
  HDG_API_BEGIN(h)
  if (!n_cg) throw std::string("null argument");
  E.cg_setup();
  *n_cg = E.cgt.ncg;
  HDG_API_END(h)
}
int hdg_cg_coordinates(hdg_handle* h, double* xy) {
  HDG_API_BEGIN(h)
  if (!xy) throw std::string("null argument");
  E.cg_setup();
  E.cg_coordinates(xy);
  HDG_API_END(h)
}
int hdg_cg_project_nodal(hdg_handle* h, const double* Qin, double* Qout) {
  HDG_API_BEGIN(h)
  if (!Qin || !Qout) throw std::string("null argument");
  E.put_Q(Qin, E.wQ1);
  E.cg_project(E.wQ1, E.wQ2);
  E.get_Q(E.wQ2, Qout);
  HDG_API_END(h)
}
int hdg_vorticity(hdg_handle* h, const double* Q, double* omega) {
  HDG_API_BEGIN(h)
  if (!omega) throw std::string("null argument");
  const double* src = E.curQ;
  if (Q) { E.put_Q(Q, E.wQ1); src = E.wQ1; }
  E.vorticity(src);
  if (hipMemcpyAsync(omega, E.cg_x, sizeof(double) * E.cgt.ncg, hipMemcpyDeviceToHost, E.stream) != hipSuccess)
    throw hdg::HipError{"hipMemcpyAsync failed"};
  HDG_API_END(h)
}
int hdg_cg_to_broken(hdg_handle* h, const double* cg_values, double* broken) {
  HDG_API_BEGIN(h)
  if (!cg_values || !broken) throw std::string("null argument");
  E.cg_setup();
  if (hipMemcpyAsync(E.cg_b, cg_values, sizeof(double) * E.cgt.ncg, hipMemcpyHostToDevice, E.stream) != hipSuccess)
    throw hdg::HipError{"hipMemcpyAsync failed"};
  const int K = E.K;
  if (E.general) E.csr(E.gcgd.R, E.cg_b, 1.0, 0.0, E.hQ_dev);
  else { E.by_degree([&](auto k) { hdg::k_cg_to_broken<k()><<<E.cell_grid(), E.bs(), 0, E.stream>>>(E.g, E.cgt, E.cg_b, E.hQ_dev); }); }
  if (hipMemcpyAsync(broken, E.hQ_dev, sizeof(double) * E.NQb / 2, hipMemcpyDeviceToHost, E.stream) != hipSuccess)
    throw hdg::HipError{"hipMemcpyAsync failed"};
  HDG_API_END(h)
}
// ---- stream function (include/hdg_streamfunction.h)
// structured meshes on one rank, between steps; 0: go on
static int psi_refusal(hdg_handle* h, const char* call) {
  if (!h || !h->eng) return HDG_ERR_ARG;
  if (h->eng->general) { h->err = std::string(call) + ": general meshes are not supported (structured meshes only)"; return HDG_ERR_UNSUPPORTED; }
  if (h->eng->comm->size > 1) { h->err = std::string(call) + ": strip partitions are not supported (one rank only)"; return HDG_ERR_UNSUPPORTED; }
  if (h->eng->step_open) { h->err = std::string(call) + ": a step is open (between hdg_begin_step and the end of the step)"; return HDG_ERR_ARG; }
  return 0;
}
static void psi_copy(hdg::Engine& E, void* dst, const void* src, long n, hipMemcpyKind kind) {
  if (hipMemcpyAsync(dst, src, sizeof(double) * n, kind, E.stream) != hipSuccess) throw hdg::HipError{"hipMemcpyAsync failed"};
}
int hdg_streamfunction(hdg_handle* h, const double* Q, double rtol, double* psi, double info[8]) {
  if (const int rc = psi_refusal(h, "hdg_streamfunction")) return rc;
  HDG_API_BEGIN(h)
  if (!psi || !info) throw std::string("null argument");
  if (!(rtol > 0.0 && rtol < 1.0)) throw std::string("hdg_streamfunction: rtol must lie in (0, 1)");
  hdg::Engine::TallyGuard keep(E);
  const double* src = E.curQ;
  if (Q) { E.put_Q(Q, E.wQ1); src = E.wQ1; }
  E.streamfunction(src, rtol, info);
  psi_copy(E, psi, E.cg_x, E.cgt.ncg, hipMemcpyDeviceToHost);
  HDG_API_END(h)
}
int hdg_apply_cg_stiffness(hdg_handle* h, const double* x, double* y) {
  if (const int rc = psi_refusal(h, "hdg_apply_cg_stiffness")) return rc;
  HDG_API_BEGIN(h)
  if (!x || !y) throw std::string("null argument");
  hdg::Engine::TallyGuard keep(E);
  E.psi_setup();
  psi_copy(E, E.cg_b, x, E.cgt.ncg, hipMemcpyHostToDevice);
  E.psi_stiff(E.cg_b, E.cg_x);
  psi_copy(E, y, E.cg_x, E.cgt.ncg, hipMemcpyDeviceToHost);
  HDG_API_END(h)
}
int hdg_psi_transfer(hdg_handle* h, int dir, const double* in, double* out) {
  if (const int rc = psi_refusal(h, "hdg_psi_transfer")) return rc;
  HDG_API_BEGIN(h)
  if (!in || !out) throw std::string("null argument");
  if (dir != 0 && dir != 1) throw std::string("hdg_psi_transfer: dir must be 0 (P) or 1 (P^T)");
  hdg::Engine::TallyGuard keep(E);
  E.psi_setup();
  if (dir == 0) {
    psi_copy(E, E.mg_b[0], in, E.psi_vertices(), hipMemcpyHostToDevice);
    E.psi_prolong(E.mg_b[0], nullptr, E.cg_x);
    psi_copy(E, out, E.cg_x, E.cgt.ncg, hipMemcpyDeviceToHost);
  } else {
    psi_copy(E, E.cg_b, in, E.cgt.ncg, hipMemcpyHostToDevice);
    E.psi_restrict(E.cg_b, E.mg_b[0]);
    psi_copy(E, out, E.mg_b[0], E.psi_vertices(), hipMemcpyDeviceToHost);
  }
  HDG_API_END(h)
}
int hdg_apply_psi_preconditioner(hdg_handle* h, int form, const double* r, double* z) {
  if (const int rc = psi_refusal(h, "hdg_apply_psi_preconditioner")) return rc;
  HDG_API_BEGIN(h)
  if (!r || !z) throw std::string("null argument");
  if (form != 0 && form != 1) throw std::string("hdg_apply_psi_preconditioner: form must be 0 (the solve's) or 1 (the diagonal alone)");
  hdg::Engine::TallyGuard keep(E);
  E.psi_setup();
  psi_copy(E, E.cg_rr, r, E.cgt.ncg, hipMemcpyHostToDevice);
  E.psi_precond(form == 1 || E.opt.psi_jacobi, E.cg_rr, E.cg_zz);
  psi_copy(E, z, E.cg_zz, E.cgt.ncg, hipMemcpyDeviceToHost);
  HDG_API_END(h)
}
int hdg_psi_vertex_count(hdg_handle* h, long* n_vertices) {
  if (const int rc = psi_refusal(h, "hdg_psi_vertex_count")) return rc;
  HDG_API_BEGIN(h)
  if (!n_vertices) throw std::string("null argument");
  E.psi_setup();
  *n_vertices = E.psi_vertices();
  HDG_API_END(h)
}
int hdg_apply_tracer_advection(hdg_handle* h, const double* q, const double* u, int project, double* out) {
  HDG_API_BEGIN(h)
  if (!q || !u || !out) throw std::string("null argument");
  E.cg_setup();
  E.tracer_alloc();
  E.put_Q(u, E.wQ1);
  const double* vel = E.wQ1;
  if (project) { E.cg_project(E.wQ1, E.uproj); vel = E.uproj; }
  E.put_P(q, E.wP1);
  E.tracer_adv(E.wP1, vel, E.q_t, 1);
  E.get_P(E.q_t, out);
  HDG_API_END(h)
}
int hdg_apply_advection(hdg_handle* h, const double* Qstar, const double* x, double gamma, double* y) {
  HDG_API_BEGIN(h)
  if (!Qstar || !x || !y) throw std::string("null argument");
  E.put_Q(Qstar, E.wQ1);
  E.put_Q(x, E.wQ2);
  E.adv_apply(E.wQ2, E.wQ1, E.wQ3, gamma);
  E.get_Q(E.wQ3, y);
  HDG_API_END(h)
}
int hdg_apply_trace_operator(hdg_handle* h, const double* lam, double* out) {
  HDG_API_BEGIN(h)
  if (!lam || !out) throw std::string("null argument");
  E.put_L(lam, E.wL1);
  E.trace_apply(E.wL1, nullptr, 0.0, 1.0, E.wL2);
  // return modal coefficients of the DUAL vector mapped back through the (orthonormal) Riesz map
  E.get_L(E.wL2, out);
  HDG_API_END(h)
}
int hdg_apply_weak_divergence(hdg_handle* h, const double* Q, int broken, double* out_p) {
  HDG_API_BEGIN(h)
  if (!Q || !out_p) throw std::string("null argument");
  E.put_Q(Q, E.wQ1);
  E.weak_div(E.wQ1, 1.0, E.wP1, broken != 0);
  E.get_P(E.wP1, out_p);
  HDG_API_END(h)
}

int hdg_node_coordinates(hdg_handle* h, double* xq, double* xp) {
  HDG_API_BEGIN(h)
  E.node_coords(xq, xp);
  HDG_API_END(h)
}
int hdg_l2_norms(hdg_handle* h, const double* Q, const double* p, double* norm_Q, double* norm_p) {
  HDG_API_BEGIN(h)
  if (Q && norm_Q) { E.put_Q(Q, E.wQ1); *norm_Q = std::sqrt(E.dot(E.NQ, E.wQ1, E.wQ1, hdg::Engine::KQ)); }
  if (p && norm_p) { E.put_P(p, E.wP1); *norm_p = std::sqrt(E.dot(E.NPv, E.wP1, E.wP1, hdg::Engine::KC)); }
  HDG_API_END(h)
}
int hdg_integrate_pressure(hdg_handle* h, const double* p, double* integral) {
  HDG_API_BEGIN(h)
  if (!p || !integral) throw std::string("null argument");
  E.put_P(p, E.wP1);
  *integral = E.general ? E.dot(E.NPv, E.wP1, E.d_int_p, hdg::Engine::KC)
                        : E.g.h / std::sqrt(2.0) * E.dot(E.g.Nc, E.wP1, E.ones_c, hdg::Engine::KC);
  HDG_API_END(h)
}
int hdg_compute_diagnostics(hdg_handle* h, const double* Q, const double* p, const double* q, double* out) {
  HDG_API_BEGIN(h)
  if (!Q || !p || !out) throw std::string("null argument");
  E.diag_compute(Q, p, q, out);
  HDG_API_END(h)
}
int hdg_set_diagnostics(hdg_handle* h, int capacity) {
  HDG_API_BEGIN(h)
  E.diag_set(capacity);
  HDG_API_END(h)
}
int hdg_get_diagnostics(hdg_handle* h, double* rows, int max_rows, int* n_rows, int reset) {
  HDG_API_BEGIN(h)
  E.log_get("diagnostics", E.diag_log, E.diag_rows, rows, max_rows, n_rows, reset);
  HDG_API_END(h)
}
int hdg_evaluate_points(hdg_handle* h, const double* Q, const double* p, const double* q, int n, const double* xy, double* out,
                        int* located) {
  HDG_API_BEGIN(h)
  if (n < 0 || (n > 0 && (!xy || !out || !located))) throw std::string("null argument");
  E.points_evaluate(Q, p, q, n, xy, out, located);
  HDG_API_END(h)
}
int hdg_set_probes(hdg_handle* h, int n, const double* xy, int capacity) {
  HDG_API_BEGIN(h)
  if (n > 0 && capacity > 0 && !xy) throw std::string("null argument");
  E.probe_set(n, xy, capacity);
  HDG_API_END(h)
}
int hdg_get_probes(hdg_handle* h, double* rows, int max_rows, int* n_rows, int reset) {
  HDG_API_BEGIN(h)
  E.log_get("probes", E.probe_log, E.pt_rows, rows, max_rows, n_rows, reset);
  HDG_API_END(h)
}
int hdg_set_particles(hdg_handle* h, int n, const double* xy, int capacity, int record_every) {
  if (h && h->eng && h->eng->general) {
    h->err = "general meshes: particles are not implemented (location on the device and leaving a polygonal boundary; "
             "structured meshes only)";
    return HDG_ERR_UNSUPPORTED;
  }
  HDG_API_BEGIN(h)
  if (n > 0 && capacity > 0 && !xy) throw std::string("null argument");
  E.particles_set(n, xy, capacity, record_every);
  HDG_API_END(h)
}
int hdg_get_particles(hdg_handle* h, double* rows, int max_rows, int* n_rows, long* counts, int reset) {
  HDG_API_BEGIN(h)
  E.log_get("particles", E.pa_log, E.pa_rows, rows, max_rows, n_rows, reset, counts);
  HDG_API_END(h)
}
int hdg_advance_particles(hdg_handle* h, double dt, int nsteps) {
  HDG_API_BEGIN(h)
  E.particles_frozen(dt, nsteps);
  HDG_API_END(h)
}
int hdg_time_kernel(hdg_handle* h, int kernel, int reps, double* ms_per_launch) {
  HDG_API_BEGIN(h)
  if (reps < 1 || !ms_per_launch) throw std::string("bad arguments");
  *ms_per_launch = E.time_kernel(kernel, reps);
  HDG_API_END(h)
}

// ---- checkpoint and restart (include/hdg_checkpoint.h)
int hdg_checkpoint_size(hdg_handle* h, long* nbytes) {
  HDG_API_BEGIN(h)
  if (!nbytes) throw std::string("null argument");
  *nbytes = E.checkpoint_size();
  HDG_API_END(h)
}
int hdg_checkpoint_save(hdg_handle* h, long step, double t, void* buf, long nbytes) {
  HDG_API_BEGIN(h)
  E.checkpoint_save(step, t, buf, nbytes);
  HDG_API_END(h)
}
int hdg_checkpoint_load(hdg_handle* h, const void* buf, long nbytes, long* step, double* t) {
  HDG_API_BEGIN(h)
  E.checkpoint_load(buf, nbytes, step, t);
  HDG_API_END(h)
}
int hdg_state_digest(hdg_handle* h, unsigned long long out[2]) {
  HDG_API_BEGIN(h)
  E.state_digest(out);
  HDG_API_END(h)
}
int hdg_digest_vector(hdg_handle* h, const double* v, long n, unsigned long long out[2]) {
  HDG_API_BEGIN(h)
  E.digest_host_vector(v, n, out);
  HDG_API_END(h)
}

// ---- transfer between engines (include/hdg_transfer.h)
// the checks of a pair that end in HDG_ERR_UNSUPPORTED, or in HDG_ERR_ARG before an engine is looked at; 0: go on
static int transfer_pair_gate(hdg_handle* a, const hdg_handle* b, const char* call, bool same_allowed, int* r) {
  if (!a || !a->eng) return HDG_ERR_ARG;
  if (!b || !b->eng) { a->err = std::string(call) + ": null engine"; return HDG_ERR_ARG; }
  if (a == b && !same_allowed) { a->err = std::string(call) + ": dst == src (an engine cannot be transferred onto itself)"; return HDG_ERR_ARG; }
  try {
    std::string unsupported;
    hdg::Engine::transfer_pair_check(*a->eng, *b->eng, call, unsupported, *r);
    if (!unsupported.empty()) { a->err = unsupported; return HDG_ERR_UNSUPPORTED; }
  } catch (const std::string& e) { a->err = e; return HDG_ERR_ARG; }
  return HDG_OK;
}
int hdg_transfer_state(hdg_handle* dst, const hdg_handle* src, int with_tracers) {
  int r = 1;
  if (const int rc = transfer_pair_gate(dst, src, "hdg_transfer_state", false, &r)) return rc;
  HDG_API_BEGIN(dst)
  E.transfer_from(*src->eng, r, with_tracers != 0);
  HDG_API_END(dst)
}
int hdg_transfer_difference(hdg_handle* a, hdg_handle* b, double* norm_Q, double* norm_p, double* norm_q) {
  int r = 1;
  if (const int rc = transfer_pair_gate(a, b, "hdg_transfer_difference", true, &r)) return rc;
  HDG_API_BEGIN(a)
  hdg::Engine::transfer_difference(E, *b->eng, r, norm_Q, norm_p, norm_q);
  HDG_API_END(a)
}


// ---- tracer diffusion (include/hdg_tracer_diffusion.h)
int hdg_set_tracer_diffusivity(hdg_handle* h, int n, const double* kappa) {
  HDG_API_BEGIN(h)
  E.set_tracer_diffusivity(n, kappa);
  HDG_API_END(h)
}
int hdg_get_tracer_diffusion_number(hdg_handle* h, double out2[2]) {
  HDG_API_BEGIN(h)
  if (!out2) throw std::string("null argument");
  E.tracer_diffusion_number(out2);
  HDG_API_END(h)
}
int hdg_apply_tracer_diffusion(hdg_handle* h, const double* q, double* out) {
  HDG_API_BEGIN(h)
  if (!q || !out) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_apply_tracer_diffusion: a step is open");
  E.diff_setup();
  E.tracer_alloc();
  E.put_P(q, E.wP1);
  E.apply_tracer_diffusion(E.wP1, E.q_t);
  E.get_P(E.q_t, out);
  HDG_API_END(h)
}


// ---- tracer wall conditions (include/hdg_tracer_walls.h)
int hdg_set_tracer_walls(hdg_handle* h, int n, const int* kind, const double* value) {
  HDG_API_BEGIN(h)
  E.set_tracer_walls(n, kind, value);
  HDG_API_END(h)
}
int hdg_get_tracer_wall_flux(hdg_handle* h, int n, double* flux) {
  HDG_API_BEGIN(h)
  if (!flux) throw std::string("null argument");
  if (!E.tracer_on) throw std::string("hdg_get_tracer_wall_flux: no tracer is set (hdg_set_tracer)");
  if (E.step_open) throw std::string("hdg_get_tracer_wall_flux: a step is open");
  if (n != E.n_tr) throw std::string("hdg_get_tracer_wall_flux: " + std::to_string(n) + " row(s) for " + std::to_string(E.n_tr) + " tracer(s)");
  E.tracer_wall_flux(flux);
  HDG_API_END(h)
}
int hdg_apply_tracer_wall_diffusion(hdg_handle* h, const int kind[4], const double value[4], const double* q, double* out) {
  HDG_API_BEGIN(h)
  if (!kind || !q || !out) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_apply_tracer_wall_diffusion: a step is open");
  E.diff_setup();
  E.tracer_alloc();
  E.put_P(q, E.wP1);
  E.apply_tracer_wall_diffusion(kind, value, E.wP1, E.q_t);
  E.get_P(E.q_t, out);
  HDG_API_END(h)
}


// ---- implicit tracer diffusion (include/hdg_tracer_implicit.h)
// structured meshes on one rank; 0: go on
static int tdi_refusal(hdg_handle* h, const char* call) {
  if (!h || !h->eng) return HDG_ERR_ARG;
  if (h->eng->general) { h->err = std::string(call) + ": general meshes are not supported (structured meshes only)"; return HDG_ERR_UNSUPPORTED; }
  if (h->eng->comm->size > 1) { h->err = std::string(call) + ": strip partitions are not supported (one rank only)"; return HDG_ERR_UNSUPPORTED; }
  return 0;
}
int hdg_set_tracer_diffusion_mode(hdg_handle* h, int mode, double rtol, int max_iterations) {
  if (const int rc = tdi_refusal(h, "hdg_set_tracer_diffusion_mode")) return rc;
  HDG_API_BEGIN(h)
  E.set_tracer_diffusion_mode(mode, rtol, max_iterations);
  HDG_API_END(h)
}
int hdg_get_tracer_diffusion_solve(hdg_handle* h, int n, int* its, double* res) {
  HDG_API_BEGIN(h)
  if (!its || !res) throw std::string("null argument");
  if (n < 1 || n > HDG_MAX_TRACERS) throw std::string("hdg_get_tracer_diffusion_solve: n = " + std::to_string(n) + " is out of range");
  for (int t = 0; t < n; t++) { its[t] = E.tdi_its[(size_t)t]; res[t] = E.tdi_res[(size_t)t]; }
  HDG_API_END(h)
}
int hdg_solve_tracer_diffusion(hdg_handle* h, int n, const double* tau, const double* q_in, double* q_out, int* its) {
  if (const int rc = tdi_refusal(h, "hdg_solve_tracer_diffusion")) return rc;
  HDG_API_BEGIN(h)
  if (!tau || !q_in || !q_out) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_solve_tracer_diffusion: a step is open (between hdg_begin_step and the end of the step)");
  if (n < 1 || n > E.n_tr) throw std::string("hdg_solve_tracer_diffusion: " + std::to_string(n) + " field(s) on an engine of " + std::to_string(E.n_tr) + " tracer(s)");
  for (int t = 0; t < n; t++)
    if (!(tau[t] >= 0.0) || !std::isfinite(tau[t])) throw std::string("hdg_solve_tracer_diffusion: tau[" + std::to_string(t) + "] is not a finite value >= 0");
  hdg::Engine::TallyGuard keep(E);
  E.tracer_alloc();
  for (int t = 0; t < n; t++) E.put_P(q_in + t * E.NPb, E.q_t + t * E.NPv);
  E.solve_tracer_diffusion(n, tau);
  for (int t = 0; t < n; t++) { E.get_P(E.q_t + t * E.NPv, q_out + t * E.NPb); if (its) its[t] = E.tdi_its[(size_t)t]; }
  if (hipStreamSynchronize(E.stream) != hipSuccess) throw hdg::HipError{"hipStreamSynchronize failed"};
  E.tdi_raise();
  HDG_API_END(h)
}


// ---- Boussinesq buoyancy (include/hdg_buoyancy.h)
int hdg_set_buoyancy(hdg_handle* h, int n, const double* beta, const double g[2]) {
  HDG_API_BEGIN(h)
  E.set_buoyancy(n, beta, g);
  HDG_API_END(h)
}
int hdg_get_buoyancy(hdg_handle* h, int n, double* beta, double g[2]) {
  HDG_API_BEGIN(h)
  if (!beta || !g) throw std::string("null argument");
  if (n != E.n_tr) throw std::string("hdg_get_buoyancy: " + std::to_string(n) + " value(s) for " + std::to_string(E.n_tr) + " tracer(s)");
  for (int t = 0; t < n; t++) beta[t] = E.by_beta.empty() ? 0.0 : E.by_beta[(size_t)t];
  g[0] = E.by_g[0]; g[1] = E.by_g[1];
  HDG_API_END(h)
}
int hdg_apply_buoyancy(hdg_handle* h, const double* q, double* f) {
  HDG_API_BEGIN(h)
  if (!q || !f) throw std::string("null argument");
  if (E.comm->size > 1) E.cg_setup();  // a strip: the tracer error of hdg_set_tracer
  if (E.step_open) throw std::string("hdg_apply_buoyancy: a step is open");
  E.tracer_alloc();
  for (int t = 0; t < E.n_tr; t++) E.put_P(q + t * E.NPb, E.q_t + t * E.NPv);
  E.zero(E.wQ1, E.NQ);
  E.buoyancy(E.q_t, E.wQ1);
  E.get_Q(E.wQ1, f);
  HDG_API_END(h)
}


// ---- viscous term (include/hdg_viscosity.h)
int hdg_set_viscosity(hdg_handle* h, double nu, int wall) {
  HDG_API_BEGIN(h)
  E.set_viscosity(nu, wall);
  HDG_API_END(h)
}
int hdg_get_viscosity(hdg_handle* h, double* nu, int* wall, double out2[2]) {
  HDG_API_BEGIN(h)
  if (!nu || !wall) throw std::string("null argument");
  *nu = E.visc_nu; *wall = E.visc_wall;
  if (out2) E.viscosity_number(E.visc_nu, E.visc_wall, out2);
  HDG_API_END(h)
}
int hdg_apply_viscosity(hdg_handle* h, int wall, const double* Q, double* out) {
  HDG_API_BEGIN(h)
  if (!Q || !out) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_apply_viscosity: a step is open");
  hdg::Engine::visc_check_wall("hdg_apply_viscosity", wall);
  E.visc_setup(wall);
  E.put_Q(Q, E.wQ1);
  E.zero(E.wQ2, E.NQ);
  E.viscosity_apply(E.wQ1, 1.0, wall, E.wQ2);
  E.get_Q(E.wQ2, out);
  HDG_API_END(h)
}

// ---- moving no-slip walls and the wall force (include/hdg_moving_walls.h)
// a general mesh has no sides to name: speeds other than zero, and the force, are HDG_ERR_UNSUPPORTED there; 0: go on
static int moving_walls_gate(hdg_handle* h, const char* call, const double* U, bool force) {
  if (!h || !h->eng) return HDG_ERR_ARG;
  if (!h->eng->general) return HDG_OK;
  if (force) { h->err = std::string(call) + ": general meshes are not supported (the structured unit square only)"; return HDG_ERR_UNSUPPORTED; }
  if (U && !(U[0] == 0.0 && U[1] == 0.0 && U[2] == 0.0 && U[3] == 0.0)) {
    h->err = std::string(call) + ": a wall velocity on a general mesh is not supported (the structured unit square only)";
    return HDG_ERR_UNSUPPORTED;
  }
  return HDG_OK;
}
int hdg_set_wall_velocity(hdg_handle* h, const double U[4]) {
  if (const int rc = moving_walls_gate(h, "hdg_set_wall_velocity", U, false)) return rc;
  HDG_API_BEGIN(h)
  E.set_wall_velocity(U);
  HDG_API_END(h)
}
int hdg_get_wall_velocity(hdg_handle* h, double U[4]) {
  HDG_API_BEGIN(h)
  if (!U) throw std::string("null argument");
  for (int w = 0; w < 4; w++) U[w] = E.wall_u[w];
  HDG_API_END(h)
}
int hdg_get_wall_force(hdg_handle* h, double F[8]) {
  if (const int rc = moving_walls_gate(h, "hdg_get_wall_force", nullptr, true)) return rc;
  HDG_API_BEGIN(h)
  if (!F) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_get_wall_force: a step is open");
  E.wall_force(E.curQ, E.visc_nu, E.visc_wall, E.wall_u, F);
  HDG_API_END(h)
}
int hdg_apply_moving_walls(hdg_handle* h, int wall, const double U[4], const double* Q, double* out) {
  if (const int rc = moving_walls_gate(h, "hdg_apply_moving_walls", U, false)) return rc;
  HDG_API_BEGIN(h)
  if (!Q || !out) throw std::string("null argument");
  hdg::Engine::visc_check_wall("hdg_apply_moving_walls", wall);
  E.check_wall_velocity("hdg_apply_moving_walls", U, wall);
  E.visc_setup(wall);
  E.put_Q(Q, E.wQ1);
  E.zero(E.wQ2, E.NQ);
  E.viscosity_apply(E.wQ1, 1.0, wall, E.wQ2, U);
  E.get_Q(E.wQ2, out);
  HDG_API_END(h)
}
int hdg_apply_wall_force(hdg_handle* h, int wall, const double U[4], const double* Q, double F[8]) {
  if (const int rc = moving_walls_gate(h, "hdg_apply_wall_force", U, true)) return rc;
  HDG_API_BEGIN(h)
  if (!Q || !F) throw std::string("null argument");
  hdg::Engine::visc_check_wall("hdg_apply_wall_force", wall);
  E.check_wall_velocity("hdg_apply_wall_force", U, wall);
  E.put_Q(Q, E.wQ1);
  E.wall_force(E.wQ1, 1.0, wall, U, F);
  HDG_API_END(h)
}

// ---- Coriolis term (include/hdg_coriolis.h)
int hdg_set_coriolis(hdg_handle* h, double f0, double beta) {
  HDG_API_BEGIN(h)
  E.set_coriolis(f0, beta);
  HDG_API_END(h)
}
int hdg_get_coriolis(hdg_handle* h, double* f0, double* beta, double out2[2]) {
  HDG_API_BEGIN(h)
  if (!f0 || !beta) throw std::string("null argument");
  *f0 = E.cor_f0; *beta = E.cor_beta;
  if (out2) {
    out2[0] = E.coriolis_bound(E.cor_f0, E.cor_beta);
    out2[1] = out2[0] * E.cfg.dt;
  }
  HDG_API_END(h)
}
int hdg_apply_coriolis(hdg_handle* h, double f0, double beta, const double* Q, double* out) {
  HDG_API_BEGIN(h)
  if (!Q || !out) throw std::string("null argument");
  E.coriolis_check("hdg_apply_coriolis", f0, beta);
  E.coriolis_setup();
  E.put_Q(Q, E.wQ1);
  E.zero(E.wQ2, E.NQ);
  E.coriolis_apply(E.wQ1, f0, beta, false, E.wQ2);
  E.get_Q(E.wQ2, out);
  HDG_API_END(h)
}

// ---- linear drag (include/hdg_drag.h)
int hdg_set_drag(hdg_handle* h, const double* sigma, const double* target, const int* region) {
  HDG_API_BEGIN(h)
  E.set_drag(sigma, target, region);
  HDG_API_END(h)
}
int hdg_get_drag(hdg_handle* h, double* sigma, double out2[2]) {
  HDG_API_BEGIN(h)
  if (sigma) {
    if (E.drag_on()) std::copy(E.drag_sigma.begin(), E.drag_sigma.end(), sigma);
    else std::fill(sigma, sigma + 3 * E.drag_cells(), 0.0);
  }
  if (out2) { out2[0] = E.drag_S; out2[1] = E.drag_S * E.cfg.dt; }
  HDG_API_END(h)
}
int hdg_apply_drag(hdg_handle* h, const double* sigma, const double* target, const double* Q, double* out) {
  HDG_API_BEGIN(h)
  if (!sigma || !Q || !out) throw std::string("null argument");
  E.drag_check("hdg_apply_drag", sigma, target, nullptr);
  hdg::Engine::DragSet D = E.drag_build(sigma, target, nullptr);
  E.put_Q(Q, E.wQ1);
  E.zero(E.wQ2, E.NQ);
  E.drag_apply(D, E.wQ1, -1.0, D.load, false, E.wQ2);
  E.get_Q(E.wQ2, out);
  E.drag_release(D);
  HDG_API_END(h)
}
int hdg_get_drag_force(hdg_handle* h, double F[12]) {
  HDG_API_BEGIN(h)
  if (!F) throw std::string("null argument");
  if (E.step_open) throw std::string("hdg_get_drag_force: a step is open");
  std::fill(F, F + 12, 0.0);
  if (E.drag_on()) E.drag_force(E.drag_set, E.curQ, F);
  HDG_API_END(h)
}
int hdg_apply_drag_force(hdg_handle* h, const double* sigma, const double* target, const int* region, const double* Q, double F[12]) {
  HDG_API_BEGIN(h)
  if (!sigma || !Q || !F) throw std::string("null argument");
  E.drag_check("hdg_apply_drag_force", sigma, target, region);
  hdg::Engine::DragSet D = E.drag_build(sigma, target, region);
  E.put_Q(Q, E.wQ1);
  E.drag_force(D, E.wQ1, F);
  E.drag_release(D);
  HDG_API_END(h)
}

// ---- adaptive time step (include/hdg_adaptive_dt.h)
int hdg_set_dt(hdg_handle* h, double dt) {
  HDG_API_BEGIN(h)
  E.set_dt(dt);
  HDG_API_END(h)
}
int hdg_get_dt(const hdg_handle* h, double* dt) {
  if (!h || !h->eng || !dt) return HDG_ERR_ARG;
  *dt = h->eng->cfg.dt;
  return HDG_OK;
}
int hdg_get_step_rates(hdg_handle* h, double rates[4]) {
  HDG_API_BEGIN(h)
  if (!rates) throw std::string("null argument");
  E.step_rates(rates);
  HDG_API_END(h)
}
int hdg_step_proposal(const hdg_step_control* control, double A, double dt, double t, double t_final, double* dt_new) {
  if (!control || !dt_new) return HDG_ERR_ARG;
  switch (hdg::step_proposal(*control, A, dt, t, t_final, *dt_new)) {
    case hdg::StepVerdict::Ok: return HDG_OK;
    case hdg::StepVerdict::NotFinite: return HDG_ERR_NOT_CONVERGED;
    default: return HDG_ERR_ARG;
  }
}
int hdg_propose_dt(hdg_handle* h, const hdg_step_control* control, double t, double t_final, double* dt_new) {
  HDG_API_BEGIN(h)
  if (!control || !dt_new) throw std::string("null argument");
  *dt_new = E.propose_dt(*control, t, t_final);
  HDG_API_END(h)
}

}  // extern "C"
