// CPU check of the host side of the general-mesh path (no GPU, no HIP): topology, assembled operators, P1 coarse space,
// smoothed-aggregation hierarchy, continuous space, repeatability of the threaded per-cell assembly.  Reads
// "nv nc / coords / cells" from argv[1], degree from argv[2]; prints "name value" lines that tests/test_host.py asserts on.
// argv[3] == "rows": only the average row length ("rowlen_<operator> <nnz / nrows>") of every operator the engine uploads
// with upload_csr (hdg_engine.hip), for the default hierarchy (HDG_AMG_MAX_COARSE unset); not printed: the inverse diagonals
// of the unfused smoother (one entry per row on every mesh) and the tau' copies of the trace operators (the same sparsity as
// the tau set).  Also "parallel_for_threads": how many threads parallel_for used on the mesh.  Compiled with g++ by the test.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <string>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_amg.hpp"

using namespace hdg;

static dvec spmv(const Csr& A, const dvec& x) {
  dvec y((size_t)A.nrows, 0.0);
  for (int r = 0; r < A.nrows; r++)
    for (int q = A.rowptr[(size_t)r]; q < A.rowptr[(size_t)r + 1]; q++) y[(size_t)r] += A.val[(size_t)q] * x[(size_t)A.col[(size_t)q]];
  return y;
}
static double maxabs(const dvec& v) { double m = 0; for (double x : v) m = std::max(m, std::fabs(x)); return m; }
static double asym(const Csr& A) {  // max |A - A^T|
  const Csr T = csr_transpose(A);
  double m = 0;
  for (int r = 0; r < A.nrows; r++) {
    int q = A.rowptr[(size_t)r], p = T.rowptr[(size_t)r];
    const int qe = A.rowptr[(size_t)r + 1], pe = T.rowptr[(size_t)r + 1];
    while (q < qe || p < pe) {
      const int ca = q < qe ? A.col[(size_t)q] : 1 << 30, ct = p < pe ? T.col[(size_t)p] : 1 << 30;
      if (ca == ct) { m = std::max(m, std::fabs(A.val[(size_t)q] - T.val[(size_t)p])); q++; p++; }
      else if (ca < ct) { m = std::max(m, std::fabs(A.val[(size_t)q])); q++; }
      else { m = std::max(m, std::fabs(T.val[(size_t)p])); p++; }
    }
  }
  return m;
}

static bool same_bits(const dvec& a, const dvec& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}
static bool same_csr(const Csr& a, const Csr& b) {
  return a.nrows == b.nrows && a.ncols == b.ncols && a.rowptr == b.rowptr && a.col == b.col && same_bits(a.val, b.val);
}
#define GENERAL_OPS(X)                                                                                                          \
  X(Pi) X(Wdiv) X(Bdiv) X(Gp) X(Gl) X(Yw) X(Yp) X(S) X(Auu) X(Aup) X(Apu) X(App) X(Wu) X(Wp) X(Dtr) X(Rq) X(Rp) X(Rb)       \
  X(Psi_p) X(Psi_l) X(Mu_u) X(Mu_p) X(Mu_l) X(Cq) X(Cqi) X(Cp) X(Cpi) X(Cl) X(Cli)
static void print_rowlen(const char* name, const Csr& A) {
  std::printf("rowlen_%s %.6f\n", name, A.nrows > 0 ? (double)A.val.size() / A.nrows : 0.0);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nv, nc;
  if (std::fscanf(f, "%d %d", &nv, &nc) != 2) return 2;
  std::vector<double> X((size_t)2 * nv);
  std::vector<int> C((size_t)3 * nc);
  for (auto& v : X) if (std::fscanf(f, "%lf", &v) != 1) return 2;
  for (auto& v : C) if (std::fscanf(f, "%d", &v) != 1) return 2;
  std::fclose(f);
  const int k = std::atoi(argv[2]);
  try {
    GMesh M;
    M.build(nv, X.data(), nc, C.data());
    GeneralTables T(k, 1.0, 1.0, 0);
    GeneralOps O;
    std::vector<CellLocal> loc;
    assemble_general(T, M, O, loc);
    std::printf("nv %d\nnc %d\nne %d\nvolume %.15e\n", M.nv, M.nc, M.ne, M.volume);
    if (argc > 3 && std::string(argv[3]) == "rows") {  // what upload_csr bases the threads per row on
#define ROWLEN(name) print_rowlen(#name, O.name);
      GENERAL_OPS(ROWLEN)
#undef ROWLEN
      const Csr P0 = p1_to_trace_matrix(T, M), R0 = csr_transpose(P0);
      print_rowlen("P0", P0);
      print_rowlen("R0", R0);
      AmgHierarchy H;
      amg_build(csr_multiply(R0, csr_multiply(O.S, P0)), H, 2000);  // the engine's default coarsening limit
      std::printf("amg_levels %d\n", (int)H.lev.size());
      for (size_t l = 0; l < H.lev.size(); l++) {
        print_rowlen(("amg_A" + std::to_string(l)).c_str(), H.lev[l].A);
        if (l + 1 < H.lev.size()) {
          print_rowlen(("amg_P" + std::to_string(l)).c_str(), H.lev[l].P);
          print_rowlen(("amg_R" + std::to_string(l)).c_str(), H.lev[l].R);
        }
      }
      if (H.coarse_pinv.nrows > 0) print_rowlen("amg_coarse_pinv", H.coarse_pinv);
      // element block-Jacobi (HDG_GENERAL_CSR_LIFT / HDG_GENERAL_BLOCK_JACOBI) and the continuous space (cg_setup)
      print_rowlen("block_jacobi", assemble_block_jacobi(T, M, loc, 0.0375));
      GeneralCG G;
      assemble_cg(T, M, O, G);
      print_rowlen("cg_M", G.M);
      print_rowlen("cg_Vort", G.Vort);
      print_rowlen("cg_R", G.R);
      for (int d = 0; d < 2; d++) {
        print_rowlen(("cg_Bp" + std::to_string(d)).c_str(), G.Bp[d]);
        print_rowlen(("cg_Ep" + std::to_string(d)).c_str(), G.Ep[d]);
      }
      return 0;
    }
    {  // how many threads parallel_for really uses on this mesh (one below 256 cells or on a one-core host)
      std::mutex mtx;
      std::set<std::thread::id> ids;
      parallel_for(M.nc, [&](int) {
        volatile double w = 0;  // a little work per cell, so that every worker gets to take a chunk
        for (int i = 0; i < 20000; i++) w = w + 1.0;
        std::lock_guard<std::mutex> lk(mtx);
        ids.insert(std::this_thread::get_id());
      });
      std::printf("parallel_for_threads %d\n", (int)ids.size());
    }
    // the per-cell work runs on several threads above 255 cells (parallel_for): a second assembly of the same mesh, and
    // of the per-cell tables of k_g_lift and the element block-Jacobi, must reproduce every bit
    {
      GeneralOps O2;
      std::vector<CellLocal> loc2;
      assemble_general(T, M, O2, loc2);
      int bad = 0;
#define SAME(name) if (!same_csr(O.name, O2.name)) { bad++; std::printf("repeat_differs %s\n", #name); }
      GENERAL_OPS(SAME)
#undef SAME
      if (!same_bits(O.one_p, O2.one_p) || !same_bits(O.int_p, O2.int_p) || !same_bits(O.one_l, O2.one_l) || !same_bits(O.xq, O2.xq) ||
          !same_bits(O.xp, O2.xp)) {
        bad++;
        std::printf("repeat_differs vectors\n");
      }
      for (const double gamma : {-1.0, 0.0, 0.0375}) {
        if (!same_bits(assemble_lift_tables(T, M, loc, gamma), assemble_lift_tables(T, M, loc2, gamma))) {
          bad++;
          std::printf("repeat_differs lift_tables %g\n", gamma);
        }
      }
      if (!same_csr(assemble_block_jacobi(T, M, loc, 0.0375), assemble_block_jacobi(T, M, loc2, 0.0375))) {
        bad++;
        std::printf("repeat_differs block_jacobi\n");
      }
      std::printf("repeat_mismatches %d\n", bad);
    }
    // condensed operator: symmetric, the constants are its kernel
    const double sscale = maxabs(O.S.val);
    std::printf("S_asym %.3e\n", asym(O.S) / sscale);
    std::printf("S_null %.3e\n", maxabs(spmv(O.S, O.one_l)) / sscale);
    // BDM projection is a projection
    {
      dvec x((size_t)O.Pi.ncols);
      unsigned long long st = 88172645463325252ULL;
      for (auto& v : x) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = (double)(st % 2000001ULL) / 1.0e6 - 1.0; }
      const dvec p1 = spmv(O.Pi, x), p2 = spmv(O.Pi, p1);
      double d = 0;
      for (size_t i = 0; i < p1.size(); i++) d = std::max(d, std::fabs(p1[i] - p2[i]));
      std::printf("Pi_idempotent %.3e\n", d / maxabs(p1));
    }
    // constraint rows of the monolithic system: the mu-row of a constant pressure with its own trace vanishes
    {
      dvec r = spmv(O.Mu_p, O.one_p);
      const dvec r2 = spmv(O.Mu_l, O.one_l);
      for (size_t i = 0; i < r.size(); i++) r[i] += r2[i];
      std::printf("mu_row_constant %.3e\n", maxabs(r));
      dvec s = spmv(O.Psi_p, O.one_p);
      const dvec s2 = spmv(O.Psi_l, O.one_l);
      for (size_t i = 0; i < s.size(); i++) s[i] += s2[i];
      std::printf("psi_row_constant %.3e\n", maxabs(s));
    }
    // P1 coarse space
    const Csr P0 = p1_to_trace_matrix(T, M);
    {
      const dvec one((size_t)M.nv, 1.0);
      const dvec t = spmv(P0, one);
      double d = 0;
      for (size_t i = 0; i < t.size(); i++) d = std::max(d, std::fabs(t[i] - O.one_l[i]));
      std::printf("P0_constants %.3e\n", d);
    }
    const Csr A0 = csr_multiply(csr_transpose(P0), csr_multiply(O.S, P0));
    AmgHierarchy H;
    amg_build(A0, H, 12, 12);  // small coarsest level so that the small test meshes get several levels
    std::printf("amg_levels %d\n", (int)H.lev.size());
    double worst_null = 0, worst_asym = 0, worst_pone = 0;
    int prev = 1 << 30, monotone = 1;
    for (size_t l = 0; l < H.lev.size(); l++) {
      const AmgLevel& L = H.lev[l];
      const dvec one((size_t)L.A.nrows, 1.0);
      const double sc = maxabs(H.lev[0].A.val);  // (a one-vertex level is the 1 x 1 zero matrix)
      worst_null = std::max(worst_null, maxabs(spmv(L.A, one)) / sc);
      worst_asym = std::max(worst_asym, asym(L.A) / sc);
      if (L.A.nrows >= prev) monotone = 0;
      prev = L.A.nrows;
      if (l + 1 < H.lev.size()) {
        const dvec onec((size_t)L.P.ncols, 1.0);
        const dvec t = spmv(L.P, onec);
        for (double v : t) worst_pone = std::max(worst_pone, std::fabs(v - 1.0));
      }
      std::printf("amg_n%d %d\n", (int)l, L.A.nrows);
    }
    std::printf("amg_null %.3e\namg_asym %.3e\namg_P_constants %.3e\namg_monotone %d\n", worst_null, worst_asym, worst_pone, monotone);
    {  // dense pseudo-inverse of the coarsest operator: A A^+ b = b for b orthogonal to the constants
      const Csr& Ac = H.lev.back().A;
      const int n = Ac.nrows;
      dvec b((size_t)n);
      double mean = 0;
      for (int i = 0; i < n; i++) { b[(size_t)i] = std::sin(1.0 + 0.7 * i); mean += b[(size_t)i]; }
      for (auto& v : b) v -= mean / n;
      const dvec x = spmv(H.coarse_pinv, b), r = spmv(Ac, x);
      double d = 0;
      for (int i = 0; i < n; i++) d = std::max(d, std::fabs(r[(size_t)i] - b[(size_t)i]));
      std::printf("coarse_pinv %.3e\n", n > 1 ? d / maxabs(b) : 0.0);  // (one vertex: the range is empty)
    }
    // continuous space
    GeneralCG G;
    assemble_cg(T, M, O, G);
    {
      const dvec one((size_t)G.ncg, 1.0);
      const dvec m1 = spmv(G.M, one);
      double vol = 0;
      for (double v : m1) vol += v;
      std::printf("ncg %d\ncg_volume %.15e\ncg_M_asym %.3e\n", G.ncg, vol, asym(G.M) / maxabs(G.M.val));
      // a constant velocity (1, 2): modal coefficients through the nodal -> modal conversion; projection data Bp = M * value
      dvec nodal((size_t)O.Cq.ncols);
      for (size_t i = 0; i < nodal.size(); i += 2) { nodal[i] = 1.0; nodal[i + 1] = 2.0; }
      const dvec modal = spmv(O.Cq, nodal);
      double d = 0;
      for (int c = 0; c < 2; c++) {
        const dvec rhs = spmv(G.Bp[c], modal);
        for (int i = 0; i < G.ncg; i++) d = std::max(d, std::fabs(rhs[(size_t)i] - (c + 1.0) * m1[(size_t)i]));
      }
      std::printf("cg_projection_rhs_constant %.3e\n", d);
      // vorticity of a rigid rotation (-y, x) is 2: Vort * modal = 2 * M * 1
      for (size_t i = 0; i < nodal.size(); i += 2) { nodal[i] = -O.xq[i + 1]; nodal[i + 1] = O.xq[i]; }
      const dvec rot = spmv(O.Cq, nodal), vr = spmv(G.Vort, rot);
      d = 0;
      for (int i = 0; i < G.ncg; i++) d = std::max(d, std::fabs(vr[(size_t)i] - 2.0 * m1[(size_t)i]));
      std::printf("cg_vorticity_rotation %.3e\n", d);
    }
  } catch (const std::string& e) {
    std::printf("error %s\n", e.c_str());
    return 1;
  }
  return 0;
}
