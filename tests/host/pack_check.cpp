// CPU check of csrc/hdg_mfma_pack.hpp (compiled by tests/test_host.py with g++): the index maps of the matrix-core kernels,
// the tile rule, the length of every packed table against the tile counts the kernels declare (LiftMfma, AdvMfmaFull in
// hdg_kernels.hpp, SchurMfma in hdg_schur_mfma.hpp; restated here, the kernel headers need hipcc), and the packed
// back-substitution table applied to a vector against Ainv r - W lambda from Tables::poissonBlock.
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_mfma_pack.hpp"

using namespace hdg;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("error line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// entry (r, c) of a matrix packed as MT x KS tiles
static double unpacked(const std::vector<double>& t, int KS, int r, int c) {
  const int mt = r / 16, ks = c / 4, l = (r % 16) + 16 * (c % 4);
  return t[((size_t)mt * KS + ks) * 64 + l];
}

static void check_index_maps(int k) {
  const int nu = n_scalar(k + 1), n2 = 2 * nu;
  std::set<int> cols, rows, mem;
  for (int n = 0; n < n2; n++) {
    CHECK(scol(nu, n) >= 0 && scol(nu, n) < 4 * sKSU(nu));
    CHECK(srow(nu, n) >= 0 && srow(nu, n) < 16 * sMTU(nu));
    CHECK(kap(nu, n) >= 0 && kap(nu, n) < n2);
    cols.insert(scol(nu, n)); rows.insert(srow(nu, n)); mem.insert(kap(nu, n));
  }
  CHECK((int)cols.size() == n2 && (int)rows.size() == n2 && (int)mem.size() == n2);
  for (int m = 0; m < nu; m++) {
    // hdg_schur_mfma.hpp, K side: a lane loads both components of mode m = 4q + lk with one 16-byte load and feeds .x to
    // K-step 2q, .y to K-step 2q + 1:  column(m, d) = 8 (m/4) + 4 d + m%4
    CHECK(scol(nu, m) == 8 * (m / 4) + m % 4);
    CHECK(scol(nu, nu + m) == scol(nu, m) + 4 && scol(nu, nu + m) / 8 == scol(nu, m) / 8);
    // M side: tile mt holds the modes 8 mt .. 8 mt + 7; lane lk finds both components of mode 8 mt + lk in registers 0, 1 and
    // of mode 8 mt + 4 + lk in registers 2, 3 (register r = row lk + 4 r):  row(m, d) = 16 (m/8) + m%4 + 4 (2 ((m%8)/4) + d)
    CHECK(srow(nu, m) == 16 * (m / 8) + m % 4 + 8 * ((m % 8) / 4));
    CHECK(srow(nu, nu + m) == srow(nu, m) + 4 && srow(nu, nu + m) / 16 == srow(nu, m) / 16);
    CHECK(kap(nu, m) == 2 * m && kap(nu, nu + m) == 2 * m + 1);
  }
}

static void check_tile_rule() {
  const int rows = 21, cols = 10, MT = 2, KS = 3;
  std::vector<double> M((size_t)rows * cols), t;
  for (size_t q = 0; q < M.size(); q++) M[q] = 1.0 + (double)q;  // distinct, non-zero
  pack_tiles(t, M, rows, cols, MT, KS);
  CHECK((int)t.size() == 64 * MT * KS);
  for (int mt = 0; mt < MT; mt++)
    for (int ks = 0; ks < KS; ks++)
      for (int l = 0; l < 64; l++) {
        const int r = 16 * mt + l % 16, c = 4 * ks + l / 16;
        const double want = (r < rows && c < cols) ? M[(size_t)r * cols + c] : 0.0;
        CHECK(t[((size_t)mt * KS + ks) * 64 + l] == want);
        CHECK(unpacked(t, KS, r, c) == want);
      }
  pack_tiles(t, M, rows, cols, 1, 1);  // appends
  CHECK((int)t.size() == 64 * MT * KS + 64);
}

static void check_lengths(int k, const Tables& T) {
  const int NU = n_scalar(k + 1), NP = n_scalar(k), NL = k + 1, NT = 3 * NL;
  CHECK(T.nu == NU && T.np == NP && T.nl == NL && T.nx_loc == 2 * NU + NP && T.ne == k + 2);
  // LiftMfma<K>
  const int KQ = (NU + 3) / 4, KS = 2 * KQ, MT = (NU + 7) / 8, KD = 5, lift_tiles = 2 * KS + 3 * KS + MT * KD;
  // AdvMfma<K> / AdvMfmaFull<K>
  const int NQ = k == 3 ? 36 : 64, MTQ = (NQ + 15) / 16, KSUa = (NU + 3) / 4, MTUa = (NU + 15) / 16;
  const int adv_tiles = 3 * MTQ * KSUa + MTUa * 4 * MTQ + 3 * 2 * KSUa + 3 * KSUa + MTUa * 6;
  CHECK(T.nqc == NQ && T.nqe == (3 * k + 5) / 2);
  // SchurMfma<K>
  const int KSU = 2 * KQ, KSP = (NP + 3) / 4, KST = (NT + 3) / 4, MTU = (NU + 7) / 8;
  const int bs_tiles = (MTU + 1) * (KSU + KSP + KST), pg_tiles = MTU * (KSP + KST), wd_tiles = 6 * KSU, wdb_tiles = KSU;
  const int cd_tiles = 4 * (KSU + KSP);
  CHECK(sKSU(NU) == KSU && sMTU(NU) == MTU);
  for (int sh = 0; sh < 2; sh++) {
    CHECK((int)pack_lift_mfma(T, sh, T.Lift[sh]).size() == 64 * lift_tiles);
    CHECK((int)pack_adv_mfma(T, sh).size() == 64 * adv_tiles);
    CHECK((int)pack_backsub_mfma(T, T.Ainv[sh], T.W[sh]).size() == 64 * bs_tiles);
    CHECK((int)pack_pgrad_mfma(T, sh).size() == 64 * pg_tiles);
    CHECK((int)pack_weakdiv_mfma(T, sh, false).size() == 64 * wd_tiles);
    CHECK((int)pack_weakdiv_mfma(T, sh, true).size() == 64 * wdb_tiles);
  }
  CHECK((int)pack_condense_mfma(T, T.Y[0], T.Y[1]).size() == 64 * cd_tiles);
}

// the packed back-substitution table times [r_w by scol | r_p | lambda] against Ainv (r_w, r_p) - W lambda, row by row
static double check_backsub(const Tables& T, double tau) {
  const int NU = T.nu, NP = T.np, NX = T.nx_loc, N2 = 2 * NU, NT = 3 * T.nl;
  const int KSU = sKSU(NU), KSP = (NP + 3) / 4, KST = (NT + 3) / 4, MTU = sMTU(NU), KSA = KSU + KSP + KST;
  double worst = 0.0;
  for (int sh = 0; sh < 2; sh++) {
    dvec Ai, W_, Y_, SK_;
    T.poissonBlock(sh, tau, Ai, W_, Y_, SK_);
    const std::vector<double> t = pack_backsub_mfma(T, Ai, W_);
    std::vector<double> r(NX), lam(NT), x((size_t)4 * KSA, 0.0);
    for (int n = 0; n < NX; n++) r[n] = std::sin(1.0 + 0.7 * n) + 0.3;
    for (int q = 0; q < NT; q++) lam[q] = std::cos(0.4 + 1.3 * q) - 0.2;
    for (int n = 0; n < N2; n++) x[scol(NU, n)] = r[n];
    for (int m = 0; m < NP; m++) x[4 * KSU + m] = r[N2 + m];
    for (int q = 0; q < NT; q++) x[4 * (KSU + KSP) + q] = lam[q];
    for (int n = 0; n < NX; n++) {
      double direct = 0.0, mag = 0.0;
      for (int c = 0; c < NX; c++) { direct += Ai[(size_t)n * NX + c] * r[c]; mag += std::fabs(Ai[(size_t)n * NX + c] * r[c]); }
      for (int q = 0; q < NT; q++) { direct -= W_[(size_t)n * NT + q] * lam[q]; mag += std::fabs(W_[(size_t)n * NT + q] * lam[q]); }
      const int row = n < N2 ? srow(NU, n) : 16 * MTU + (n - N2);
      double packed = 0.0;
      for (int c = 0; c < 4 * KSA; c++) packed += unpacked(t, KSA, row, c) * x[c];
      const double rel = std::fabs(packed - direct) / mag;
      if (rel > worst) worst = rel;
      CHECK(std::fabs(packed - direct) <= 1e-13 * mag);
    }
    // rows of the table no dof maps to are zero
    std::set<int> used;
    for (int n = 0; n < NX; n++) used.insert(n < N2 ? srow(NU, n) : 16 * MTU + (n - N2));
    for (int row = 0; row < 16 * (MTU + 1); row++)
      if (!used.count(row))
        for (int c = 0; c < 4 * KSA; c++) CHECK(unpacked(t, KSA, row, c) == 0.0);
  }
  return worst;
}

int main() {
  check_tile_rule();
  for (int k = 3; k <= 4; k++) {
    check_index_maps(k);
    const Tables T(k, 1.0 / 64, 1.0, 1.0, 0);
    check_lengths(k, T);
    for (double tau : {1.0, 40.0}) std::printf("k = %d tau = %g: back-substitution rows agree to %.2e of sum |a_i x_i|\n", k, tau, check_backsub(T, tau));
  }
  for (int k = 1; k <= 2; k++) check_index_maps(k);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
