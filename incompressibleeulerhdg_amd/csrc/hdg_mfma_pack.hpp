// Host side of the matrix-core kernels (k >= 3): the local tables in A-operand lane order and the index maps the kernels
// and these packers share.  Plain C++ (no HIP header, tests/host/pack_check.cpp compiles it with g++): functions of the
// reference tables (hdg_tables.hpp) alone; the engine uploads what they return.
//
// Tile (mt, ks) of a dense rows x cols matrix M: 64 doubles, entry l = M[16 mt + l % 16][4 ks + l / 16] (zero outside M) --
// lane l of a wave holds its A operand of v_mfma_f64_16x16x4 for M-tile mt and K-step ks.  pack_tiles is the only place
// that rule is written.
#pragma once
#include <vector>

#include "hdg_tables.hpp"

namespace hdg {

// tiles [mt][ks] of M appended to dst: 64 * MT * KS doubles
inline void pack_tiles(std::vector<double>& dst, const std::vector<double>& M, int rows, int cols, int MT, int KS) {
  for (int mt = 0; mt < MT; mt++)
    for (int ks = 0; ks < KS; ks++)
      for (int l = 0; l < 64; l++) {
        const int r = 16 * mt + l % 16, c = 4 * ks + l / 16;
        dst.push_back((r < rows && c < cols) ? M[(size_t)r * cols + c] : 0.0);
      }
}

// Velocity dofs are numbered n = d * nu + m in the tables (component d of basis function m).
inline int kap(int nu, int n) { return 2 * (n % nu) + n / nu; }  // memory position in the component-pair layout
// K slot / result row of dof n in the matrix-core kernels (16-byte accesses: hdg_schur_mfma.hpp, k_edge_lift_mfma)
inline int scol(int nu, int n) { const int m = n % nu, d = n / nu; return 8 * (m / 4) + 4 * d + m % 4; }
inline int srow(int nu, int n) { const int m = n % nu, d = n / nu; return 16 * (m / 8) + m % 4 + 4 * (2 * ((m % 8) / 4) + d); }
inline int sKSU(int nu) { return 2 * ((nu + 3) / 4); }  // K-steps of a velocity source (4 sKSU columns)
inline int sMTU(int nu) { return (nu + 7) / 8; }        // M-tiles of a velocity result (16 sMTU rows)

// ---- lift (k_edge_lift_mfma).  Order: W (2 M-tiles), N'_0..2, G.  Out[e]: 2nu x ne row-major lifting tables of shape s
// (Lift_e for the projection, (I - Dinv) Lift_e for the hybrid preconditioner).
inline std::vector<double> pack_lift_mfma(const Tables& T, int s, const dvec* Out) {
  const int nu = T.nu, n2 = 2 * nu, ne = T.ne, KS = sKSU(nu), MT = sMTU(nu), KD = 5;
  std::vector<double> packed;
  // W: rows (e, a) packed as tile 0 = edges 0, 1, tile 1 = edge 2;  W = -N[s][e]
  const int nc = 4 * KS;  // padded column count of the coefficient side
  std::vector<double> W((size_t)32 * nc, 0.0);
  for (int e = 0; e < 3; e++)
    for (int a = 0; a < ne; a++)
      for (int n = 0; n < n2; n++) W[(size_t)((e < 2 ? e * ne + a : 16 + a)) * nc + scol(nu, n)] = -T.N[s][e][a * n2 + n];
  pack_tiles(packed, W, 32, nc, 2, KS);
  // N'_e = N[1 - s][e], rows at their position inside the tile
  for (int e = 0; e < 3; e++) {
    std::vector<double> Np((size_t)16 * nc, 0.0);
    for (int a = 0; a < ne; a++)
      for (int n = 0; n < n2; n++) Np[(size_t)((e == 1 ? ne : 0) + a) * nc + scol(nu, n)] = T.N[1 - s][e][a * n2 + n];
    pack_tiles(packed, Np, 16, nc, 1, KS);
  }
  // G: columns = packed moments, K index q: q < 12 -> tile 0 row q, q >= 12 -> tile 1 row q - 12
  std::vector<double> Gm((size_t)(16 * MT) * 20, 0.0);
  for (int e = 0; e < 3; e++)
    for (int a = 0; a < ne; a++) {
      const int q = e < 2 ? e * ne + a : 12 + a;
      for (int n = 0; n < n2; n++) Gm[(size_t)srow(nu, n) * 20 + q] = Out[e][(size_t)n * ne + a];
    }
  pack_tiles(packed, Gm, 16 * MT, 20, MT, KD);
  return packed;
}

// ---- advection (k_adv_mfma): Phi, Gx, Gy (rows = quadrature points, columns = basis functions), then
// A2[m][q] = -w_q Phi[q][m] (rows = basis functions, columns = quadrature points), then the facet tables
inline std::vector<double> pack_adv_mfma(const Tables& T, int s) {
  const int nu = T.nu, nq = T.nqc, MTQ = (nq + 15) / 16, KSU = (nu + 3) / 4, MTU = (nu + 15) / 16;
  std::vector<double> packed;
  for (const dvec* M : {&T.cPhi[s], &T.cGx[s], &T.cGy[s]}) pack_tiles(packed, *M, nq, nu, MTQ, KSU);
  std::vector<double> A2((size_t)nu * nq);
  for (int m = 0; m < nu; m++) for (int q = 0; q < nq; q++) A2[(size_t)m * nq + q] = -T.cw[q] * T.cPhi[s][(size_t)q * nu + m];
  pack_tiles(packed, A2, nu, nq, MTU, 4 * MTQ);
  // facet tables: edge-point rows packed 8 per edge, tile 0 = edges 0, 1, tile 1 = edge 2
  const int nqe = T.nqe;
  auto erow = [&](int e, int q) { return (e < 2 ? 8 * e : 16) + q; };
  std::vector<double> EO((size_t)32 * nu, 0.0), EQX(EO), EQY(EO);
  for (int e = 0; e < 3; e++)
    for (int q = 0; q < nqe; q++)
      for (int m = 0; m < nu; m++) {
        const double po = T.ePhi[s][e][(size_t)q * nu + m];
        EO[(size_t)erow(e, q) * nu + m] = po;
        EQX[(size_t)erow(e, q) * nu + m] = T.enx[e] * po;
        EQY[(size_t)erow(e, q) * nu + m] = T.eny[e] * po;
      }
  for (const std::vector<double>* M : {&EO, &EQX, &EQY}) pack_tiles(packed, *M, 32, nu, 2, KSU);
  for (int e = 0; e < 3; e++) {  // neighbour trace rows of edge e inside its tile, zero elsewhere
    std::vector<double> EN((size_t)16 * nu, 0.0);
    for (int q = 0; q < nqe; q++)
      for (int m = 0; m < nu; m++) EN[(size_t)((e == 1 ? 8 : 0) + q) * nu + m] = T.ePhi[1 - s][e][(size_t)q * nu + m];
    pack_tiles(packed, EN, 16, nu, 1, KSU);
  }
  std::vector<double> ET((size_t)nu * 24, 0.0);  // test: rows m, columns (e, q) packed: 8 e + q
  for (int e = 0; e < 3; e++)
    for (int q = 0; q < nqe; q++)
      for (int m = 0; m < nu; m++) ET[(size_t)m * 24 + 8 * e + q] = T.ePhi[s][e][(size_t)q * nu + m];
  pack_tiles(packed, ET, nu, 24, MTU, 6);
  return packed;
}

// ---- Schur kernels (hdg_schur_mfma.hpp).
// back-substitution  (u, phi) = Ainv (r_w, r_p) - W lambda:  rows [u by srow, padded to 16 MTU | phi],
// columns [r_w by scol, padded to 4 KSU | r_p padded to 4 KSP | lambda padded to 4 KST]
inline std::vector<double> pack_backsub_mfma(const Tables& T, const dvec& Ai, const dvec& W_) {
  const int NU = T.nu, NP = T.np, NX = T.nx_loc, N2 = 2 * NU, NT = 3 * T.nl;
  const int KSU = sKSU(NU), KSP = (NP + 3) / 4, KST = (NT + 3) / 4, MTU = sMTU(NU);
  const int rows = 16 * (MTU + 1), cols = 4 * (KSU + KSP + KST);
  std::vector<double> M((size_t)rows * cols, 0.0);
  for (int n = 0; n < NX; n++) {
    const int r = n < N2 ? srow(NU, n) : 16 * MTU + (n - N2);
    for (int c = 0; c < N2; c++) M[(size_t)r * cols + scol(NU, c)] = Ai[(size_t)n * NX + c];
    for (int m = 0; m < NP; m++) M[(size_t)r * cols + 4 * KSU + m] = Ai[(size_t)n * NX + N2 + m];
    for (int q = 0; q < NT; q++) M[(size_t)r * cols + 4 * (KSU + KSP) + q] = -W_[(size_t)n * NT + q];
  }
  std::vector<double> out;
  pack_tiles(out, M, rows, cols, MTU + 1, KSU + KSP + KST);
  return out;
}
// condensation: one M-tile with rows (H, D, V) x NL; block 0 = Y_L (local edges 0, 1, 2 -> H, D, V), blocks 1, 2, 3 = the
// rows of Y_U that belong to D (local edge 1), H (0), V (2); columns [r_w by scol | r_p] per block
inline std::vector<double> pack_condense_mfma(const Tables& T, const dvec& Y0, const dvec& Y1) {
  const int NU = T.nu, NP = T.np, NL = T.nl, NX = T.nx_loc, N2 = 2 * NU;
  const int KSU = sKSU(NU), KSP = (NP + 3) / 4, KSA = KSU + KSP, cols = 4 * KSA;
  std::vector<double> out;
  for (int q = 0; q < 4; q++) {
    std::vector<double> M((size_t)16 * cols, 0.0);
    const dvec& Y = q == 0 ? Y0 : Y1;
    for (int e = 0; e < 3; e++) {
      if (q == 1 && e != 1) continue;
      if (q == 2 && e != 0) continue;
      if (q == 3 && e != 2) continue;
      for (int a = 0; a < NL; a++) {
        const int r = e * NL + a;  // local-edge order (0, 1, 2) = (H, D, V): the row order of the result tile
        for (int c = 0; c < N2; c++) M[(size_t)r * cols + scol(NU, c)] = Y[(size_t)r * NX + c];
        for (int m = 0; m < NP; m++) M[(size_t)r * cols + 4 * KSU + m] = Y[(size_t)r * NX + N2 + m];
      }
    }
    pack_tiles(out, M, 16, cols, 1, KSA);
  }
  return out;
}
// pressure gradient: rows = velocity dofs by srow, columns [p | lambda (e, m)]:  B^T p - sum_e sigma_e N_e^T lambda_e
inline std::vector<double> pack_pgrad_mfma(const Tables& T, int sh) {
  const int NU = T.nu, NP = T.np, NL = T.nl, N2 = 2 * NU, NT = 3 * NL;
  const int KSP = (NP + 3) / 4, KST = (NT + 3) / 4, MTU = sMTU(NU), cols = 4 * (KSP + KST);
  std::vector<double> M((size_t)16 * MTU * cols, 0.0);
  for (int n = 0; n < N2; n++) {
    for (int m = 0; m < NP; m++) M[(size_t)srow(NU, n) * cols + m] = T.B[sh][(size_t)m * N2 + n];
    for (int e = 0; e < 3; e++)
      for (int m = 0; m < NL; m++) M[(size_t)srow(NU, n) * cols + 4 * KSP + e * NL + m] = -T.sig[sh][e] * T.N[sh][e][(size_t)m * N2 + n];
  }
  std::vector<double> out;
  pack_tiles(out, M, 16 * MTU, cols, MTU, KSP + KST);
  return out;
}
// weak divergence: six NP x 2NU blocks (see k_weak_div_mfma); broken: the single block B
inline std::vector<double> pack_weakdiv_mfma(const Tables& T, int sh, bool broken) {
  const int NU = T.nu, NP = T.np, NL = T.nl, N2 = 2 * NU, KSU = sKSU(NU), cols = 4 * KSU;
  auto E = [&](int e, int from) {  // (sigma_e / 2) Pt_e^T N_e[0:NL] with N of shape `from`
    std::vector<double> M((size_t)16 * cols, 0.0);
    for (int r = 0; r < NP; r++)
      for (int n = 0; n < N2; n++) {
        double acc = 0.0;
        for (int m = 0; m < NL; m++) acc += T.Pt[sh][e][(size_t)m * NP + r] * T.N[from][e][(size_t)m * N2 + n];
        M[(size_t)r * cols + scol(NU, n)] = 0.5 * T.sig[sh][e] * acc;
      }
    return M;
  };
  std::vector<double> out;
  std::vector<double> base((size_t)16 * cols, 0.0);
  const dvec& B0 = broken ? T.B[sh] : T.D0[sh];
  for (int r = 0; r < NP; r++)
    for (int n = 0; n < N2; n++) base[(size_t)r * cols + scol(NU, n)] = B0[(size_t)r * N2 + n];
  if (broken) { pack_tiles(out, base, 16, cols, 1, KSU); return out; }
  const std::vector<double> E1 = E(1, sh);
  for (size_t q = 0; q < base.size(); q++) base[q] += E1[q];
  pack_tiles(out, base, 16, cols, 1, KSU);
  pack_tiles(out, E(0, sh), 16, cols, 1, KSU);
  pack_tiles(out, E(2, sh), 16, cols, 1, KSU);
  pack_tiles(out, E(0, 1 - sh), 16, cols, 1, KSU);
  pack_tiles(out, E(1, 1 - sh), 16, cols, 1, KSU);
  pack_tiles(out, E(2, 1 - sh), 16, cols, 1, KSU);
  return out;
}

}  // namespace hdg
