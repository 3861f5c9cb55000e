// Host check of the wall tables of TracerDiffusionTables (csrc/hdg_tables.hpp; g++, no HIP): assembles M^-1 (D + sum_w D_w) of
// the nx x nx unit square from Vol / Own / Nbr / Wall exactly as k_tracer_diff<., ., true> walks a cell's edges, for the set of
// fixed sides given as a bit mask (bit w: side w of bottom, right, top, left), with the load vector of g = 1 and the flux
// functional of every fixed side, maps them from the orthonormal modal basis to the nodal one and writes them for
// tests/test_tracer_walls_cpu.py to compare with the numpy reference.  Its own checks: Wall is symmetric, the modal operator is
// symmetric, its largest absolute row sum does not exceed lambda_walls, and Wall^T coef(1) = - wvec (the flux functional).
//   usage: tracer_walls_check k nx mask out.bin      cell order 2 (j nx + i) + s, as the oracle's mesh
//   out:   lambda_walls, N, wone, then the operator (N x N), 4 load vectors (N each), 4 flux functionals (N each), nodal
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

int main(int argc, char** argv) {
  if (argc != 5) { std::printf("usage: k nx mask out\n"); return 2; }
  const int k = std::atoi(argv[1]), nx = std::atoi(argv[2]), mask = std::atoi(argv[3]);
  if (k < 1 || k > 4 || nx < 2 || nx > 16 || mask < 0 || mask > 15) { std::printf("arguments out of range\n"); return 2; }
  const double h = 1.0 / nx;
  const TracerDiffusionTables D(k, h);
  const Tables T(k, h, 1.0, 1.0, 0);
  const int np = D.np, nc = 2 * nx * nx;
  const size_t N = (size_t)nc * np;
  bool fixed[4];
  for (int w = 0; w < 4; w++) fixed[w] = (mask >> w & 1) != 0;
  const double lam = D.lambda_walls(fixed);
  int fails = 0;
  // the tables themselves
  for (int s = 0; s < 2; s++)
    for (int e = 0; e < 3; e += 2) {
      double wmax = 0.0, asym = 0.0, func = 0.0, fmax = 0.0;
      // coef(1): the constant is mode 0 alone; its coefficient c0 from the mass normalisation, psi_0^2 |K| = 1
      const double c0 = h / std::sqrt(2.0);
      for (int r = 0; r < np; r++) {
        for (int m = 0; m < np; m++) {
          wmax = std::fmax(wmax, std::fabs(D.Wall[s][e][(size_t)r * np + m]));
          asym = std::fmax(asym, std::fabs(D.Wall[s][e][(size_t)r * np + m] - D.Wall[s][e][(size_t)m * np + r]));
        }
        func = std::fmax(func, std::fabs(c0 * D.Wall[s][e][(size_t)0 * np + r] + D.wvec[s][e][(size_t)r]));  // (Wall^T coef(1))_r = - wvec_r
        fmax = std::fmax(fmax, std::fabs(D.wvec[s][e][(size_t)r]));
      }
      if (asym > 1e-13 * wmax) { fails++; std::printf("FAIL Wall[%d][%d] symmetry %.3e of %.3e\n", s, e, asym, wmax); }
      if (func > 1e-12 * fmax) { fails++; std::printf("FAIL Wall[%d][%d]^T coef(1) + wvec %.3e of %.3e\n", s, e, func, fmax); }
    }
  if (std::fabs(D.wone - D.eta_b * h) > 1e-14 * D.wone) { fails++; std::printf("FAIL wone\n"); }
  std::vector<double> A(N * N, 0.0), load(4 * N, 0.0), fun(4 * N, 0.0);  // modal
  auto cell = [&](int i, int j, int s) { return 2 * (j * nx + i) + s; };
  auto add = [&](int cr, int cc, const dvec& B) {
    for (int r = 0; r < np; r++)
      for (int m = 0; m < np; m++) A[((size_t)cr * np + r) * N + (size_t)cc * np + m] += B[(size_t)r * np + m];
  };
  for (int j = 0; j < nx; j++)
    for (int i = 0; i < nx; i++)
      for (int s = 0; s < 2; s++) {
        const int c = cell(i, j, s);
        add(c, c, D.Vol[s]);
        for (int e = 0; e < 3; e++) {
          int in = i, jn = j;
          if (e == 0) jn = s == 0 ? j - 1 : j + 1;
          if (e == 2) in = s == 0 ? i - 1 : i + 1;
          if (in < 0 || in >= nx || jn < 0 || jn >= nx) {  // a wall leg
            const int w = TracerDiffusionTables::wall_side(s, e);
            if (!fixed[w]) continue;
            add(c, c, D.Wall[s][e]);
            for (int r = 0; r < np; r++) {
              load[(size_t)w * N + (size_t)c * np + r] += D.wvec[s][e][(size_t)r];
              fun[(size_t)w * N + (size_t)c * np + r] -= D.wvec[s][e][(size_t)r];
            }
            continue;
          }
          add(c, c, D.Own[s][e]);
          add(c, cell(in, jn, 1 - s), D.Nbr[s][e]);
        }
      }
  double amax = 0.0, asym = 0.0, rowsum = 0.0;
  for (size_t r = 0; r < N; r++) {
    double sum = 0.0;
    for (size_t c = 0; c < N; c++) {
      amax = std::fmax(amax, std::fabs(A[r * N + c]));
      asym = std::fmax(asym, std::fabs(A[r * N + c] - A[c * N + r]));
      sum += std::fabs(A[r * N + c]);
    }
    rowsum = std::fmax(rowsum, sum);
  }
  if (asym > 1e-12 * amax) { fails++; std::printf("FAIL symmetry %.3e of %.3e\n", asym, amax); }
  if (rowsum > lam * (1 + 1e-14)) { fails++; std::printf("FAIL row sum %.17g above lambda %.17g\n", rowsum, lam); }
  if (lam < D.lambda) { fails++; std::printf("FAIL lambda_walls %.17g below lambda %.17g\n", lam, D.lambda); }
  // nodal: block (a, b) -> Vp block Vpinv; a vector -> Vp v; a functional -> Vpinv^T f
  std::vector<double> Bn(N * N, 0.0), tmp((size_t)np * np), ln(4 * N, 0.0), fn(4 * N, 0.0);
  for (int a = 0; a < nc; a++)
    for (int b = 0; b < nc; b++) {
      bool any = false;
      for (int r = 0; r < np && !any; r++)
        for (int m = 0; m < np; m++) if (A[((size_t)a * np + r) * N + (size_t)b * np + m] != 0.0) { any = true; break; }
      if (!any) continue;
      for (int r = 0; r < np; r++)
        for (int m = 0; m < np; m++) {
          long double acc = 0;
          for (int l = 0; l < np; l++) acc += (long double)T.Vp[(size_t)r * np + l] * A[((size_t)a * np + l) * N + (size_t)b * np + m];
          tmp[(size_t)r * np + m] = (double)acc;
        }
      for (int r = 0; r < np; r++)
        for (int m = 0; m < np; m++) {
          long double acc = 0;
          for (int l = 0; l < np; l++) acc += (long double)tmp[(size_t)r * np + l] * T.Vpinv[(size_t)l * np + m];
          Bn[((size_t)a * np + r) * N + (size_t)b * np + m] = (double)acc;
        }
    }
  for (int w = 0; w < 4; w++)
    for (int c = 0; c < nc; c++)
      for (int r = 0; r < np; r++) {
        long double av = 0, af = 0;
        for (int l = 0; l < np; l++) {
          av += (long double)T.Vp[(size_t)r * np + l] * load[(size_t)w * N + (size_t)c * np + l];
          af += (long double)T.Vpinv[(size_t)l * np + r] * fun[(size_t)w * N + (size_t)c * np + l];
        }
        ln[(size_t)w * N + (size_t)c * np + r] = (double)av;
        fn[(size_t)w * N + (size_t)c * np + r] = (double)af;
      }
  FILE* f = std::fopen(argv[4], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[4]); return 2; }
  const double head[3] = {lam, (double)N, D.wone};
  const bool ok = std::fwrite(head, sizeof(double), 3, f) == 3 && std::fwrite(Bn.data(), sizeof(double), Bn.size(), f) == Bn.size() &&
                  std::fwrite(ln.data(), sizeof(double), ln.size(), f) == ln.size() && std::fwrite(fn.data(), sizeof(double), fn.size(), f) == fn.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("k %d nx %d mask %d lambda %.17g (no walls %.17g) rowsum %.17g asym %.3e\n", k, nx, mask, lam, D.lambda, rowsum, asym);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
