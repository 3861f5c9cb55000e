// Host check of the viscosity tables of csrc/hdg_tables.hpp (g++, no HIP): assembles M^-1 V of an nx x nx structured mesh (unit
// square with free-slip or no-slip walls, or the doubly periodic square) from Vol / Own / Nbr / Wall exactly as k_viscosity
// walks a cell's edges, maps it from the orthonormal modal basis to the nodal one (V A V^-1 per block) and writes it, with the
// bound lambda in front, for tests/test_viscosity_cpu.py to compare with the numpy reference.  Its own checks: the modal
// operator is symmetric and its largest absolute row sum does not exceed lambda.
//   usage: viscosity_check k nx periodic L no_slip out.bin    cell order 2 (j nx + i) + s, dof ((cell nu + mode) 2 + component)
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

int main(int argc, char** argv) {
  if (argc != 7) { std::printf("usage: k nx periodic L no_slip out\n"); return 2; }
  const int k = std::atoi(argv[1]), nx = std::atoi(argv[2]), per = std::atoi(argv[3]), no_slip = std::atoi(argv[5]);
  const double L = std::atof(argv[4]), h = L / nx;
  if (k < 1 || k > 4 || nx < 2 || nx > 8) { std::printf("arguments out of range\n"); return 2; }
  const ViscosityTables D(k, h);
  const Tables T(k, h, 1.0, 1.0, 0);
  const int nu = D.nu, nc = 2 * nx * nx;
  const size_t N = (size_t)nc * nu * 2;
  std::vector<double> A(N * N, 0.0);  // modal
  auto cell = [&](int i, int j, int s) { return 2 * (j * nx + i) + s; };
  auto add = [&](int cr, int cc, const dvec& B, int comp) {  // comp: 0, 1, or 2 = both
    for (int d = 0; d < 2; d++) {
      if (comp != 2 && comp != d) continue;
      for (int r = 0; r < nu; r++)
        for (int m = 0; m < nu; m++) A[(((size_t)cr * nu + r) * 2 + d) * N + ((size_t)cc * nu + m) * 2 + d] += B[(size_t)r * nu + m];
    }
  };
  for (int j = 0; j < nx; j++)
    for (int i = 0; i < nx; i++)
      for (int s = 0; s < 2; s++) {
        const int c = cell(i, j, s);
        add(c, c, D.Vol[s], 2);
        for (int e = 0; e < 3; e++) {
          int in = i, jn = j;
          if (e == 0) jn = s == 0 ? j - 1 : j + 1;
          if (e == 2) in = s == 0 ? i - 1 : i + 1;
          if (in < 0 || in >= nx || jn < 0 || jn >= nx) {
            if (!per) {  // a wall: the normal component, both with no slip
              add(c, c, D.Wall[s][e], no_slip ? 2 : ViscosityTables::wall_normal_component(e));
              continue;
            }
            in = (in + nx) % nx; jn = (jn + nx) % nx;
          }
          add(c, c, D.Own[s][e], 2);
          add(c, cell(in, jn, 1 - s), D.Nbr[s][e], 2);
        }
      }
  int fails = 0;
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
  if (rowsum > D.lambda * (1 + 1e-14)) { fails++; std::printf("FAIL row sum %.17g above lambda %.17g\n", rowsum, D.lambda); }
  // nodal: block (a, b) of component d -> Vu block Vuinv
  std::vector<double> Bn(N * N, 0.0), tmp((size_t)nu * nu);
  for (int a = 0; a < nc; a++)
    for (int b = 0; b < nc; b++)
      for (int d = 0; d < 2; d++) {
        auto at = [&](int r, int m) -> double& { return A[(((size_t)a * nu + r) * 2 + d) * N + ((size_t)b * nu + m) * 2 + d]; };
        bool any = false;
        for (int r = 0; r < nu && !any; r++)
          for (int m = 0; m < nu; m++) if (at(r, m) != 0.0) { any = true; break; }
        if (!any) continue;
        for (int r = 0; r < nu; r++)
          for (int m = 0; m < nu; m++) {
            long double acc = 0;
            for (int l = 0; l < nu; l++) acc += (long double)T.Vu[(size_t)r * nu + l] * at(l, m);
            tmp[(size_t)r * nu + m] = (double)acc;
          }
        for (int r = 0; r < nu; r++)
          for (int m = 0; m < nu; m++) {
            long double acc = 0;
            for (int l = 0; l < nu; l++) acc += (long double)tmp[(size_t)r * nu + l] * T.Vuinv[(size_t)l * nu + m];
            Bn[(((size_t)a * nu + r) * 2 + d) * N + ((size_t)b * nu + m) * 2 + d] = (double)acc;
          }
      }
  FILE* f = std::fopen(argv[6], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[6]); return 2; }
  const double head[2] = {D.lambda, (double)N};
  const bool ok = std::fwrite(head, sizeof(double), 2, f) == 2 && std::fwrite(Bn.data(), sizeof(double), Bn.size(), f) == Bn.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("k %d nx %d periodic %d no_slip %d lambda %.17g rowsum %.17g asym %.3e\n", k, nx, per, no_slip, D.lambda, rowsum, asym);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
