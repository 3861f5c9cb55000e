// Host check of the tracer-diffusion tables of csrc/hdg_tables.hpp (g++, no HIP): assembles M^-1 D of an nx x nx structured mesh
// (unit square with walls, or the doubly periodic square) from Vol / Own / Nbr exactly as the device kernel walks a cell's
// edges, maps it from the orthonormal modal basis to the nodal one (V A V^-1 per block) and writes it, with the bound lambda
// in front, for tests/test_tracer_diffusion_cpu.py to compare with the numpy reference.  Its own checks: the modal operator
// is symmetric, constants are in its null space, and its largest absolute row sum does not exceed lambda.
//   usage: tracer_diffusion_check k nx periodic L out.bin      cell order 2 (j nx + i) + s, as the oracle's mesh
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

int main(int argc, char** argv) {
  if (argc != 6) { std::printf("usage: k nx periodic L out\n"); return 2; }
  const int k = std::atoi(argv[1]), nx = std::atoi(argv[2]), per = std::atoi(argv[3]);
  const double L = std::atof(argv[4]), h = L / nx;
  if (k < 1 || k > 4 || nx < 2 || nx > 16) { std::printf("arguments out of range\n"); return 2; }
  const TracerDiffusionTables D(k, h);
  const Tables T(k, h, 1.0, 1.0, 0);
  const int np = D.np, nc = 2 * nx * nx;
  const size_t N = (size_t)nc * np;
  std::vector<double> A(N * N, 0.0);  // modal
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
          if (in < 0 || in >= nx || jn < 0 || jn >= nx) {
            if (!per) continue;  // a wall: no term
            in = (in + nx) % nx; jn = (jn + nx) % nx;
          }
          add(c, c, D.Own[s][e]);
          add(c, cell(in, jn, 1 - s), D.Nbr[s][e]);
        }
      }
  int fails = 0;
  double amax = 0.0, asym = 0.0, null = 0.0, rowsum = 0.0;
  for (size_t r = 0; r < N; r++) {
    double sum = 0.0, c0 = 0.0;
    for (size_t c = 0; c < N; c++) {
      amax = std::fmax(amax, std::fabs(A[r * N + c]));
      asym = std::fmax(asym, std::fabs(A[r * N + c] - A[c * N + r]));
      sum += std::fabs(A[r * N + c]);
      if (c % np == 0) c0 += A[r * N + c];  // mode 0 of every cell is the constant, with the same coefficient in every cell
    }
    rowsum = std::fmax(rowsum, sum);
    null = std::fmax(null, std::fabs(c0));
  }
  if (asym > 1e-12 * amax) { fails++; std::printf("FAIL symmetry %.3e of %.3e\n", asym, amax); }
  if (null > 1e-12 * amax) { fails++; std::printf("FAIL constants %.3e of %.3e\n", null, amax); }
  if (rowsum > D.lambda * (1 + 1e-14)) { fails++; std::printf("FAIL row sum %.17g above lambda %.17g\n", rowsum, D.lambda); }
  // nodal: block (a, b) -> Vp block Vpinv
  std::vector<double> Bn(N * N, 0.0), tmp((size_t)np * np);
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
  FILE* f = std::fopen(argv[5], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[5]); return 2; }
  const double head[2] = {D.lambda, (double)N};
  const bool ok = std::fwrite(head, sizeof(double), 2, f) == 2 && std::fwrite(Bn.data(), sizeof(double), Bn.size(), f) == Bn.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("k %d nx %d periodic %d lambda %.17g rowsum %.17g asym %.3e null %.3e\n", k, nx, per, D.lambda, rowsum, asym, null);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
