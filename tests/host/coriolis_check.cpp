// Host check of the Coriolis tables of csrc/hdg_tables.hpp (g++, no HIP): assembles M^-1 C of an nx x nx structured mesh (unit
// square, or the doubly periodic square with beta = 0) from Y_s exactly as k_coriolis forms a cell's block,
// (f_c(y_{j+s}) I + beta h Y_s) (x) J, maps it from the orthonormal modal basis to the nodal one (V B V^-1 per block) and writes
// it for tests/test_coriolis_cpu.py to compare with the numpy reference.  Its own checks: L_1, L_2 and Y_s are symmetric, and
// the general-mesh form of the same cells, f_0 I + (f_1 - f_0) L_1 + (f_2 - f_0) L_2 from the three vertex ordinates, gives
// the same block.
//   usage: coriolis_check k nx periodic L f0 beta out.bin    cell order 2 (j nx + i) + s, dof ((cell nu + mode) 2 + component)
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

int main(int argc, char** argv) {
  if (argc != 8) { std::printf("usage: k nx periodic L f0 beta out\n"); return 2; }
  const int k = std::atoi(argv[1]), nx = std::atoi(argv[2]), per = std::atoi(argv[3]);
  const double L = std::atof(argv[4]), h = L / nx, f0 = std::atof(argv[5]), beta = std::atof(argv[6]);
  if (k < 1 || k > 4 || nx < 2 || nx > 8 || (per && beta != 0.0)) { std::printf("arguments out of range\n"); return 2; }
  const CoriolisTables D(k);
  const Tables T(k, h, 1.0, 1.0, 0);
  const int nu = D.nu, nc = 2 * nx * nx;
  const size_t N = (size_t)nc * nu * 2, nn = (size_t)nu * nu;
  int fails = 0;
  auto asym = [&](const dvec& A) {
    double a = 0.0;
    for (int r = 0; r < nu; r++)
      for (int m = 0; m < nu; m++) a = std::fmax(a, std::fabs(A[(size_t)r * nu + m] - A[(size_t)m * nu + r]));
    return a;
  };
  const double worst_asym = std::fmax(std::fmax(asym(D.L[0]), asym(D.L[1])), std::fmax(asym(D.Y[0]), asym(D.Y[1])));
  if (worst_asym > 1e-15) { fails++; std::printf("FAIL symmetry of the tables %.3e\n", worst_asym); }
  if (D.packed().size() != 2 * nn || D.general().size() != 2 * nn) { fails++; std::printf("FAIL packed sizes\n"); }
  std::vector<double> Bn(N * N, 0.0), B(nn), tmp(nn);
  double twoforms = 0.0;
  for (int j = 0; j < nx; j++)
    for (int i = 0; i < nx; i++)
      for (int s = 0; s < 2; s++) {
        const size_t c = 2 * ((size_t)j * nx + i) + s;
        const double fr = f0 + beta * h * (j + s);
        // the general-mesh form: shape L has the vertices (x_i, y_j), (x_{i+1}, y_j), (x_i, y_{j+1}); shape U the vertices
        // (x_{i+1}, y_{j+1}), (x_i, y_{j+1}), (x_{i+1}, y_j)
        const double y0 = h * (j + s), y1 = y0, y2 = s == 0 ? h * (j + 1) : h * j;
        for (int r = 0; r < nu; r++)
          for (int m = 0; m < nu; m++) {
            B[(size_t)r * nu + m] = (r == m ? fr : 0.0) + beta * h * D.Y[s][(size_t)r * nu + m];
            const double gen = (r == m ? f0 + beta * y0 : 0.0) + beta * (y1 - y0) * D.L[0][(size_t)r * nu + m] + beta * (y2 - y0) * D.L[1][(size_t)r * nu + m];
            twoforms = std::fmax(twoforms, std::fabs(gen - B[(size_t)r * nu + m]));
          }
        for (int r = 0; r < nu; r++)
          for (int m = 0; m < nu; m++) {
            long double acc = 0;
            for (int l = 0; l < nu; l++) acc += (long double)T.Vu[(size_t)r * nu + l] * B[(size_t)l * nu + m];
            tmp[(size_t)r * nu + m] = (double)acc;
          }
        for (int r = 0; r < nu; r++)
          for (int m = 0; m < nu; m++) {
            long double acc = 0;
            for (int l = 0; l < nu; l++) acc += (long double)tmp[(size_t)r * nu + l] * T.Vuinv[(size_t)l * nu + m];
            Bn[((c * nu + r) * 2 + 0) * N + (c * nu + m) * 2 + 1] = (double)acc;   // out_x =   f_c u_y
            Bn[((c * nu + r) * 2 + 1) * N + (c * nu + m) * 2 + 0] = -(double)acc;  // out_y = - f_c u_x
          }
      }
  if (twoforms > 1e-14 * (std::fabs(f0) + std::fabs(beta) * L)) { fails++; std::printf("FAIL the two forms of a block differ by %.3e\n", twoforms); }
  FILE* f = std::fopen(argv[7], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[7]); return 2; }
  const double head[1] = {(double)N};
  const bool ok = std::fwrite(head, sizeof(double), 1, f) == 1 && std::fwrite(Bn.data(), sizeof(double), Bn.size(), f) == Bn.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("k %d nx %d periodic %d f0 %.17g beta %.17g asym %.3e two forms %.3e\n", k, nx, per, f0, beta, worst_asym, twoforms);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
