// Host check of the moving-wall load vectors of ViscosityTables (csrc/hdg_tables.hpp; g++, no HIP): places lvec[s][e] on the
// wall legs of the nx x nx unit square exactly as k_viscosity<., true> does (side from (s, e), tangential component), one unit
// speed per side, maps the four vectors M^-1 l from the orthonormal modal basis to the nodal one and writes them, with the four
// force constants wone * (cells of the side), for tests/test_moving_walls_cpu.py to compare with the numpy reference.  Its own
// checks: lvec = - Wall coef(1) at 1e-11 max|entry|, wone = eta_b h, and packed_moving() is packed() followed by the four vectors.
//   usage: moving_walls_check k nx out.bin    cell order 2 (j nx + i) + s, dof ((cell nu + mode) 2 + component)
//   out:   N, wone, then 4 vectors of N doubles
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"

using namespace hdg;

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("usage: k nx out\n"); return 2; }
  const int k = std::atoi(argv[1]), nx = std::atoi(argv[2]);
  if (k < 1 || k > 4 || nx < 2 || nx > 16) { std::printf("arguments out of range\n"); return 2; }
  const double h = 1.0 / nx;
  const ViscosityTables D(k, h);
  const Tables T(k, h, 1.0, 1.0, 0);
  const int nu = D.nu, nc = 2 * nx * nx;
  const size_t N = (size_t)nc * nu * 2;
  int fails = 0;
  // coef(1): the constant is mode 0 alone; its coefficient c0 from the mass normalisation, psi_0^2 |K| = 1
  const double c0 = h / std::sqrt(2.0);
  for (int s = 0; s < 2; s++) {
    if (!D.lvec[s][1].empty()) { fails++; std::printf("FAIL lvec[%d][1] is not empty\n", s); }
    for (int e = 0; e < 3; e += 2) {
      if ((int)D.lvec[s][e].size() != nu) { fails++; std::printf("FAIL lvec[%d][%d] has %zu entries\n", s, e, D.lvec[s][e].size()); continue; }
      double dev = 0.0, lmax = 0.0;
      for (int r = 0; r < nu; r++) {
        dev = std::fmax(dev, std::fabs(c0 * D.Wall[s][e][(size_t)r * nu + 0] + D.lvec[s][e][(size_t)r]));  // (Wall coef(1))_r = - lvec_r
        lmax = std::fmax(lmax, std::fabs(D.lvec[s][e][(size_t)r]));
      }
      if (!(dev <= 1e-11 * lmax)) { fails++; std::printf("FAIL Wall[%d][%d] coef(1) + lvec %.3e of %.3e\n", s, e, dev, lmax); }
    }
  }
  if (std::fabs(D.wone - D.eta_b * h) > 1e-14 * D.wone) { fails++; std::printf("FAIL wone\n"); }
  {
    const dvec P = D.packed(), Pm = D.packed_moving();
    bool same = P.size() == (size_t)2 * ViscosityTables::NBLK * nu * nu && Pm.size() == P.size() + (size_t)4 * nu;
    for (size_t n = 0; same && n < P.size(); n++) same = P[n] == Pm[n];
    size_t at = P.size();
    for (int s = 0; same && s < 2; s++)
      for (int e = 0; same && e < 3; e += 2)
        for (int r = 0; same && r < nu; r++) same = Pm[at++] == D.lvec[s][e][(size_t)r];
    if (!same) { fails++; std::printf("FAIL packed_moving is not packed() followed by the four vectors\n"); }
  }
  std::vector<double> load(4 * N, 0.0), ln(4 * N, 0.0);  // modal, nodal
  auto cell = [&](int i, int j, int s) { return 2 * (j * nx + i) + s; };
  for (int j = 0; j < nx; j++)
    for (int i = 0; i < nx; i++)
      for (int s = 0; s < 2; s++)
        for (int e = 0; e < 3; e += 2) {
          const int in = e == 2 ? (s == 0 ? i - 1 : i + 1) : i, jn = e == 0 ? (s == 0 ? j - 1 : j + 1) : j;
          if (in >= 0 && in < nx && jn >= 0 && jn < nx) continue;  // a neighbour: no wall
          const int w = ViscosityTables::wall_side(s, e), comp = 1 - ViscosityTables::wall_normal_component(e);
          for (int r = 0; r < nu; r++) load[(size_t)w * N + ((size_t)cell(i, j, s) * nu + r) * 2 + comp] += D.lvec[s][e][(size_t)r];
        }
  for (int w = 0; w < 4; w++)
    for (int c = 0; c < nc; c++)
      for (int d = 0; d < 2; d++)
        for (int r = 0; r < nu; r++) {
          long double acc = 0;
          for (int l = 0; l < nu; l++) acc += (long double)T.Vu[(size_t)r * nu + l] * load[(size_t)w * N + ((size_t)c * nu + l) * 2 + d];
          ln[(size_t)w * N + ((size_t)c * nu + r) * 2 + d] = (double)acc;
        }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) { std::printf("cannot write %s\n", argv[3]); return 2; }
  const double head[2] = {(double)N, D.wone};
  const bool ok = std::fwrite(head, sizeof(double), 2, f) == 2 && std::fwrite(ln.data(), sizeof(double), ln.size(), f) == ln.size();
  std::fclose(f);
  if (!ok) { std::printf("short write\n"); return 2; }
  std::printf("k %d nx %d nu %d wone %.17g\n", k, nx, nu, D.wone);
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
