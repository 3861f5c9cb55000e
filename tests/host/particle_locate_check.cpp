// CPU check that the host / device square_locate of csrc/hdg_points.hpp (run on the device by the particle kernels of
// csrc/hdg_particles.hpp) locates every point as the host-only function did before it was shared.  Compiled with g++ by
// tests/test_particles_cpu.py; prints "name value" lines the test asserts on.
//   usage: particle_locate_check nx L periodic
// 10^5 seeded points: random ones over [-L, 2 L]^2, exact cell vertices, edge midpoints and diagonal points, the seam and the
// corners, and each of those moved by one unit in the last place either way.  Compared: the return value and, for located
// points, (i, j, s, xi, eta) bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_points.hpp"

using namespace hdg;

// the rule as it stood on the host alone (include/hdg_mi355x.h: ownership), one operation per statement
static bool locate_before(double x, double y, int nx, int ny, double L, bool periodic, int& i, int& j, int& s, double& xi,
                          double& eta) {
  const double h = L / nx;
  const double Lx = L, Ly = ny == nx ? L : ny * h;
  if (!(std::isfinite(x) && std::isfinite(y))) return false;
  if (periodic) {
    const double wx = std::floor(x / Lx) * Lx;
    const double wy = std::floor(y / Ly) * Ly;
    x -= wx;
    y -= wy;
    if (x >= Lx || x < 0.0) x = 0.0;
    if (y >= Ly || y < 0.0) y = 0.0;
  } else {
    const double tx = POINT_TOL * Lx, ty = POINT_TOL * Ly;
    if (x < -tx || x > Lx + tx || y < -ty || y > Ly + ty) return false;
    x = std::fmin(std::fmax(x, 0.0), Lx);
    y = std::fmin(std::fmax(y, 0.0), Ly);
  }
  i = (int)std::floor(x / h);
  j = (int)std::floor(y / h);
  if (i > nx - 1) i = nx - 1;
  if (j > ny - 1) j = ny - 1;
  const double fx = x / h - i;
  const double fy = y / h - j;
  s = (fx + fy <= 1.0) ? 0 : 1;
  xi = s == 0 ? fx : 1.0 - fx;
  eta = s == 0 ? fy : 1.0 - fy;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("error usage\n"); return 1; }
  const int nx = std::atoi(argv[1]);
  const double L = std::atof(argv[2]);
  const bool periodic = std::atoi(argv[3]) != 0;
  const double h = L / nx;
  std::vector<double> xs, ys;
  auto add = [&](double x, double y) {
    const double dx[3] = {x, std::nextafter(x, -INFINITY), std::nextafter(x, INFINITY)};
    const double dy[3] = {y, std::nextafter(y, -INFINITY), std::nextafter(y, INFINITY)};
    for (double a : dx)
      for (double b : dy) { xs.push_back(a); ys.push_back(b); }
  };
  for (int j = 0; j <= nx; j++)
    for (int i = 0; i <= nx; i++) {
      add(i * h, j * h);                                  // vertices: the corners and the seam among them
      add((i + 0.5) * h, j * h);                          // horizontal edges
      add(i * h, (j + 0.5) * h);                          // vertical edges
      add((i + 0.25) * h, (j + 0.75) * h);                // the diagonal
      add((i + 0.5) * h, (j + 0.5) * h);
    }
  const double seam[] = {0.0, L, -L, 2 * L, 3 * L, -0.0, L * (1 + 1e-13), -1e-13 * L, L * (1 + 1e-9), -1e-9 * L};
  for (double a : seam)
    for (double b : seam) add(a, b);
  long special = (long)xs.size();
  std::mt19937_64 rng(20261016);
  std::uniform_real_distribution<double> U(-L, 2 * L);
  while (xs.size() < 100000) { xs.push_back(U(rng)); ys.push_back(U(rng)); }
  xs.push_back(NAN); ys.push_back(0.5 * L);
  xs.push_back(0.5 * L); ys.push_back(INFINITY);
  xs.push_back(1e300); ys.push_back(-1e300);
  long mismatch = 0, located = 0;
  for (size_t t = 0; t < xs.size(); t++) {
    int i0 = -1, j0 = -1, s0 = -1, i1 = -1, j1 = -1, s1 = -1;
    double a0 = 0, b0 = 0, a1 = 0, b1 = 0;
    const bool r0 = locate_before(xs[t], ys[t], nx, nx, L, periodic, i0, j0, s0, a0, b0);
    const bool r1 = square_locate(xs[t], ys[t], nx, nx, L, periodic, i1, j1, s1, a1, b1);
    if (r0 != r1) { mismatch++; continue; }
    if (!r0) continue;
    located++;
    if (i0 != i1 || j0 != j1 || s0 != s1 || std::memcmp(&a0, &a1, 8) != 0 || std::memcmp(&b0, &b1, 8) != 0) mismatch++;
    if (i1 < 0 || i1 >= nx || j1 < 0 || j1 >= nx) mismatch++;
  }
  std::printf("locate_points %ld\nlocate_special %ld\nlocate_located %ld\nlocate_mismatch %ld\n", (long)xs.size(), special,
              located, mismatch);
  return 0;
}
