// CPU check of the host / device parts of point evaluation (csrc/hdg_points.hpp, the GLocator of csrc/hdg_general.hpp).
// Compiled with g++ by tests/test_probes_cpu.py; prints "name value" lines the test asserts on.
//   basis                    dubiner_at<D> against Dubiner::eval (hdg_tables.hpp, long double) for D = 1..5: values and
//                            reference gradients at random points, the three vertices (eta = 1 included), points on the
//                            three edges: basis_points, basis_max_err (max |a - b| / max(1, |b|))
//   locate MESHFILE          the bucket locator against a brute-force search over all cells ("nv nc / coords / cells"):
//                            random points over the widened bounding box, every vertex and edge midpoint, every vertex
//                            pushed 1e-9 and 1e-13 (relative) away from the origin: locate_checked, locate_mismatch,
//                            locate_outside, locate_inside
//   square nx ny L periodic POINTFILE
//                            square_locate for every "x y" line: "pt <index> <i> <j> <s> <xi> <eta>" or "pt <index> out"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tables.hpp"
#include "../../incompressibleeulerhdg_amd/csrc/hdg_general.hpp"
#include "../../incompressibleeulerhdg_amd/csrc/hdg_points.hpp"

using namespace hdg;

template <int D>
static double check_degree(const std::vector<double>& xs, const std::vector<double>& ys) {
  constexpr int N = (D + 1) * (D + 2) / 2;
  Dubiner U(D);
  double err = 0.0;
  for (size_t t = 0; t < xs.size(); t++) {
    real v[N], gx[N], gy[N];
    double w[N], hx[N], hy[N];
    U.eval((real)xs[t], (real)ys[t], v, gx, gy);
    dubiner_at<D>(xs[t], ys[t], w, hx, hy);
    for (int m = 0; m < N; m++) {
      err = std::max(err, std::fabs(w[m] - (double)v[m]) / std::max(1.0, std::fabs((double)v[m])));
      err = std::max(err, std::fabs(hx[m] - (double)gx[m]) / std::max(1.0, std::fabs((double)gx[m])));
      err = std::max(err, std::fabs(hy[m] - (double)gy[m]) / std::max(1.0, std::fabs((double)gy[m])));
      if (!std::isfinite(w[m]) || !std::isfinite(hx[m]) || !std::isfinite(hy[m])) err = INFINITY;
    }
  }
  return err;
}

static int run_basis() {
  std::mt19937_64 rng(20261016);
  std::uniform_real_distribution<double> U01(0.0, 1.0);
  std::vector<double> xs, ys;
  for (int t = 0; t < 400; t++) {
    double a = U01(rng), b = U01(rng);
    if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
    xs.push_back(a); ys.push_back(b);
  }
  const double V[3][2] = {{0, 0}, {1, 0}, {0, 1}};
  for (auto& v : V) { xs.push_back(v[0]); ys.push_back(v[1]); }
  for (int t = 0; t <= 20; t++) {
    const double s = t / 20.0;
    xs.push_back(s); ys.push_back(0.0);          // eta = 0
    xs.push_back(1.0 - s); ys.push_back(s);      // hypotenuse
    xs.push_back(0.0); ys.push_back(s);          // xi = 0
  }
  double err = 0.0;
  err = std::max(err, check_degree<1>(xs, ys));
  err = std::max(err, check_degree<2>(xs, ys));
  err = std::max(err, check_degree<3>(xs, ys));
  err = std::max(err, check_degree<4>(xs, ys));
  err = std::max(err, check_degree<5>(xs, ys));
  std::printf("basis_points %zu\nbasis_max_err %.3e\n", xs.size(), err);
  return 0;
}

static int run_locate(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::printf("error cannot_open\n"); return 1; }
  int nv, nc;
  if (std::fscanf(f, "%d %d", &nv, &nc) != 2) { std::printf("error header\n"); return 1; }
  std::vector<double> X((size_t)2 * nv);
  std::vector<int> Cc((size_t)3 * nc);
  for (auto& x : X) if (std::fscanf(f, "%lf", &x) != 1) { std::printf("error coords\n"); return 1; }
  for (auto& c : Cc) if (std::fscanf(f, "%d", &c) != 1) { std::printf("error cells\n"); return 1; }
  std::fclose(f);
  GMesh M;
  M.build(nv, X.data(), nc, Cc.data());
  GLocator Lc;
  Lc.build(M);
  double x0 = X[0], x1 = X[0], y0 = X[1], y1 = X[1];
  for (int v = 0; v < nv; v++) {
    x0 = std::min(x0, X[2 * v]); x1 = std::max(x1, X[2 * v]);
    y0 = std::min(y0, X[2 * v + 1]); y1 = std::max(y1, X[2 * v + 1]);
  }
  std::vector<double> px, py;
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U01(0.0, 1.0);
  for (int t = 0; t < 20000; t++) {
    px.push_back(x0 - 0.05 * (x1 - x0) + 1.1 * (x1 - x0) * U01(rng));
    py.push_back(y0 - 0.05 * (y1 - y0) + 1.1 * (y1 - y0) * U01(rng));
  }
  for (int v = 0; v < nv; v++) {
    px.push_back(X[2 * v]); py.push_back(X[2 * v + 1]);
    for (double eps : {1e-9, 1e-13}) { px.push_back(X[2 * v] * (1 + eps)); py.push_back(X[2 * v + 1] * (1 + eps)); }
  }
  for (int e = 0; e < M.ne; e++) {
    const int a = M.ev[2 * (size_t)e], b = M.ev[2 * (size_t)e + 1];
    px.push_back(0.5 * (X[2 * a] + X[2 * b])); py.push_back(0.5 * (X[2 * a + 1] + X[2 * b + 1]));
  }
  long mismatch = 0, outside = 0, inside = 0;
  for (size_t t = 0; t < px.size(); t++) {
    double a = 0, b = 0, c = 0, d = 0;
    const int cl = Lc.locate(M, px[t], py[t], POINT_TOL, a, b);
    const int cb = gcell_brute_force(M, px[t], py[t], POINT_TOL, c, d);
    if (cl != cb || (cl >= 0 && (a != c || b != d))) mismatch++;
    (cb < 0 ? outside : inside)++;
  }
  std::printf("locate_checked %zu\nlocate_mismatch %ld\nlocate_outside %ld\nlocate_inside %ld\n", px.size(), mismatch, outside,
              inside);
  return 0;
}

static int run_square(int nx, int ny, double L, int periodic, const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::printf("error cannot_open\n"); return 1; }
  double x, y;
  int t = 0;
  while (std::fscanf(f, "%lf %lf", &x, &y) == 2) {
    int i, j, s;
    double xi, eta;
    if (square_locate(x, y, nx, ny, L, periodic != 0, i, j, s, xi, eta))
      std::printf("pt %d %d %d %d %.17g %.17g\n", t, i, j, s, xi, eta);
    else
      std::printf("pt %d out\n", t);
    t++;
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "basis")) return run_basis();
    if (argc >= 3 && !std::strcmp(argv[1], "locate")) return run_locate(argv[2]);
    if (argc >= 7 && !std::strcmp(argv[1], "square"))
      return run_square(std::atoi(argv[2]), std::atoi(argv[3]), std::atof(argv[4]), std::atoi(argv[5]), argv[6]);
  } catch (const std::string& e) {
    std::printf("error %s\n", e.c_str());
    return 1;
  }
  std::printf("error usage\n");
  return 2;
}
