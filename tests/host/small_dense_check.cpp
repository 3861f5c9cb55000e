// CPU check of csrc/hdg_small_dense.hpp and csrc/hdg_dispatch.hpp (compiled by tests/test_host.py with g++).
//   hessenberg_eig  on the symmetric tridiagonal Toeplitz matrix (diagonal a, off-diagonals b): eigenvalues
//                   a + 2 b cos(j pi / (n + 1)).  The matrix is normal, so an eigenvalue moves by at most the norm of what
//                   deflation discards: at most n - 1 = 31 subdiagonals of at most 2e-14 |H| each, 6.2e-13 |H|; the bound
//                   1e-11 (|a| + 2|b|) leaves a factor 16 for the rounding of the rotations.
//   sstep_ls        on Gram matrices formed in long double from explicit vectors: orthogonal columns (the Cholesky factor of
//                   the scaled set is the identity, only long double rounding enters: 1e-12 relative), and a set whose last
//                   column is the sum of the first two (rank 2, the rank-2 residual).  The right-hand side is chosen so that the
//                   residual is O(1): rho is a difference of Gram entries and cancels for residuals far below |K_0|.
//   with_int / with_bool  call f with the listed value as a type; a value outside the list throws std::string.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_dispatch.hpp"
#include "../../incompressibleeulerhdg_amd/csrc/hdg_small_dense.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("error line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void check_eig(int n, double a, double b) {
  std::vector<double> H((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) {
    H[(size_t)i * n + i] = a;
    if (i + 1 < n) H[(size_t)i * n + i + 1] = H[(size_t)(i + 1) * n + i] = b;
  }
  const std::vector<std::complex<double>> ev = hdg::hessenberg_eig(H, n);
  CHECK((int)ev.size() == n);
  if ((int)ev.size() != n) return;
  const double scale = std::fabs(a) + 2.0 * std::fabs(b), pi = std::acos(-1.0);
  std::vector<double> got(n), want(n);
  double worst = 0.0, worst_im = 0.0;
  for (int j = 0; j < n; j++) {
    got[j] = ev[j].real();
    want[j] = a + 2.0 * b * std::cos((j + 1) * pi / (n + 1));
    worst_im = std::max(worst_im, std::fabs(ev[j].imag()));
  }
  std::sort(got.begin(), got.end());
  std::sort(want.begin(), want.end());
  for (int j = 0; j < n; j++) worst = std::max(worst, std::fabs(got[j] - want[j]));
  std::printf("hessenberg_eig n = %d a = %g b = %g: error %.2e, imaginary parts %.2e (of |a| + 2|b|)\n", n, a, b, worst / scale, worst_im / scale);
  CHECK(worst <= 1e-11 * scale);
  CHECK(worst_im <= 1e-11 * scale);
}

typedef std::vector<long double> lvec;
static long double dotl(const lvec& x, const lvec& y) {
  long double acc = 0.0L;
  for (size_t q = 0; q < x.size(); q++) acc += x[q] * y[q];
  return acc;
}
// Gram matrix of K_0 .. K_sl, row-major
static lvec gram(const std::vector<lvec>& Kv) {
  const int nv = (int)Kv.size();
  lvec G((size_t)nv * nv);
  for (int i = 0; i < nv; i++)
    for (int j = 0; j < nv; j++) G[(size_t)i * nv + j] = dotl(Kv[i], Kv[j]);
  return G;
}

static void check_sstep_ls() {
  const lvec K0 = {1.0L, 2.0L, -1.0L, 1.5L, 0.5L};
  {  // orthogonal columns with O(1) norms: y_i = K_0[i] / c_i, residual = the components no column reaches
    const lvec K1 = {2.0L, 0, 0, 0, 0}, K2 = {0, 0.5L, 0, 0, 0}, K3 = {0, 0, 3.0L, 0, 0};
    const lvec G = gram({K0, K1, K2, K3});
    lvec y;
    double rho = 0.0;
    const int rank = hdg::sstep_ls(G, 4, 3, y, rho);
    CHECK(rank == 3 && y.size() == 3);
    const long double want[3] = {0.5L, 4.0L, -1.0L / 3.0L};
    double worst = 0.0;
    for (int i = 0; i < 3; i++) worst = std::max(worst, (double)(std::fabs(y[i] - want[i]) / std::fabs(want[i])));
    const double rho_want = std::sqrt(1.5 * 1.5 + 0.5 * 0.5);
    std::printf("sstep_ls orthogonal set: y error %.2e, rho error %.2e (relative)\n", worst, std::fabs(rho - rho_want) / rho_want);
    CHECK(worst <= 1e-12);
    CHECK(std::fabs(rho - rho_want) <= 1e-12 * rho_want);
  }
  {  // the third column is the sum of the first two: the factorisation stops at rank 2
    const lvec K1 = {2.0L, 0, 0, 0, 0}, K2 = {0, 0.5L, 0, 0, 0}, K3 = {2.0L, 0.5L, 0, 0, 0};
    const lvec G = gram({K0, K1, K2, K3});
    lvec y;
    double rho = 0.0;
    const int rank = hdg::sstep_ls(G, 4, 3, y, rho);
    CHECK(rank == 2);
    CHECK(y.size() == 3 && y[2] == 0.0L);
    const double rho_want = std::sqrt(1.0 + 1.5 * 1.5 + 0.5 * 0.5);  // what K_1, K_2 cannot reach
    std::printf("sstep_ls dependent set: rank %d, rho error %.2e (relative)\n", rank, std::fabs(rho - rho_want) / rho_want);
    CHECK(std::fabs(rho - rho_want) <= 1e-12 * rho_want);
  }
}

static void check_transpose() {
  const std::vector<double> a = {1, 2, 3, 4, 5, 6};  // 2 x 3
  const std::vector<double> t = hdg::transpose(a, 2, 3);
  CHECK((t == std::vector<double>{1, 4, 2, 5, 3, 6}));
}

template <int V, bool B> static int tagged() { return B ? V : -V; }
static void check_dispatch() {
  int got = 0, calls = 0;
  for (int x : {1, 2, 4})
    for (bool b : {false, true}) {
      hdg::with_int<1, 2, 4>(x, "value", [&](auto v) { hdg::with_bool(b, [&](auto f) { got = tagged<v(), f()>(); calls++; }); });
      CHECK(got == (b ? x : -x));
    }
  CHECK(calls == 6);
  bool thrown = false;
  try {
    hdg::with_int<1, 2, 4>(3, "value", [&](auto) { calls++; });
  } catch (const std::string& e) {
    thrown = e.find("value = 3") != std::string::npos;
  }
  CHECK(thrown && calls == 6);
}

int main() {
  for (int n : {8, 16, 32}) {
    check_eig(n, 2.0, -1.0);
    check_eig(n, -0.5, 0.75);
  }
  check_sstep_ls();
  check_transpose();
  check_dispatch();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
