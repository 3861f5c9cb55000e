// CPU check of csrc/hdg_krylov_host.hpp and csrc/hdg_tent_policy.hpp (compiled by tests/test_host.py with g++): the Givens
// least squares of the Arnoldi cycles against the normal equations in long double, and every decision of the
// tentative-velocity solver -- check schedule, verdicts of the Chebyshev monitor, Ritz interval, ellipse, s-step cycle
// lengths, the checkpoint columns of the stage records -- as literal values.  The expected values were derived by hand from
// the rules the engine's loops followed before the headers existed (the arithmetic is written out beside each case), not
// from the functions under test.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_krylov_host.hpp"
#include "../../incompressibleeulerhdg_amd/csrc/hdg_tent_policy.hpp"

using namespace hdg;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("error line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

// minimiser and residual norm of |beta e1 - H y| over the leading (n + 1) x n block, by the normal equations in long double
// (Gaussian elimination with partial pivoting)
static long double normal_equations(const double Hm[7][6], int n, double beta, std::vector<long double>& y) {
  std::vector<long double> A((size_t)n * n, 0.0L), b((size_t)n, 0.0L);
  for (int a = 0; a < n; a++) {
    for (int c = 0; c < n; c++)
      for (int r = 0; r <= n; r++) A[(size_t)a * n + c] += (long double)Hm[r][a] * (long double)Hm[r][c];
    b[(size_t)a] = (long double)Hm[0][a] * (long double)beta;
  }
  for (int p = 0; p < n; p++) {
    int best = p;
    for (int r = p + 1; r < n; r++) if (std::fabs(A[(size_t)r * n + p]) > std::fabs(A[(size_t)best * n + p])) best = r;
    for (int c = 0; c < n; c++) std::swap(A[(size_t)p * n + c], A[(size_t)best * n + c]);
    std::swap(b[(size_t)p], b[(size_t)best]);
    for (int r = p + 1; r < n; r++) {
      const long double f = A[(size_t)r * n + p] / A[(size_t)p * n + p];
      for (int c = p; c < n; c++) A[(size_t)r * n + c] -= f * A[(size_t)p * n + c];
      b[(size_t)r] -= f * b[(size_t)p];
    }
  }
  y.assign((size_t)n, 0.0L);
  for (int r = n - 1; r >= 0; r--) {
    long double acc = b[(size_t)r];
    for (int c = r + 1; c < n; c++) acc -= A[(size_t)r * n + c] * y[(size_t)c];
    y[(size_t)r] = acc / A[(size_t)r * n + r];
  }
  long double ss = 0.0L;
  for (int r = 0; r <= n; r++) {
    long double v = r == 0 ? (long double)beta : 0.0L;
    for (int c = 0; c < n; c++) v -= (long double)Hm[r][c] * y[(size_t)c];
    ss += v * v;
  }
  return std::sqrt(ss);
}

static void givens() {
  // upper Hessenberg, 7 x 6: a diagonal of 2 .. 3, a sub-diagonal that decays like the hn of a converging cycle
  const double Hm[7][6] = {{2.0, 0.5, -0.3, 0.2, 0.1, -0.05},
                           {1.0, 2.5, 0.4, -0.2, 0.3, 0.1},
                           {0.0, 0.8, 3.0, 0.6, -0.1, 0.2},
                           {0.0, 0.0, 0.6, 2.2, 0.5, -0.3},
                           {0.0, 0.0, 0.0, 0.4, 2.8, 0.7},
                           {0.0, 0.0, 0.0, 0.0, 0.3, 2.4},
                           {0.0, 0.0, 0.0, 0.0, 0.0, 0.2}};
  const double beta = 1.7;
  GivensLsq L(6, true);
  L.start(beta);
  for (int j = 0; j < 6; j++) {
    double h[6];
    for (int l = 0; l <= j; l++) h[l] = Hm[l][j];
    const double res = L.add_column(j, h, Hm[j + 1][j]);
    std::vector<long double> yn;
    const long double rn = normal_equations(Hm, j + 1, beta, yn);
    CHECK(near(res, (double)rn, 1e-12 * beta));  // the value returned is the least-squares residual of the leading block
    const std::vector<double> y = L.solve(j + 1);
    CHECK((int)y.size() == j + 1);
    long double ymax = 0.0L;
    for (long double v : yn) ymax = std::max(ymax, std::fabs(v));
    for (int l = 0; l <= j; l++) CHECK(near(y[(size_t)l], (double)yn[(size_t)l], 1e-12 * (double)ymax));
  }
  // the unrotated matrix is kept next to the rotated one: leading 4 x 4 block, dense
  const std::vector<double> U = L.unrotated(4);
  for (int a = 0; a < 4; a++) for (int c = 0; c < 4; c++) CHECK(U[(size_t)a * 4 + c] == Hm[a][c]);
  CHECK(GivensLsq(6).Hraw.empty());
  // hn == 0: with a zero diagonal entry as well rr == 0 -> cs = 1, sn = 0, nothing is divided; otherwise cs = 1, sn = 0 from rr
  {
    GivensLsq Z(3);
    Z.start(1.0);
    const double h0[1] = {0.0};
    const double r0 = Z.add_column(0, h0, 0.0);
    CHECK(Z.cs[0] == 1.0 && Z.sn[0] == 0.0 && r0 == 0.0 && Z.gv[0] == 1.0);
    GivensLsq W(3);
    W.start(1.0);
    const double h1[1] = {2.0};
    const double r1 = W.add_column(0, h1, 0.0);
    CHECK(W.cs[0] == 1.0 && W.sn[0] == 0.0 && r1 == 0.0 && W.solve(1)[0] == 0.5);
  }
}

static std::vector<int> checks(const ChebMonitor& m, int kmax) {
  std::vector<int> v;
  for (int k = 1; k <= kmax; k++) if (m.check_at(k)) v.push_back(k);
  return v;
}

static void schedule() {
  Options o;
  CHECK(o.cheb_fine_step == 2);
  {
    ChebStage st;  // no history: every 4th
    ChebMonitor m(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m.kfine == 0 && checks(m, 16) == (std::vector<int>{4, 8, 12, 16}));
  }
  {
    ChebStage st;
    st.last = 22;  // kfine = max(4, (22 - 6 - 4) & ~1) = 12: every 8th below it, every 2nd from it
    ChebMonitor m(st, 6, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m.kfine == 12 && checks(m, 18) == (std::vector<int>{8, 12, 14, 16, 18}));
    o.cheb_fine_step = 3;
    CHECK(checks(m, 18) == (std::vector<int>{8, 12, 15, 18}));
    o.cheb_fine_step = 2;
  }
  {
    ChebStage st;
    st.last = 9;  // (9 - 0 - 4) & ~1 = 4; a short history never gives less than 4: last = 7 -> max(4, 2) = 4
    ChebMonitor m(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m.kfine == 4 && checks(m, 10) == (std::vector<int>{4, 6, 8, 10}));
    st.last = 7;
    CHECK(ChebMonitor(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000).kfine == 4);
  }
}

// target 1e-10, beta0 = 1 (so the monitor starts with last = stall_ref = 1), expected = 30, iteration limit 1000
static void verdicts() {
  const Options o;
  CHECK(o.cheb_min_k == 6 && o.cheb_max_expected == 64 && !o.tail_gmres);
  // ---- growing: nz > 100 * (smallest norm seen)
  {
    ChebStage st;
    st.lmin = 1.0; st.lmax = 4.0;
    ChebMonitor m(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m.observe(4, 4, 0.5) == ChebVerdict::Continue && m.last == 0.5);
    CHECK(m.observe(8, 8, 50.0) == ChebVerdict::Continue && m.last == 0.5);  // 50 = 100 * 0.5: not above
    CHECK(m.observe(12, 12, 60.0) == ChebVerdict::Growing && !m.tail);
    CHECK(st.lmin == -1.0 && st.lmax == -1.0 && st.widen == 1.25 && st.slow == 0 && st.last == 0 && st.hand == 0);
    // 1.25^n: 1.5625, 1.953125, 2.44140625, 3.0517578125, 3.814697265625, then 4.768... is cut to 4
    for (int n = 2; n <= 6; n++) CHECK(ChebMonitor(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000).observe(4, 4, 101.0) == ChebVerdict::Growing);
    CHECK(st.widen == 3.814697265625);
    for (int n = 7; n <= 9; n++) {
      CHECK(ChebMonitor(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000).observe(4, 4, 101.0) == ChebVerdict::Growing);
      CHECK(st.widen == 4.0);
    }
  }
  // ---- stalled: eight checks in a row that do not halve stall_ref; sets slow, does not widen
  {
    ChebStage st;
    st.lmin = 1.0; st.lmax = 4.0;
    ChebMonitor m(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    for (int c = 1; c <= 7; c++) CHECK(m.observe(4 * c, 4 * c, 0.9) == ChebVerdict::Continue && m.stall_checks == c);
    CHECK(m.observe(32, 32, 0.9) == ChebVerdict::Stalled && !m.tail);
    CHECK(st.slow == 1 && st.widen == 1.0 && st.lmin == 1.0 && st.lmax == 4.0 && st.hand == 0 && st.last == 0);
    // a halving in between starts the count again: 0.9 x 3, 0.4 (< 0.5 * 1), 0.39 x 7 -> still running
    ChebStage s2;
    ChebMonitor m2(s2, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    for (int c = 1; c <= 3; c++) CHECK(m2.observe(c, c, 0.9) == ChebVerdict::Continue);
    CHECK(m2.observe(4, 4, 0.4) == ChebVerdict::Continue && m2.stall_checks == 0 && m2.stall_ref == 0.4);
    for (int c = 5; c <= 11; c++) CHECK(m2.observe(c, c, 0.39) == ChebVerdict::Continue);
    CHECK(m2.observe(12, 12, 0.39) == ChebVerdict::Stalled && s2.slow == 1);
    // far beyond the prediction: k > 6 * expected + 64 = 244; and the iteration limit
    ChebStage s3;
    ChebMonitor m3(s3, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m3.observe(244, 244, 0.4) == ChebVerdict::Continue);
    CHECK(m3.observe(245, 245, 0.1) == ChebVerdict::Stalled && s3.slow == 1);
    ChebStage s4;
    CHECK(ChebMonitor(s4, 0, 30, o, 0.0, 1e-10, 1.0, 1000).observe(4, 1000, 0.4) == ChebVerdict::Stalled && s4.slow == 1);
    CHECK(ChebMonitor(s4, 0, 30, o, 0.0, 1e-10, 1.0, 1000).observe(4, 999, 0.4) == ChebVerdict::Continue);
  }
  // ---- deliberate hand-over at rate 0.3: nz(4) = 1e-2, nz(8) = 1e-3: observed rate 0.1^(1/4) = 0.562 > 0.3, remaining
  // log(1e-10 / 1e-3) / log(0.562) = 28 > 6, k = 8 >= min_k = 6 -> slow tail; the slow segment began at k = 4
  {
    ChebStage st;
    ChebMonitor m(st, 6, 30, o, 0.3, 1e-10, 1.0, 1000);
    CHECK(m.observe(4, 10, 1e-2) == ChebVerdict::Continue && st.hand == 0);
    CHECK(m.observe(8, 14, 1e-3) == ChebVerdict::SlowTail && m.tail);
    CHECK(st.hand == 4 && st.last == 14 && st.slow == 0 && st.widen == 1.0 && st.lmin == -1.0);
    // the next solve of the stage hands over at the first check with k >= 4, without measuring a rate again
    // (k = 5 < min_k, so the rate rule itself is silent: (0.05 / 0.1)^(1/2) = 0.707 > 0.3 notwithstanding)
    ChebMonitor n(st, 0, 30, o, 0.3, 1e-10, 1.0, 1000);
    CHECK(n.observe(3, 3, 0.1) == ChebVerdict::Continue && !n.tail);
    CHECK(n.observe(5, 5, 0.05) == ChebVerdict::SlowTail && n.tail && st.hand == 4 && st.last == 5);
    // ... unless the GMRES tail is chosen (its iterations cost more: the rate is confirmed every time)
    Options og;
    og.tail_gmres = true;
    ChebMonitor g(st, 0, 30, og, 0.3, 1e-10, 1.0, 1000);
    CHECK(g.observe(3, 3, 0.1) == ChebVerdict::Continue && g.observe(5, 5, 0.05) == ChebVerdict::Continue && !g.tail);
    // growth seen at the learnt point: the record goes by the growth, the finishing solver is still the tail's
    ChebMonitor w(st, 0, 30, o, 0.3, 1e-10, 1.0, 1000);
    CHECK(w.observe(4, 4, 101.0) == ChebVerdict::Growing && w.tail && st.widen == 1.25 && st.hand == 4);
    // before min_k the rate rule is silent: the same norms at k = 2, 5 (rate 0.1^(1/3) = 0.464 > 0.3, remaining 21 > 6)
    ChebStage s2;
    ChebMonitor e(s2, 0, 30, o, 0.3, 1e-10, 1.0, 1000);
    CHECK(e.observe(2, 2, 1e-2) == ChebVerdict::Continue && e.observe(5, 5, 1e-3) == ChebVerdict::Continue && s2.hand == 0);
    // a few iterations from the end it is silent too: nz(4) = 1e-7, nz(8) = 1e-9: rate 0.316 > 0.3, remaining 2 <= 6
    ChebStage s3;
    ChebMonitor f(s3, 0, 30, o, 0.3, 1e-10, 1.0, 1000);
    CHECK(f.observe(4, 4, 1e-7) == ChebVerdict::Continue && f.observe(8, 8, 1e-9) == ChebVerdict::Continue && s3.hand == 0);
  }
  // ---- handover = 0: none of that; only k >= 16 with an observed rate > 0.75 that needs > 24 further iterations
  {
    ChebStage st;
    ChebMonitor m(st, 6, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(m.observe(4, 10, 1e-2) == ChebVerdict::Continue && m.observe(8, 14, 1e-3) == ChebVerdict::Continue && st.hand == 0 && !m.tail);
    // nz(12) = 1e-3 (no progress: no rate), nz(16) = 8e-4: rate 0.8^(1/4) = 0.946, remaining log(1.25e-7) / log(0.946) = 285
    CHECK(m.observe(12, 18, 1e-3) == ChebVerdict::Continue);
    CHECK(m.observe(16, 22, 8e-4) == ChebVerdict::SlowTail && m.tail && st.hand == 12 && st.last == 22);
    st.hand = 7;  // a learnt point is not used without a hand-over rate
    ChebMonitor n(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(n.observe(11, 11, 1e-3) == ChebVerdict::Continue && n.observe(15, 15, 8e-4) == ChebVerdict::Continue);  // k = 15 < 16
    CHECK(st.hand == 7);
    ChebMonitor p(st, 0, 30, o, 0.0, 1e-10, 1.0, 1000);
    CHECK(p.observe(12, 12, 1e-3) == ChebVerdict::Continue && p.observe(16, 16, 3e-4) == ChebVerdict::Continue);  // rate 0.74
  }
  // ---- convergence: slow exactly when its > 64 + 32 = 96
  {
    ChebStage st;
    st.slow = 1;
    CHECK(ChebMonitor(st, 0, 30, o, 0.3, 1e-10, 1.0, 1000).observe(90, 96, 1e-10) == ChebVerdict::Converged && st.slow == 0 && st.last == 96);
    CHECK(ChebMonitor(st, 0, 30, o, 0.3, 1e-10, 1.0, 1000).observe(91, 97, 5e-11) == ChebVerdict::Converged && st.slow == 1 && st.last == 97);
    CHECK(st.hand == 0 && st.widen == 1.0);
  }
}

static void interval() {
  using C = std::complex<double>;
  const std::vector<C> ritz = {C(2.0, 0.7), C(1.1, 0.0), C(3.2, -0.4), C(2.0, -0.7)};
  Options o;
  ChebStage st;
  CHECK(ritz_interval(ritz, st, o, true, 2) && near(st.lmin, 0.99, 1e-14) && near(st.lmax, 4.16, 1e-14));  // 1.1 * 0.9, 3.2 * 1.3
  st.lmin = 0.9; st.lmax = 4.0;
  CHECK(ritz_interval(ritz, st, o, true, 2) && st.lmin == 0.9 && near(st.lmax, 4.16, 1e-14));  // the widest seen
  st = ChebStage{};
  CHECK(ritz_interval(ritz, st, o, true, 1) && near(st.lmin, 0.99, 1e-14) && near(st.lmax, 4.8, 1e-14));  // 3.2 * 1.5
  st = ChebStage{};
  CHECK(ritz_interval(ritz, st, o, true, 3) && near(st.lmax, 4.16, 1e-14));
  st = ChebStage{};
  CHECK(ritz_interval(ritz, st, o, false, 2) && near(st.lmin, 0.88, 1e-14) && near(st.lmax, 3.68, 1e-14));  // 0.8, 1.15
  st = ChebStage{};
  st.widen = 1.25;
  CHECK(ritz_interval(ritz, st, o, true, 2) && near(st.lmin, 0.99, 1e-14) && near(st.lmax, 5.2, 1e-14));  // 3.2 * 1.3 * 1.25
  st = ChebStage{};
  o.cheb_flo = 0.5; o.cheb_fhi = 2.0;
  CHECK(ritz_interval(ritz, st, o, true, 2) && near(st.lmin, 0.55, 1e-14) && near(st.lmax, 6.4, 1e-14));
  st.widen = 1.25;  // the override is widened like the default
  st.lmin = st.lmax = -1.0;
  CHECK(ritz_interval(ritz, st, o, false, 1) && near(st.lmax, 8.0, 1e-14));
  // rejected: a non-positive lower end, an empty interval, no values; the record is left alone
  st = ChebStage{};
  st.lmin = 0.9; st.lmax = 4.0;
  CHECK(!ritz_interval({C(-0.1, 0.0), C(2.0, 0.0)}, st, Options{}, true, 2));
  CHECK(!ritz_interval({C(0.0, 0.0), C(2.0, 0.0)}, st, Options{}, true, 2));
  CHECK(!ritz_interval({C(2.0, 1.0), C(2.0, -1.0)}, st, Options{}, true, 2));
  CHECK(!ritz_interval({}, st, Options{}, true, 2));
  CHECK(st.lmin == 0.9 && st.lmax == 4.0);
}

static void ellipse() {
  const ChebEllipse e(1.0, 4.8, 0.3);
  // theta = 2.9, a = 1.9, b = 0.57, delta^2 = 3.61 - 0.3249 = 3.2851, theta^2 - delta^2 = 8.41 - 3.2851 = 5.1249
  const double delta = std::sqrt(3.2851), rate = 2.47 / (2.9 + std::sqrt(5.1249));
  CHECK(near(e.theta, 2.9, 1e-14) && near(e.aax, 1.9, 1e-14) && near(e.bim, 0.57, 1e-14));
  CHECK(near(e.delta, delta, 1e-14) && near(e.sigma, 2.9 / delta, 1e-14) && near(e.rate, rate, 1e-14));
  // rate = 0.47833: log(1e-10) / log(rate) = 31.2 -> 31 + 8
  CHECK(e.expected(1e-10) == (int)(std::log(1e-10) / std::log(rate)) + 8 && e.expected(1e-10) == 39);
  CHECK(e.expected(1.0) == 8 && e.expected(0.0) == (int)(std::log(1e-300) / std::log(rate)) + 8);
  // a real interval: delta = a, rate = a / (theta + sqrt(theta^2 - a^2)); [1, 3]: 1 / (2 + sqrt 3)
  const ChebEllipse r(1.0, 3.0, 0.0);
  CHECK(near(r.delta, 1.0, 1e-14) && near(r.sigma, 2.0, 1e-14) && near(r.rate, 1.0 / (2.0 + std::sqrt(3.0)), 1e-14));
  // wide: [0.05, 6] at 0.3 has the rate 0.9497: 446 + 8 iterations for ten decades, far above cheb_max_expected = 64
  CHECK(ChebEllipse(0.05, 6.0, 0.3).expected(1e-10) > 64 && ChebEllipse(0.05, 6.0, 0.3).expected(1e-10) > 400);
  // the default shape and hand-over rate, by preconditioner (hybrid or not), degree and tail
  Options o;
  CHECK(cheb_ellipse_frac(o, true, 1) == 0.5 && cheb_ellipse_frac(o, true, 2) == 0.3 && cheb_ellipse_frac(o, true, 4) == 0.3 && cheb_ellipse_frac(o, false, 2) == 0.0);
  CHECK(cheb_handover_rate(o, true, 1) == 0.0 && cheb_handover_rate(o, true, 2) == 0.3 && cheb_handover_rate(o, true, 3) == 0.4 &&
        cheb_handover_rate(o, true, 4) == 0.4 && cheb_handover_rate(o, false, 2) == 0.0);
  o.tail_gmres = true;
  CHECK(cheb_handover_rate(o, true, 2) == 0.6 && cheb_handover_rate(o, true, 3) == 0.4);
  o.cheb_ell = 0.0; o.cheb_handover = 0.0;
  CHECK(cheb_ellipse_frac(o, true, 2) == 0.0 && cheb_handover_rate(o, true, 3) == 0.0);
  o.cheb_ell = 0.7; o.cheb_handover = 0.45;
  CHECK(cheb_ellipse_frac(o, false, 1) == 0.7 && cheb_handover_rate(o, false, 1) == 0.45);
}

static void sstep_lengths() {
  CHECK(Options{}.sstep_per_decade == 1.7 && Options{}.sstep_max == 6);
  CHECK(sstep_first_length(-1.0, 1e-10, 1.7, 6) == 6 && sstep_first_length(0.0, 1e-10, 1.7, 6) == 6);  // not known: min(6, smax)
  CHECK(sstep_first_length(-1.0, 1e-10, 1.7, 4) == 4 && sstep_first_length(-1.0, -1e-10, 1.7, 8) == 6);
  // three decades: ceil(1.7 * 3) + 1 = 7, cut to smax
  CHECK(sstep_first_length(1000.0, 1.0, 1.7, 8) == 7 && sstep_first_length(1000.0, 1.0, 1.7, 6) == 6);
  CHECK(sstep_first_length(10.0, 1.0, 1.7, 8) == 3);  // ceil(1.7) + 1
  // never below 2: nothing left to reduce gives 0 + 1
  CHECK(sstep_first_length(1.0, 1.0, 1.7, 6) == 2 && sstep_first_length(0.5, 1.0, 1.7, 6) == 2 && sstep_first_length(1.0, 1.0, 1.7, 2) == 2);
  // the step is taken: predicted residual inside the margin 0.7 * target, rank deficient, or no room
  CHECK(sstep_extend(0.7, 1.0, 3, 3, 6, 1.7) == 3 && sstep_extend(0.5, 1.0, 3, 3, 6, 1.7) == 3);
  CHECK(sstep_extend(5.0, 1.0, 3, 2, 6, 1.7) == 3 && sstep_extend(5.0, 1.0, 6, 6, 6, 1.7) == 6);
  // otherwise longer by the iterations for rho / 0.7 -> target, at least one: 0.8 / 0.7 = 1.14: ceil(1.7 * 0.058) = 1;
  // 70 / 0.7 = 100: ceil(3.4) = 4, cut to smax
  CHECK(sstep_extend(0.8, 1.0, 3, 3, 6, 1.7) == 4 && sstep_extend(0.71, 1.0, 2, 2, 6, 1.7) == 3);
  CHECK(sstep_extend(70.0, 1.0, 3, 3, 8, 1.7) == 7 && sstep_extend(70.0, 1.0, 3, 3, 6, 1.7) == 6);
}

static void checkpoint_columns() {
  std::vector<ChebStage> st(3);
  st[0].count = 7;
  st[1].lmin = 0.99; st[1].lmax = 4.16; st[1].count = 130; st[1].widen = 1.25; st[1].last = 22; st[1].slow = 1; st[1].hand = 12;
  st[2].lmin = 0.9; st[2].lmax = 5.5; st[2].count = 129; st[2].last = 17; st[2].hand = 8;
  ckpt::ByteWriter got, want;
  write_cheb_stages(got, st);
  // the format: lmin, lmax, widen (double), count (long), last, hand (int), slow (char), each a length and the values
  want.vec(std::vector<double>{-1.0, 0.99, 0.9});
  want.vec(std::vector<double>{-1.0, 4.16, 5.5});
  want.vec(std::vector<double>{1.0, 1.25, 1.0});
  want.vec(std::vector<long>{7, 130, 129});
  want.vec(std::vector<int>{0, 22, 17});
  want.vec(std::vector<int>{0, 12, 8});
  want.vec(std::vector<char>{0, 1, 0});
  CHECK(got.b == want.b && got.b.size() == 7 * 8 + 3 * (3 * 8 + 8 + 2 * 4 + 1));
  {
    ckpt::ByteReader r(got.b.data(), got.b.size());
    std::vector<ChebStage> back;
    CHECK(read_cheb_stages(r, 3, back).empty() && r.done() && back.size() == 3);
    for (size_t i = 0; i < back.size() && i < 3; i++)
      CHECK(back[i].lmin == st[i].lmin && back[i].lmax == st[i].lmax && back[i].count == st[i].count && back[i].widen == st[i].widen &&
            back[i].last == st[i].last && back[i].slow == st[i].slow && back[i].hand == st[i].hand);
    ckpt::ByteReader r4(got.b.data(), got.b.size());
    CHECK(read_cheb_stages(r4, 4, back) == "section 'solver': Chebyshev bounds of another stage count" && back.empty());
  }
  // no history: seven empty columns (56 bytes), read back as no records
  CHECK(cheb_history_empty(std::vector<ChebStage>(4)) && !cheb_history_empty(st) && cheb_history_empty({}));
  ckpt::ByteWriter e;
  write_cheb_stages(e, {});
  CHECK(e.b == std::vector<unsigned char>(56, 0));
  ckpt::ByteReader re(e.b.data(), e.b.size());
  std::vector<ChebStage> back(2);
  CHECK(read_cheb_stages(re, 3, back).empty() && re.done() && back.empty());
  // a history column of another length than the bounds
  ckpt::ByteWriter bad;
  bad.vec(std::vector<double>{}); bad.vec(std::vector<double>{}); bad.vec(std::vector<double>{1.0, 1.0});
  bad.vec(std::vector<long>{}); bad.vec(std::vector<int>{}); bad.vec(std::vector<int>{}); bad.vec(std::vector<char>{});
  ckpt::ByteReader rb(bad.b.data(), bad.b.size());
  CHECK(read_cheb_stages(rb, 3, back) == "section 'solver': Chebyshev history of another stage count");
}

int main() {
  givens();
  schedule();
  verdicts();
  interval();
  ellipse();
  sstep_lengths();
  checkpoint_columns();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
