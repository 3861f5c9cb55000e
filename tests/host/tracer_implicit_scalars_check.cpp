// csrc/hdg_tracer_implicit_host.hpp on the host (g++, AddressSanitizer and UBSan): the scalar rule of the implicit tracer
// diffusion drives the recurrences of the device (w = A r; p = r + beta p, y = w + beta y, x += alpha p, r -= alpha y) on
// A = I + tau L, L the 1-D Laplacian (2, -1) of n points, next to a textbook CG with the same start and stop; then the edges
// of the rule.  usage: tracer_implicit_scalars_check N TAU RTOL MAXIT -> "its_rule its_plain err_rule err_plain res state"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_tracer_implicit_host.hpp"

using vec = std::vector<double>;

static vec apply(const vec& v, double tau) {
  const size_t n = v.size();
  vec o(n);
  for (size_t i = 0; i < n; i++) o[i] = v[i] + tau * (2.0 * v[i] - (i > 0 ? v[i - 1] : 0.0) - (i + 1 < n ? v[i + 1] : 0.0));
  return o;
}
static double dot(const vec& a, const vec& b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); i++) s += a[i] * b[i];
  return s;
}

static int fail(const char* what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 5) return fail("usage");
  const int n = std::atoi(argv[1]), maxit = std::atoi(argv[4]);
  const double tau = std::atof(argv[2]), rtol = std::atof(argv[3]), rtol2 = rtol * rtol;
  vec b((size_t)n);
  for (int i = 0; i < n; i++) b[(size_t)i] = std::sin(0.7 * i) + 0.3 * ((i * 37) % 11 - 5);
  // the solution, by the Thomas algorithm
  vec exact = b;
  {
    vec c((size_t)n), dgn((size_t)n);
    const double d = 1.0 + 2.0 * tau, o = -tau;
    dgn[0] = d;
    for (int i = 1; i < n; i++) { c[(size_t)i] = o / dgn[(size_t)i - 1]; dgn[(size_t)i] = d - c[(size_t)i] * o; exact[(size_t)i] -= c[(size_t)i] * exact[(size_t)i - 1]; }
    exact[(size_t)n - 1] /= dgn[(size_t)n - 1];
    for (int i = n - 2; i >= 0; i--) exact[(size_t)i] = (exact[(size_t)i] - o * exact[(size_t)i + 1]) / dgn[(size_t)i];
  }
  auto err = [&](const vec& x) { double e = 0.0; for (int i = 0; i < n; i++) e = std::fmax(e, std::fabs(x[(size_t)i] - exact[(size_t)i])); return e; };
  // the device's recurrences under the rule
  double st[hdg::TDI_NSC] = {0};
  vec x = b, r = b, p((size_t)n, std::numeric_limits<double>::quiet_NaN()), y = p;  // p, y: written before they are read
  {
    const vec Ax = apply(x, tau);
    for (int i = 0; i < n; i++) r[(size_t)i] = b[(size_t)i] - Ax[(size_t)i];
  }
  const double bb = dot(b, b);
  double rr = dot(r, r);
  int launched = 0;
  for (int it = 0; it < maxit && st[hdg::TDI_STATE] == hdg::TDI_ITERATING; it++, launched++) {
    const vec w = apply(r, tau);
    hdg::tdi_scalar_rule(st, rr, dot(r, w), bb, it == 0, false, rtol2);
    if (st[hdg::TDI_STATE] != hdg::TDI_ITERATING) break;
    const double alpha = st[hdg::TDI_ALPHA], beta = st[hdg::TDI_BETA];
    for (int i = 0; i < n; i++) {
      const size_t k = (size_t)i;
      p[k] = beta != 0.0 ? beta * p[k] + r[k] : r[k];
      y[k] = beta != 0.0 ? beta * y[k] + w[k] : w[k];
      x[k] += alpha * p[k];
      r[k] -= alpha * y[k];
    }
    rr = dot(r, r);
  }
  if (st[hdg::TDI_STATE] == hdg::TDI_ITERATING) hdg::tdi_scalar_rule(st, rr, 0.0, bb, false, true, rtol2);
  // the textbook iteration
  vec xp = b, rp((size_t)n), pp;
  {
    const vec Ax = apply(xp, tau);
    for (int i = 0; i < n; i++) rp[(size_t)i] = b[(size_t)i] - Ax[(size_t)i];
  }
  pp = rp;
  double rrp = dot(rp, rp);
  int itp = 0;
  while (rrp > rtol2 * bb && itp < maxit) {
    const vec yp = apply(pp, tau);
    const double alpha = rrp / dot(pp, yp);
    for (int i = 0; i < n; i++) { xp[(size_t)i] += alpha * pp[(size_t)i]; rp[(size_t)i] -= alpha * yp[(size_t)i]; }
    const double rn = dot(rp, rp);
    for (int i = 0; i < n; i++) pp[(size_t)i] = rp[(size_t)i] + rn / rrp * pp[(size_t)i];
    rrp = rn;
    itp++;
  }
  std::printf("%d %d %.17g %.17g %.17g %d\n", (int)st[hdg::TDI_ITS], itp, err(x), err(xp), st[hdg::TDI_RES], (int)st[hdg::TDI_STATE]);

  // the edges of the rule
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto fresh = [&](double* s) { for (int i = 0; i < hdg::TDI_NSC; i++) s[i] = 0.0; };
  double s[hdg::TDI_NSC];
  fresh(s); hdg::tdi_scalar_rule(s, 0.0, 0.0, 0.0, true, false, rtol2);  // a zero right-hand side: converged at once, residual 0
  if (s[hdg::TDI_STATE] != hdg::TDI_CONVERGED || s[hdg::TDI_ITS] != 0.0 || s[hdg::TDI_RES] != 0.0) return fail("zero right-hand side");
  fresh(s); hdg::tdi_scalar_rule(s, nan, 1.0, 1.0, true, false, rtol2);
  if (s[hdg::TDI_STATE] != hdg::TDI_BROKE_DOWN) return fail("NaN residual");
  fresh(s); hdg::tdi_scalar_rule(s, 1.0, nan, 1.0, true, false, rtol2);
  if (s[hdg::TDI_STATE] != hdg::TDI_BROKE_DOWN) return fail("NaN curvature");
  fresh(s); hdg::tdi_scalar_rule(s, 1.0, -1.0, 1.0, true, false, rtol2);
  if (s[hdg::TDI_STATE] != hdg::TDI_BROKE_DOWN || s[hdg::TDI_ITS] != 0.0) return fail("negative curvature");
  fresh(s); hdg::tdi_scalar_rule(s, 1.0, 2.0, 4.0, true, false, 1e-2);  // one ordinary step: alpha = rr / rw, beta = 0
  if (s[hdg::TDI_STATE] != hdg::TDI_ITERATING || s[hdg::TDI_ALPHA] != 0.5 || s[hdg::TDI_BETA] != 0.0 || s[hdg::TDI_ITS] != 1.0 ||
      s[hdg::TDI_RR] != 1.0 || s[hdg::TDI_BB] != 4.0 || s[hdg::TDI_RES] != 0.5) return fail("first step");
  hdg::tdi_scalar_rule(s, 0.25, 1.0, nan, false, false, 1e-2);  // beta = 1/4, curvature 1 - (1/4)(1/4)/(1/2) = 7/8; bb is not read
  if (s[hdg::TDI_BETA] != 0.25 || s[hdg::TDI_ALPHA] != 0.25 / 0.875 || s[hdg::TDI_ITS] != 2.0 || s[hdg::TDI_BB] != 4.0) return fail("second step");
  double keep[hdg::TDI_NSC];
  hdg::tdi_scalar_rule(s, 0.04, nan, nan, false, true, 1e-2);  // the last check: rr = rtol^2 bb exactly is converged, rw unread
  if (s[hdg::TDI_STATE] != hdg::TDI_CONVERGED || s[hdg::TDI_ITS] != 2.0) return fail("last check, met");
  for (int i = 0; i < hdg::TDI_NSC; i++) keep[i] = s[i];
  hdg::tdi_scalar_rule(s, 7.0, 7.0, 7.0, true, false, 1e-2);  // a frozen tracer: nothing is written
  for (int i = 0; i < hdg::TDI_NSC; i++) if (s[i] != keep[i]) return fail("frozen tracer");
  fresh(s); hdg::tdi_scalar_rule(s, 1.0, 2.0, 4.0, true, false, 1e-2);
  hdg::tdi_scalar_rule(s, 0.5, nan, nan, false, true, 1e-2);
  if (s[hdg::TDI_STATE] != hdg::TDI_OUT_OF_ITERATIONS || s[hdg::TDI_ITS] != 1.0) return fail("last check, missed");
  fresh(s); s[hdg::TDI_STATE] = hdg::TDI_IDLE; hdg::tdi_scalar_rule(s, 1.0, 1.0, 1.0, true, false, 1e-2);
  if (s[hdg::TDI_STATE] != hdg::TDI_IDLE || s[hdg::TDI_ITS] != 0.0) return fail("idle tracer");
  std::printf("ok\n");
  return 0;
}
