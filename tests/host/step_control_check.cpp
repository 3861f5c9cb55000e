// csrc/hdg_step_control.hpp on the host (g++, AddressSanitizer and UBSan): the proposals of a table of cases, printed as
// hexadecimal floats, which tests/test_adaptive_dt_cpu.py compares bit for bit with the numpy twin of
// tests/adaptive_dt_reference.py.  One line per case: the inputs, the verdict and the proposal.
//   cfl dt_min dt_max grow band cap0 cap1 cap2 A dt t t_final -> verdict p
#include <cstdio>
#include <limits>
#include <vector>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_step_control.hpp"

struct Case {
  hdg_step_control c;
  double A, dt, t, t_final;
};

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double dt = 0.01, b1 = 1.0 + 0.1;
  std::vector<Case> cases;
  auto add = [&](double cfl, double dmin, double dmax, double grow, double band, double c0, double c1, double c2, double A, double dt_,
                 double t, double tf) { cases.push_back(Case{hdg_step_control{cfl, dmin, dmax, grow, band, {c0, c1, c2}}, A, dt_, t, tf}); };
  // A = 0, tiny, inf, NaN; a negative rate
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 0.0, dt, 0.0, 1.0);
  add(0.3, 0, 0.02, 0, 0, 0, 0, 0, 0.0, 0.019, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 1e-300, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 4.9e-324, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, inf, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, nan, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, -1.0, dt, 0.0, 1.0);
  // the rate decides: shrink, and grow outside the band
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 70.0, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 25.0, dt, 0.0, 1.0);
  // the growth limit active, default and given
  add(0.3, 0, 0, 0, 0, 0, 0, 0, 3.0, dt, 0.0, 1.0);
  add(0.3, 0, 0, 2.0, 0, 0, 0, 0, 3.0, dt, 0.0, 1.0);
  // both edges of the band: p == dt, just below dt, p == (1 + band) dt, the next double above it
  add(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, std::nextafter(dt, 0.0), 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, b1 * dt, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, std::nextafter(b1 * dt, 1.0), 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 0.0105, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 0.0105, 0, 0.01, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  // every cap active in turn, and dt_max
  add(0.3, 0, 1.0, 0, 0, 0.004, 0.005, 0.006, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 1.0, 0, 0, 0.005, 0.004, 0.006, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 1.0, 0, 0, 0.006, 0.005, 0.004, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 0.003, 0, 0, 0.006, 0.005, 0.004, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 1.0, 0, 0, inf, 0.0121, inf, 1.0, dt, 0.0, 1.0);
  // dt_min violated, met exactly, and not tested on the landing branch
  add(0.3, 0.005, 0, 0, 0, 0, 0, 0, 100.0, dt, 0.0, 1.0);
  add(0.3, 0.003, 0, 0, 0, 0, 0, 0, 100.0, dt, 0.0, 1.0);
  add(0.3, 0.005, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.999, 1.0);
  // the landing branch: the rest shorter than, equal to and longer than the proposal
  add(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.995, 1.0);
  add(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.75, 0.76);
  add(0.3, 0, 0.25, 0, 0, 0, 0, 0, 0.0, 0.25, 0.75, 1.0);
  add(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.5, 1.0);
  add(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 1.0, 1.0);
  // bad controls
  add(0.0, 0, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(-0.3, 0, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(nan, 0, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, -1.0, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.0, 1.0);
  add(0.3, 0, 0, 0, 0, nan, 0, 0, 1.0, dt, 0.0, 1.0);
  static const char* names[] = {"ok", "below_min", "not_finite", "bad_control"};
  for (const Case& k : cases) {
    double p;
    const hdg::StepVerdict v = hdg::step_proposal(k.c, k.A, k.dt, k.t, k.t_final, p);
    printf("%a %a %a %a %a %a %a %a %a %a %a %a -> %s %a\n", k.c.cfl, k.c.dt_min, k.c.dt_max, k.c.grow, k.c.band, k.c.caps[0], k.c.caps[1],
           k.c.caps[2], k.A, k.dt, k.t, k.t_final, names[(int)v], p);
  }
  printf("%zu cases\n", cases.size());
  return 0;
}
