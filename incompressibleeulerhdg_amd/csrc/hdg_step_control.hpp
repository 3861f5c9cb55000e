// Step-size rule of the adaptive time step (include/hdg_adaptive_dt.h): the one place the policy lives.
// Plain C++.  Every statement below is one IEEE operation (a comparison, a selection, or one of * / + -), in a fixed order, so
// that a twin written in another language reproduces every proposal bit for bit from the same inputs.
#pragma once
#include <cmath>
#include <limits>

#include "../../include/hdg_adaptive_dt.h"

namespace hdg {

enum class StepVerdict { Ok, BelowMin, NotFinite, BadControl };

// the struct with every zeroed field replaced by its default (policy defaults, not measurements)
inline hdg_step_control step_control_defaults(const hdg_step_control& c) {
  const double inf = std::numeric_limits<double>::infinity();
  hdg_step_control d = c;
  if (d.dt_max == 0.0) d.dt_max = inf;
  if (d.grow == 0.0) d.grow = 1.25;
  if (d.band == 0.0) d.band = 0.1;
  for (double& cap : d.caps)
    if (cap == 0.0) cap = inf;
  return d;
}
// cfl > 0, and nothing negative or NaN
inline bool step_control_valid(const hdg_step_control& c) {
  bool ok = c.cfl > 0.0 && c.dt_min >= 0.0 && c.dt_max >= 0.0 && c.grow >= 0.0 && c.band >= 0.0;
  for (double cap : c.caps) ok = ok && cap >= 0.0;
  return ok;
}
// a < b ? a : b: a NaN in `a` is never taken (the fields are validated, and A is tested before it is used)
inline double step_min(double a, double b) { return a < b ? a : b; }

// The proposal for the step from t with the rate A = max |u| / h and the step size dt that is held.  p is written for every
// verdict but NotFinite / BadControl (BelowMin: the value that fell below dt_min).
inline StepVerdict step_proposal(const hdg_step_control& control, double A, double dt, double t, double t_final, double& p) {
  const double inf = std::numeric_limits<double>::infinity();
  p = std::numeric_limits<double>::quiet_NaN();
  if (!step_control_valid(control)) return StepVerdict::BadControl;
  if (!(A >= 0.0) || A == inf) return StepVerdict::NotFinite;
  const hdg_step_control c = step_control_defaults(control);
  const double q = A == 0.0 ? inf : c.cfl / A;
  p = c.dt_max;
  p = step_min(c.caps[0], p);
  p = step_min(c.caps[1], p);
  p = step_min(c.caps[2], p);
  p = step_min(q, p);
  const double g = c.grow * dt;
  p = step_min(g, p);
  const double b1 = 1.0 + c.band;
  const double hi = b1 * dt;
  if (dt <= p && p <= hi) p = dt;
  const double rem = t_final - t;
  if (p >= rem) p = rem;
  else if (p < c.dt_min) return StepVerdict::BelowMin;
  return StepVerdict::Ok;
}

}  // namespace hdg
