/* Adaptive time step of libhdg_mi355x.so: change dt between steps, and hold a target CFL number.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h and the headers of the terms, and a binding
 * resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: ADAPTIVE_DT_SIGNATURES): the table of
 * hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the
 * message through hdg_last_error.
 *
 * dt enters no operator table of the engine: it is read as gamma = a_ii dt where a stage is solved and in the stage
 * coefficients, both formed from the configuration at every use, and the block-Jacobi tables of the tentative-velocity solve
 * are keyed by gamma and follow on their own.  So a new dt costs what the first step of a run costs and no more: the spectral
 * bounds of the Chebyshev iteration are estimated again.
 *
 * The controller is a rule on four rates whose product with dt has to stay bounded,
 *   rates[0]  A = max_K (max nodal |u| in K) / h_K of the current velocity: the CFL number of the diagnostics row without
 *             its factor dt (the same nodes, the same h_K = shortest edge of K)
 *   rates[1]  kappa_max Lambda   of the tracer diffusion          (0 while it is off)
 *   rates[2]  nu Lambda_u        of the viscous term              (0 while it is off); while the linear drag of
 *             include/hdg_drag.h is on, nu Lambda_u + S: the real-axis rate of the whole velocity-linear part (both
 *             spectra are real and non-positive, so the rates add); with the drag off it is what it was
 *   rates[3]  F = max |f_c|      of the Coriolis term             (0 while it is off)
 * rates[1..3] are the numbers the three stability reports divide by: report = rate * dt.
 *
 * The rule (csrc/hdg_step_control.hpp, one IEEE operation per line, in this order), with the dt that is held:
 *   p = min(dt_max, caps[0], caps[1], caps[2], cfl / A)       cfl / A = +inf when A == 0
 *   p = min(p, grow * dt)
 *   if dt <= p <= (1 + band) * dt:  p = dt                    no new solver bounds for a small gain
 *   if p >= t_final - t:            p = t_final - t           land on t_final
 *   else if p < dt_min:             error
 * The caller stops when t_final - t <= 1e-12 * t_final.  The defaults are policy, not measurements.
 */
#ifndef HDG_ADAPTIVE_DT_H
#define HDG_ADAPTIVE_DT_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A zeroed field means its default. */
typedef struct hdg_step_control {
  double cfl;     /* target of A * dt; must be > 0 */
  double dt_min;  /* a proposal below it is an error; default 0 */
  double dt_max;  /* default +inf */
  double grow;    /* largest factor between two step sizes; default 1.25 */
  double band;    /* a gain of at most this fraction keeps dt; default 0.1 */
  double caps[3]; /* upper limits from the explicit terms (tracer diffusion, viscosity, rotation); default +inf */
} hdg_step_control;

/* Change the step size between completed steps; every mesh kind and every stepper family.  dt must be finite and > 0, and no
 * step may be open: otherwise HDG_ERR_ARG, and the engine is untouched.  The per-stage history of the Chebyshev iteration is
 * cleared (the next tentative-velocity solve estimates its bounds as the first solve of a run does), the predictor of the
 * particles is formed again from the k1 in place, and the three stability reports use the new value from then on.  A call
 * with the value already held does nothing at all: the steps after it are bit for bit those of a run without the call.
 * Steppers that key a preconditioner by tau / dt (the monolithic and the DG step) build one set per distinct dt and keep
 * it.  On a strip partition every rank calls it with the same value; nothing is communicated. */
int hdg_set_dt(hdg_handle* h, double dt);
/* the step size the engine holds */
int hdg_get_dt(const hdg_handle* h, double* dt);
/* The four rates of the current state.  rates[0] costs one pass over the velocity (two kernel launches) and an 8-byte read; it is not
 * finite when the velocity is not finite anywhere.  On a strip partition the call is collective and every rank gets the
 * global maximum.  Refused inside an open step. */
int hdg_get_step_rates(hdg_handle* h, double rates[4]);
/* The rule alone for a given rate A and held step size dt: no engine, nothing is launched.  0 and *dt_new on success;
 * HDG_ERR_NOT_CONVERGED when A is not finite (or negative); HDG_ERR_ARG when the proposal falls below dt_min (*dt_new then holds
 * the value that fell below it) or the control is bad (*dt_new is NaN).  A time loop that keeps the rate it measured calls
 * hdg_get_step_rates and this; hdg_propose_dt is the two in one call. */
int hdg_step_proposal(const hdg_step_control* control, double A, double dt, double t, double t_final, double* dt_new);
/* The rule above applied to hdg_get_step_rates and the dt that is held; it sets nothing.  HDG_ERR_NOT_CONVERGED when rates[0]
 * is not finite ("velocity is not finite"); HDG_ERR_ARG when the proposal falls below dt_min (the message names both), when
 * cfl is not > 0, or when a field of the struct is negative or NaN. */
int hdg_propose_dt(hdg_handle* h, const hdg_step_control* control, double t, double t_final, double* dt_new);

#ifdef __cplusplus
}
#endif

#endif /* HDG_ADAPTIVE_DT_H */
