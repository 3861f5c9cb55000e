/* Boussinesq buoyancy of libhdg_mi355x.so: the tracers force the flow.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, include/hdg_checkpoint.h,
 * include/hdg_transfer.h and include/hdg_tracer_diffusion.h, and a binding resolves them from a table of its own
 * (incompressibleeulerhdg_amd/_lib.py: BUOYANCY_SIGNATURES): the table of hdg_mi355x.h is pinned by the tests and stays what it
 * is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the message through hdg_last_error.
 *
 *   du/dt + (u . grad) u + grad p = f(t) + sum_t beta_t q_t g          g = (g_x, g_y) constant, beta_t real
 *
 * beta_t = 0 keeps tracer t passive; the default, all zero, is off.  There is no reference value: between walls a shift
 * q -> q + c only changes the pressure; on the doubly periodic square it adds the uniform acceleration beta c g, so runs there
 * should start from sum_t beta_t mean(q_t) = 0.  The term is explicit, like the forcing: wherever the scheme uses the forcing
 * slot b_rhs[j] it uses b_rhs[j] + B(q^(j)), B(q) = sum_t beta_t q_t g in the velocity space, q^(j) the stage tracer of slot j
 * (slot s, the pressure reconstruction: the tracer at the end of the step); the two implicit steppers take the tracer at the
 * start of the step.  The slots are filled inside hdg_tracer_begin_step / hdg_tracer_stage and the fused steps: no new call
 * in a time loop.  The user's forcing (hdg_set_forcing_*) keeps its meaning exactly.
 * beta and g are configuration, like dt and the diffusivities: they enter the fingerprint of a checkpoint when some beta_t != 0
 * (a restart into an engine with other values, or none, is refused), hdg_transfer_state does not carry them, and
 * hdg_set_tracer(NULL) leaves them (without a tracer nothing forces the flow).
 */
#ifndef HDG_BUOYANCY_H
#define HDG_BUOYANCY_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* beta[n], n = the engine's tracer count, and g[2] (NULL: (0, -1)); beta == NULL or all zeros switches the term off (the engine
 * then issues no launch more and computes bit for bit what it did without).  HDG_ERR_ARG: no tracer is set (hdg_set_tracer),
 * another n, a beta_t or a component of g that is not finite (the message names its index), a call between hdg_begin_step and
 * the end of the step; on a strip partition the error of hdg_set_tracer.  A refused call changes nothing. */
int hdg_set_buoyancy(hdg_handle* h, int n, const double* beta, const double g[2]);
/* beta[n] (n = the engine's tracer count; all zero while the term is off) and g[2] as they are set */
int hdg_get_buoyancy(hdg_handle* h, int n, double* beta, double g[2]);
/* test hook: f = B(q) with the beta, g currently set.  q: nodal tracer fields (n_tracers, N_c n_p), the layout of
 * hdg_set_tracer; f: the nodal velocity-space field (N_c n_u, 2), the layout hdg_get_field uses for Q.  A tracer with
 * beta_t = 0 is not read on the device. */
int hdg_apply_buoyancy(hdg_handle* h, const double* q, double* f);

#ifdef __cplusplus
}
#endif

#endif /* HDG_BUOYANCY_H */
