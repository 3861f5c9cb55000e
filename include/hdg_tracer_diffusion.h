/* Molecular diffusivity of the passive tracers of libhdg_mi355x.so.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, include/hdg_checkpoint.h and
 * include/hdg_transfer.h, and a binding resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py:
 * TRACER_DIFFUSION_SIGNATURES): the table of hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on
 * success or a negative HDG_ERR_* code, the message through hdg_last_error.
 *
 * Tracer t has a diffusivity kappa_t >= 0 (default 0).  Wherever the engine forms a tracer tendency M^-1 T(q, P(Q)) -- the
 * stages of hdg_tracer_begin_step / hdg_tracer_stage, the fused steps, the forward-Euler update of the two implicit steppers --
 * it forms M^-1 T(q, P(Q)) + kappa_t M^-1 D q instead, D the symmetric interior-penalty form on DG_k with no-flux walls:
 *   D(chi, q) = - sum_K int_K grad chi . grad q + sum_{interior e} int_e ( [chi]{grad q . n} + [q]{grad chi . n} - eta_e [chi][q] )
 *   [v] = v+ - v-, {g} = (g+ + g-)/2, n out of the '+' cell, eta_e = (k+1)(k+2)/4 max(P_K+/|K+|, P_K-/|K-|)  (P = perimeter)
 * The term is explicit: kappa_max dt rho(M^-1 D) has to lie inside the real-axis stability interval of the explicit tableau.
 * The diffusivities are configuration, like dt: they enter the fingerprint of a checkpoint when some kappa_t != 0 (a restart
 * into an engine with other values is refused), hdg_transfer_state does not carry them, and hdg_set_tracer(NULL) leaves them.
 */
#ifndef HDG_TRACER_DIFFUSION_H
#define HDG_TRACER_DIFFUSION_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kappa[n], n = the engine's tracer count; NULL or all zeros switches the term off (the engine then issues no launch more and
 * computes bit for bit what it did without).  HDG_ERR_ARG: another n, a value that is negative or not finite (the message names
 * its index), a call between hdg_begin_step and the end of the step; on a strip partition the error of hdg_set_tracer */
int hdg_set_tracer_diffusivity(hdg_handle* h, int n, const double* kappa);
/* out2[0] = Lambda, a host-side upper bound of the spectral radius of M^-1 D (the infinity norm of the operator in the
 * orthonormal basis, in which it is symmetric); out2[1] = the diffusion number kappa_max dt Lambda */
int hdg_get_tracer_diffusion_number(hdg_handle* h, double out2[2]);
/* test hook: out = M^-1 D q for one nodal DG_k field (layout of hdg_set_tracer with one tracer), without kappa */
int hdg_apply_tracer_diffusion(hdg_handle* h, const double* q, double* out);

#ifdef __cplusplus
}
#endif

#endif /* HDG_TRACER_DIFFUSION_H */
