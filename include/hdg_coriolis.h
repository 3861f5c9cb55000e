/* Coriolis term of libhdg_mi355x.so: rotation and a beta-plane.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, include/hdg_checkpoint.h,
 * include/hdg_transfer.h, include/hdg_tracer_diffusion.h, include/hdg_buoyancy.h and include/hdg_viscosity.h, and a binding
 * resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: CORIOLIS_SIGNATURES): the table of hdg_mi355x.h is
 * pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the message through
 * hdg_last_error.
 *
 *   du/dt + (u . grad) u + grad p = f(t) + sum_t beta_t q_t g + nu Laplace u - f_c(y) k x u
 *   f_c(y) = f0 + beta y,    - f_c k x u = ( f_c u_y, - f_c u_x )
 *
 * y is the mesh's own ordinate: 0 .. 1 on the unit square, 0 .. L on the periodic square, the vertex ordinates of a general
 * mesh.  The Galerkin term C(w, u) = sum_K int_K f_c (w_x u_y - w_y u_x) on [DG_{k+1}]^2 is added to the momentum equation.
 * M^-1 C is block diagonal per cell and M-antisymmetric (the term does no work); its spectral radius is at most
 * F = max over the mesh vertices of |f_c|.  The term is explicit, like the forcing and the viscous term: wherever the scheme
 * uses the forcing slot b_rhs[j] it adds M^-1 C Q^(j), Q^(j) the stage velocity of slot j (slot 0: Q_n; slot s, the pressure
 * reconstruction: Q_{n+1}); the two implicit steppers take Q_n (forward Euler).  The eigenvalues are imaginary, so F dt has to
 * be judged against the imaginary-axis stability of the explicit tableau.  The slots are filled inside the solves that read
 * them: no new call in a time loop.  f0 and beta are configuration, like dt: they enter the fingerprint of a checkpoint when
 * one of them is non-zero (a restart into an engine with other values, or none, is refused) and hdg_transfer_state does not
 * carry them.
 */
#ifndef HDG_CORIOLIS_H
#define HDG_CORIOLIS_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* f0 and beta finite, of either sign; f0 = beta = 0 switches the term off (the engine then issues no launch more and computes
 * bit for bit what it did without).  HDG_ERR_ARG: a non-finite value, a call between hdg_begin_step and the end of the step,
 * beta != 0 on the doubly periodic square (f_c would jump at the wrap; f0 alone is fine there).  A refused call changes
 * nothing. */
int hdg_set_coriolis(hdg_handle* h, double f0, double beta);
/* f0 and beta as they are set; out2 (may be NULL): out2[0] = F, the largest |f_c| over the mesh vertices, an upper bound of
 * the spectral radius of M^-1 C; out2[1] = the rotation number F dt */
int hdg_get_coriolis(hdg_handle* h, double* f0, double* beta, double out2[2]);
/* test hook: out = M^-1 C Q for a nodal velocity-space field (N_c n_u, 2), the layout hdg_get_field uses for Q, with the f0
 * and beta given.  It sets nothing.  Refused inside an open step, and for beta != 0 on the doubly periodic square. */
int hdg_apply_coriolis(hdg_handle* h, double f0, double beta, const double* Q, double* out);

#ifdef __cplusplus
}
#endif

#endif /* HDG_CORIOLIS_H */
