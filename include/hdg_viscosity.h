/* Viscous term of libhdg_mi355x.so: explicit interior-penalty Navier-Stokes.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, include/hdg_checkpoint.h,
 * include/hdg_transfer.h, include/hdg_tracer_diffusion.h and include/hdg_buoyancy.h, and a binding resolves them from a table
 * of its own (incompressibleeulerhdg_amd/_lib.py: VISCOSITY_SIGNATURES): the table of hdg_mi355x.h is pinned by the tests and
 * stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the message through hdg_last_error.
 *
 *   du/dt + (u . grad) u + grad p = f(t) + sum_t beta_t q_t g + nu Laplace u
 *
 * nu V(w, u) is added to the momentum equation, V the symmetric interior-penalty form on [DG_p]^2, p = k + 1:
 *   V(w, u) = - sum_K int_K grad w : grad u
 *             + sum_{interior e} int_e ( [w].{dn u} + [u].{dn w} - eta_e [w].[u] )
 *             + sum_{wall e}     int_e ( (w.n)(n.dn u) + (u.n)(n.dn w) - eta_b (w.n)(u.n) )     normal component: always
 *             + sum_{wall e}     int_e ( (w.t)(t.dn u) + (u.t)(t.dn w) - eta_b (w.t)(u.t) )     tangential: no slip only
 *   [v] = v+ - v-, {g} = (g+ + g-)/2, dn u = (grad u) n, n out of the '+' cell (out of the domain on a wall), t normal to n
 *   eta_e = (p+1)(p+2)/4 max(P_K+/|K+|, P_K-/|K-|),  eta_b = (p+1)(p+2)/2 P_K/|K|            (P = perimeter)
 * Wall data is homogeneous unless include/hdg_moving_walls.h gives the no-slip walls a speed.  The term is explicit, like the forcing: wherever the scheme uses the forcing slot b_rhs[j] it uses
 * b_rhs[j] + B(q^(j)) + nu M^-1 V Q^(j), Q^(j) the stage velocity of slot j (slot 0: Q_n; slot s, the pressure reconstruction:
 * Q_{n+1}); the two implicit steppers take Q_n (forward Euler).  So nu dt rho(M^-1 V) has to lie inside the real-axis stability
 * interval of the explicit tableau.  The slots are filled inside the solves that read them: no new call in a time loop.
 * nu and the wall mode are configuration, like dt: they enter the fingerprint of a checkpoint when nu != 0 (a restart into an
 * engine with other values, or none, is refused) and hdg_transfer_state does not carry them.
 */
#ifndef HDG_VISCOSITY_H
#define HDG_VISCOSITY_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDG_WALL_FREE_SLIP 0
#define HDG_WALL_NO_SLIP 1

/* nu >= 0 and finite; nu = 0 switches the term off (the engine then issues no launch more and computes bit for bit what it did
 * without).  wall: HDG_WALL_FREE_SLIP or HDG_WALL_NO_SLIP.  HDG_ERR_ARG: a negative or non-finite nu, an unknown wall, a call
 * between hdg_begin_step and the end of the step.  A refused call changes nothing. */
int hdg_set_viscosity(hdg_handle* h, double nu, int wall);
/* nu and wall as they are set; out2 (may be NULL): out2[0] = Lambda_u, a host-side upper bound of the spectral radius of
 * M^-1 V in that wall mode (the infinity norm of the operator in the orthonormal basis, in which it is symmetric),
 * out2[1] = the viscous diffusion number nu dt Lambda_u */
int hdg_get_viscosity(hdg_handle* h, double* nu, int* wall, double out2[2]);
/* test hook: out = M^-1 V Q for a nodal velocity-space field (N_c n_u, 2), the layout hdg_get_field uses for Q, in the given
 * wall mode and without nu.  Refused inside an open step. */
int hdg_apply_viscosity(hdg_handle* h, int wall, const double* Q, double* out);

#ifdef __cplusplus
}
#endif

#endif /* HDG_VISCOSITY_H */
