/* Moving no-slip walls and the viscous wall force of libhdg_mi355x.so.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h and the headers of the other terms, and a
 * binding resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: MOVING_WALL_SIGNATURES): the table of
 * hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the
 * message through hdg_last_error.
 *
 * The sides of the structured unit square in the order of include/hdg_tracer_walls.h: 0 bottom (y = 0), 1 right, 2 top, 3 left.
 * U_w is the constant Cartesian tangential speed of side w: the wall's u_x on bottom and top, its u_y on left and right.  With
 * no-slip walls the tangential Nitsche term of the viscous form V (include/hdg_viscosity.h) acts on u.t - U_w instead of u.t,
 * so the momentum equation gains nu M^-1 l(U),
 *   l(w; U) = sum_{wall e on side s} U_s int_e ( eta_b (w.t) - t.dn w ) ds,      t = e_x on bottom / top, e_y on left / right
 * in every slot that holds nu M^-1 V Q^(j): no launch more per step.  The normal condition u.n = 0 is untouched.
 *
 * The viscous wall force on the fluid through side w is the form tested against the constants e_c, restricted to w:
 *   F_w . e_c = nu int_w (e_c.n)( n.dn u - eta_b u.n ) ds                     always
 *             + nu int_w (e_c.t)( t.dn u - eta_b (u.t - U_w) ) ds             no slip only
 * so sum_w F_w = int nu M^-1 (V u + l(U)) dx for every broken u.  The pressure force is not part of it.
 *
 * The speeds are configuration, like nu: they enter the fingerprint of a checkpoint, one line per side with U_w != 0 (a restart
 * into an engine with other speeds, or none, is refused), and hdg_transfer_state does not carry them.  On a strip partition every
 * rank must be given the same speeds; this is required and not checked.
 */
#ifndef HDG_MOVING_WALLS_H
#define HDG_MOVING_WALLS_H

#include "hdg_viscosity.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The four speeds; NULL or all zeros switches the feature off (the engine then computes bit for bit what it did without).  They
 * may be changed between steps.  nu = 0 with speeds set is allowed and has no effect.
 * HDG_ERR_ARG: a speed that is not finite (the message names the side); a non-zero speed on the doubly periodic square; a
 * non-zero speed while the wall mode (hdg_set_viscosity) is not HDG_WALL_NO_SLIP; a call between hdg_begin_step and the end of
 * the step.  HDG_ERR_UNSUPPORTED: a non-zero speed on a general mesh.  A refused call changes nothing.  While a speed is
 * non-zero, hdg_set_viscosity(..., HDG_WALL_FREE_SLIP) is HDG_ERR_ARG. */
int hdg_set_wall_velocity(hdg_handle* h, const double U[4]);
/* the speeds as they are set */
int hdg_get_wall_velocity(hdg_handle* h, double U[4]);
/* F[2 w + c]: component c of the viscous force through side w, of the current velocity with the nu, the wall mode and the
 * speeds that are set; free slip gives the normal part only.  All zero on the periodic square.  On a strip partition it is a
 * collective call and every rank returns the same values.  HDG_ERR_UNSUPPORTED on a general mesh; refused inside an open step. */
int hdg_get_wall_force(hdg_handle* h, double F[8]);
/* test hook: out = M^-1 (V Q + l(U)) for a nodal velocity-space field, the layout of hdg_apply_viscosity, in the given wall mode
 * and without nu; it sets nothing.  With all U zero (or NULL) it is hdg_apply_viscosity bit for bit.  The errors of
 * hdg_set_wall_velocity, with `wall` in the place of the wall mode that is set. */
int hdg_apply_moving_walls(hdg_handle* h, int wall, const double U[4], const double* Q, double* out);
/* test hook: the force F[8] of a given nodal velocity-space field without nu; it sets nothing */
int hdg_apply_wall_force(hdg_handle* h, int wall, const double U[4], const double* Q, double F[8]);

#ifdef __cplusplus
}
#endif

#endif /* HDG_MOVING_WALLS_H */
