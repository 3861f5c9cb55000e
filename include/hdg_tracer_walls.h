/* Wall conditions of the tracers of libhdg_mi355x.so: fixed-value walls and the wall flux.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h and include/hdg_tracer_diffusion.h, and a
 * binding resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: TRACER_WALL_SIGNATURES): the table of
 * hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the
 * message through hdg_last_error.
 *
 * Per wall side w, tracer t is either no-flux (kind 0, the default: the form D of hdg_tracer_diffusion.h) or held at a fixed
 * value g_{t,w} (kind 1), one finite real, constant along the side and in time.  On a fixed-value wall edge e of cell K, n out
 * of the domain, the diffusion form gains the Nitsche terms
 *   D_w(chi, q) = int_e ( chi dn q + q dn chi - eta_b chi q ),   l_w(chi; g) = g int_e ( eta_b chi - dn chi ),
 *   eta_b = (k+1)(k+2)/2 P_K / |K|,
 *   tendency_t = M^-1 T(q_t, P(Q)) + kappa_t M^-1 ( D q_t + sum_w D_w q_t + sum_w l_w(.; g_{t,w}) ).
 * The transport flux at a wall stays zero.  A fixed value with kappa_t = 0 has no effect; that is allowed.
 * Sides: the structured unit square has four, in the order bottom (y = 0), right (x = 1), top (y = 1), left (x = 0); the doubly
 * periodic square has none; a general mesh has one, the whole boundary, at index 0.
 * The wall flux of tracer t through side w, positive into the domain, is the form tested against chi = 1:
 *   Phi_{t,w} = kappa_t int_w ( dn q_t - eta_b (q_t - g_{t,w}) ) ds     (0 on a no-flux side),
 * so that d/dt int q_t = sum_w Phi_{t,w} for the discrete operator at zero velocity.
 * The walls are configuration, like kappa: one line per fixed (tracer, side) enters the fingerprint of a checkpoint, and only
 * then; hdg_transfer_state does not carry them; hdg_set_tracer(NULL) and hdg_set_tracer_diffusivity leave them.
 */
#ifndef HDG_TRACER_WALLS_H
#define HDG_TRACER_WALLS_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind[n * 4], value[n * 4], n = the engine's tracer count, entry t * 4 + w; NULL kinds or all zeros switches the feature off
 * (the engine then issues the launches and computes the bits it did without).  HDG_ERR_ARG: another n, a kind other than 0
 * or 1, a value that is not finite on a fixed side (the message names tracer and side), a fixed side on the periodic square or
 * at index 1 .. 3 of a general mesh, a call between hdg_begin_step and the end of the step; on a strip partition the error of
 * hdg_set_tracer.  A refused call changes nothing.  With walls set, hdg_get_tracer_diffusion_number reports the bound Lambda
 * that includes the wall blocks. */
int hdg_set_tracer_walls(hdg_handle* h, int n, const int* kind, const double* value);
/* flux[n * 4]: Phi_{t,w} of the engine's current tracers with the kappa and walls that are set.  HDG_ERR_ARG without a tracer
 * (hdg_set_tracer), for another n, inside an open step.  Two calls on the same state return the same bits. */
int hdg_get_tracer_wall_flux(hdg_handle* h, int n, double* flux);
/* test hook: out = M^-1 (D + sum_w D_w) q + M^-1 sum_w l_w for one nodal DG_k field (layout of hdg_set_tracer with one tracer),
 * without kappa; it sets nothing.  With all kinds 0 it equals hdg_apply_tracer_diffusion bit for bit. */
int hdg_apply_tracer_wall_diffusion(hdg_handle* h, const int kind[4], const double value[4], const double* q, double* out);

#ifdef __cplusplus
}
#endif

#endif /* HDG_TRACER_WALLS_H */
