/* Implicit tracer diffusion of libhdg_mi355x.so: a backward-Euler solve per step on the device.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, include/hdg_tracer_diffusion.h and
 * include/hdg_tracer_walls.h, and a binding resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py:
 * TRACER_IMPLICIT_SIGNATURES): the table of hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on
 * success or a negative HDG_ERR_* code, the message through hdg_last_error.
 *
 * Mode 0 (explicit, the default) is the engine of hdg_tracer_diffusion.h, bit for bit.  In mode 1 (implicit) a step transports
 * the tracers as if every kappa_t were 0 -- the stage tracers, which the buoyancy reads, carry advection only -- and where the
 * step forms its new tracers q~ (hdg_tracer_finish_step, the fused steps, the end of hdg_implicit_step and
 * hdg_dg_implicit_step) every tracer with kappa_t != 0 is replaced by the solution of
 *   (I - dt kappa_t M^-1 D_w) q = q~ + dt kappa_t M^-1 l_w,
 * D_w and l_w the form and the load of that tracer's walls (hdg_tracer_walls.h), dt the step taken.  This is a Lie splitting:
 * first order in dt, unconditionally stable in the diffusivity.  The system is solved by conjugate gradients on the device from
 * x_0 = q~ until |r| <= rtol |b| per tracer; a tracer with kappa_t = 0 is neither read nor written.
 * Structured meshes (the unit square with its walls, the doubly periodic square) on one rank.
 * The mode is configuration: in implicit mode the fingerprint of a checkpoint holds one line more, so a restart into the other
 * mode is refused; the iteration counts of the last solve are not state (zeros in a restored engine until its next step).
 */
#ifndef HDG_TRACER_IMPLICIT_H
#define HDG_TRACER_IMPLICIT_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mode 0 explicit, 1 implicit; rtol and max_iterations of the solve (1e-10 and 2000 in an engine that was never told).
 * HDG_ERR_ARG: another mode, an rtol that is not finite or not > 0, max_iterations < 1, a call between hdg_begin_step and the end
 * of the step.  HDG_ERR_UNSUPPORTED: a general mesh, a strip partition (either mode; the explicit term keeps working there).
 * A refused call changes nothing.  A solve that does not reach rtol within max_iterations leaves that tracer at q~, completes the
 * step and returns HDG_ERR_NOT_CONVERGED from the call that ended the step. */
int hdg_set_tracer_diffusion_mode(hdg_handle* h, int mode, double rtol, int max_iterations);
/* its[n], res[n]: iterations and final relative residual |r| / |b| per tracer of the last solve (0 for a tracer with kappa_t = 0,
 * and before any solve) */
int hdg_get_tracer_diffusion_solve(hdg_handle* h, int n, int* its, double* res);
/* test hook: q_out[t] = the solution of (I - tau[t] M^-1 D_w) x = q_in[t] + tau[t] M^-1 l_w for n <= n_tracers nodal DG_k fields
 * (layout of hdg_set_tracer), field t with the walls set for tracer t, to the rtol and max_iterations that are set; its[n] may be
 * NULL.  It sets nothing and leaves the launch census alone.  HDG_ERR_ARG inside an open step or for a tau that is negative or
 * not finite; HDG_ERR_UNSUPPORTED as above; HDG_ERR_NOT_CONVERGED with q_out[t] = q_in[t] for the tracer that failed. */
int hdg_solve_tracer_diffusion(hdg_handle* h, int n, const double* tau, const double* q_in, double* q_out, int* its);

#ifdef __cplusplus
}
#endif

#endif /* HDG_TRACER_IMPLICIT_H */
