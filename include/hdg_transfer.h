/* Transfer of a state between two engines of libhdg_mi355x.so on nested meshes, of any two degrees.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h and include/hdg_checkpoint.h, and a binding
 * resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: TRANSFER_SIGNATURES): the table of hdg_mi355x.h
 * is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the message
 * through hdg_last_error of the FIRST handle of the call.
 *
 * A state is the current velocity (broken [P_{k+1}]^2), the pressure (P_k) and, when switched on, the n_tracers tracers (P_k).
 * The pair: both engines from hdg_create (one rank each) on the same device, the same mesh kind (unit square or doubly
 * periodic square) and the same length, ny = nx, and nested meshes: nx of the one is r times nx of the other, 1 <= r <= 16.
 * Degrees 1 .. 4, any pair.  The transferred field is the L2 projection of the source's piecewise polynomial onto the
 * destination's space, component by component: exact injection when the destination space contains the source (finer or equal
 * mesh and degree at least the source's), otherwise the orthogonal projection, which preserves cell means and hence the
 * integrals of the pressure, of every tracer and of each velocity component.
 *
 * Refusals: HDG_ERR_ARG, with a message naming the cause, for dst == src, a different mesh kind, a different length, a different
 * device, meshes that are not nested or r > 16, a tracer mismatch, and either engine between hdg_begin_step and the end of its
 * step; HDG_ERR_UNSUPPORTED for general meshes and engines with more than one rank.  A refused call leaves both engines as they
 * were.
 */
#ifndef HDG_TRANSFER_H
#define HDG_TRANSFER_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dst takes the state of src: afterwards dst is in the state hdg_set_state would have left it in, had it been given the
 * transferred fields (pressure mean removed, particle predictor refreshed, warm starts untouched), and with with_tracers != 0
 * also in the state hdg_set_tracer would have left (tracer switched on); that needs a source whose tracer is on and the same
 * n_tracers on both */
int hdg_transfer_state(hdg_handle* dst, const hdg_handle* src, int with_tracers);
/* L2 norms of the differences of the current states of a and b, exact on the common refinement: velocity, pressure and
 * (norm_q[n_tracers], or NULL) every tracer; any of the three may be NULL.  a == b is allowed and gives exactly 0 */
int hdg_transfer_difference(hdg_handle* a, hdg_handle* b, double* norm_Q, double* norm_p, double* norm_q);

#ifdef __cplusplus
}
#endif

#endif /* HDG_TRANSFER_H */
