/* Stream function of the velocity of libhdg_mi355x.so.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h and the headers of the other terms, and a
 * binding resolves them from a table of its own (incompressibleeulerhdg_amd/_lib.py: STREAMFUNCTION_SIGNATURES): the table of
 * hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_* code, the
 * message through hdg_last_error.
 *
 * psi lies in the continuous space CG_{k+1} of the vorticity diagnostic and minimises |u - curl psi|_{L2} over the whole
 * space, curl psi = (d_y psi, -d_x psi), with no essential boundary condition:
 *
 *   (grad psi, grad tau) = int (u_x d_y tau - u_y d_x tau) dx   for all tau in CG_{k+1}.
 *
 * The problem is the Neumann one: singular by constants, and its right-hand side sums to zero.  It needs no assumption on
 * u . n, so a moving lid is as good as a wall.  Gauge: on the unit square the arithmetic mean of psi over the 4 nx boundary
 * mesh vertices is zero (psi ~ 0 on impermeable walls); on the doubly periodic square the mean over all mesh vertices is
 * zero, and the mean flow ubar = int u / |Omega|, which a periodic psi cannot carry, is returned beside psi.  The defect
 * |u - ubar - curl psi|_{L2} (ubar subtracted on the periodic square only) measures the part of u that is not solenoidal.
 * Solver: conjugate gradients on the stiffness matrix, preconditioned by its diagonal plus one V-cycle of the P1 vertex
 * grid; every reduction runs in a fixed order, so two calls return the same bits.
 *
 * Structured meshes on one rank.  A general mesh and a strip partition return HDG_ERR_UNSUPPORTED.  Every call here is a
 * between-step call: inside an open step (between hdg_begin_step and the end of the step) it is refused with HDG_ERR_ARG.
 * None of them changes the state, the step path, its timers or its launch tallies.
 */
#ifndef HDG_STREAMFUNCTION_H
#define HDG_STREAMFUNCTION_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Q: a nodal velocity-space field (N_c n_u, 2) in the layout hdg_get_field uses; NULL: the current velocity.  rtol: the
 * iteration stops when (r, B r) <= rtol^2 (r0, B r0), B the preconditioner; 0 < rtol < 1 (1e-12 is the usual value).  psi
 * receives the n_cg values in the order of hdg_cg_size / hdg_cg_coordinates.
 * info = { iterations, final relative preconditioned residual sqrt((r, B r) / (r0, B r0)), defect, |u|_{L2}, ubar_x, ubar_y,
 * min psi, max psi };  ubar is zero on the unit square.  More than 2000 iterations: HDG_ERR_NOT_CONVERGED. */
int hdg_streamfunction(hdg_handle* h, const double* Q, double rtol, double* psi, double info[8]);
/* test hook: y = K x, K the stiffness matrix of CG_{k+1} (n_cg values each).  It sets nothing. */
int hdg_apply_cg_stiffness(hdg_handle* h, const double* x, double* y);
/* test hook: the nested P1 interpolation between the mesh vertices and CG_{k+1}.  dir 0: out (n_cg) = P in (vertices);
 * dir 1: out (vertices) = P^T in (n_cg).  Vertex (i, j) is entry j (nx + 1) + i, on the periodic square j nx + i: the index of
 * its dof in CG_{k+1}.  It sets nothing. */
int hdg_psi_transfer(hdg_handle* h, int dir, const double* in, double* out);
/* test hook: z = B r (n_cg values each).  form 0: the preconditioner the solve uses; form 1: the diagonal alone.  It sets nothing. */
int hdg_apply_psi_preconditioner(hdg_handle* h, int form, const double* r, double* z);
/* the number of mesh vertices: (nx + 1)^2, on the periodic square nx^2 */
int hdg_psi_vertex_count(hdg_handle* h, long* n_vertices);

#ifdef __cplusplus
}
#endif

#endif /* HDG_STREAMFUNCTION_H */
