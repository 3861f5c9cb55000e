/* Checkpoint and restart of an engine of libhdg_mi355x.so.
 *
 * These entry points live in a header of their own, beside include/hdg_mi355x.h, and a binding resolves them from a table of
 * its own (incompressibleeulerhdg_amd/_lib.py: CHECKPOINT_SIGNATURES, walked by load_library together with SIGNATURES): the
 * table of hdg_mi355x.h is pinned by the tests and stays what it is.  Same conventions: 0 on success or a negative HDG_ERR_*
 * code, the message through hdg_last_error; plain pointers and sizes; the caller owns every host buffer.
 *
 * Invariant: after hdg_checkpoint_load the engine IS the engine that was saved.  Everything observable through the C-ABI
 * afterwards -- fields, tracers, particle positions and counters, recorder rows, iteration statistics, solver events -- is
 * what the saved engine would have given, bit for bit.  Timers and the launch census are the exception: they start at zero.
 *
 * A blob is bound to the engine that wrote it: constructor, every field of hdg_config but the device ordinal, mesh (general
 * meshes: vertex and cell counts and the digests of both arrays), rank and number of ranks, and the memory layout (vector
 * lengths with ghost and padding rows).  A load into any other engine is HDG_ERR_ARG with a message that names the field.
 * Environment switches (HDG_*) are not part of it: a run may be continued with another HDG_CHEB_EVERY, and is then simply no
 * longer the same run.
 *
 * A save is valid between steps only: between hdg_begin_step / hdg_tracer_begin_step and the hdg_finish_step (with a tracer:
 * hdg_tracer_finish_step) that completes the step, hdg_checkpoint_size, hdg_checkpoint_save and hdg_state_digest are
 * HDG_ERR_ARG.  A load validates the whole blob -- fingerprint, table bounds, the digest of every section's bytes -- before it
 * touches the engine: a refused load leaves the engine exactly as it was.
 */
#ifndef HDG_CHECKPOINT_H
#define HDG_CHECKPOINT_H

#include "hdg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes a checkpoint of the engine's present state needs (it grows with the rows the recorders have written) */
int hdg_checkpoint_size(hdg_handle* h, long* nbytes);
/* write the state into buf[nbytes] (nbytes from hdg_checkpoint_size); step and t are the caller's and come back from a load */
int hdg_checkpoint_save(hdg_handle* h, long step, double t, void* buf, long nbytes);
/* make the engine the one that wrote buf[nbytes]; step, t (either may be NULL): what the save was given */
int hdg_checkpoint_load(hdg_handle* h, const void* buf, long nbytes, long* step, double* t);
/* 16 bytes that say whether two engines are in the same state, without downloading either: the digest of the digests of
 * every section a checkpoint would hold, in section order */
int hdg_state_digest(hdg_handle* h, unsigned long long out[2]);
/* operator hook, like hdg_apply_*: the digest kernel on a host vector of n doubles with bit patterns b_i,
 * out[0] = sum b_i, out[1] = sum b_i (2 i + 1), both mod 2^64 */
int hdg_digest_vector(hdg_handle* h, const double* v, long n, unsigned long long out[2]);

#ifdef __cplusplus
}
#endif

#endif /* HDG_CHECKPOINT_H */
