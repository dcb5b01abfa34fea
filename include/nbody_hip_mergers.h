/* nbody_hip_mergers.h -- the calls of the ensemble MERGERS (nbody_hip.h: the model, the flags,
 * nbody_hip_batch_merger_state_t and nbody_hip_batch_merger_t) on a block-step Hermite ensemble handle.  Additive:
 * NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.21. */
#ifndef NBODY_HIP_MERGERS_H
#define NBODY_HIP_MERGERS_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Turns the mergers of the handle on (flags = NBODY_HIP_BATCH_MERGERS_ON) or off (0).  On: nbody_hip_batch_mergers_apply
 * may be called.  The advance launches what it launched before.  It needs a layout (ERR_STATE before one; set_layout
 * drops the configuration).  Unknown flag bits: ERR_VALIDATION.  It allocates at its first use on a handle, by capacity
 * (68 bytes per body and 36 per system), and cannot be recorded.  From that first use on, prime resets the ids, the live
 * counts and the log of the handle, and nbody_hip_hermite_batch_diagnostics covers the live bodies of every system only
 * (a second form of its kernel that takes the live counts).  Turning the mergers off keeps what has merged: the live
 * counts stay in force until prime restores them. */
NBODY_HIP_API int nbody_hip_batch_mergers_set(nbody_hip_hermite_batch* h, int flags);
/* The pass: every system that stopped on contact merges its recorded pair, shrinks by one body, is primed again and
 * runs on.  d: the primed arrays (ERR_STATE otherwise).  Asynchronous on the context's stream, allocates nothing, reads
 * nothing back; after one eager call since the priming it can be recorded into a step graph, so [advance(k), apply]
 * replays with no host in the loop.  ERR_STATE: unprimed; mergers not configured; events not configured with radii and
 * STOP_ON_CONTACT.  The pass writes the radii of what it merged (the merged radius, 0 in the dead slot): a later priming
 * of the handle from fresh data needs nbody_hip_hermite_batch_set_events again. */
NBODY_HIP_API int nbody_hip_batch_mergers_apply(nbody_hip_hermite_batch* h, nbody_particle_data* d);
/* The merger state of all n_systems systems into state_host, and (each may be NULL) the log and the ids of all n_bodies
 * bodies into log_host_or_null and ids_host_or_null; the sizes must be the layout's (ERR_VALIDATION).  The entries of
 * system s are log[offsets[s] .. offsets[s] + n_mergers); the rest of the table is zero.  On a handle that never had
 * mergers configured: n_live = n, no entries, ids 0 .. n-1.  Blocking.  Unprimed: ERR_STATE. */
NBODY_HIP_API int nbody_hip_batch_mergers_get(nbody_hip_hermite_batch* h, nbody_hip_batch_merger_state_t* state_host,
                                              size_t n_systems, nbody_hip_batch_merger_t* log_host_or_null,
                                              unsigned int* ids_host_or_null, size_t n_bodies);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_MERGERS_H */
