/* nbody_hip_hierarchy.h -- the calls of the ensemble HIERARCHIES (nbody_hip.h: the model, the flag,
 * nbody_hip_batch_hierarchy_t and nbody_hip_batch_node_t) on a block-step Hermite ensemble handle.  Additive:
 * NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.20. */
#ifndef NBODY_HIP_HIERARCHY_H
#define NBODY_HIP_HIERARCHY_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Configures the examination of every system of the layout.  sep_radii_host_or_null: B floats, r_sep[s] >= 0, 0 no
 * examination for system s (NULL: none); kappa: the isolation factor, >= 0, 0 turns that criterion off; flags:
 * NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED.  With radii given, advance launches a form of the resident kernel with
 * records and stop words that examines every system with a radius at every macro boundary; with NULL, 0, 0 the handle
 * returns to the form it would launch otherwise: the outcomes form if outcomes are on, the event form if events are on,
 * else the plain form.  The configuration is independent of nbody_hip_hermite_batch_set_events and
 * nbody_hip_batch_outcomes_set, in any order.
 * It needs a layout (ERR_STATE before one; set_layout drops the configuration).  ERR_VALIDATION, with a message that
 * names the system where there is one: a radius that is negative or not finite; a radius > 0 on a system of more than
 * NBODY_HIP_BATCH_HIERARCHY_MAX bodies; kappa negative or not finite; STOP_ON_RESOLVED with no radius > 0; unknown flag
 * bits.  The data is copied on the context's stream, so it is ordered with the advance calls queued before and after;
 * the call returns when the host array has been read.  It allocates at its first use on a handle (128 bytes per body
 * and 68 bytes per system of capacity, and the event buffers if there are none yet) and cannot be recorded.  It keeps
 * the records and the priming.  A recorded step graph keeps the kernel form it recorded: after changing the
 * configuration run one eager advance and record again. */
NBODY_HIP_API int nbody_hip_batch_hierarchy_set(nbody_hip_hermite_batch* h, const float* sep_radii_host_or_null, float kappa,
                                                int flags);
/* The hierarchy records of all n_systems systems of the layout into records_host and, if nodes_host_or_null is given,
 * the node tables into it: n_slots must be 2 * offsets[n_systems], system s has the slots [2 offsets[s],
 * 2 offsets[s + 1]).  n_systems must be the layout's (ERR_VALIDATION).  On a handle that never had hierarchies
 * configured every record is "none" and every node slot is zero.  Blocking.  Unprimed: ERR_STATE. */
NBODY_HIP_API int nbody_hip_batch_hierarchy_get(nbody_hip_hermite_batch* h, nbody_hip_batch_hierarchy_t* records_host,
                                                size_t n_systems, nbody_hip_batch_node_t* nodes_host_or_null, size_t n_slots);
/* The decomposition of the state as it is now, of every system with 2 <= n <= NBODY_HIP_BATCH_HIERARCHY_MAX, stopped
 * systems included, by a kernel of its own into scratch records and tables: the run's own records are not touched.  The
 * resolved field uses the configured r_sep and kappa, 0 for both on a handle never configured; macro is the system's
 * completed macro steps.  Systems of 1 or more than 64 bodies get "none" and zero slots.  The pointer, count and primed
 * checks of advance; n_systems and n_slots as for _get, nodes_host required.  Blocking; cannot be recorded.  It
 * allocates at its first use (128 bytes per body and 64 bytes per system of capacity). */
NBODY_HIP_API int nbody_hip_batch_hierarchy_snapshot(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                     nbody_hip_batch_hierarchy_t* records_host, size_t n_systems,
                                                     nbody_hip_batch_node_t* nodes_host, size_t n_slots);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_HIERARCHY_H */
