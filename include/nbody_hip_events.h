/* nbody_hip_events.h -- the calls of the ensemble EVENTS (nbody_hip.h: the model, the flags and nbody_hip_batch_event_t)
 * on a block-step Hermite ensemble handle.  Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.15. */
#ifndef NBODY_HIP_EVENTS_H
#define NBODY_HIP_EVENTS_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Configures the events of every system of the layout.  radii_host_or_null: offsets[B] floats, one per body of the
 * ensemble (NULL: no radii, every r = 0); limits_host_or_null: B values, limit[s] in macro steps since the priming, 0 no
 * limit (NULL: no limits); flags: NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST | NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT.
 * With any of the three given, advance launches the event form of the resident kernel; with NULL, NULL, 0 the handle
 * returns to the plain kernel, which knows neither records nor stop words (a stopped system would run on).
 * It needs a layout (ERR_STATE before one; set_layout drops the configuration).  ERR_VALIDATION, with a message that names
 * the body and its system: a radius that is negative or not finite; STOP_ON_CONTACT without radii; unknown flag bits.
 * The data is copied on the context's stream, so it is ordered with the advance calls queued before and after; the call
 * returns when the host arrays have been read.  It allocates at its first use on a handle (4 bytes per body and 72 per
 * system of capacity) and cannot be recorded.  It keeps the records and the priming; records accumulate only under
 * launches of the event form.  A recorded step graph keeps the kernel form it recorded: after changing the
 * configuration run one eager advance and record again. */
NBODY_HIP_API int nbody_hip_hermite_batch_set_events(nbody_hip_hermite_batch* h, const float* radii_host_or_null,
                                                     const unsigned long long* limits_host_or_null, int flags);
/* The records of all n_systems systems of the layout into out_host (n_systems must be the layout's: ERR_VALIDATION).
 * macro_steps_done is the system's counter whatever kernel form ran.  On a handle that never had events configured
 * every record is "none" with stopped = 0.  Blocking.  Unprimed: ERR_STATE. */
NBODY_HIP_API int nbody_hip_hermite_batch_events(nbody_hip_hermite_batch* h, nbody_hip_batch_event_t* out_host,
                                                 size_t n_systems);
/* The number of systems with stopped == 0 and no status error, so that a host can loop while (running) advance(k).
 * Blocking.  Unprimed: ERR_STATE. */
NBODY_HIP_API int nbody_hip_hermite_batch_running(nbody_hip_hermite_batch* h, size_t* n_running);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_EVENTS_H */
