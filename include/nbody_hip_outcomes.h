/* nbody_hip_outcomes.h -- the calls of the ensemble OUTCOMES (nbody_hip.h: the model, the flag and
 * nbody_hip_batch_outcome_t) on a block-step Hermite ensemble handle.  Additive: NBODY_HIP_ABI_VERSION stays 1.
 * DESIGN.md section 4.19. */
#ifndef NBODY_HIP_OUTCOMES_H
#define NBODY_HIP_OUTCOMES_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Configures the escape test of every system of the layout.  escape_radii_host_or_null: B floats, r_esc[s] >= 0, 0 no
 * test for system s (NULL: none); flags: NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE.  With radii given, advance launches a
 * form of the resident kernel with records and stop words that runs the test at every macro boundary; with NULL, 0 the
 * handle returns to the form it launched without outcomes.  The configuration is independent of
 * nbody_hip_hermite_batch_set_events: either one alone, or both, selects a form with records and stop words (whichever
 * comes first allocates the event records), and set_events(NULL, NULL, 0) with outcomes still on stays in one.  Without
 * events configured that form runs the untracked sweep: no radii, no budget, no closest approach.
 * It needs a layout (ERR_STATE before one; set_layout drops the configuration).  ERR_VALIDATION: a radius that is
 * negative or not finite, with a message that names the system; STOP_ON_ESCAPE with no radius > 0; unknown flag bits.
 * The data is copied on the context's stream, so it is ordered with the advance calls queued before and after; the call
 * returns when the host array has been read.  It allocates at its first use on a handle (68 bytes per system of
 * capacity, and the event buffers if there are none yet) and cannot be recorded.  It keeps the records and the priming.
 * A recorded step graph keeps the kernel form it recorded: after changing the configuration run one eager advance and
 * record again. */
NBODY_HIP_API int nbody_hip_batch_outcomes_set(nbody_hip_hermite_batch* h, const float* escape_radii_host_or_null,
                                               int flags);
/* The outcome records of all n_systems systems of the layout into out_host (n_systems must be the layout's:
 * ERR_VALIDATION).  On a handle that never had outcomes configured every record is "none".  Blocking.  Unprimed:
 * ERR_STATE. */
NBODY_HIP_API int nbody_hip_batch_outcomes_get(nbody_hip_hermite_batch* h, nbody_hip_batch_outcome_t* out_host,
                                               size_t n_systems);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_OUTCOMES_H */
