/* nbody_hip_diag.h -- the ensemble diagnostics (nbody_hip_system_diag, nbody_hip.h: the model, the struct and the generic
 * call nbody_hip_systems_diagnostics) for the systems of the block-step Hermite handles.  Additive: NBODY_HIP_ABI_VERSION
 * stays 1.  One workgroup per system, fp64 from the full hi + lo state; DESIGN.md section 4.14. */
#ifndef NBODY_HIP_DIAG_H
#define NBODY_HIP_DIAG_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The systems of an ensemble handle: its layout (a device copy of the offsets is made at set_layout), its residuals in
 * extended mode, and the primed G and eps.  It REQUIRES a primed handle: without a layout, unprimed, or with another
 * count or pos_x pointer than the primed ones it fails with ERR_STATE.  out_device: n_systems structs.  Asynchronous,
 * allocates nothing, reads nothing back, can be recorded into a step graph.  A system whose schedule went out of range
 * still gets the struct of the bodies as they stand. */
NBODY_HIP_API int nbody_hip_hermite_batch_diagnostics(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                      nbody_hip_system_diag* out_device);
/* One system: all d->count <= 4,096 bodies of a single-system block-step handle, with its residuals in extended mode,
 * into out_device[0].  G and eps are the caller's (the handle need not be primed).  In the middle of a macro step the
 * bodies are not synchronised: ERR_STATE.  More than 4,096 bodies: ERR_VALIDATION.  In resident scheduling it waits
 * for the stream and reads the device schedule first, like the calls listed at set_scheduling (so it cannot be
 * recorded into a step graph then; with the schedule on the host it is asynchronous and can be). */
NBODY_HIP_API int nbody_hip_hermite_block_diagnostics(nbody_hip_hermite_block* h, nbody_particle_data* d, float G,
                                                      float eps, nbody_hip_system_diag* out_device);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_DIAG_H */
