// system_diag.h -- the launch of system_diag.hip, for the entry points that own the handles (hermite_batch.hip,
// hermite_block.hip; their diagnostics calls are declared in include/nbody_hip_diag.h).
#pragma once

#include "common.h"
#include "nbody_hip_diag.h"

namespace nbh {

// the residuals of a handle in extended state precision, one array per component (null pointers: none)
struct DiagLo {
  const float *x, *y, *z, *vx, *vy, *vz;
};

// One workgroup per system on ctx->stream: asynchronous, allocates nothing, reads nothing back.  offsets_device == null:
// the one system [0, d->count).  The caller has checked ctx, d (pos_*, vel_*, mass, count) and eps >= 0.
// live_device != null (ensemble MERGERS): the form with live counts, system s is the first
// live_device[s * live_stride] bodies of its range.
int system_diag_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const DiagLo* lo, const float4* pos_lo4,
                       const float4* vel_lo4, const unsigned long long* offsets_device, size_t n_systems, float G, float eps,
                       nbody_hip_system_diag* out_device, const unsigned int* live_device = nullptr, int live_stride = 0);

}  // namespace nbh
