/* nbody_hip_groups.h -- friends-of-friends GROUPS on a spatial-hash grid as last built (nbody_hip.h: nbody_hip_grid).
 * Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.25.
 *
 * THE MODEL.  On the grid as last built, two DISTINCT bodies are linked when
 *   (1) their cells differ by at most 1 along every axis (each lies in the other's 27-cell window), and
 *   (2) d2 < fl(b * b) in fp32, with d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 coordinate differences -- the
 *       force kernels' value and their strict `<`.
 * There is no guard: coincident bodies (d2 = 0) are linked whatever eps is; eps and G play no part.  Groups are the
 * connected components of that graph.  The label of a body is the LOWEST ORIGINAL BODY INDEX of its group (a singleton
 * is labelled with itself), so the labels do not depend on any lane, wave or atomic order, and every output of these
 * calls is bitwise reproducible.
 *
 * Precondition b <= the cell size of the last build (a larger b would silently miss links: it is refused).  With it
 * the model is plain friends-of-friends with linking length b over all bodies -- with ONE exception: a pair closer than
 * b whose fp32 cell coordinates round two cells apart (each coordinate is floorf(fl(fl(p - lo) / cell)): two bodies
 * just under one cell apart can land in cells c and c + 2 when both divisions round outwards) is not linked, because
 * (1) fails.  That needs b within a few ulp of the cell size and a pair within a few ulp of b.
 *
 * THE CATALOGUE.  The groups of at least min_members bodies, ascending by label; inside a group the members ascending
 * by body index.  offsets[g] .. offsets[g + 1] delimit group g in members[]; offsets has n_groups + 1 entries and
 * offsets[n_groups] = n_members.  Bodies of smaller groups are in no list (their labels are still written).
 *
 * Single-GPU grids only: a grid with a slab set (nbody_hip_grid_set_slab) is refused.  Neither the search nor the
 * copy can be recorded into a step graph.  They write no acc_* and leave the grid's statistics, tuning, work-list counters and the result of
 * the next force call untouched bit for bit.  The fp64 properties of the groups of a catalogue: nbody_hip_group_props.h. */
#ifndef NBODY_HIP_GROUPS_H
#define NBODY_HIP_GROUPS_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Finds the groups of the grid as last built (nbody_hip_grid_build, _drift_build or _build_packed without a slab) and
 * keeps their catalogue on the handle until the next call or the next build.  labels_dev: built_count ints in ORIGINAL
 * body order, device memory, may be NULL.  counts_host[2]: {n_groups, n_members} of the groups of at least min_members
 * bodies; the call blocks until they are there.  The workspace (28 bytes per body and the temporary storage of one
 * sort) is allocated at the first call and grows on demand.  A refused call touches nothing, an earlier catalogue included.
 * ERR_STATE: null grid; grid not built; a slab set.  ERR_VALIDATION: linking_length not positive and finite;
 * linking_length > the cell size of the last build; min_members < 1; null counts_host. */
NBODY_HIP_API int nbody_hip_grid_groups(nbody_hip_grid* g, float linking_length, int min_members, int* labels_dev,
                                        long long* counts_host);
/* Copies the catalogue of the last nbody_hip_grid_groups to device memory: offsets_dev n_groups + 1 ints, members_dev
 * n_members ints (either may be NULL: not copied).  Asynchronous on the context's stream.
 * ERR_STATE: null grid; no successful nbody_hip_grid_groups since the last build. */
NBODY_HIP_API int nbody_hip_grid_groups_copy(nbody_hip_grid* g, int* offsets_dev, int* members_dev);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_GROUPS_H */
