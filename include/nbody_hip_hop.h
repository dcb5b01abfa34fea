/* nbody_hip_hop.h -- density-peak (HOP) GROUPS from neighbour lists and densities, with saddle regrouping.
 * Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.29.  After Eisenstein & Hut (1998): every body hops to
 * its densest neighbour, chains end at density maxima, and the basins are regrouped by the density of the saddles
 * between them.  Integer pointer work plus one fp64 max: every output is bitwise reproducible, no lane, wave or atomic
 * order plays a part, and there is no floating-point atomic.
 *
 * INPUTS.  count bodies; k (1 <= k <= 32); index[count * k] int32, row i in original body order -- what
 * nbody_hip_grid_neighbours writes, or any lists; rho[count] fp64; the parameters n_hop (1 .. k), n_merge (0 .. k) and
 * min_members (>= 1); the fp64 thresholds delta_outer, delta_saddle, delta_peak, finite with
 * 0 <= delta_outer <= delta_saddle <= delta_peak.
 * Only the first n_hop / n_merge slots of a row are read.  Any negative entry is "no neighbour" and is skipped.  An
 * entry >= count in a slot below max(n_hop, n_merge) is caught on the device: status 1, n_groups = 0, rounds = 0,
 * n_peaks = 0, every label and peak -1, and the catalogue holds no group.  A row may name its own body: such an entry
 * changes nothing.
 *
 * ORDER.  better(j, b) := rho[j] > rho[b] || (rho[j] == rho[b] && j < b), compared in fp64.  A NaN density is never
 * better and is never beaten: such a body is its own peak and nobody's target.  -0 and +0 are equal densities.
 *
 * HOP.  next[i] starts at b = i; the first n_hop slots, in slot order, replace b by a candidate j while better(j, b).
 * next[i] != i is strictly better than i, so chains cannot cycle.  peak[i] is the fixed point of next from i.
 *
 * LIVE.  live(i) := rho[i] >= delta_outer (false for a NaN).  A dead peak has an all-dead basin.
 *
 * SADDLES.  Take every live i, every slot s < n_merge with j = index[i * k + s] >= 0, and j live with
 * peak[i] != peak[j].  b(i, j) = (rho[i] + rho[j]) * 0.5 in fp64, two roundings, nothing fused; a -0 result counts as
 * +0.  S{P, Q} is the maximum of b over all such pairs, with {peak[i], peak[j]} = {P, Q}, found from either side: the
 * lists are not symmetric, and an edge exists as soon as one side names the other.
 *
 * REGROUP.  viable(P) := live(P) && rho[P] >= delta_peak, for a peak P.
 *   1. Viable peaks P, Q with S{P, Q} >= delta_saddle are united; the root of a component is its lowest peak index.
 *      Viable peaks start anchored ("anchored in round 0"), root[P] being the root of P's component.
 *   2. Rounds r = 1, 2, ... follow.  In round r every live, non-viable peak P not yet anchored looks at its edges
 *      {P, Q} with Q anchored before round r.  If there are any, P takes the one with the greatest S, ties to the lowest
 *      Q, sets root[P] = root[Q] and is anchored from round r + 1 on.  The rounds end with the first that anchors
 *      nothing; `rounds` counts it too, so rounds >= 1, and rounds <= max(1, n_peaks).
 *   3. Peaks never anchored are dropped.
 *
 * OUTPUTS.  label[i] = root[peak[i]] if i is live and its peak is anchored, else -1.  peak[i] is written for every
 * body.  The catalogue holds the groups of at least min_members labelled bodies, ascending by label, members ascending
 * by body index, offsets with n_groups + 1 entries: exactly the layout of nbody_hip_groups.h, so
 * nbody_hip_groups_properties and nbody_hip_groups_radial_profile take it as it is.  group_peak[g] is the
 * better-maximal peak among the anchored peaks whose root is the label of group g.
 * counts_host[5] = {n_groups, n_members, n_peaks, rounds, status}; n_peaks counts every body that is its own peak, dead
 * ones and NaN densities included.
 *
 * The regrouping rule is a parallel restatement of the `regroup` program distributed with HOP, not that program's
 * greedy sweep over the boundaries in descending density: DESIGN.md section 4.29 has the case where the two differ. */
#ifndef NBODY_HIP_HOP_H
#define NBODY_HIP_HOP_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_HIP_HOP_MAX_K 32
#define NBODY_HIP_HOP_STAGES 6

typedef struct {
  int n_hop, n_merge, min_members, reserved; /* reserved: 0 */
  double delta_outer, delta_saddle, delta_peak;
} nbody_hip_hop_params_t;

/* Finds the groups and keeps their catalogue on the context until the next accepted call.  index_dev, rho_dev: device
 * memory.  labels_dev, peak_dev: count ints each, device memory, either may be NULL.  counts_host[5]: see above.
 * THE CALL BLOCKS: it reads back the number of boundary records (to size their workspace), one word per attachment
 * round, and the counts.  It cannot be recorded into a step graph.  The workspace (about 80 bytes per body, 32 bytes per
 * directed boundary record and the temporary storage of two sorts) and the catalogue live on the context and grow on
 * demand.  A refused call touches nothing, an earlier catalogue included.
 * ERR_STATE: null context, index_dev, rho_dev, params or counts_host; the context is recording a step graph.
 * ERR_VALIDATION: count 0 or above 2^30; k, n_hop, n_merge or min_members out of range; reserved not 0; a threshold not
 * finite or the thresholds out of order.  ERR_RESOURCE: more than 2^31 - 1 directed boundary records (outputs and
 * the earlier catalogue untouched), or no memory for a workspace. */
NBODY_HIP_API int nbody_hip_hop_groups(nbody_hip_ctx* ctx, int count, int k, const int* index_dev, const double* rho_dev,
                                       const nbody_hip_hop_params_t* params, int* labels_dev, int* peak_dev,
                                       long long* counts_host);
/* Copies the catalogue of the last accepted nbody_hip_hop_groups to device memory: offsets_dev n_groups + 1 ints,
 * members_dev n_members ints, group_peak_dev n_groups ints (each may be NULL: not copied).  Asynchronous on the
 * context's stream.  ERR_STATE: null context; no successful nbody_hip_hop_groups on this context yet; recording. */
NBODY_HIP_API int nbody_hip_hop_groups_copy(nbody_hip_ctx* ctx, int* offsets_dev, int* members_dev, int* group_peak_dev);

/* The device time in milliseconds of the six stages of the last nbody_hip_hop_groups on this context that ended with
 * status 0, between events recorded on the stream: hop; peaks; boundary records (count, scan, the read-back the call
 * blocks for, fill); sort and fold; unite and attach (the round words' read-backs included); catalogue.  A measuring aid:
 * the search records seven events whether or not this is called.  ERR_STATE: null context or ms_host; no such search. */
NBODY_HIP_API int nbody_hip_hop_stage_times(nbody_hip_ctx* ctx, float* ms_host /* [NBODY_HIP_HOP_STAGES] */);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_HOP_H */
