/* nbody_hip_group_props.h -- GROUP PROPERTIES: fp64 mass, centre, bulk velocity, spin, internal kinetic energy, inertia
 * tensor, extent and potential minimum of every group of a catalogue (nbody_hip_groups.h: what nbody_hip_grid_groups
 * finds, or any lists of the caller's), for groups of ANY size, in one asynchronous pass.
 * Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.26.
 *
 * THE MODEL.  Group g is the bodies members[offsets[g]] .. members[offsets[g + 1] - 1], n = offsets[g + 1] - offsets[g]
 * of them, taken in that order (position p = 0 .. n - 1).  Every input is widened exactly: x = (double)pos, v =
 * (double)vel, m = (double)mass, phi = (double)phi.  All arithmetic is fp64, every +, -, * and / and the one sqrt
 * rounded once to nearest (no fused multiply-add: a product and the add that takes it are two roundings).
 *   PASS 1.  mass = sum m;  P = sum m * x;  Q = sum m * v (per axis).  X = P / mass, V = Q / mass: one division each,
 *            {0, 0, 0} when mass == 0.
 *   PASS 2, about those ROUNDED X and V: d = x - X, u = v - V per axis, and per member the terms
 *            ang_mom:  m * ((dy * uz) - (dz * uy)),  m * ((dz * ux) - (dx * uz)),  m * ((dx * uy) - (dy * ux))
 *            T:        m * (((ux * ux) + (uy * uy)) + (uz * uz))                 kinetic = 0.5 * sum T
 *            inertia:  m * (dx * dx), m * (dy * dy), m * (dz * dz), m * (dx * dy), m * (dx * dz), m * (dy * dz)
 *            W:        m * phi                                                    potential = 0.5 * sum W
 *            r2 = ((dx * dx) + (dy * dy)) + (dz * dz);  r_max = sqrt(max r2), r_max_body the member that has it
 *            phi_min = min phi, phi_min_body the member that has it.
 *            Equal values go to the LOWEST BODY INDEX (a compare of (value, index) pairs, whatever the order of the
 *            members); a NaN is never taken (all NaN: the body is -1 and the value 0).
 *   THE ORDER OF EVERY SUM is a function of n alone.  Every sum starts from +0 and a partial sum is only ever added as
 *   (earlier members) + (later members).
 *     n <= 32:  p = 0, 1, .., n - 1 in turn.
 *     n > 32:   the group is cut into chunks of 1,024 positions, chunk k = positions [1024 k, min(1024 (k + 1), n)).
 *               In a chunk, position q = 256 j + t (j = 0 .. 3, t = 0 .. 255): sum s_t takes the positions of t in the
 *               order j = 0, 1, 2, 3 (a t without positions has the sum +0).  The 256 sums are folded in four runs of
 *               64 (t = 64 w + l):  s_l += s_(l + 32) for l < 32, then s_l += s_(l + 16) for l < 16, .. 8, 4, 2, 1;
 *               the chunk's sum is ((run 0 + run 1) + run 2) + run 3.  The K chunk sums are folded the same way: sum
 *               c_l takes the chunks l, l + 64, l + 128, .. in that order (l = 0 .. 63), the 64 sums are folded
 *               32, 16, 8, 4, 2, 1 as above, and c_0 is the group's sum.
 *   So a group's struct is bitwise reproducible and does not depend on where the group stands in the catalogue, on the
 *   other groups of the call or on the launch.  There are no floating-point atomics.
 *
 * A LEGAL group has 0 <= offsets[g] < offsets[g + 1] <= n_members and every member index in [0, count).  Any other
 * group (an empty one included) gets status = 1, n = 0 and zeros everywhere else; the other groups of the call are
 * unaffected.  (Ranges of different groups may overlap; a catalogue whose ranges overlap so much that its groups of
 * more than 32 members have more than n_members / 1024 + n_members / 33 chunks between them -- no catalogue of disjoint
 * ranges has -- gets status = 1 in the groups beyond that.) */
#ifndef NBODY_HIP_GROUP_PROPS_H
#define NBODY_HIP_GROUP_PROPS_H

#include "nbody_hip_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbody_hip_group_props {
  double mass;        /* sum m_i */
  double com[3];      /* X = (sum m_i x_i) / mass; {0,0,0} when mass == 0 */
  double vel[3];      /* V = (sum m_i v_i) / mass; {0,0,0} when mass == 0 */
  double ang_mom[3];  /* sum m_i (x_i - X) x (v_i - V) */
  double kinetic;     /* 1/2 sum m_i |v_i - V|^2  (internal; dispersion^2 = 2 kinetic / mass is the caller's) */
  double inertia[6];  /* sum m_i d_a d_b, d = x_i - X: xx, yy, zz, xy, xz, yz */
  double r_max;       /* sqrt(max_i |x_i - X|^2) */
  double potential;   /* 1/2 sum m_i phi_i; 0 when no phi is given */
  double phi_min;     /* min_i phi_i; 0 when no phi is given */
  int n;              /* members */
  int label;          /* members[offsets[g]]: for a findGroups catalogue the group's label */
  int r_max_body;     /* ORIGINAL body index; ties: the lowest index */
  int phi_min_body;   /* ties: the lowest index; -1 when no phi is given */
  int status;         /* 0 ok; 1: offsets of this group not a legal range, or a member index outside [0, count) */
  int reserved[3];    /* 0 */
} nbody_hip_group_props; /* 192 bytes */

/* The properties of the n_groups groups of ANY catalogue in device memory (offsets_dev: n_groups + 1 ints, members_dev:
 * n_members ints) into out_dev[n_groups].  Of d only pos_*, vel_* and mass are read; phi_dev_or_null: d->count floats in
 * ORIGINAL body order (the per-body potential of any force method), or NULL.  Asynchronous on the context's stream;
 * reads nothing back; offsets and members are checked on the device, per group.  The workspace (8 bytes per group, 112
 * per possible chunk, the temporary storage of one scan) lives on the context and grows on demand; a call that fits the
 * workspace as it is may be recorded into a step graph.  n_groups == 0 succeeds and does nothing.
 * ERR_STATE: null context, particle data, arrays of it, offsets, members (with n_members > 0) or out.
 * ERR_VALIDATION: a negative count; n_members > 2^31 - 1; n_groups > 2^31 - 2; d->count 0 or above 2^30; particle data
 * on another device than the context's. */
NBODY_HIP_API int nbody_hip_groups_properties(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev,
                                              const int* members_dev, long long n_groups, long long n_members,
                                              const float* phi_dev_or_null, nbody_hip_group_props* out_dev);
/* The same pass over the catalogue the grid handle holds (out_dev: n_groups structs of the last nbody_hip_grid_groups).
 * ERR_STATE: null grid; no successful nbody_hip_grid_groups since the last build.  Else as above. */
NBODY_HIP_API int nbody_hip_grid_groups_properties(nbody_hip_grid* g, const nbody_particle_data* d,
                                                   const float* phi_dev_or_null, nbody_hip_group_props* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_GROUP_PROPS_H */
