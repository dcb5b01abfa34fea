/* nbody_hip_radial.h -- RADIAL PROFILES: Lagrangian radii and shell moments of every group of a catalogue
 * (nbody_hip_groups.h: what nbody_hip_grid_groups finds, or any ORDERED lists of the caller's) about centres the caller
 * picks, for groups of ANY size, in one asynchronous pass: a selection per group by radius, where
 * nbody_hip_group_props.h has sums.  Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.28.
 *
 * THE MODEL.  Group g is the bodies members[offsets[g]] .. members[offsets[g + 1] - 1] (members == NULL: the identity
 * list, body p at position p), n of them, position p = 0 .. n - 1; its centre c = centres[3 g ..] and bulk velocity
 * V = vels[3 g ..] (NULL: zeros) are doubles.  Every input is widened exactly; all arithmetic is fp64, every +, -, *, /
 * and sqrt rounded once to nearest (no fused multiply-add).  Per member:
 *     d = x - c            u = v - V            (per axis)
 *     r2 = ((dx*dx) + (dy*dy)) + (dz*dz)        q = (float)r2      (round to nearest; overflow gives +inf)
 *     s  = ((ux*dx) + (uy*dy)) + (uz*dz)        u2 = ((ux*ux) + (uy*uy)) + (uz*uz)
 *     r  = sqrt(r2)        vr = r2 > 0 ? s / r : 0        vr2 = vr*vr        vt2 = u2 - vr2
 *     terms of a shell sum:  m,  m*vr,  m*vr2,  m*vt2
 * THE RADIAL ORDER of a group is ascending by (bits(q), p): q >= +0, so its bit pattern orders as the float does; equal
 * q goes to the earlier position.  Rank s = 0 .. n - 1.  Every reported radius is sqrt((double)q).
 * ENCLOSED MASS.  E(s) = the sum of m over the ranks 0 .. s, M = E(n - 1), in an order that is a function of n alone; a
 * partial sum is only ever added as (earlier ranks) + (later ranks).
 *     n <= 32:  E(0) = m_0, E(s) = E(s - 1) + m_s.
 *     n > 32:   the group is cut into chunks of 1,024 ranks, chunk k = ranks [1024 k, min(1024 (k + 1), n)), filled up to
 *               1,024 with +0.  In a chunk, local rank l = 4 t + j (t = 0 .. 255, j = 0 .. 3):
 *               a(t, 0) = m_(4t), a(t, j) = a(t, j - 1) + m_(4t + j); P_t = a(t, 3); then eight rounds o = 1, 2, 4, .., 128
 *               of P_t <- P_(t - o) + P_t for every t >= o, all t of a round from the values before the round;
 *               W(l) = a(0, j) for t = 0, else P_(t - 1) + a(t, j).  The chunk's total is C_k = P_255.
 *               B_1 = C_0, B_k = B_(k - 1) + C_(k - 1);  E(1024 k + l) = W(l) for k = 0, else B_k + W(l).
 * THE CUTS (n_cuts of them, strictly ascending, the same for every group).  K_c = the leading ranks inside cut c:
 *     NBODY_HIP_RADIAL_MASS    fraction f in (0, 1]:  T = f * M (one rounding); K_c = the SMALLEST K in 1 .. n with
 *                              E(K - 1) >= T, an integer minimum over the ranks (E need not be monotone); none: K_c = n.
 *     NBODY_HIP_RADIAL_NUMBER  fraction f in (0, 1]:  K_c = min(n, max(1, (long long)ceil(f * (double)n))).
 *     NBODY_HIP_RADIAL_RADIUS  radius R >= 0, finite or +inf:  K_c = the number of ranks with sqrt((double)q) <= R (0 .. n).
 *     K_c is then raised to K_(c - 1) where the rule gives less (only a negative M can do that).
 * THE SHELLS.  Shell c = the ranks [K_(c - 1), K_c), K_(-1) = 0.  Its four sums run over its ranks as positions
 * 0 .. count - 1 counted from the shell's own first rank, in THE ORDER OF EVERY SUM of nbody_hip_group_props.h (at most 32
 * positions in turn, else chunks of 1,024 with its folds): a shell is a group of the sorted list.  An empty shell has zeros.
 * So every row is bitwise reproducible and does not depend on where the group stands in the catalogue, on the other
 * groups of the call or on the launch.  There are no floating-point atomics.
 *
 * THE CATALOGUE MUST BE ORDERED: 0 <= offsets[0], offsets[g] <= offsets[g + 1], offsets[n_groups] <= n_members (a
 * position of members has at most one owner; stricter than the group properties).  If any adjacent pair is out of
 * order EVERY group of the call gets status 1.  An empty group gets status 1 alone; so does a group with a member index
 * outside [0, count).  A group with a member whose r2 is a NaN gets status 2 (status 1 wins where both hold).  A group
 * with a non-zero status has n = 0 and zeros elsewhere in its struct, and zeros in all of its shell rows. */
#ifndef NBODY_HIP_RADIAL_H
#define NBODY_HIP_RADIAL_H

#include "nbody_hip_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_HIP_RADIAL_MAX_CUTS 16

#define NBODY_HIP_RADIAL_MASS 0   /* cuts are mass fractions */
#define NBODY_HIP_RADIAL_NUMBER 1 /* cuts are number fractions */
#define NBODY_HIP_RADIAL_RADIUS 2 /* cuts are absolute radii */

typedef struct nbody_hip_radial_group {
  double mass;     /* M */
  double r_max;    /* sqrt((double)q) of the last rank */
  int n;           /* members */
  int status;      /* 0 ok; 1 catalogue / range / member index; 2 a NaN distance */
  int reserved[2]; /* 0 */
} nbody_hip_radial_group; /* 32 bytes */

typedef struct nbody_hip_radial_shell {
  double radius;        /* fraction modes: sqrt((double)q) of rank K_c - 1; radius mode: R_c */
  double enclosed_mass; /* E(K_c - 1); 0 when K_c == 0 */
  double mass;          /* the shell's four sums: m */
  double m_vr;          /* m * vr */
  double m_vr2;         /* m * vr2 */
  double m_vt2;         /* m * vt2 */
  int count;            /* K_c - K_(c-1) */
  int enclosed_count;   /* K_c */
  int reserved[2];      /* 0 */
} nbody_hip_radial_shell; /* 64 bytes; row g * n_cuts + c */

/* The profiles of the n_groups groups of an ordered catalogue in device memory (offsets_dev: n_groups + 1 ints;
 * members_dev_or_null: n_members ints, NULL = the identity list, so offsets {0, count} is "all bodies as one group")
 * about centres_dev[3 n_groups] (doubles) and vels_dev_or_null[3 n_groups] (doubles; NULL: zeros), into
 * groups_out_dev[n_groups] and shells_out_dev[n_groups * n_cuts].  cuts_host: n_cuts doubles in HOST memory, copied into
 * the launch arguments.  Of d only pos_*, vel_* and mass are read.  Two optional outputs of n_members entries each:
 *   sorted_members_dev_or_null: at position offsets[g] + s the body index of rank s; -1 at positions of no group and in
 *     groups with a non-zero status (with it and offsets[g] + K_c any shell can go to nbody_hip_groups_properties);
 *   sorted_q_dev_or_null: the matching q (floats); 0 where the member is -1.
 * Asynchronous on the context's stream; reads nothing back; sized from the arguments alone.  The workspace (64 bytes per
 * member, 16 per group, 12 per cut of a group, 48 per possible chunk, the temporary storage of one radix sort and of one
 * scan) lives on the context and grows on demand; a call that fits the workspace as it is may be recorded into a step
 * graph.  n_groups == 0 succeeds and touches nothing.
 * ERR_STATE: null context, particle data, arrays of it, offsets, centres, cuts or outputs.
 * ERR_VALIDATION: a negative count; n_members > 2^31 - 1; n_groups > 2^31 - 2; n_cuts outside 1 .. 16; an unknown mode;
 * a cut outside its range or cuts not strictly ascending; n_groups * n_cuts > 2^31 - 1; d->count 0 or above 2^30;
 * particle data on another device than the context's. */
NBODY_HIP_API int nbody_hip_groups_radial_profile(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev,
                                                  const int* members_dev_or_null, long long n_groups, long long n_members,
                                                  const double* centres_dev, const double* vels_dev_or_null,
                                                  const double* cuts_host, int n_cuts, int mode,
                                                  nbody_hip_radial_group* groups_out_dev,
                                                  nbody_hip_radial_shell* shells_out_dev, int* sorted_members_dev_or_null,
                                                  float* sorted_q_dev_or_null);
/* The same pass over the catalogue the grid handle holds (the groups of the last nbody_hip_grid_groups).
 * ERR_STATE: null grid; no successful nbody_hip_grid_groups since the last build.  Else as above. */
NBODY_HIP_API int nbody_hip_grid_groups_radial_profile(nbody_hip_grid* g, const nbody_particle_data* d,
                                                       const double* centres_dev, const double* vels_dev_or_null,
                                                       const double* cuts_host, int n_cuts, int mode,
                                                       nbody_hip_radial_group* groups_out_dev,
                                                       nbody_hip_radial_shell* shells_out_dev,
                                                       int* sorted_members_dev_or_null, float* sorted_q_dev_or_null);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_RADIAL_H */
