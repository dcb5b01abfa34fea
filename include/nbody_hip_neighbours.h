/* nbody_hip_neighbours.h -- the K NEAREST NEIGHBOURS of every body on a spatial-hash grid as last built (nbody_hip.h:
 * nbody_hip_grid), the Casertano-Hut LOCAL DENSITY from them, and the DENSITY CENTRE of a set of bodies.
 * Additive: NBODY_HIP_ABI_VERSION stays 1.  DESIGN.md section 4.27.
 *
 * THE MODEL.  On the grid as last built, the CANDIDATES of body i are the bodies whose cells differ from i's by at most 1
 * along every axis (its 27-cell window), except i itself.  The body itself is skipped by its position in the list, not
 * by distance: a coincident body is a neighbour with d2 = 0.
 *   d2  = fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 coordinate differences candidate - i: the force kernels' value.
 *         A candidate whose d2 is a NaN is never taken.
 *   key = ((unsigned 64-bit) bits(d2) << 32) | original body index.  d2 >= +0, so the bit pattern orders as the float
 *         does; equal distances go to the lowest original index.
 * The K NEAREST are the k smallest keys, 1 <= k <= 32.  Row i (ORIGINAL body order) holds them ascending by key:
 * index[i * k + s], dist2[i * k + s], s = 0 .. k - 1.  Slots without a candidate hold index -1 and d2 = +inf.
 *
 * status[i], with d2_k the distance of slot k - 1 and cell the cell size of the last build:
 *   3  k were found and d2_k == 0: the k-th neighbour is coincident
 *   0  exact: k were found and d2_k < fl(cell * cell) (fp32) -- or the grid has at most 2 cells along every axis, so
 *      that the window is the whole grid
 *   1  window-limited: k were found but d2_k >= fl(cell * cell): a nearer body may sit outside the window
 *   2  fewer than k candidates (in a grid of at most 2 cells per axis this means count - 1 < k, and is final)
 * Status 0 means "the true k nearest of all bodies" -- with ONE exception, that of nbody_hip_groups.h: a pair closer
 * than the cell size whose fp32 cell coordinates round two cells apart (each coordinate is
 * floorf(fl(fl(p - lo) / cell)): two bodies just under one cell apart can land in cells c and c + 2 when both divisions
 * round outwards) are not each other's candidates.  That needs d2_k within a few ulp of fl(cell * cell).
 *
 * THE DENSITY is Casertano and Hut (1985), in fp64, every operation rounded once (nothing is fused):
 *   msum = the sum of (double)m of the neighbours of slots 0 .. k - 2 (all but the k-th), in that order, from +0
 *          (k = 1: msum = 0);   r = sqrt((double)d2_k);   rho = msum / (C * ((r * r) * r)),
 *   C = NBODY_HIP_SPHERE_4PI_3 below.  rho = 0 for status 2 and 3.  Status 1 is computed from what the window holds --
 *   and is flagged.
 *
 * REFINEMENT.  With refine != 0, a body whose status_dev[i] is 0 on entry is skipped: NONE of its outputs is written.
 * Every other body is recomputed.  So a caller resolves the window-limited bodies on a coarser build (twice the cell,
 * and again) without redoing the rest; in a grid of at most 2 cells per axis nothing is left to resolve.
 *
 * Every output is bitwise reproducible: no lane, wave or atomic order plays a part.
 *
 * THE DENSITY CENTRE of a set of n bodies (all of them, or an index list, taken in that order: position p = 0 .. n - 1)
 * with weights rho, in fp64, inputs widened exactly, every operation rounded once (nothing is fused):
 *   PASS 1.  S1 = sum rho;  P = sum rho * x (per axis);  x_d = P / S1.
 *   PASS 2, about the ROUNDED x_d: d = x - x_d per axis, r2 = ((dx * dx) + (dy * dy)) + (dz * dz);
 *            S2 = sum rho * rho;  R = sum (rho * rho) * r2;  core_radius = sqrt(R / S2) (0 when S2 == 0).
 *   When S1 == 0 the centre, the radius and both sums are zeros.
 *   THE ORDER OF EVERY SUM is a function of n alone -- that of nbody_hip_group_props.h.  Every sum starts from +0 and a
 *   partial sum is only ever added as (earlier positions) + (later positions).
 *     n <= 32:  p = 0, 1, .., n - 1 in turn.
 *     n > 32:   chunks of 1,024 positions, chunk c = positions [1024 c, min(1024 (c + 1), n)).  In a chunk, position
 *               q = 256 j + t (j = 0 .. 3, t = 0 .. 255): sum s_t takes the positions of t in the order j = 0, 1, 2, 3 (a
 *               t without positions has the sum +0).  The 256 sums are folded in four runs of 64 (t = 64 w + l):
 *               s_l += s_(l + 32) for l < 32, then s_l += s_(l + 16) for l < 16, .. 8, 4, 2, 1; the chunk's sum is
 *               ((run 0 + run 1) + run 2) + run 3.  The chunk sums are folded the same way: sum c_l takes the chunks
 *               l, l + 64, l + 128, .. in that order (l = 0 .. 63), the 64 sums are folded 32, 16, 8, 4, 2, 1 as above,
 *               and c_0 is the sum.
 *   There are no floating-point atomics.  A member index outside [0, count) gives status = 1, and zeros in the rest. */
#ifndef NBODY_HIP_NEIGHBOURS_H
#define NBODY_HIP_NEIGHBOURS_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_HIP_NEIGHBOURS_MAX_K 32
/* the fp64 nearest to 4 pi / 3 */
#define NBODY_HIP_SPHERE_4PI_3 4.1887902047863905

/* The k nearest candidates of every body of the grid as last built (nbody_hip_grid_build, _drift_build or
 * _build_packed without a slab).  index_dev, dist2_dev: built_count * k ints / floats; rho_dev: built_count doubles;
 * status_dev: built_count ints; all in ORIGINAL body order, device memory.  Each may be NULL (not written), but not all
 * of them; with refine != 0 status_dev is required (it is read, then written).  Asynchronous on the context's stream;
 * allocates nothing and reads nothing back.  Writes only its outputs: the grid's statistics, tuning, work list and
 * counters, a group catalogue and the bits of the next force call are untouched.  A refused call touches nothing.
 * ERR_STATE: null grid; grid not built; a slab set.
 * ERR_VALIDATION: k outside 1 .. 32; all outputs NULL; refine without status_dev. */
NBODY_HIP_API int nbody_hip_grid_neighbours(nbody_hip_grid* g, int k, int refine, int* index_dev, float* dist2_dev,
                                            double* rho_dev, int* status_dev);

typedef struct nbody_hip_density_centre_t {
  double centre[3];   /* x_d = (sum rho x) / (sum rho); {0,0,0} when sum rho == 0 */
  double core_radius; /* sqrt((sum rho^2 |x - x_d|^2) / (sum rho^2)) */
  double rho_sum;     /* S1 */
  double rho2_sum;    /* S2 */
  int n;              /* bodies of the set */
  int status;         /* 0 ok; 1: a member index outside [0, count) -- then everything else is 0 */
  int reserved[2];    /* 0 */
} nbody_hip_density_centre_t; /* 64 bytes */

/* The density centre of one set of bodies of d: all d->count bodies when members_dev_or_null is NULL (n_members is then
 * ignored), else the n_members indices of the list (a slice of a group catalogue's members, for one).  rho_dev: d->count
 * doubles in ORIGINAL body order (what nbody_hip_grid_neighbours wrote, or any weights).  Of d only pos_* are read.
 * out_dev: one struct in device memory.  Asynchronous on the context's stream; reads nothing back.  The workspace (32
 * bytes per chunk of 1,024 bodies) lives on the context and grows on demand.
 * ERR_STATE: null context, particle data, position arrays, rho or out.
 * ERR_VALIDATION: d->count 0 or above 2^30; n_members negative or above 2^31 - 1. */
NBODY_HIP_API int nbody_hip_density_centre(nbody_hip_ctx* ctx, const nbody_particle_data* d, const double* rho_dev,
                                           const int* members_dev_or_null, long long n_members,
                                           nbody_hip_density_centre_t* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_NEIGHBOURS_H */
