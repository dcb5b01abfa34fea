// grid_groups.inc -- friends-of-friends groups on the grid as last built (nbody_hip_groups.h: the model; DESIGN.md
// section 4.25).  Included at the end of spatial_hash.hip, so it sees the grid record, CellLookup / window_run,
// hash_dist2 and the array tables.
//
// THE LINK PASS.  One lane per body of the cell-ordered list, modelled on hash_body_potential_kernel: the same nine runs
// (start array, or binary search on sparse grids), entries k > t only, so every pair of the 27-cell windows is seen once.
// A pair with d2 < b2 is united in a lock-free union-find over ORIGINAL body indices:
//   * parent[x] <= x, always: a root is hooked under a SMALLER index only (atomicCAS on the root's own word, expected
//     value = itself), so a root is the lowest index of its tree and a parent chain is strictly decreasing;
//   * whatever parent[x] ever holds is an ancestor of x, and ancestors stay ancestors (hooks happen at roots, path
//     halving replaces a parent by a grandparent through atomicMin): a stale read costs steps, not correctness;
//   * find follows parents with relaxed atomic loads down a strictly decreasing chain: at most x steps;
//   * unite retries only when its CAS met a root that another lane had hooked in the meantime, and goes on from where
//     that root hangs now -- strictly lower.  At most n - 1 hooks ever succeed, so the retries are bounded.
// No lane waits for another lane: no locks, no flags, no spinning.  The atomics are vector atomics on global memory.
// THE LABEL PASS (after the kernel boundary): labels[i] = root of i = the lowest index of its group; group sizes by
// integer atomicAdd (order independent), the lanes of a wave that share a root folded into one add.
// THE CATALOGUE: key = label when the group has >= min_members bodies, else the sentinel n; ONE stable sort of
// (key, body index) through the public sort of body_sort.h; head flags, one exclusive scan (rocprim's public one), and a
// scatter give offsets[n_groups + 1].  No floating-point sum anywhere.
// THE SHARED PART.  The union-find, the wave-folded size count and the head / offset kernels of the catalogue are also what
// the density-peak groups need (hop_groups.hip, DESIGN.md section 4.29): that file defines NBH_GROUPS_SHARED_PART_ONLY and
// includes this one, which then ends after this part -- one text, two users.  It needs common.h alone; its kernels are
// `static`, so each of the two translation units launches its own copy.
#ifndef NBH_GROUPS_SHARED_PART
#define NBH_GROUPS_SHARED_PART
namespace nbh {

__device__ __forceinline__ int group_parent(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way (atomicMin: a parent is only ever replaced by a lower ancestor)
__device__ __forceinline__ int group_find(int* parent, int x) {
  int p = group_parent(parent, x);
  while (p != x) {  // p < x
    const int gp = group_parent(parent, p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void group_unite(int* parent, int a, int b) {
  for (;;) {
    a = group_find(parent, a);
    b = group_find(parent, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;  // hi was hooked by another lane meanwhile (old < hi): go on from there
    b = lo;
  }
}

// (the sizes: the lanes of a wave that share a root add once, not once per body -- the bodies of a group that holds most
// of the box would otherwise all add to one word, and one word takes about 88 atomics per microsecond: 33 ms at 2.9 M
// members, DESIGN.md section 4.25)
// kSizeRounds rounds, each folding the lanes that share the root of the lowest lane still to do; whoever is left
// adds for itself.  A group that holds a share p of a wave escapes the rounds with probability (1 - p)^kSizeRounds,
// and a wave of 64 different roots (small b: nearly every body alone) pays four rounds, not 64.
// Every lane of the wave calls this; `valid` lanes add 1 to sizes[r].
__device__ __forceinline__ void group_size_add(bool valid, int r, int* __restrict__ sizes) {
  constexpr int kSizeRounds = 4;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long todo = __ballot(valid);  // the same word in every lane: the loop is uniform
  for (int round = 0; round < kSizeRounds && todo; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const int root = __shfl(r, leader);
    const unsigned long long same = __ballot(valid && r == root) & todo;
    if (lane == leader) atomicAdd(sizes + root, (int)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(sizes + r, 1);
}

// the sorted keys: kept entries (key < n) first, group by group; a head is the first entry of a kept group
__device__ __forceinline__ bool group_head(const unsigned int* __restrict__ keys, int j, int n) {
  const unsigned int k = keys[j];
  return k < (unsigned int)n && (j == 0 || keys[j - 1] != k);
}

static __global__ __launch_bounds__(kBlock) void group_heads_kernel(int n, const unsigned int* __restrict__ keys,
                                                                   int* __restrict__ flags) {
  const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (j >= n) return;
  flags[j] = group_head(keys, j, n) ? 1 : 0;
}

// ord[j] = heads before j.  Every head writes its offset; the first dropped entry (or, when none is dropped, the last
// entry) writes the closing offset and the two counts.
static __global__ __launch_bounds__(kBlock) void group_offsets_kernel(int n, const unsigned int* __restrict__ keys,
                                                                     const int* __restrict__ ord, int* __restrict__ offsets,
                                                                     long long* __restrict__ counts) {
  const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (j >= n) return;
  const bool head = group_head(keys, j, n);
  const bool kept = keys[j] < (unsigned int)n;
  if (head) offsets[ord[j]] = j;
  if (!kept && (j == 0 || keys[j - 1] < (unsigned int)n)) {
    offsets[ord[j]] = j;
    counts[0] = ord[j];
    counts[1] = j;
  }
  if (kept && j == n - 1) {
    const int groups = ord[j] + (head ? 1 : 0);
    offsets[groups] = n;
    counts[0] = groups;
    counts[1] = n;
  }
}

}  // namespace nbh
#endif  // NBH_GROUPS_SHARED_PART

#ifndef NBH_GROUPS_SHARED_PART_ONLY
#include <rocprim/device/device_scan.hpp>

#include "nbody_hip_groups.h"
#include "nbody_hip_group_props.h"
#include "nbody_hip_radial.h"

namespace nbh {

using GroupSort = BodySort<unsigned int, false, false>;  // (key, body index) pairs, the public sort alone

__global__ __launch_bounds__(kBlock) void group_init_kernel(int n, int* __restrict__ parent, int* __restrict__ sizes,
                                                            int* __restrict__ body) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  parent[i] = i;
  sizes[i] = 0;
  body[i] = i;
}

__global__ __launch_bounds__(kBlock) void group_link_kernel(
    const float4* __restrict__ sorted, const unsigned int* __restrict__ keys, const int* __restrict__ idx,
    const int* __restrict__ lb, long long lb_base, long long lb_count, int n, int gx, int gy, int gz, float b2,
    int* parent) {
  const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (t >= n) return;
  const CellLookup look{{sorted, lb, idx, lb_base, lb_count}, keys, n};
  const CellXYZ cc = cell_xyz(keys[t], gx, gy);
  const float4 p = sorted[t];
  const int it = idx[t];
  for (int r = 0; r < 9; r++) {
    int k0, k1;
    if (!window_run(look, cc, r, gx, gy, gz, k0, k1)) continue;
    k0 = max(k0, t + 1);
    k1 = min(k1, n);
    for (int k = k0; k < k1; k++) {
      const float4 e = sorted[k];
      const float dx = e.x - p.x, dy = e.y - p.y, dz = e.z - p.z;
      if (hash_dist2(dx, dy, dz) < b2) group_unite(parent, it, idx[k]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void group_label_kernel(int n, int* parent, int* __restrict__ labels,
                                                             int* __restrict__ sizes) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  const bool valid = i < n;
  int r = -1;
  if (valid) {
    r = group_find(parent, i);
    atomicMin(parent + i, r);  // (the root is the lowest ancestor: parent[i] = r from here on)
    if (labels) labels[i] = r;
  }
  group_size_add(valid, r, sizes);  // (the shared part above: the lanes of a wave that share a root add once)
}

__global__ __launch_bounds__(kBlock) void group_keys_kernel(int n, const int* __restrict__ parent,
                                                            const int* __restrict__ sizes, int min_members,
                                                            unsigned int* __restrict__ keys) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  const int r = parent[i];
  keys[i] = sizes[r] >= min_members ? (unsigned int)r : (unsigned int)n;
}

}  // namespace nbh

static int grid_group_workspace(nbody_hip_grid* g, size_t n) {
  if (n <= g->group_cap) return NBODY_HIP_OK;
  const hipStream_t st = g->ctx->stream;
  NBH_HIP(hipStreamSynchronize(st));  // (an earlier call may still read the old arrays)
  ArraySlot slots[kMaxSlots];
  g->group_cap = 0;
  g->groups_valid = false;
  const size_t cap = group_capacity(n, g->max_particles);
  const GroupSizes s = group_sizes(cap);
  size_t sort_bytes = 0, scan_bytes = 0;
  int e = (int)GroupSort::run(SortImpl::Public, nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cap, 0,
                              32, st);  // (the sizes of the two temporary storages)
  if (e == 0)
    e = (int)rocprim::exclusive_scan(nullptr, scan_bytes, static_cast<int*>(nullptr), static_cast<int*>(nullptr), 0, cap,
                                     rocprim::plus<int>(), st);
  g->gtmp_bytes = std::max(sort_bytes, scan_bytes);
  if (e == 0) e = replace_arrays(slots, group_slots(g, s, slots), nullptr, 0, dev_alloc, dev_free, dev_zero);
  if (e != 0) {
    release_arrays(slots, group_slots(g, s, slots), nullptr, dev_free);  // (whichever failed: nothing is left)
    return NBH_FAIL(alloc_code(e), "group workspace of the grid (%zu bodies): %s", cap, alloc_text(e));
  }
  g->group_cap = cap;
  return NBODY_HIP_OK;
}

// Groups of the grid as last built.  Ignores the force-kernel tuning and leaves the grid's occupancy statistics, its
// work list and its counters alone: it reads d_sorted, d_keys_b, d_idx_b and the start array, and writes its own arrays.
extern "C" int nbody_hip_grid_groups(nbody_hip_grid* g, float linking_length, int min_members, int* labels_dev,
                                     long long* counts_host) {
  if (!g) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null grid");
  nbody_hip_ctx* ctx = g->ctx;
  NBH_NOT_CAPTURABLE(ctx, "a group search");
  if (g->built_count == 0) return NBH_FAIL(NBODY_HIP_ERR_STATE, "grid has not been built");
  if (g->slab_nz > 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "groups are found on single-GPU grids only: this grid holds a slab (nbody_hip_grid_set_slab)");
  if (!(linking_length > 0.0f) || !(linking_length < INFINITY))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "linking length must be positive and finite");
  if (linking_length > g->built_cell)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION,
                    "linking length %g exceeds the cell size %g of the grid as built: links across two cells would be missed "
                    "(rebuild with a cell of at least the linking length)",
                    (double)linking_length, (double)g->built_cell);
  if (min_members < 1) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "min_members must be at least 1");
  if (!counts_host) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null counts_host");
  NBH_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  g->groups_valid = false;
  if (int rc = grid_group_workspace(g, g->built_count)) return rc;
  const int n = (int)g->built_count;
  const unsigned blocks = grid_blocks(n);
  const float b2 = linking_length * linking_length;
  const int* lb = g->lb_valid ? g->d_cell_lb : nullptr;
  hipLaunchKernelGGL(group_init_kernel, dim3(blocks), dim3(kBlock), 0, st, n, g->d_gparent, g->d_gsizes, g->d_gbody);
  hipLaunchKernelGGL(group_link_kernel, dim3(blocks), dim3(kBlock), 0, st, g->d_sorted, g->d_keys_b, g->d_idx_b, lb, g->lb_base,
                     g->lb_count, n, g->info.dims[0], g->info.dims[1], g->info.dims[2], b2, g->d_gparent);
  hipLaunchKernelGGL(group_label_kernel, dim3(blocks), dim3(kBlock), 0, st, n, g->d_gparent, labels_dev, g->d_gsizes);
  hipLaunchKernelGGL(group_keys_kernel, dim3(blocks), dim3(kBlock), 0, st, n, g->d_gparent, g->d_gsizes, min_members,
                     g->d_gkeys_a);
  NBH_LAUNCH_CHECK();
  size_t tmp = g->gtmp_bytes;
  NBH_HIP(GroupSort::run(SortImpl::Public, g->d_gtmp, tmp, g->d_gkeys_a, g->d_gkeys_b, nullptr, nullptr, g->d_gbody,
                         g->d_gmembers, (size_t)n, 0u, (unsigned)group_key_bits((size_t)n), st));
  // (the unsorted keys and the sizes are dead from here: their arrays take the head flags and the scan's result)
  int* flags = reinterpret_cast<int*>(g->d_gkeys_a);
  int* ord = g->d_gsizes;
  hipLaunchKernelGGL(group_heads_kernel, dim3(blocks), dim3(kBlock), 0, st, n, g->d_gkeys_b, flags);
  NBH_LAUNCH_CHECK();
  tmp = g->gtmp_bytes;
  NBH_HIP(rocprim::exclusive_scan(g->d_gtmp, tmp, flags, ord, 0, (size_t)n, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(group_offsets_kernel, dim3(blocks), dim3(kBlock), 0, st, n, g->d_gkeys_b, ord, g->d_goffsets, g->d_gcounts);
  NBH_LAUNCH_CHECK();
  long long counts[2] = {0, 0};
  NBH_HIP(hipMemcpyAsync(counts, g->d_gcounts, sizeof(counts), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  counts_host[0] = counts[0];
  counts_host[1] = counts[1];
  g->group_count = counts[0];
  g->group_members = counts[1];
  g->groups_valid = true;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_grid_groups_copy(nbody_hip_grid* g, int* offsets_dev, int* members_dev) {
  if (!g) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null grid");
  NBH_NOT_CAPTURABLE(g->ctx, "a group catalogue copy");
  if (!g->groups_valid)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "no group catalogue: call nbody_hip_grid_groups after the last build first");
  NBH_HIP(hipSetDevice(g->ctx->device));
  const hipStream_t st = g->ctx->stream;
  if (offsets_dev)
    NBH_HIP(hipMemcpyAsync(offsets_dev, g->d_goffsets, (size_t)(g->group_count + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (members_dev && g->group_members > 0)
    NBH_HIP(hipMemcpyAsync(members_dev, g->d_gmembers, (size_t)g->group_members * sizeof(int), hipMemcpyDeviceToDevice, st));
  return NBODY_HIP_OK;
}

// The properties of the catalogue the handle holds: the generic pass of group_props.hip on the grid's own arrays.
extern "C" int nbody_hip_grid_groups_properties(nbody_hip_grid* g, const nbody_particle_data* d, const float* phi_dev_or_null,
                                                nbody_hip_group_props* out_dev) {
  if (!g) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null grid");
  if (!g->groups_valid)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "no group catalogue: call nbody_hip_grid_groups after the last build first");
  return group_props_launch(g->ctx, d, g->d_goffsets, g->d_gmembers, g->group_count, g->group_members, phi_dev_or_null,
                            out_dev);
}

// The radial profiles of the catalogue the handle holds: the generic pass of radial_profile.hip on the grid's own arrays.
extern "C" int nbody_hip_grid_groups_radial_profile(nbody_hip_grid* g, const nbody_particle_data* d, const double* centres_dev,
                                                    const double* vels_dev_or_null, const double* cuts_host, int n_cuts,
                                                    int mode, nbody_hip_radial_group* groups_out_dev,
                                                    nbody_hip_radial_shell* shells_out_dev, int* sorted_members_dev_or_null,
                                                    float* sorted_q_dev_or_null) {
  if (!g) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null grid");
  if (!g->groups_valid)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "no group catalogue: call nbody_hip_grid_groups after the last build first");
  return radial_profile_launch(g->ctx, d, g->d_goffsets, g->d_gmembers, g->group_count, g->group_members, centres_dev,
                               vels_dev_or_null, cuts_host, n_cuts, mode, groups_out_dev, shells_out_dev,
                               sorted_members_dev_or_null, sorted_q_dev_or_null);
}
#endif  // NBH_GROUPS_SHARED_PART_ONLY
