// grid_neighbours.inc -- the k nearest neighbours and the local density of every body on the grid as last built
// (nbody_hip_neighbours.h: the model; DESIGN.md section 4.27).  Included at the end of spatial_hash.hip, so it sees the
// grid record, CellLookup / window_run and hash_dist2.  The keys, the insertion, the status rule and the density are
// neighbours_common.h, which the CPU program neighbours_check.cpp runs too.
//
// One lane per body of the cell-ordered list, modelled on hash_body_potential_kernel and group_link_kernel: the same nine
// runs (start array, or binary search on sparse grids).  A lane keeps its K smallest keys sorted in registers (and, for
// the density, the mass of each); a candidate is first held against the last key's distance alone -- only then is its
// body index loaded, the full key compared, and an accepted key sunk into place by K - 1 unrolled compare-and-swap steps.
// Every register index is a compile-time constant: no scratch.  No atomics, no LDS, no cross-lane step: a lane never
// waits for another, and every loop is bounded by the population of the lane's window, so the kernel ends.
// __launch_bounds__(kBlock) alone: a workgroup is one wave per SIMD, so the allocator may take what K = 32 needs (64
// registers of keys, 32 of masses) without spilling; nothing asks for an occupancy the list could not afford.
#include "neighbours_common.h"

namespace nbh {

template <int K, bool LISTS, bool RHO>
__global__ __launch_bounds__(kBlock) void grid_neighbours_kernel(
    const float4* __restrict__ sorted, const unsigned int* __restrict__ keys, const int* __restrict__ idx,
    const int* __restrict__ lb, long long lb_base, long long lb_count, int n, int gx, int gy, int gz, int k, int refine,
    float cell2, int* __restrict__ index, float* __restrict__ dist2, double* __restrict__ rho, int* status) {
  const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (t >= n) return;
  const int it = idx[t];
  if (refine && status[it] == 0) return;
  const CellLookup look{{sorted, lb, idx, lb_base, lb_count}, keys, n};
  const CellXYZ cc = cell_xyz(keys[t], gx, gy);
  const float4 p = sorted[t];
  NeighList<K, RHO> L;
  neigh_clear(L);
  for (int r = 0; r < 9; r++) {
    int k0, k1;
    if (!window_run(look, cc, r, gx, gy, gz, k0, k1)) continue;
    k1 = min(k1, n);
    for (int c = max(k0, 0); c < k1; c++) {
      const float4 e = sorted[c];
      const float dx = e.x - p.x, dy = e.y - p.y, dz = e.z - p.z;
      const float d2 = hash_dist2(dx, dy, dz);
      // (the distance alone first: a key cannot be below the last one when its high word is above that one's)
      if (c == t || !neigh_takes(d2) || neigh_bits(d2) > (unsigned int)(L.a[K - 1] >> 32)) continue;
      const NeighKey key = neigh_key(d2, idx[c]);
      if (neigh_accepts(L, key)) neigh_insert(L, key, e.w);
    }
  }
  const NeighKey kth = neigh_kth(L, k);
  const int st = neigh_status(kth, cell2, neigh_whole_grid(gx, gy, gz));
  if (LISTS) {
    const size_t row = (size_t)it * (size_t)k;
#pragma unroll
    for (int s = 0; s < K; s++) {
      if (s < k) {
        if (index) index[row + s] = neigh_key_index(L.a[s]);
        if (dist2) dist2[row + s] = neigh_key_dist2(L.a[s]);
      }
    }
  }
  if constexpr (RHO) rho[it] = neigh_density(neigh_msum(L, k), kth, st);
  if (status) status[it] = st;
}

}  // namespace nbh

// The k nearest of the grid as last built.  Ignores the force-kernel tuning and leaves the grid's occupancy statistics,
// its work list, its counters and a group catalogue alone: it reads d_sorted, d_keys_b, d_idx_b and the start array, and
// writes the caller's arrays.
extern "C" int nbody_hip_grid_neighbours(nbody_hip_grid* g, int k, int refine, int* index_dev, float* dist2_dev,
                                         double* rho_dev, int* status_dev) {
  if (!g) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null grid");
  nbody_hip_ctx* ctx = g->ctx;
  if (g->built_count == 0) return NBH_FAIL(NBODY_HIP_ERR_STATE, "grid has not been built");
  if (g->slab_nz > 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE,
                    "neighbours are found on single-GPU grids only: this grid holds a slab (nbody_hip_grid_set_slab)");
  switch (neigh_args(k, index_dev != nullptr, dist2_dev != nullptr, rho_dev != nullptr, status_dev != nullptr, refine)) {
    case kNeighArgsK:
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "k must lie in 1 .. %d, got %d", NBODY_HIP_NEIGHBOURS_MAX_K, k);
    case kNeighArgsNoOutput:
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "every output is NULL: nothing to compute");
    case kNeighArgsRefine:
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "a refining call reads the earlier status: status_dev may not be NULL");
    case kNeighArgsOk:
      break;
  }
  NBH_HIP(hipSetDevice(ctx->device));
  const int n = (int)g->built_count;
  const unsigned blocks = grid_blocks(n);
  const int* lb = g->lb_valid ? g->d_cell_lb : nullptr;
  const float cell2 = neigh_cell2(g->built_cell);
  const bool lists = index_dev != nullptr || dist2_dev != nullptr;
  with_int<4, 8, 16, 32>(neigh_pick_K(k), [&](auto KK) {
    with_flag(lists, [&](auto LS) {
      with_flag(rho_dev != nullptr, [&](auto RH) {
        hipLaunchKernelGGL((grid_neighbours_kernel<decltype(KK)::value, decltype(LS)::value, decltype(RH)::value>),
                           dim3(blocks), dim3(kBlock), 0, ctx->stream, g->d_sorted, g->d_keys_b, g->d_idx_b, lb, g->lb_base,
                           g->lb_count, n, g->info.dims[0], g->info.dims[1], g->info.dims[2], k, refine, cell2, index_dev,
                           dist2_dev, rho_dev, status_dev);
      });
    });
  });
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}
