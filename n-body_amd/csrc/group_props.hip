// group_props.hip -- fp64 properties of the groups of a catalogue, for groups of any size (no reference counterpart).
// The model is in include/nbody_hip_group_props.h (nbody_hip_group_props) and DESIGN.md section 4.26; the per-member
// arithmetic is group_props_common.h, which the CPU program group_props_check.cpp runs too; the sizes, the launch
// bounds and the workspace table are group_props_plan.h (group_props_plan_check.cpp).  This file is built with
// -ffp-contract=off (Makefile): no product is fused into the add that takes it.
//
// A gather-bound pass: per member one index and seven floats (eight with phi) from wherever the body lies, twice.
//   group_props_count_kernel    one lane per group: the range check (bad[g]) and the group's chunk count
//   rocprim::exclusive_scan     chunk_start[g] = chunks before group g; chunk_start[n_groups] = chunks of the call
//   group_props_small_kernel    one lane per group of at most S members: both passes serially, the whole struct
//   group_props_chunk_kernel<1> one workgroup per chunk (grid stride): the chunk's owner by binary search in
//                               chunk_start, 4 members per thread, a shuffle tree per wave, the four waves in order
//   group_props_combine_kernel<1>  one wave per group in the chunked form: its chunk partials, then X and V
//   group_props_chunk_kernel<2>, group_props_combine_kernel<2>  the same about X and V; the struct
// Launch sizes come from n_groups and n_members alone (group_props_plan), so nothing is read back.  A member index is
// checked before it is used as one; a bad one raises bad[g] by an integer atomicOr (order independent) and is skipped.
// Chunk numbers are below the plan's chunk_cap wherever a partial record is written or read.

#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "group_props_common.h"
#include "group_props_plan.h"

namespace nbh {

static_assert(sizeof(nbody_hip_group_props) == 192, "nbody_hip_group_props is 192 bytes (include/nbody_hip_group_props.h)");
static_assert(kGroupPartialDoubles >= kGroupSums2 + 3 && kGroupPartialDoubles >= kGroupSums1, "partial record");
constexpr int kGroupWaves = kGroupThreads / kWave;

struct GroupArgs {
  const float *x, *y, *z, *vx, *vy, *vz, *m, *phi;  // phi null: none
  const int *offsets, *members;
  long long n_groups, n_members, chunk_cap;
  int count;
  int *nchunks, *chunk_start, *bad;
  double* partials;
  nbody_hip_group_props* out;
};

// chunk counts saturate instead of wrapping: only overlapping ranges can reach the cap, and a saturated start is beyond
// chunk_cap, which marks the group bad
struct GroupSatAdd {
  __host__ __device__ int operator()(int a, int b) const {
    const long long s = (long long)a + (long long)b;
    return s > 0x7fffffffLL ? 0x7fffffff : (int)s;
  }
};

__device__ __forceinline__ bool group_index_ok(int i, int count) { return (unsigned int)i < (unsigned int)count; }

__device__ __forceinline__ GroupBody group_load(const GroupArgs& A, int i) {
  return group_body(A.x[i], A.y[i], A.z[i], A.vx[i], A.vy[i], A.vz[i], A.m[i]);
}

__global__ __launch_bounds__(kGroupThreads) void group_props_count_kernel(const GroupArgs A) {
  const long long g = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (g > A.n_groups) return;
  if (g == A.n_groups) {  // (the scan's last entry: the chunks of the call)
    A.nchunks[g] = 0;
    return;
  }
  const long long o0 = A.offsets[g], o1 = A.offsets[g + 1];
  const bool legal = o0 >= 0 && o0 < o1 && o1 <= A.n_members;
  A.nchunks[g] = legal ? group_chunks(o1 - o0) : 0;
  A.bad[g] = legal ? 0 : 1;
}

__global__ __launch_bounds__(kGroupThreads) void group_props_small_kernel(const GroupArgs A) {
  const long long g = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (g >= A.n_groups) return;
  if (A.bad[g]) {
    A.out[g] = group_props_bad();
    return;
  }
  const long long o0 = A.offsets[g];
  const int n = (int)(A.offsets[g + 1] - o0);  // 1 <= n: the range is legal
  if (n > kGroupSmall) {
    if ((long long)A.chunk_start[g] + A.nchunks[g] > A.chunk_cap) {  // (overlapping ranges only: group_props_plan.h)
      A.bad[g] = 1;
      A.out[g] = group_props_bad();
    }
    return;
  }
  const bool has_phi = A.phi != nullptr;
  GroupSums1 s1;
  group_sums1_zero(s1);
  for (int p = 0; p < n; p++) {
    const int i = A.members[o0 + p];
    if (!group_index_ok(i, A.count)) {
      A.out[g] = group_props_bad();
      return;
    }
    group_sums1_add(s1, group_load(A, i));
  }
  const GroupCentre c = group_centre(s1);
  GroupSums2 s2;
  group_sums2_zero(s2);
  for (int p = 0; p < n; p++) {
    const int i = A.members[o0 + p];  // (checked by the first loop)
    group_sums2_add(s2, group_load(A, i), i, c, has_phi, has_phi ? A.phi[i] : 0.0f);
  }
  A.out[g] = group_props_finish(c, s2, n, A.members[o0], has_phi);
}

// the group that owns chunk c (0 <= c < chunk_start[n_groups]): the LAST g with chunk_start[g] <= c -- the groups
// without chunks that stand before it share its start, and chunk_start[g + 1] > c
__device__ __forceinline__ long long group_of_chunk(const int* __restrict__ chunk_start, long long n_groups, long long c) {
  long long lo = 0, hi = n_groups;  // chunk_start[lo] <= c < chunk_start[hi]
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if ((long long)chunk_start[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long group_chunk_total(const GroupArgs& A) {
  const long long t = A.chunk_start[A.n_groups];
  return t < A.chunk_cap ? t : A.chunk_cap;
}

__device__ __forceinline__ void group_wave_fold(GroupSums1& s) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    GroupSums1 o;
    for (int k = 0; k < kGroupSums1; k++) o.v[k] = __shfl_down(s.v[k], off, kWave);
    group_sums1_merge(s, o);
  }
}
__device__ __forceinline__ void group_wave_fold(GroupSums2& s) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    GroupSums2 o;
    for (int k = 0; k < kGroupSums2; k++) o.v[k] = __shfl_down(s.v[k], off, kWave);
    o.r2 = __shfl_down(s.r2, off, kWave);
    o.phi = __shfl_down(s.phi, off, kWave);
    o.r2_body = __shfl_down(s.r2_body, off, kWave);
    o.phi_body = __shfl_down(s.phi_body, off, kWave);
    group_sums2_merge(s, o);
  }
}

__device__ __forceinline__ void group_partial_store(double* __restrict__ rec, const GroupSums1& s) {
  for (int k = 0; k < kGroupSums1; k++) rec[k] = s.v[k];
}
__device__ __forceinline__ void group_partial_load(const double* __restrict__ rec, GroupSums1& s) {
  for (int k = 0; k < kGroupSums1; k++) s.v[k] = rec[k];
}
__device__ __forceinline__ void group_partial_store(double* __restrict__ rec, const GroupSums2& s) {
  for (int k = 0; k < kGroupSums2; k++) rec[k] = s.v[k];
  rec[kGroupSums2] = s.r2;
  rec[kGroupSums2 + 1] = s.phi;
  rec[kGroupSums2 + 2] = __longlong_as_double(((long long)s.r2_body << 32) | (long long)(unsigned int)s.phi_body);
}
__device__ __forceinline__ void group_partial_load(const double* __restrict__ rec, GroupSums2& s) {
  for (int k = 0; k < kGroupSums2; k++) s.v[k] = rec[k];
  s.r2 = rec[kGroupSums2];
  s.phi = rec[kGroupSums2 + 1];
  const long long bodies = __double_as_longlong(rec[kGroupSums2 + 2]);  // (moved as bits, never computed with)
  s.r2_body = (int)(bodies >> 32);
  s.phi_body = (int)(unsigned int)(bodies & 0xffffffffLL);
}

__device__ __forceinline__ void group_zero(GroupSums1& s) { group_sums1_zero(s); }
__device__ __forceinline__ void group_zero(GroupSums2& s) { group_sums2_zero(s); }
__device__ __forceinline__ void group_merge(GroupSums1& a, const GroupSums1& b) { group_sums1_merge(a, b); }
__device__ __forceinline__ void group_merge(GroupSums2& a, const GroupSums2& b) { group_sums2_merge(a, b); }

__device__ __forceinline__ GroupCentre group_centre_of(const nbody_hip_group_props& o) {
  GroupCentre c;
  c.mass = o.mass;
  for (int a = 0; a < 3; a++) {
    c.x[a] = o.com[a];
    c.v[a] = o.vel[a];
  }
  return c;
}

// PASS 1 or 2 over the chunks of the call.  Everything that decides a branch around a barrier (c, g, bad[g]) is the same
// in every thread of the workgroup: bad[] is only written by pass 1 and only read by the later kernels.
template <int PASS>
__global__ __launch_bounds__(kGroupThreads) void group_props_chunk_kernel(const GroupArgs A) {
  using Sums = typename std::conditional<PASS == 1, GroupSums1, GroupSums2>::type;
  __shared__ double wave_rec[kGroupWaves][kGroupPartialDoubles];
  const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const long long total = group_chunk_total(A);
  const bool has_phi = A.phi != nullptr;
  for (long long c = blockIdx.x; c < total; c += gridDim.x) {
    const long long g = group_of_chunk(A.chunk_start, A.n_groups, c);
    if (PASS == 2 && A.bad[g]) continue;
    const long long o0 = A.offsets[g], o1 = A.offsets[g + 1];  // a legal range: the group has chunks
    const long long base = o0 + (c - (long long)A.chunk_start[g]) * kGroupChunk;  // < o1: the chunk is one of the group's
    const long long end = base + kGroupChunk < o1 ? base + kGroupChunk : o1;
    GroupCentre centre = {};
    if (PASS == 2) centre = group_centre_of(A.out[g]);
    int idx[kGroupPerThread];
#pragma unroll
    for (int j = 0; j < kGroupPerThread; j++) {
      const long long p = base + (long long)j * kGroupThreads + t;
      idx[j] = p < end ? A.members[p] : -1;
    }
    Sums s;
    group_zero(s);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kGroupPerThread; j++) {
      const long long p = base + (long long)j * kGroupThreads + t;
      if (p >= end) continue;
      const int i = idx[j];
      if (!group_index_ok(i, A.count)) {  // (pass 2 never meets one: the group would be bad)
        bad = true;
        continue;
      }
      const GroupBody b = group_load(A, i);
      if constexpr (PASS == 1) group_sums1_add(s, b);
      else group_sums2_add(s, b, i, centre, has_phi, has_phi ? A.phi[i] : 0.0f);
    }
    if (PASS == 1 && bad) atomicOr(A.bad + g, 1);
    group_wave_fold(s);
    if (lane == 0) group_partial_store(wave_rec[wave], s);
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kGroupWaves; w++) {
        Sums o;
        group_partial_load(wave_rec[w], o);
        group_merge(s, o);
      }
      group_partial_store(A.partials + c * kGroupPartialDoubles, s);  // c < chunk_cap
    }
    __syncthreads();  // (wave_rec is written again by the next chunk)
  }
}

// One wave per chunk number; the wave that meets the FIRST chunk of a group folds the group's chunk partials.
template <int PASS>
__global__ __launch_bounds__(kGroupThreads) void group_props_combine_kernel(const GroupArgs A) {
  using Sums = typename std::conditional<PASS == 1, GroupSums1, GroupSums2>::type;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const long long total = group_chunk_total(A);
  const long long stride = (long long)gridDim.x * kGroupWaves;
  for (long long c = (long long)blockIdx.x * kGroupWaves + threadIdx.x / kWave; c < total; c += stride) {
    const long long g = group_of_chunk(A.chunk_start, A.n_groups, c);
    if ((long long)A.chunk_start[g] != c) continue;
    if (A.bad[g]) {
      if (PASS == 2 && lane == 0) A.out[g] = group_props_bad();
      continue;
    }
    const int nch = A.nchunks[g];  // c + nch <= chunk_cap: else the small kernel had marked the group bad
    Sums s;
    group_zero(s);
    for (int k = lane; k < nch; k += kWave) {
      Sums o;
      group_partial_load(A.partials + (c + k) * kGroupPartialDoubles, o);
      group_merge(s, o);
    }
    group_wave_fold(s);
    if (lane != 0) continue;
    if constexpr (PASS == 1) {
      const GroupCentre centre = group_centre(s);
      nbody_hip_group_props* const o = A.out + g;  // (kept here for pass 2; the struct is finished by pass 2)
      o->mass = centre.mass;
      for (int a = 0; a < 3; a++) {
        o->com[a] = centre.x[a];
        o->vel[a] = centre.v[a];
      }
    } else {
      const long long o0 = A.offsets[g];
      const GroupCentre centre = group_centre_of(A.out[g]);
      A.out[g] = group_props_finish(centre, s, (int)(A.offsets[g + 1] - o0), A.members[o0], A.phi != nullptr);
    }
  }
}

static int group_scan(void* tmp, size_t& bytes, int* in, int* out, size_t count, hipStream_t st) {
  return (int)rocprim::exclusive_scan(tmp, bytes, in, out, 0, count, GroupSatAdd(), st);
}

int group_props_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev, const int* members_dev,
                       long long n_groups, long long n_members, const float* phi_dev_or_null,
                       nbody_hip_group_props* out_dev) {
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (!d->pos_x || !d->pos_y || !d->pos_z || !d->vel_x || !d->vel_y || !d->vel_z || !d->mass)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null arrays");
  if (!offsets_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null offsets array");
  if (n_groups < 0 || n_members < 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "negative group or member count");
  if (n_members > kGroupMaxMembers) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 1 members");
  if (n_groups > kGroupMaxGroups) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 2 groups");
  if (n_groups == 0) return NBODY_HIP_OK;
  if (!members_dev && n_members > 0) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null members array");
  if (!out_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  if (d->count == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (d->count > 0x40000000u) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "body count exceeds 2^30");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, d->pos_x) != hipSuccess) {
    (void)hipGetLastError();  // memory the runtime does not know: the launch will tell
  } else if (at.type == hipMemoryTypeDevice && at.device != ctx->device) {
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle data lives on device %d, the context on device %d", at.device,
                    ctx->device);
  }
  NBH_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  size_t scan_bytes = 0;
  NBH_HIP((hipError_t)group_scan(nullptr, scan_bytes, nullptr, nullptr, (size_t)n_groups + 1, st));  // (a size query: no launch)
  const GroupPropsPlan p = group_props_plan(n_groups, n_members, scan_bytes);
  if (ctx->capturing && ctx->groups.bytes < p.bytes) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "group properties cannot be recorded into a step graph before their workspace "
                    "exists: run the call once eagerly with these sizes");
  }
  if (int rc = ctx->groups.reserve(p.bytes)) return rc;
  char* const ws = static_cast<char*>(ctx->groups.ptr);
  GroupArgs A;
  A.x = d->pos_x; A.y = d->pos_y; A.z = d->pos_z;
  A.vx = d->vel_x; A.vy = d->vel_y; A.vz = d->vel_z;
  A.m = d->mass;
  A.phi = phi_dev_or_null;
  A.offsets = offsets_dev;
  A.members = members_dev;
  A.n_groups = n_groups;
  A.n_members = n_members;
  A.chunk_cap = p.chunk_cap;
  A.count = (int)d->count;
  A.nchunks = reinterpret_cast<int*>(ws + p.off_nchunks);
  A.chunk_start = reinterpret_cast<int*>(ws + p.off_chunk_start);
  A.bad = reinterpret_cast<int*>(ws + p.off_bad);
  A.partials = reinterpret_cast<double*>(ws + p.off_partials);
  A.out = out_dev;
  hipLaunchKernelGGL(group_props_count_kernel, dim3(p.count_blocks), dim3(kGroupThreads), 0, st, A);
  NBH_LAUNCH_CHECK();
  NBH_HIP((hipError_t)group_scan(ws + p.off_scan_tmp, scan_bytes, A.nchunks, A.chunk_start, p.scan_count, st));
  hipLaunchKernelGGL(group_props_small_kernel, dim3(p.small_blocks), dim3(kGroupThreads), 0, st, A);
  if (p.chunk_blocks > 0) {
    hipLaunchKernelGGL(group_props_chunk_kernel<1>, dim3(p.chunk_blocks), dim3(kGroupThreads), 0, st, A);
    hipLaunchKernelGGL(group_props_combine_kernel<1>, dim3(p.combine_blocks), dim3(kGroupThreads), 0, st, A);
    hipLaunchKernelGGL(group_props_chunk_kernel<2>, dim3(p.chunk_blocks), dim3(kGroupThreads), 0, st, A);
    hipLaunchKernelGGL(group_props_combine_kernel<2>, dim3(p.combine_blocks), dim3(kGroupThreads), 0, st, A);
  }
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

}  // namespace nbh

using namespace nbh;

extern "C" int nbody_hip_groups_properties(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev,
                                           const int* members_dev, long long n_groups, long long n_members,
                                           const float* phi_dev_or_null, nbody_hip_group_props* out_dev) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  return group_props_launch(ctx, d, offsets_dev, members_dev, n_groups, n_members, phi_dev_or_null, out_dev);
}
