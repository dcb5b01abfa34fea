// system_diag.hip -- ensemble diagnostics: per-system fp64 energies, momenta, closest and most bound pairs, ONE
// WORKGROUP PER SYSTEM in one launch (no reference counterpart).  The model is in include/nbody_hip.h
// (nbody_hip_system_diag) and DESIGN.md section 4.14; the arithmetic is system_diag_common.h, which the CPU program
// system_diag_check.cpp runs too.
//
// system_diag_kernel, grid = n_systems workgroups of 256 threads.  Workgroup s reads its two offsets, checks them
// (offsets[s] < offsets[s+1] <= count, at most 4,096 bodies; else status = 1, n = 0 and out) and moves first / n to
// scalar registers.  The bodies go through LDS in fp64 tiles of 512 ({X, V, m}: 56 bytes a body, 28 KiB a tile -- the
// 224 KiB of 4,096 bodies do not fit the 160 KiB of a compute unit); the thread that stores body k adds its terms to the
// per-body sums.  The n (n - 1) / 2 pairs are the cells of diag_cells, dealt to the threads in contiguous runs of
// q = ceil(ceil(n / 2) (n - 1) / 256): per tile a thread walks the rows of its run, holds the row's body (the target)
// in registers and takes the sources j of its cells from the tile, each pair i < j once.  Per thread: 12 fp64 sums and
// two (value, i, j) minima; they are reduced over the wave by shuffles at distances 32, 16, .., 1 and over the four
// waves in wave order by thread 0, which finishes the struct.  No atomics, no communication between workgroups, no wait
// on memory; every index is bounded by the validated n.

#include "common.h"
#include "system_diag.h"
#include "system_diag_common.h"

namespace nbh {

constexpr int kDiagThreads = 256;
constexpr int kDiagWaves = kDiagThreads / kWave;
constexpr int kDiagTile = 512;
constexpr int kDiagMaxN = NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX;
static_assert(sizeof(nbody_hip_system_diag) == 152, "nbody_hip_system_diag is 152 bytes (include/nbody_hip.h)");

struct DiagArgs {
  const float *x, *y, *z, *vx, *vy, *vz, *m;
  DiagLo lo;                           // a handle's residuals (null pointers: none)
  const float4 *pos_lo4, *vel_lo4;     // or rows {lx, ly, lz, 0} (null: none)
  const unsigned long long* offsets;   // n_systems + 1 entries; null: the one system [0, single_n)
  unsigned long long single_n, count;
  double G, eps2;
  nbody_hip_system_diag* out;
};

__device__ __forceinline__ int diag_uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long diag_uniform_u64(unsigned long long v) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

// body g of the particle data (g < count: the caller's index is first + k with k < n)
__device__ __forceinline__ DiagBody diag_load(const DiagArgs& A, size_t g) {
  float lx = 0.f, ly = 0.f, lz = 0.f, ux = 0.f, uy = 0.f, uz = 0.f;
  if (A.pos_lo4) {  // (uniform)
    const float4 l = A.pos_lo4[g];
    lx = l.x; ly = l.y; lz = l.z;
  } else if (A.lo.x) {
    lx = A.lo.x[g]; ly = A.lo.y[g]; lz = A.lo.z[g];
  }
  if (A.vel_lo4) {
    const float4 l = A.vel_lo4[g];
    ux = l.x; uy = l.y; uz = l.z;
  } else if (A.lo.vx) {
    ux = A.lo.vx[g]; uy = A.lo.vy[g]; uz = A.lo.vz[g];
  }
  return diag_body(A.x[g], A.y[g], A.z[g], lx, ly, lz, A.vx[g], A.vy[g], A.vz[g], ux, uy, uz, A.m[g]);
}

__device__ __forceinline__ DiagMin diag_min_shfl_down(const DiagMin& m, int off) {
  DiagMin o;
  o.v = __shfl_down(m.v, off, kWave);
  o.i = __shfl_down(m.i, off, kWave);
  o.j = __shfl_down(m.j, off, kWave);
  return o;
}

__global__ __launch_bounds__(kDiagThreads) void system_diag_kernel(const DiagArgs A) {
  constexpr bool LIVE = false;
  const unsigned int* const live = nullptr;  // (never read: LIVE is false)
  constexpr int live_stride = 0;
  // the included text reads exactly these names, which must be in scope here: A (DiagArgs), LIVE and, when LIVE, live and
  // live_stride
#include "system_diag_body.inc"
}

// the form with per-system live counts (ensemble MERGERS): system s is the first
// live[s * live_stride] bodies of its range
__global__ __launch_bounds__(kDiagThreads) void system_diag_live_kernel(const DiagArgs A,
                                                                         const unsigned int* __restrict__ live,
                                                                         const int live_stride) {
  constexpr bool LIVE = true;
  // the included text reads exactly these names, which must be in scope here: A (DiagArgs), LIVE and, when LIVE, live and
  // live_stride
#include "system_diag_body.inc"
}

int system_diag_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const DiagLo* lo, const float4* pos_lo4,
                       const float4* vel_lo4, const unsigned long long* offsets_device, size_t n_systems, float G, float eps,
                       nbody_hip_system_diag* out_device, const unsigned int* live_device, int live_stride) {
  if (n_systems == 0) return NBODY_HIP_OK;
  if (n_systems > 0x7fffffffu) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 1 systems");
  DiagArgs A;
  A.x = d->pos_x; A.y = d->pos_y; A.z = d->pos_z;
  A.vx = d->vel_x; A.vy = d->vel_y; A.vz = d->vel_z;
  A.m = d->mass;
  A.lo = lo ? *lo : DiagLo{};
  A.pos_lo4 = pos_lo4;
  A.vel_lo4 = vel_lo4;
  A.offsets = offsets_device;
  A.single_n = offsets_device ? 0ull : (unsigned long long)d->count;
  A.count = (unsigned long long)d->count;
  A.G = (double)G;
  A.eps2 = (double)(eps * eps);  // the fp32 product
  A.out = out_device;
  NBH_HIP(hipSetDevice(ctx->device));
  if (live_device)
    hipLaunchKernelGGL(system_diag_live_kernel, dim3((unsigned int)n_systems), dim3(kDiagThreads), 0, ctx->stream, A,
                       live_device, live_stride);
  else
    hipLaunchKernelGGL(system_diag_kernel, dim3((unsigned int)n_systems), dim3(kDiagThreads), 0, ctx->stream, A);
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

}  // namespace nbh

using namespace nbh;

extern "C" int nbody_hip_systems_diagnostics(nbody_hip_ctx* ctx, const nbody_particle_data* d,
                                             const nbody_float4* pos_lo_or_null, const nbody_float4* vel_lo_or_null,
                                             const unsigned long long* offsets_device, size_t n_systems, float G, float eps,
                                             nbody_hip_system_diag* out_device) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (!offsets_device) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null offsets array");
  if (!out_device) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  if (!d->pos_x || !d->pos_y || !d->pos_z || !d->vel_x || !d->vel_y || !d->vel_z || !d->mass)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null arrays");
  if (n_systems == 0) return NBODY_HIP_OK;
  if (d->count == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (d->count > 0x3fffffffu) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "body count exceeds 2^30");
  if (!(eps >= 0.0f)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Softening parameter must be non-negative");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, d->pos_x) != hipSuccess) {
    (void)hipGetLastError();  // memory the runtime does not know: the launch will tell
  } else if (at.type == hipMemoryTypeDevice && at.device != ctx->device) {
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle data lives on device %d, the context on device %d", at.device,
                    ctx->device);
  }
  return system_diag_launch(ctx, d, nullptr, reinterpret_cast<const float4*>(pos_lo_or_null),
                            reinterpret_cast<const float4*>(vel_lo_or_null), offsets_device, n_systems, G, eps, out_device);
}
