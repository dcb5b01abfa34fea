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
  __shared__ double tile[7][kDiagTile];
  __shared__ double wave_sum[kDiagWaves][kDiagSums];
  __shared__ DiagMin wave_min[kDiagWaves][2];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  nbody_hip_system_diag* const out = A.out + s;

  // the system's range, checked before anything is indexed by it
  unsigned long long o0 = 0ull, o1 = A.single_n;
  if (A.offsets) {
    o0 = A.offsets[s];
    o1 = A.offsets[s + 1];
  }
  o0 = diag_uniform_u64(o0);
  o1 = diag_uniform_u64(o1);
  if (!(o0 < o1 && o1 <= A.count && o1 - o0 <= (unsigned long long)kDiagMaxN)) {  // (uniform)
    if (tid == 0) {
      out->n = 0;
      out->status = 1;
    }
    return;
  }
  const size_t first = (size_t)o0;
  const int n = diag_uniform_i((int)(o1 - o0));  // 1 <= n <= 4,096

  const DiagCells cells = diag_cells(n, kDiagThreads);
  int a, b, r0, r1;
  diag_worker_cells(cells, tid, &a, &b, &r0, &r1);

  DiagSums sums;
  diag_sums_zero(sums);
  DiagMin sep = diag_min_none(INFINITY), bind = diag_min_none(0.0);

  for (int t0 = 0; t0 < n; t0 += kDiagTile) {  // (uniform trip count: the barriers)
    const int t1 = min(t0 + kDiagTile, n);
    if (t0 != 0) __syncthreads();  // the last tile has been read
    for (int k = t0 + tid; k < t1; k += kDiagThreads) {
      const DiagBody q = diag_load(A, first + (size_t)k);
      const int e = k - t0;
      tile[0][e] = q.x; tile[1][e] = q.y; tile[2][e] = q.z;
      tile[3][e] = q.vx; tile[4][e] = q.vy; tile[5][e] = q.vz;
      tile[6][e] = q.m;
      diag_body_add(sums, q);
    }
    __syncthreads();
    for (int r = r0; r < r1; r++) {
      DiagRun run[2];
      diag_row_runs(cells, a, b, r, t0, t1, &run[0], &run[1]);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (run[h].jlo >= run[h].jhi) continue;
        const int i = run[h].i;  // i < n
        const DiagBody ti = diag_load(A, first + (size_t)i);
        for (int j = run[h].jlo; j < run[h].jhi; j++) {  // t0 <= j < t1
          const int e = j - t0;
          const DiagBody sj{tile[0][e], tile[1][e], tile[2][e], tile[3][e], tile[4][e], tile[5][e], tile[6][e]};
          const DiagPair p = diag_pair(ti, sj, A.G, A.eps2);
          sums.v[kDiagSums - 1] += p.term;
          diag_min_take(sep, p.r, i, j);
          if (p.bindable) diag_min_take(bind, p.eb, i, j);
        }
      }
    }
  }

  // the wave: lane l takes lane l + off at off = 32, 16, .., 1; then the four waves in order
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) sums.v[k] += __shfl_down(sums.v[k], off, kWave);
    diag_min_merge(sep, diag_min_shfl_down(sep, off));
    diag_min_merge(bind, diag_min_shfl_down(bind, off));
  }
  if ((tid & (kWave - 1)) == 0) {
    const int w = tid / kWave;
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) wave_sum[w][k] = sums.v[k];
    wave_min[w][0] = sep;
    wave_min[w][1] = bind;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < kDiagWaves; w++) {
#pragma unroll
    for (int k = 0; k < kDiagSums; k++) sums.v[k] += wave_sum[w][k];
    diag_min_merge(sep, wave_min[w][0]);
    diag_min_merge(bind, wave_min[w][1]);
  }
  DiagBody bi{}, bj{};
  if (bind.i >= 0 && bind.v < 0.0) {  // 0 <= bind.i < bind.j < n
    bi = diag_load(A, first + (size_t)bind.i);
    bj = diag_load(A, first + (size_t)bind.j);
  }
  diag_finish(sums, sep, bind, bi, bj, A.G, n, out);
}

int system_diag_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const DiagLo* lo, const float4* pos_lo4,
                       const float4* vel_lo4, const unsigned long long* offsets_device, size_t n_systems, float G, float eps,
                       nbody_hip_system_diag* out_device) {
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
