// density_centre.hip -- the density centre and the core radius of one set of bodies (include/nbody_hip_neighbours.h:
// nbody_hip_density_centre), in fp64, in the summation order nbody_hip_group_props.h defines.
// The per-body terms and the merges are neighbours_common.h, which the CPU program neighbours_check.cpp runs too.  This
// file is built with -ffp-contract=off (Makefile): no product is fused into the add that takes it.
//
//   n <= 32:  centre_small_kernel     one lane: both passes in turn, the struct
//   n > 32:   centre_chunk_kernel<1>  one workgroup per chunk of 1,024 positions (grid stride): 4 positions per thread, a
//                                     shuffle tree per wave, the four waves in order; a bad index raises the flag
//             centre_fold_kernel<1>   one wave: the chunk sums l, l + 64, .. per lane, the shuffle tree; x_d
//             centre_chunk_kernel<2>, centre_fold_kernel<2>   the same about x_d; the struct
// A member index is checked before it is used as one.  The flag is an int raised by atomicOr (order independent).

#include "common.h"
#include "neighbours_common.h"

namespace nbh {

static_assert(sizeof(nbody_hip_density_centre_t) == 64, "nbody_hip_density_centre_t is 64 bytes");
constexpr int kCentreWaves = kCentreThreads / kWave;
constexpr long long kCentreMaxBlocks = 4096;

struct CentreArgs {
  const float *x, *y, *z;
  const double* rho;
  const int* members;  // null: the bodies 0 .. n - 1
  long long n, chunks;
  int count;
  double* partials;    // chunks * kCentreSums
  CentrePoint* point;  // pass 1's result, read by pass 2
  int* bad;
  nbody_hip_density_centre_t* out;
};

// the body at position p, or -1 for an index outside [0, count)
__device__ __forceinline__ int centre_body(const CentreArgs& A, long long p) {
  const int i = A.members ? A.members[p] : (int)p;
  return (unsigned int)i < (unsigned int)A.count ? i : -1;
}

__device__ __forceinline__ void centre_wave_fold(CentreSums& s) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    CentreSums o;
    for (int a = 0; a < kCentreSums; a++) o.v[a] = __shfl_down(s.v[a], off, kWave);
    centre_merge(s, o);
  }
}

__global__ void centre_small_kernel(const CentreArgs A) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int n = (int)A.n;  // <= kCentreSmall
  CentreSums s1, s2;
  centre_zero(s1);
  centre_zero(s2);
  for (int p = 0; p < n; p++) {
    const int i = centre_body(A, p);
    if (i < 0) {
      *A.out = centre_bad();
      return;
    }
    centre_add1(s1, A.rho[i], A.x[i], A.y[i], A.z[i]);
  }
  const CentrePoint c = centre_point(s1);
  for (int p = 0; p < n; p++) {
    const int i = centre_body(A, p);  // (checked by the first loop)
    centre_add2(s2, A.rho[i], A.x[i], A.y[i], A.z[i], c);
  }
  *A.out = centre_finish(c, s2, n);
}

// Everything that decides a branch around a barrier is the same in every thread of the workgroup.
template <int PASS>
__global__ __launch_bounds__(kCentreThreads) void centre_chunk_kernel(const CentreArgs A) {
  __shared__ double wave_rec[kCentreWaves][kCentreSums];
  const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  CentrePoint c = {};
  if (PASS == 2) c = *A.point;
  for (long long ch = blockIdx.x; ch < A.chunks; ch += gridDim.x) {
    const long long base = ch * kCentreChunk;
    const long long end = base + kCentreChunk < A.n ? base + kCentreChunk : A.n;
    CentreSums s;
    centre_zero(s);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kCentrePerThread; j++) {
      const long long p = base + (long long)j * kCentreThreads + t;
      if (p >= end) continue;
      const int i = centre_body(A, p);
      if (i < 0) {
        bad = true;
        continue;
      }
      if constexpr (PASS == 1) centre_add1(s, A.rho[i], A.x[i], A.y[i], A.z[i]);
      else centre_add2(s, A.rho[i], A.x[i], A.y[i], A.z[i], c);
    }
    if (PASS == 1 && bad) atomicOr(A.bad, 1);
    centre_wave_fold(s);
    if (lane == 0)
      for (int a = 0; a < kCentreSums; a++) wave_rec[wave][a] = s.v[a];
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kCentreWaves; w++) {
        CentreSums o;
        for (int a = 0; a < kCentreSums; a++) o.v[a] = wave_rec[w][a];
        centre_merge(s, o);
      }
      for (int a = 0; a < kCentreSums; a++) A.partials[ch * kCentreSums + a] = s.v[a];  // ch < chunks
    }
    __syncthreads();  // (wave_rec is written again by the next chunk)
  }
}

// one wave
template <int PASS>
__global__ __launch_bounds__(kWave) void centre_fold_kernel(const CentreArgs A) {
  if (blockIdx.x != 0) return;
  const int lane = (int)threadIdx.x;
  CentreSums s;
  centre_zero(s);
  for (long long ch = lane; ch < A.chunks; ch += kWave) {
    CentreSums o;
    for (int a = 0; a < kCentreSums; a++) o.v[a] = A.partials[ch * kCentreSums + a];
    centre_merge(s, o);
  }
  centre_wave_fold(s);
  if (lane != 0) return;
  if constexpr (PASS == 1) {
    *A.point = centre_point(s);
  } else {
    *A.out = *A.bad ? centre_bad() : centre_finish(*A.point, s, (int)A.n);
  }
}

}  // namespace nbh

using namespace nbh;

extern "C" int nbody_hip_density_centre(nbody_hip_ctx* ctx, const nbody_particle_data* d, const double* rho_dev,
                                        const int* members_dev_or_null, long long n_members,
                                        nbody_hip_density_centre_t* out_dev) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (!d->pos_x || !d->pos_y || !d->pos_z) return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null position arrays");
  if (!rho_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null rho array");
  if (!out_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  if (d->count == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (d->count > 0x40000000u) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "body count exceeds 2^30");
  const long long n = members_dev_or_null ? n_members : (long long)d->count;
  if (n < 0 || n > 0x7fffffffLL) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "n_members must lie in 0 .. 2^31 - 1");
  NBH_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  CentreArgs A = {};
  A.x = d->pos_x; A.y = d->pos_y; A.z = d->pos_z;
  A.rho = rho_dev;
  A.members = members_dev_or_null;
  A.n = n;
  A.count = (int)d->count;
  A.out = out_dev;
  if (n <= kCentreSmall) {
    hipLaunchKernelGGL(centre_small_kernel, dim3(1), dim3(kWave), 0, st, A);
    NBH_LAUNCH_CHECK();
    return NBODY_HIP_OK;
  }
  A.chunks = centre_chunks(n);
  // the workspace: the flag and the centre of pass 1 in the first 64 bytes, then the chunk sums
  const size_t bytes = 64 + (size_t)A.chunks * kCentreSums * sizeof(double);
  static_assert(sizeof(CentrePoint) + sizeof(int) <= 64, "the head of the workspace");
  if (ctx->capturing && ctx->centre.bytes < bytes) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "a density centre cannot be recorded into a step graph before its workspace "
                    "exists: run the call once eagerly with this size");
  }
  if (int rc = ctx->centre.reserve(bytes)) return rc;
  char* const ws = static_cast<char*>(ctx->centre.ptr);
  A.point = reinterpret_cast<CentrePoint*>(ws);
  A.bad = reinterpret_cast<int*>(ws + sizeof(CentrePoint));
  A.partials = reinterpret_cast<double*>(ws + 64);
  NBH_HIP(hipMemsetAsync(A.bad, 0, sizeof(int), st));
  const unsigned blocks = (unsigned)(A.chunks < kCentreMaxBlocks ? A.chunks : kCentreMaxBlocks);
  hipLaunchKernelGGL(centre_chunk_kernel<1>, dim3(blocks), dim3(kCentreThreads), 0, st, A);
  hipLaunchKernelGGL(centre_fold_kernel<1>, dim3(1), dim3(kWave), 0, st, A);
  hipLaunchKernelGGL(centre_chunk_kernel<2>, dim3(blocks), dim3(kCentreThreads), 0, st, A);
  hipLaunchKernelGGL(centre_fold_kernel<2>, dim3(1), dim3(kWave), 0, st, A);
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}
