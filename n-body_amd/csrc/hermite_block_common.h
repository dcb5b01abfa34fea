// hermite_block_common.h -- the device bodies the block-step Hermite integrator (hermite_block.hip) and its ensemble form
// (hermite_batch.hip) share: the level rules, the three bodies of the narrow sweep and the finalize of one active body.
// One definition each: an ensemble's system is advanced by the expressions of the single-system resident form, in the
// same order, which is the whole of their bit equality (DESIGN.md sections 4.10, 4.12, 4.13).
#pragma once

#include <cmath>

#include "hermite_common.h"

namespace nbh {

constexpr unsigned int kTickNone = 0xffffffffu;
constexpr int kMaxLevel = 20;
constexpr int kNarrowS = 4;   // sources per lane of the narrow form: a block sweeps 1,024 sources
constexpr int kNarrowT = 4;   // targets per block of the narrow form
// counters on the device: level_steps[0..20], floor_hits
constexpr int kCounters = kMaxLevel + 2;
// the resident forms: one workgroup of 512 threads, two 256-lane sub-blocks (hermite_block.hip)
constexpr int kResidentBlock = 512;
constexpr int kResidentSub = kResidentBlock / kBlock;  // 256-lane sub-blocks

// fp64 expressions of the level rules as the restatement (tests/hermite_block_ref.py) forms them: every operation
// rounded on its own, in the order written
__device__ __forceinline__ double norm2_3(double x, double y, double z) {
#pragma clang fp contract(off)
  return x * x + y * y + z * z;
}

// smallest level whose step is not longer than `want`, from level k upwards
__device__ __forceinline__ int level_for(double want, double dt_max, int k, int L) {
#pragma clang fp contract(off)
  while (k < L && want < dt_max / (double)(1u << k)) k++;
  return k;
}

// Priming of one body from its (a, j): want = eta_s |a| / |j| (+inf when |j| = 0) and the smallest level with
// dt_max 2^-k <= want.  The expressions of block_prime_kernel (hermite_block.hip), which keeps its own copy.
__device__ __forceinline__ int block_prime_level(const float ax, const float ay, const float az, const float4 j,
                                                 const float eta_s, const float dt_max, const int L, float* want_out) {
#pragma clang fp contract(off)
  const double na = sqrt(norm2_3((double)ax, (double)ay, (double)az));
  const double nj = sqrt(norm2_3((double)j.x, (double)j.y, (double)j.z));
  const double w = nj > 0.0 ? ((double)eta_s * na) / nj : (double)INFINITY;
  *want_out = (float)w;
  return level_for(w, (double)dt_max, 0, L);
}

// ---------------------------------------------------------------------------------
// The three bodies of the narrow form (the lane's sources, one target against them, the row), shared by
// direct_jerk_active_narrow_kernel and the resident forms, whose 256-lane sub-blocks run them in the same order.
// ---------------------------------------------------------------------------------
// the lane's sources of source block j0 / 1024: {xp, m}, {vp, 0} and, in extended state precision, {xp_lo, 0}
template <bool EXT>
__device__ __forceinline__ void narrow_load_sources(const float4* posm, const float4* vel, const float4* plo, const int j0,
                                                    const int lane, const int n, float4 (&sp)[kNarrowS],
                                                    float4 (&sv)[kNarrowS], float4 (&sl)[kNarrowS]) {
#pragma unroll
  for (int s = 0; s < kNarrowS; s++) {
    const int j = j0 + s * kBlock + lane;
    sp[s] = sv[s] = sl[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n) {
      sp[s] = posm[j];
      sv[s] = vel[j];
      if constexpr (EXT) sl[s] = plo[j];
    }
  }
}

struct NarrowSums { double v[6]; };

// one target against the lane's sources: fp32 sums over them, then fp64 over the wave (xor butterfly): v = {a, j} of the
// wave, in every lane.  EXT: d = (hi_j - hi_i) + (lo_j - lo_i) (hermite_common.h), the rest is the same.
template <bool GUARD, bool EXT>
__device__ __forceinline__ NarrowSums narrow_target(const float4 (&sp)[kNarrowS], const float4 (&sv)[kNarrowS],
                                              const float4 (&sl)[kNarrowS], const float4 tp, const float4 tv,
                                              const float4 tl, const float eps2) {
  float a[3] = {0.f, 0.f, 0.f}, jj[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < kNarrowS; s++) {
    float dx, dy, dz;
    if constexpr (EXT) {
      dx = (sp[s].x - tp.x) + (sl[s].x - tl.x);
      dy = (sp[s].y - tp.y) + (sl[s].y - tl.y);
      dz = (sp[s].z - tp.z) + (sl[s].z - tl.z);
    } else {
      dx = sp[s].x - tp.x;
      dy = sp[s].y - tp.y;
      dz = sp[s].z - tp.z;
    }
    const float wx = sv[s].x - tv.x, wy = sv[s].y - tv.y, wz = sv[s].z - tv.z;
    const float dw = __builtin_fmaf(dx, wx, __builtin_fmaf(dy, wy, dz * wz));
    float inv;
    if constexpr (GUARD) {
      const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
      inv = d2 > 0.0f ? rsq(d2 + eps2) : 0.0f;
    } else {
      inv = rsq(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, eps2))));
    }
    const float inv2 = inv * inv;
    const float f = (sp[s].w * inv) * inv2;
    const float qq = (dw * inv2) * -3.0f;
    a[0] = __builtin_fmaf(f, dx, a[0]);
    a[1] = __builtin_fmaf(f, dy, a[1]);
    a[2] = __builtin_fmaf(f, dz, a[2]);
    jj[0] = __builtin_fmaf(f, __builtin_fmaf(qq, dx, wx), jj[0]);
    jj[1] = __builtin_fmaf(f, __builtin_fmaf(qq, dy, wy), jj[1]);
    jj[2] = __builtin_fmaf(f, __builtin_fmaf(qq, dz, wz), jj[2]);
  }
  double v[6] = {(double)a[0], (double)a[1], (double)a[2], (double)jj[0], (double)jj[1], (double)jj[2]};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] += __shfl_xor(v[c], off, 64);
  }
  return NarrowSums{{v[0], v[1], v[2], v[3], v[4], v[5]}};
}

// ---------------------------------------------------------------------------------
// The TRACKED sweep body of the ensemble's event form (batch_resident_events_kernel): the a and
// j expressions of narrow_target in its order -- a copy, so that narrow_target keeps its instruction stream -- and, beside
// them, the separation of every SEEN pair folded into two lane-local minima of 64-bit keys.
//   d2  = fma(dx, dx, fma(dy, dy, dz dz)) of the differences the force terms use (the GUARD form's own d2)
//   seen: j < n (no padded source), j != i as an index (a coincident pair of two bodies counts), d2 finite
//   key = bits(d2) << 32 | i << 12 | j, system-local indices; d2 >= 0, so the keys order as d2, then i, then j
//   contact: rs = r_i + r_j in fp32, rs > 0 and d2 < rs rs
// A minimum of unsigned integers depends on no lane, wave or sub-block order.
// ---------------------------------------------------------------------------------
constexpr unsigned long long kKeyNone = ~0ull;  // no pair: above every key (bits(d2) of a finite d2 < 0x7f800000)

__device__ __forceinline__ unsigned long long pair_key(const float d2, const int i, const int j) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | ((unsigned long long)(unsigned int)i << 12) |
         (unsigned long long)(unsigned int)j;
}

// the radii of the lane's sources of source block j0 / 1024 (narrow_load_sources' indices); padded source: 0
__device__ __forceinline__ void narrow_load_radii(const float* radii, const int j0, const int lane, const int n,
                                                  float (&sr)[kNarrowS]) {
#pragma unroll
  for (int s = 0; s < kNarrowS; s++) {
    const int j = j0 + s * kBlock + lane;
    sr[s] = j < n ? radii[j] : 0.f;
  }
}

// the minimum of a key over the wave, in every lane
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long k) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(k, off, 64);
    k = o < k ? o : k;
  }
  return k;
}

// target i (radius tr) against the lane's sources j0 + s 256 + lane (radii sr): narrow_target's sums, and the lane's
// minima of the keys of the seen pairs (closest) and of those in contact (contact) carried on
template <bool GUARD, bool EXT>
__device__ __forceinline__ NarrowSums narrow_target_track(const float4 (&sp)[kNarrowS], const float4 (&sv)[kNarrowS],
                                                          const float4 (&sl)[kNarrowS], const float (&sr)[kNarrowS],
                                                          const float4 tp, const float4 tv, const float4 tl,
                                                          const float tr, const int i, const int j0, const int lane,
                                                          const int n, const float eps2, unsigned long long& closest,
                                                          unsigned long long& contact) {
  float a[3] = {0.f, 0.f, 0.f}, jj[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < kNarrowS; s++) {
    float dx, dy, dz;
    if constexpr (EXT) {
      dx = (sp[s].x - tp.x) + (sl[s].x - tl.x);
      dy = (sp[s].y - tp.y) + (sl[s].y - tl.y);
      dz = (sp[s].z - tp.z) + (sl[s].z - tl.z);
    } else {
      dx = sp[s].x - tp.x;
      dy = sp[s].y - tp.y;
      dz = sp[s].z - tp.z;
    }
    const float wx = sv[s].x - tv.x, wy = sv[s].y - tv.y, wz = sv[s].z - tv.z;
    const float dw = __builtin_fmaf(dx, wx, __builtin_fmaf(dy, wy, dz * wz));
    const float d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    float inv;
    if constexpr (GUARD) {
      inv = d2 > 0.0f ? rsq(d2 + eps2) : 0.0f;
    } else {
      inv = rsq(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, eps2))));
    }
    const float inv2 = inv * inv;
    const float f = (sp[s].w * inv) * inv2;
    const float qq = (dw * inv2) * -3.0f;
    a[0] = __builtin_fmaf(f, dx, a[0]);
    a[1] = __builtin_fmaf(f, dy, a[1]);
    a[2] = __builtin_fmaf(f, dz, a[2]);
    jj[0] = __builtin_fmaf(f, __builtin_fmaf(qq, dx, wx), jj[0]);
    jj[1] = __builtin_fmaf(f, __builtin_fmaf(qq, dy, wy), jj[1]);
    jj[2] = __builtin_fmaf(f, __builtin_fmaf(qq, dz, wz), jj[2]);
    // the pair (i, j): beside the force terms, nothing of it enters them
    const int j = j0 + s * kBlock + lane;
    if (j < n && j != i && d2 < __builtin_inff()) {  // (a NaN compares false)
      const unsigned long long key = pair_key(d2, i, j);
      closest = key < closest ? key : closest;
      const float rs = tr + sr[s];
      if (rs > 0.0f && d2 < rs * rs) contact = key < contact ? key : contact;
    }
  }
  double v[6] = {(double)a[0], (double)a[1], (double)a[2], (double)jj[0], (double)jj[1], (double)jj[2]};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] += __shfl_xor(v[c], off, 64);
  }
  return NarrowSums{{v[0], v[1], v[2], v[3], v[4], v[5]}};
}

// one component of the row of a (source block, target): the four waves' sums added in wave order (the caller rounds)
__device__ __forceinline__ double narrow_row(const double (&red)[kBlock / kWave]) {
  double s = red[0];
#pragma unroll
  for (int w = 1; w < kBlock / kWave; w++) s += red[w];
  return s;
}

// The new level of a body corrected at tick t over h = dt_max 2^-k from (a0, j0) to (a1, j1): the Aarseth criterion
// on the second and third derivatives the Hermite interpolation gives at the END of the step.  All fp32 values taken
// in fp64; *want_out the step the criterion asks for (+inf when its denominator is 0); *floor_hit set when level L is
// still too long.
__device__ __forceinline__ int block_new_level(const double (&a0)[3], const double (&j0)[3], const double (&a1)[3],
                                               const double (&j1)[3], double h, double dt_max, double eta, int k, int L,
                                               unsigned int t, double* want_out, bool* floor_hit) {
#pragma clang fp contract(off)
  double a2[3], a3[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double da = a0[c] - a1[c];
    a2[c] = (-6.0 * da - h * (4.0 * j0[c] + 2.0 * j1[c])) / (h * h);
    a3[c] = (12.0 * da + 6.0 * h * (j0[c] + j1[c])) / (h * h * h);
    a2[c] = a2[c] + h * a3[c];
  }
  const double a1s = norm2_3(a1[0], a1[1], a1[2]), j1s = norm2_3(j1[0], j1[1], j1[2]);
  const double a2s = norm2_3(a2[0], a2[1], a2[2]), a3s = norm2_3(a3[0], a3[1], a3[2]);
  const double num = eta * (sqrt(a1s) * sqrt(a2s) + j1s);
  const double den = sqrt(j1s) * sqrt(a3s) + a2s;
  const double want = den == 0.0 ? (double)INFINITY : sqrt(num / den);
  *want_out = want;
  *floor_hit = false;
  if (want < h) {
    k = level_for(want, dt_max, k, L);
    *floor_hit = want < dt_max / (double)(1u << k);
  } else if (want >= 2.0 * h && k > 0 && (t % (2u << (L - k))) == 0u) {
    k--;
  }
  return k;
}

// Finalize of active body i = list[k]: a1 = G sum_splits pa, j1 = G sum_splits pj (fp64, split order), rounded to fp32;
// the corrector over the body's own step; acc_old <- a, acc <- a1, jerk <- j1, tick <- t (0 at the end of the macro
// step: the re-basing), the new level and want; the body's level and a floor hit counted in hist (LDS).  Shared by the
// host-scheduled finalize kernels and the resident forms.
template <bool EXT>
__device__ __forceinline__ void block_finalize_body(const float4* pa, const float4* pj, const int splits, const int n_pad,
                                                    const int k, const int i, const float G, const float dt_max,
                                                    const int L, const unsigned int t, const float eta,
                                                    const HermiteArrays d, const HermiteLo lo, float4* jerk, int* level,
                                                    unsigned int* tick, float* want, unsigned int* hist) {
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < splits; q++) {
    const float4 p = pa[(size_t)q * n_pad + k], r = pj[(size_t)q * n_pad + k];
    s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z;
    s[3] += (double)r.x; s[4] += (double)r.y; s[5] += (double)r.z;
  }
  const float a1x = (float)((double)G * s[0]), a1y = (float)((double)G * s[1]), a1z = (float)((double)G * s[2]);
  const float j1x = (float)((double)G * s[3]), j1y = (float)((double)G * s[4]), j1z = (float)((double)G * s[5]);
  const int lev = level[i];
  const double h = (double)dt_max / (double)(1u << lev);
  const float4 j0 = jerk[i];
  const double a0[3] = {(double)d.ax[i], (double)d.ay[i], (double)d.az[i]};
  const double j0d[3] = {(double)j0.x, (double)j0.y, (double)j0.z};
  const double a1[3] = {(double)a1x, (double)a1y, (double)a1z};
  const double j1[3] = {(double)j1x, (double)j1y, (double)j1z};
  if constexpr (EXT)
    hermite_correct_ext(h, d, lo, i, jerk, a1x, a1y, a1z, j1x, j1y, j1z);
  else
    hermite_correct(h, d, i, jerk, a1x, a1y, a1z, j1x, j1y, j1z);
  jerk[i] = make_float4(j1x, j1y, j1z, 0.f);
  double w;
  bool floor_hit;
  level[i] = block_new_level(a0, j0d, a1, j1, h, (double)dt_max, (double)eta, lev, L, t, &w, &floor_hit);
  want[i] = (float)w;
  tick[i] = t == (1u << L) ? 0u : t;
  atomicAdd(&hist[lev], 1u);
  if (floor_hit) atomicAdd(&hist[kMaxLevel + 1], 1u);
}

}  // namespace nbh
