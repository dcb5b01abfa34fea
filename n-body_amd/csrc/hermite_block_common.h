// hermite_block_common.h -- the device bodies the block-step Hermite integrator (hermite_block.hip) and its ensemble form
// (hermite_batch.hip) share: the level rules, the three bodies of the narrow sweep, the finalize of one active body and
// the resident block step built from them.  One definition each: the host-scheduled narrow form, the single-system
// resident form, the ensemble and the ensemble with events run the same expressions in the same order between the same
// barriers, which is the whole of their bit equality (DESIGN.md sections 4.10, 4.12, 4.13, 4.15, 4.16).
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
// dt_max 2^-k <= want: the rule of block_prime_kernel (hermite_block.hip) and of the ensemble's priming.
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

// ---------------------------------------------------------------------------------
// What the TRACKED sweep of the ensemble's event form adds to a pair: beside the a and j terms
// the separation of every SEEN pair is folded into two lane-local minima of 64-bit keys.
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

// what only a tracking caller hands to narrow_target: target i (radius tr), the lane's sources j0 + s 256 + lane (radii
// sr) of a system of n bodies, and the lane's minima of the keys of the seen pairs (closest) and of those in contact
struct NarrowTrack {
  const float (&sr)[kNarrowS];
  float tr;
  int i, j0, lane, n;
  unsigned long long &closest, &contact;
};

// one target against the lane's sources: fp32 sums over them, then fp64 over the wave (xor butterfly): v = {a, j} of the
// wave, in every lane.  EXT: d = (hi_j - hi_i) + (lo_j - lo_i) (hermite_common.h), the rest is the same.  TRACK: the keys
// of the pairs carried on in *k, beside the force terms -- nothing of them enters the sums.
template <bool GUARD, bool EXT, bool TRACK = false>
__device__ __forceinline__ NarrowSums narrow_target(const float4 (&sp)[kNarrowS], const float4 (&sv)[kNarrowS],
                                                    const float4 (&sl)[kNarrowS], const float4 tp, const float4 tv,
                                                    const float4 tl, const float eps2, const NarrowTrack* k = nullptr) {
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
    float d2 = 0.f, inv;
    if constexpr (GUARD || TRACK) d2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
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
    if constexpr (TRACK) {
      const int j = k->j0 + s * kBlock + k->lane;
      if (j < k->n && j != k->i && d2 < __builtin_inff()) {  // (a NaN compares false)
        const unsigned long long key = pair_key(d2, k->i, j);
        k->closest = key < k->closest ? key : k->closest;
        const float rs = k->tr + k->sr[s];
        if (rs > 0.0f && d2 < rs * rs) k->contact = key < k->contact ? key : k->contact;
      }
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
  hermite_correct<EXT>(h, d, lo, i, jerk, a1x, a1y, a1z, j1x, j1y, j1z);
  jerk[i] = make_float4(j1x, j1y, j1z, 0.f);
  double w;
  bool floor_hit;
  level[i] = block_new_level(a0, j0d, a1, j1, h, (double)dt_max, (double)eta, lev, L, t, &w, &floor_hit);
  want[i] = (float)w;
  tick[i] = t == (1u << L) ? 0u : t;
  atomicAdd(&hist[lev], 1u);
  if (floor_hit) atomicAdd(&hist[kMaxLevel + 1], 1u);
}

// ---------------------------------------------------------------------------------
// The resident block step (DESIGN.md sections 4.12, 4.13, 4.15, 4.16): ONE block step of ONE system by the 512 threads
// of a workgroup, the one definition block_resident_kernel (hermite_block.hip) and batch_resident_kernel
// (hermite_batch.hip) call.  The workgroup is two 256-lane sub-blocks, each of which does what one block of
// direct_jerk_active_narrow_kernel does (narrow_load_sources, narrow_target, narrow_row) for one (source block, target
// group) at a time, and block_finalize_body adds the rows in source-block order: per target the summation order of the
// host-scheduled narrow form.  (512 threads, not 1,024: at 128 registers per thread the compiler kept the hoisted
// per-thread addresses of the two dozen arrays in scratch, at 256 it needs none.)
// ---------------------------------------------------------------------------------
// (values every thread holds alike are moved to scalar registers: loop state and offsets cost no vector registers)
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ size_t uniform_u64(unsigned long long v) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(v >> 32));
  return ((size_t)hi << 32) | (size_t)lo;
}

// the arrays of a resident launch: the state, the predicted sources and the rows
struct ResidentArrays {
  HermiteArrays d;
  HermiteLo lo;                // (extended state precision only)
  const float* mass;
  float4* jerk;
  int* level;
  unsigned int* tick;
  float* want;
  float4 *posm, *vel, *plo;    // predicted sources (plo: extended only)
  float4 *pa, *pj;             // rows [source block][target]
};

// everything a block step knows about "its system": the arrays start at the system's first body and first row
struct ResidentSystem {
  ResidentArrays p;
  unsigned long long* counters;  // [kCounters]
  const float* radii;            // (TRACK only, else null)
  int n, L;
  float G, eps2, dt_max, eta;
};

// what a block step hands back: its tick and the size of its active set (also when the schedule was out of range) and,
// TRACK, the workgroup-uniform minima of the step's pair keys
struct ResidentStep {
  unsigned int t, n_active;
  unsigned long long closest, contact;
};

// One block step from tick `cur`.  False: the schedule cannot be (empty active set, t not ahead of cur or beyond 2^L),
// and nothing of the state was written.  The workgroup's LDS is declared here; every loop is bounded.
template <bool EXT, bool GUARD, bool TRACK>
__device__ __forceinline__ bool resident_block_step(const ResidentSystem& S, const unsigned int cur, ResidentStep& out) {
  __shared__ double red[2][kResidentSub][kNarrowT][6][kBlock / kWave];
  __shared__ unsigned long long kred[2][kResidentBlock / kWave];  // (TRACK) the waves' minima: closest, contact
  __shared__ unsigned int wave_min[kResidentBlock / kWave];
  __shared__ unsigned int hist[kCounters];
  __shared__ unsigned int n_act;
  __shared__ int list[NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX];  // the active set: never leaves the compute unit
  const int tid = threadIdx.x, sub = tid >> 8, lt = tid & (kBlock - 1);
  const ResidentArrays& P = S.p;
  const int n = S.n, L = S.L;
  const int splits = (n + kBlock * kNarrowS - 1) / (kBlock * kNarrowS);  // source blocks of 1,024

  // 1. t = min_i (tick_i + 2^(L - k_i))
  unsigned int nt = kTickNone;
  for (int i = tid; i < n; i += kResidentBlock) nt = min(nt, P.tick[i] + (1u << (L - P.level[i])));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nt = min(nt, (unsigned int)__shfl_down((int)nt, off, 64));
  if ((tid & 63) == 0) wave_min[tid >> 6] = nt;
  if (tid < kCounters) hist[tid] = 0u;
  if (tid == 0) n_act = 0u;
  __syncthreads();
  unsigned int t = wave_min[0];
#pragma unroll
  for (int k = 1; k < kResidentBlock / kWave; k++) t = min(t, wave_min[k]);
  t = (unsigned int)uniform_i((int)t);

  // 2. every body predicted to t, the active ones appended to the list (its order does not matter)
  for (int base = 0; base < n; base += kResidentBlock) {  // (uniform trip count: whole waves reach the ballot)
    const int i = base + tid;
    bool active = false;
    if (i < n) {
      const unsigned int ti = P.tick[i];
      const double h = (double)(t - ti) * (double)S.dt_max / (double)(1u << L);
      hermite_predict<EXT>(h, P.d.x, P.d.y, P.d.z, P.d.vx, P.d.vy, P.d.vz, P.d.ax, P.d.ay, P.d.az, P.mass, P.lo, P.jerk, i,
                           P.posm, P.vel, P.plo);
      active = ti + (1u << (L - P.level[i])) == t;
    }
    const unsigned long long mask = __ballot(active);
    if (mask != 0ull) {  // (wave-uniform)
      const int lane = tid & 63;
      unsigned int at = 0u;
      if (lane == 0) at = atomicAdd(&n_act, (unsigned int)__popcll(mask));
      at = (unsigned int)__shfl((int)at, 0, 64);
      if (active) list[at + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull))] = i;  // (at most n entries)
    }
  }
  __syncthreads();
  const unsigned int n_active = (unsigned int)uniform_i((int)n_act);
  out.t = t;
  out.n_active = n_active;
  if (n_active == 0u || n_active > (unsigned int)n || t <= cur || t > (1u << L)) return false;  // (uniform)

  // 3. the sweep: per (source block, group of four targets) the body of the narrow kernel.  The items, source block by
  // source block, are dealt to the sub-blocks in turn: a sub-block loads its sources again only when its source block
  // changes.  TRACK: the lane's key minima of this block step run through all its trips.
  const int groups = (int)((n_active + kNarrowT - 1) / kNarrowT);
  const int n_pad = groups * kNarrowT;  // <= ceil4(n): inside the system's rows
  float4 sp[kNarrowS], sv[kNarrowS], sl[kNarrowS];
  float sr[kNarrowS];
  unsigned long long kc = kKeyNone, kt = kKeyNone;
  const int items = splits * groups;
  const int trips = (items + kResidentSub - 1) / kResidentSub;
  int bx = -1;
  for (int trip = 0; trip < trips; trip++) {  // (uniform trip count: the barrier below)
    const int item = trip * kResidentSub + sub;
    const bool mine = item < items;  // (uniform over the sub-block)
    const int g = mine ? item % groups : 0;
    const int k0 = g * kNarrowT;
    const int buf = trip & 1;  // rows are read while the next trip's sums are written
    if (mine && item / groups != bx) {
      bx = item / groups;
      narrow_load_sources<EXT>(P.posm, P.vel, P.plo, bx * (kBlock * kNarrowS), lt, n, sp, sv, sl);
      if constexpr (TRACK) narrow_load_radii(S.radii, bx * (kBlock * kNarrowS), lt, n, sr);
    }
    if (mine) {
      // the group's targets in one round trip to memory (a target past the end: the last one again, not used; the
      // duplicate gives duplicate keys, harmless for a minimum)
      float4 tp[kNarrowT], tv[kNarrowT], tl[kNarrowT];
      float tr[kNarrowT];
      int ti[kNarrowT];
#pragma unroll
      for (int q = 0; q < kNarrowT; q++) {
        const int i = list[min(k0 + q, (int)n_active - 1)];
        ti[q] = i;
        tp[q] = P.posm[i];
        tv[q] = P.vel[i];
        tr[q] = 0.f;
        if constexpr (TRACK) tr[q] = S.radii[i];
        tl[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (EXT) tl[q] = P.plo[i];
      }
      // all four targets without a branch between them: four independent chains of pair arithmetic and butterflies
      // for the scheduler to interleave
      NarrowSums r[kNarrowT];
#pragma unroll
      for (int q = 0; q < kNarrowT; q++) {
        const NarrowTrack k{sr, tr[q], ti[q], bx * (kBlock * kNarrowS), lt, n, kc, kt};
        r[q] = narrow_target<GUARD, EXT, TRACK>(sp, sv, sl, tp[q], tv[q], tl[q], S.eps2, &k);
      }
      if ((lt & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kNarrowT; q++) {
#pragma unroll
          for (int c = 0; c < 6; c++) red[buf][sub][q][c][lt >> 6] = r[q].v[c];
        }
      }
    }
    __syncthreads();
    if (mine && lt < kNarrowT && k0 + lt < (int)n_active) {
      double s[6];
#pragma unroll
      for (int c = 0; c < 6; c++) s[c] = narrow_row(red[buf][sub][lt][c]);
      const size_t o = (size_t)bx * n_pad + (k0 + lt);
      P.pa[o] = make_float4((float)s[0], (float)s[1], (float)s[2], 0.f);
      P.pj[o] = make_float4((float)s[3], (float)s[4], (float)s[5], 0.f);
    }
  }
  // TRACK: the keys, once per block step: every wave's minima into LDS before the barrier the sweep ends with anyway.
  // kred is next written one block step on, behind the barriers of phases 4, 1 and 2: no wave is still reading it then.
  if constexpr (TRACK) {
    kc = wave_min_key(kc);
    kt = wave_min_key(kt);
    if ((tid & 63) == 0) {
      kred[0][tid >> 6] = kc;
      kred[1][tid >> 6] = kt;
    }
  }
  __syncthreads();
  if constexpr (TRACK) {
    unsigned long long c = kred[0][0], x = kred[1][0];
#pragma unroll
    for (int k = 1; k < kResidentBlock / kWave; k++) {
      c = kred[0][k] < c ? kred[0][k] : c;
      x = kred[1][k] < x ? kred[1][k] : x;
    }
    out.closest = uniform_u64(c);
    out.contact = uniform_u64(x);
  }

  // 4. the corrector and the new levels of the active bodies; the histogram of their levels into the counters
  for (int k = tid; k < (int)n_active; k += kResidentBlock)
    block_finalize_body<EXT>(P.pa, P.pj, splits, n_pad, k, list[k], S.G, S.dt_max, L, t, S.eta, P.d, P.lo, P.jerk, P.level,
                             P.tick, P.want, hist);
  __syncthreads();
  if (tid < kCounters && hist[tid]) S.counters[tid] += (unsigned long long)hist[tid];  // (the system's only workgroup)
  return true;
}

}  // namespace nbh
