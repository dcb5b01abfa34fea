// radial_profile.hip -- Lagrangian radii and shell moments of the groups of an ordered catalogue, for groups of any size
// (no reference counterpart).  The model is in include/nbody_hip_radial.h and DESIGN.md section 4.28; the per-member
// arithmetic, the key and the cut rules are radial_common.h, which the CPU program radial_check.cpp runs too; the key
// bits, the chunk bound, the launch sizes and the workspace table are radial_plan.h (radial_plan_check.cpp).  This file
// is built with -ffp-contract=off (Makefile): no product is fused into the add that takes it.
//
// A gather- and sort-bound pass:
//   radial_check_kernel        one lane per group: its range, the adjacent order (flag: the catalogue is not ordered),
//                              the empty group (bad[g]), the group's chunk count
//   rocprim::exclusive_scan    chunk_start[g] = group chunks before group g
//   radial_key_kernel          one lane per position of members: its owner by binary search in offsets, the member
//                              index check, r2, q, the key (ordinal << 32) | bits(q); -1 / 0 into the optional outputs
//   rocprim::radix_sort_pairs  ONE stable sort of (key, position) over the plan's key bits
//   radial_first_kernel        one lane per sorted entry: first[g] = where the group's ranks begin in the sorted list
//   radial_terms_kernel        one lane per sorted entry: the member's four terms (the second gather), the optional outputs
//   radial_small_kernel        one lane per group: the struct of a bad group; a group of at most S ranks in turn
//   radial_scan_kernel         one workgroup per group chunk: the chunk's prefix W and total C
//   radial_base_kernel         one wave per group in the chunked form: the bases B of its chunks, M, the struct
//   radial_cut_kernel          one workgroup per group chunk: E = B + W, the cuts by integer atomicMin
//   radial_row_kernel          one lane per group: K raised in cut order, the heads of its shell rows, the shells' chunks
//   rocprim::exclusive_scan    schunk_start[row] = shell chunks before the row
//   radial_shell_small_kernel  one lane per shell row: a shell of at most S ranks in turn
//   radial_shell_chunk_kernel, radial_shell_combine_kernel   the chunked form, in the order of group_props.hip
// Launch sizes come from n_groups, n_members and n_cuts alone (radial_plan), so nothing is read back.  No value read
// from offsets or members is used as an index before it is checked; chunk numbers are below the plan's chunk_cap
// wherever a record is written or read.  Integer atomicOr / atomicMin alone: both are order independent.

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "radial_common.h"
#include "radial_plan.h"

namespace nbh {

static_assert(sizeof(nbody_hip_radial_group) == 32, "nbody_hip_radial_group is 32 bytes (include/nbody_hip_radial.h)");
static_assert(sizeof(nbody_hip_radial_shell) == 64, "nbody_hip_radial_shell is 64 bytes (include/nbody_hip_radial.h)");
static_assert(kRadialMaxCuts == NBODY_HIP_RADIAL_MAX_CUTS && kRadialModeMass == NBODY_HIP_RADIAL_MASS &&
              kRadialModeNumber == NBODY_HIP_RADIAL_NUMBER && kRadialModeRadius == NBODY_HIP_RADIAL_RADIUS, "plan and header");
constexpr int kRadialWaves = kGroupThreads / kWave;
constexpr int kRadialNone = 0x7fffffff;

struct RadialArgs {
  const float *x, *y, *z, *vx, *vy, *vz, *m;
  const int *offsets, *members;  // members null: the identity list
  const double *centres, *vels;  // vels null: zeros
  long long n_groups, n_members, n_rows, chunk_cap;
  int count, n_cuts, mode;
  double cuts[kRadialMaxCuts];
  int *flag, *bad, *nchunks, *chunk_start, *first;
  int *k, *snchunks, *schunk_start;
  unsigned long long *keys_in, *keys_out;
  int *pos_in, *pos_out;
  double *terms, *enclosed, *ctotal, *cbase, *partials;
  nbody_hip_radial_group* groups;
  nbody_hip_radial_shell* shells;
  int* sorted_members;
  float* sorted_q;
};

struct RadialSatAdd {  // chunk counts saturate instead of wrapping (only a catalogue that is not ordered can reach the cap)
  __host__ __device__ int operator()(int a, int b) const {
    const long long s = (long long)a + (long long)b;
    return s > 0x7fffffffLL ? 0x7fffffff : (int)s;
  }
};

__device__ __forceinline__ RadialCentre radial_centre_of(const RadialArgs& A, long long g) {
  RadialCentre c;
  for (int a = 0; a < 3; a++) {
    c.c[a] = A.centres[3 * g + a];
    c.v[a] = A.vels ? A.vels[3 * g + a] : 0.0;
  }
  return c;
}
__device__ __forceinline__ long long radial_ordinal(unsigned long long key) { return (long long)(key >> 32); }
__device__ __forceinline__ float radial_key_q(unsigned long long key) { return radial_q_from_bits((unsigned int)key); }

__global__ __launch_bounds__(kGroupThreads) void radial_check_kernel(const RadialArgs A) {
  const long long g = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (g > A.n_groups) return;
  if (g == A.n_groups) {  // (the scan's last entry: the group chunks of the call)
    A.nchunks[g] = 0;
    return;
  }
  const long long o0 = A.offsets[g], o1 = A.offsets[g + 1];
  const bool ordered = o0 >= 0 && o0 <= o1 && o1 <= A.n_members;  // every lane's own pair: together the whole order
  if (!ordered) atomicOr(A.flag, 1);
  A.nchunks[g] = ordered ? group_chunks(o1 - o0) : 0;
  A.bad[g] = ordered && o0 < o1 ? 0 : 1;
}

__global__ __launch_bounds__(kGroupThreads) void radial_key_kernel(const RadialArgs A) {
  const long long p = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (p >= A.n_members) return;
  if (A.sorted_members) A.sorted_members[p] = -1;
  if (A.sorted_q) A.sorted_q[p] = 0.0f;
  A.pos_in[p] = (int)p;
  unsigned long long key = radial_key(A.n_groups, 0u);  // a position of no group
  if (*A.flag == 0 && p >= (long long)A.offsets[0] && p < (long long)A.offsets[A.n_groups]) {
    long long lo = 0, hi = A.n_groups;  // offsets[lo] <= p < offsets[hi]: the owner is the LAST g with offsets[g] <= p
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if ((long long)A.offsets[mid] <= p) lo = mid; else hi = mid;
    }
    const int i = A.members ? A.members[p] : (int)p;
    key = radial_key(lo, 0u);
    if ((unsigned int)i >= (unsigned int)A.count) {
      atomicOr(A.bad + lo, 1);
    } else {
      const double r2 = radial_r2((double)A.x[i], (double)A.y[i], (double)A.z[i], radial_centre_of(A, lo));
      if (r2 != r2) atomicOr(A.bad + lo, 2);
      else key = radial_key(lo, radial_q_bits(radial_q(r2)));
    }
  }
  A.keys_in[p] = key;
}

__global__ __launch_bounds__(kGroupThreads) void radial_first_kernel(const RadialArgs A) {
  const long long j = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (j >= A.n_members) return;
  const long long g = radial_ordinal(A.keys_out[j]);
  if (g < A.n_groups && (j == 0 || radial_ordinal(A.keys_out[j - 1]) != g)) A.first[g] = (int)j;
}

__global__ __launch_bounds__(kGroupThreads) void radial_terms_kernel(const RadialArgs A) {
  const long long j = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (j >= A.n_members || *A.flag) return;
  const unsigned long long key = A.keys_out[j];
  const long long g = radial_ordinal(key);
  if (g >= A.n_groups || A.bad[g]) return;
  const int p = A.pos_out[j];                 // a position of group g: the key kernel put it there
  const int i = A.members ? A.members[p] : p;  // in [0, count): else the key kernel had raised bad[g]
  const RadialTerms t = radial_terms((double)A.x[i], (double)A.y[i], (double)A.z[i], (double)A.vx[i], (double)A.vy[i],
                                     (double)A.vz[i], (double)A.m[i], radial_centre_of(A, g));
  for (int k = 0; k < kRadialSums; k++) A.terms[(long long)k * A.n_members + j] = t.t[k];
  const long long at = (long long)A.offsets[g] + (j - (long long)A.first[g]);  // < offsets[g + 1]: rank < n
  if (A.sorted_members) A.sorted_members[at] = i;
  if (A.sorted_q) A.sorted_q[at] = radial_key_q(key);
}

__global__ __launch_bounds__(kGroupThreads) void radial_small_kernel(const RadialArgs A) {
  const long long g = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (g >= A.n_groups) return;
  const int status = *A.flag ? 1 : radial_status(A.bad[g]);
  if (status) {
    A.groups[g] = radial_group_bad(status);
    return;
  }
  const int n = A.offsets[g + 1] - A.offsets[g];  // 1 <= n: the group is legal
  if (n > kGroupSmall) return;
  const long long j0 = A.first[g];
  double m[kGroupSmall], E[kGroupSmall];
  float q[kGroupSmall];
  for (int s = 0; s < n; s++) {
    m[s] = A.terms[j0 + s];
    q[s] = radial_key_q(A.keys_out[j0 + s]);
  }
  radial_enclosed_small(m, n, E);
  for (int s = 0; s < n; s++) A.enclosed[j0 + s] = E[s];
  for (int c = 0; c < A.n_cuts; c++) A.k[g * A.n_cuts + c] = radial_k_serial(A.mode, A.cuts[c], E, q, n);
  A.groups[g] = radial_group_finish(E[n - 1], q[n - 1], n);
}

// the range that owns chunk c (0 <= c < start[n]): the LAST r with start[r] <= c (group_props.hip: group_of_chunk)
__device__ __forceinline__ long long radial_of_chunk(const int* __restrict__ start, long long n, long long c) {
  long long lo = 0, hi = n;  // start[lo] <= c < start[hi]
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if ((long long)start[mid] <= c) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long long radial_chunk_total(const int* __restrict__ start, long long n, long long cap) {
  const long long t = start[n];
  return t < cap ? t : cap;
}

// W and C of every group chunk.  c, g and bad[g] are the same in every thread of the workgroup.
__global__ __launch_bounds__(kGroupThreads) void radial_scan_kernel(const RadialArgs A) {
  __shared__ double P_sh[kGroupThreads];
  if (*A.flag) return;
  const int t = (int)threadIdx.x;
  const long long total = radial_chunk_total(A.chunk_start, A.n_groups, A.chunk_cap);
  for (long long c = blockIdx.x; c < total; c += gridDim.x) {
    const long long g = radial_of_chunk(A.chunk_start, A.n_groups, c);
    if (A.bad[g]) continue;
    const long long n = (long long)A.offsets[g + 1] - A.offsets[g];
    const long long r0 = (c - (long long)A.chunk_start[g]) * kGroupChunk;  // < n: the chunk is one of the group's
    const long long j0 = (long long)A.first[g] + r0;
    const int in_chunk = (int)(n - r0 < kGroupChunk ? n - r0 : kGroupChunk);
    double a[kGroupPerThread];
#pragma unroll
    for (int j = 0; j < kGroupPerThread; j++) {
      const int l = kGroupPerThread * t + j;
      const double m = l < in_chunk ? A.terms[j0 + l] : 0.0;
      a[j] = j == 0 ? m : a[j - 1] + m;
    }
    double P = a[kGroupPerThread - 1];
    for (int o = 1; o < kGroupThreads; o <<= 1) {
      P_sh[t] = P;
      __syncthreads();
      if (t >= o) P = P_sh[t - o] + P;
      __syncthreads();
    }
    P_sh[t] = P;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGroupPerThread; j++) {
      const int l = kGroupPerThread * t + j;
      if (l < in_chunk) A.enclosed[j0 + l] = t == 0 ? a[j] : P_sh[t - 1] + a[j];
    }
    if (t == kGroupThreads - 1) A.ctotal[c] = P;  // c < chunk_cap
    __syncthreads();  // (P_sh is written again by the next chunk)
  }
}

// One wave per chunk number; the wave that meets the FIRST chunk of a group walks the group's chunk totals in order.
__global__ __launch_bounds__(kGroupThreads) void radial_base_kernel(const RadialArgs A) {
  if (*A.flag) return;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const long long total = radial_chunk_total(A.chunk_start, A.n_groups, A.chunk_cap);
  const long long stride = (long long)gridDim.x * kRadialWaves;
  for (long long c = (long long)blockIdx.x * kRadialWaves + threadIdx.x / kWave; c < total; c += stride) {
    const long long g = radial_of_chunk(A.chunk_start, A.n_groups, c);
    if ((long long)A.chunk_start[g] != c || A.bad[g]) continue;
    const int nch = A.nchunks[g];
    if (c + nch > A.chunk_cap) continue;  // (no ordered catalogue gets here: radial_plan.h)
    double B = 0.0;  // B_k before chunk k; not a term of any sum while k == 0
    double base = 0.0;
    for (int k0 = 0; k0 < nch; k0 += kWave) {
      const int k = k0 + lane;
      const double mine = k < nch ? A.ctotal[c + k] : 0.0;
      const int steps = nch - k0 < kWave ? nch - k0 : kWave;
      for (int i = 0; i < steps; i++) {  // every lane walks the same chain; lane i keeps the base of its chunk
        const double C = __shfl(mine, i, kWave);
        if (i == lane) base = B;
        B = (k0 + i) == 0 ? C : B + C;
      }
      if (k < nch && k > 0) A.cbase[c + k] = base;
    }
    const double Bl = __shfl(base, (nch - 1) & (kWave - 1), kWave);  // the base of the last chunk: its lane has it
    if (lane != 0) continue;
    const int n = A.offsets[g + 1] - A.offsets[g];
    const long long last = (long long)A.first[g] + n - 1;
    const double W = A.enclosed[last];
    const double M = nch > 1 ? Bl + W : W;
    A.groups[g] = radial_group_finish(M, radial_key_q(A.keys_out[last]), n);
    for (int cut = 0; cut < A.n_cuts; cut++)
      A.k[g * A.n_cuts + cut] = A.mode == NBODY_HIP_RADIAL_NUMBER ? radial_k_number(A.cuts[cut], n) : n;
  }
}

// E = B + W of every rank of a group chunk, and the cuts: the least candidate of the chunk, then an integer atomicMin
__global__ __launch_bounds__(kGroupThreads) void radial_cut_kernel(const RadialArgs A) {
  __shared__ int k_sh[kRadialMaxCuts];
  if (*A.flag) return;
  const int t = (int)threadIdx.x, lane = t & (kWave - 1);
  const long long total = radial_chunk_total(A.chunk_start, A.n_groups, A.chunk_cap);
  for (long long c = blockIdx.x; c < total; c += gridDim.x) {
    const long long g = radial_of_chunk(A.chunk_start, A.n_groups, c);
    if (A.bad[g] || (long long)A.chunk_start[g] + A.nchunks[g] > A.chunk_cap) continue;
    const long long n = (long long)A.offsets[g + 1] - A.offsets[g];
    const long long kc = c - (long long)A.chunk_start[g];
    const long long r0 = kc * kGroupChunk;
    const long long j0 = (long long)A.first[g] + r0;
    const int in_chunk = (int)(n - r0 < kGroupChunk ? n - r0 : kGroupChunk);
    const double B = kc > 0 ? A.cbase[c] : 0.0;
    const double M = A.groups[g].mass;
    if (t < kRadialMaxCuts) k_sh[t] = kRadialNone;
    __syncthreads();
    int cand[kRadialMaxCuts];
#pragma unroll
    for (int cut = 0; cut < kRadialMaxCuts; cut++) cand[cut] = kRadialNone;
    for (int j = kGroupPerThread - 1; j >= 0; j--) {  // (downwards: the least rank is taken last)
      const int l = kGroupPerThread * t + j;
      if (l >= in_chunk) continue;
      const double W = A.enclosed[j0 + l];
      const double E = kc > 0 ? B + W : W;
      A.enclosed[j0 + l] = E;
      const int s = (int)(r0 + l);
      if (A.mode == NBODY_HIP_RADIAL_MASS) {
#pragma unroll
        for (int cut = 0; cut < kRadialMaxCuts; cut++)
          if (cut < A.n_cuts && radial_mass_candidate(E, radial_mass_threshold(A.cuts[cut], M))) cand[cut] = s + 1;
      } else if (A.mode == NBODY_HIP_RADIAL_RADIUS) {
        const float q = radial_key_q(A.keys_out[j0 + l]);
#pragma unroll
        for (int cut = 0; cut < kRadialMaxCuts; cut++)
          if (cut < A.n_cuts && !radial_inside(q, A.cuts[cut])) cand[cut] = s;  // the first rank outside: K = its rank
      }
    }
    if (A.mode != NBODY_HIP_RADIAL_NUMBER) {
#pragma unroll
      for (int cut = 0; cut < kRadialMaxCuts; cut++) {
        if (cut >= A.n_cuts) continue;  // (the same in every lane)
        int v = cand[cut];
        for (int off = kWave / 2; off > 0; off >>= 1) {
          const int o = __shfl_down(v, off, kWave);
          v = o < v ? o : v;
        }
        if (lane == 0 && v != kRadialNone) atomicMin(k_sh + cut, v);
      }
      __syncthreads();
      if (t < A.n_cuts && k_sh[t] != kRadialNone) atomicMin(A.k + g * A.n_cuts + t, k_sh[t]);
    }
    __syncthreads();  // (k_sh is written again by the next chunk)
  }
}

__global__ __launch_bounds__(kGroupThreads) void radial_row_kernel(const RadialArgs A) {
  const long long g = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (g > A.n_groups) return;
  if (g == A.n_groups) {  // (the scan's last entry: the shell chunks of the call)
    A.snchunks[A.n_rows] = 0;
    return;
  }
  const bool bad = *A.flag || A.bad[g] ||
                   (A.nchunks[g] > 0 && (long long)A.chunk_start[g] + A.nchunks[g] > A.chunk_cap);
  int prev = 0;
  for (int c = 0; c < A.n_cuts; c++) {
    const long long row = g * A.n_cuts + c;
    if (bad) {
      const nbody_hip_radial_shell zero = {};
      A.shells[row] = zero;
      A.snchunks[row] = 0;
      continue;
    }
    int K = A.k[row];
    if (K < prev) K = prev;
    const long long at = (long long)A.first[g] + K - 1;
    A.shells[row] = radial_shell_head(A.mode, A.cuts[c], prev, K, K > 0 ? A.enclosed[at] : 0.0,
                                      K > 0 ? radial_key_q(A.keys_out[at]) : 0.0f);
    A.snchunks[row] = group_chunks(K - prev);
    prev = K;
  }
}

__device__ __forceinline__ void radial_store_sums(nbody_hip_radial_shell* o, const double* s) {
  o->mass = s[0];
  o->m_vr = s[1];
  o->m_vr2 = s[2];
  o->m_vt2 = s[3];
}

__global__ __launch_bounds__(kGroupThreads) void radial_shell_small_kernel(const RadialArgs A) {
  const long long row = (long long)blockIdx.x * kGroupThreads + threadIdx.x;
  if (row >= A.n_rows) return;
  const int cnt = A.shells[row].count;  // 0 in every row of a bad group
  if (cnt <= 0 || cnt > kGroupSmall) return;
  const long long g = row / A.n_cuts;
  const long long j0 = (long long)A.first[g] + (A.shells[row].enclosed_count - cnt);
  double s[kRadialSums];
  for (int k = 0; k < kRadialSums; k++) {
    s[k] = 0.0;
    for (int p = 0; p < cnt; p++) s[k] = s[k] + A.terms[(long long)k * A.n_members + j0 + p];
  }
  radial_store_sums(A.shells + row, s);
}

__device__ __forceinline__ void radial_wave_fold(double* s) {
  for (int off = kWave / 2; off > 0; off >>= 1)
    for (int k = 0; k < kRadialSums; k++) s[k] = s[k] + __shfl_down(s[k], off, kWave);
}

// The chunks of the shells in the chunked form, in the order of group_props.hip: position 256 j + t, a shuffle tree per
// wave, the four waves in order.
__global__ __launch_bounds__(kGroupThreads) void radial_shell_chunk_kernel(const RadialArgs A) {
  __shared__ double wave_rec[kRadialWaves][kRadialSums];
  if (*A.flag) return;
  const int t = (int)threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const long long total = radial_chunk_total(A.schunk_start, A.n_rows, A.chunk_cap);
  for (long long c = blockIdx.x; c < total; c += gridDim.x) {
    const long long row = radial_of_chunk(A.schunk_start, A.n_rows, c);
    const long long g = row / A.n_cuts;
    const int cnt = A.shells[row].count;  // > S: the shell has chunks
    const long long base = (long long)A.first[g] + (A.shells[row].enclosed_count - cnt) +
                           (c - (long long)A.schunk_start[row]) * kGroupChunk;
    const long long end_all = (long long)A.first[g] + A.shells[row].enclosed_count;
    const long long end = base + kGroupChunk < end_all ? base + kGroupChunk : end_all;
    double s[kRadialSums] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kGroupPerThread; j++) {
      const long long p = base + (long long)j * kGroupThreads + t;
      if (p >= end) continue;
      for (int k = 0; k < kRadialSums; k++) s[k] = s[k] + A.terms[(long long)k * A.n_members + p];
    }
    radial_wave_fold(s);
    if (lane == 0)
      for (int k = 0; k < kRadialSums; k++) wave_rec[wave][k] = s[k];
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kRadialWaves; w++)
        for (int k = 0; k < kRadialSums; k++) s[k] = s[k] + wave_rec[w][k];
      for (int k = 0; k < kRadialSums; k++) A.partials[c * kRadialSums + k] = s[k];  // c < chunk_cap
    }
    __syncthreads();  // (wave_rec is written again by the next chunk)
  }
}

// One wave per chunk number; the wave that meets the FIRST chunk of a shell folds the shell's chunk partials.
__global__ __launch_bounds__(kGroupThreads) void radial_shell_combine_kernel(const RadialArgs A) {
  if (*A.flag) return;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const long long total = radial_chunk_total(A.schunk_start, A.n_rows, A.chunk_cap);
  const long long stride = (long long)gridDim.x * kRadialWaves;
  for (long long c = (long long)blockIdx.x * kRadialWaves + threadIdx.x / kWave; c < total; c += stride) {
    const long long row = radial_of_chunk(A.schunk_start, A.n_rows, c);
    if ((long long)A.schunk_start[row] != c) continue;
    const int nch = A.snchunks[row];
    if (c + nch > A.chunk_cap) continue;  // (no ordered catalogue gets here: the sums stay zero)
    double s[kRadialSums] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < nch; k += kWave)
      for (int i = 0; i < kRadialSums; i++) s[i] = s[i] + A.partials[(c + k) * kRadialSums + i];
    radial_wave_fold(s);
    if (lane == 0) radial_store_sums(A.shells + row, s);
  }
}

static hipError_t radial_scan(void* tmp, size_t& bytes, int* in, int* out, size_t count, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, 0, count, RadialSatAdd(), st);
}
static hipError_t radial_sort(void* tmp, size_t& bytes, unsigned long long* keys_in, unsigned long long* keys_out,
                              int* pos_in, int* pos_out, size_t count, int bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, pos_in, pos_out, count, 0u, (unsigned)bits, st);
}

int radial_profile_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev, const int* members_dev,
                          long long n_groups, long long n_members, const double* centres_dev, const double* vels_dev_or_null,
                          const double* cuts_host, int n_cuts, int mode, nbody_hip_radial_group* groups_out_dev,
                          nbody_hip_radial_shell* shells_out_dev, int* sorted_members_dev_or_null,
                          float* sorted_q_dev_or_null) {
  if (!d) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null particle data");
  if (!d->pos_x || !d->pos_y || !d->pos_z || !d->vel_x || !d->vel_y || !d->vel_z || !d->mass)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "particle data has null arrays");
  if (!offsets_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null offsets array");
  if (!cuts_host) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null cuts array");
  if (n_groups < 0 || n_members < 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "negative group or member count");
  if (n_members > kGroupMaxMembers) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 1 members");
  if (n_groups > kGroupMaxGroups) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 2 groups");
  if (const int why = radial_cuts_check(cuts_host, n_cuts, mode))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", radial_cuts_message(why));
  if (n_groups * n_cuts > kRadialMaxRows) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "more than 2^31 - 1 shell rows");
  if (n_groups == 0) return NBODY_HIP_OK;
  if (!centres_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null centres array");
  if (!groups_out_dev || !shells_out_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
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
  const int key_bits = radial_key_bits(n_groups);
  size_t sort_bytes = 0, scan_bytes = 0, scan_rows = 0;  // (size queries: no launch)
  if (n_members > 0)
    NBH_HIP(radial_sort(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n_members, key_bits, st));
  NBH_HIP(radial_scan(nullptr, scan_bytes, nullptr, nullptr, (size_t)n_groups + 1, st));
  NBH_HIP(radial_scan(nullptr, scan_rows, nullptr, nullptr, (size_t)(n_groups * n_cuts) + 1, st));
  if (scan_rows > scan_bytes) scan_bytes = scan_rows;
  const RadialPlan p = radial_plan(n_groups, n_members, n_cuts, sort_bytes, scan_bytes);
  if (ctx->capturing && ctx->radial.bytes < p.bytes) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "radial profiles cannot be recorded into a step graph before their workspace "
                    "exists: run the call once eagerly with these sizes");
  }
  if (int rc = ctx->radial.reserve(p.bytes)) return rc;
  char* const ws = static_cast<char*>(ctx->radial.ptr);
  RadialArgs A;
  A.x = d->pos_x; A.y = d->pos_y; A.z = d->pos_z;
  A.vx = d->vel_x; A.vy = d->vel_y; A.vz = d->vel_z;
  A.m = d->mass;
  A.offsets = offsets_dev;
  A.members = members_dev;
  A.centres = centres_dev;
  A.vels = vels_dev_or_null;
  A.n_groups = n_groups;
  A.n_members = n_members;
  A.n_rows = p.n_rows;
  A.chunk_cap = p.chunk_cap;
  A.count = (int)d->count;
  A.n_cuts = n_cuts;
  A.mode = mode;
  for (int c = 0; c < kRadialMaxCuts; c++) A.cuts[c] = c < n_cuts ? cuts_host[c] : 0.0;
  auto ints = [ws](size_t off) { return reinterpret_cast<int*>(ws + off); };
  auto doubles = [ws](size_t off) { return reinterpret_cast<double*>(ws + off); };
  A.flag = ints(p.off_flag);
  A.bad = ints(p.off_bad);
  A.nchunks = ints(p.off_nchunks);
  A.chunk_start = ints(p.off_chunk_start);
  A.first = ints(p.off_first);
  A.k = ints(p.off_k);
  A.snchunks = ints(p.off_snchunks);
  A.schunk_start = ints(p.off_schunk_start);
  A.keys_in = reinterpret_cast<unsigned long long*>(ws + p.off_keys_in);
  A.keys_out = reinterpret_cast<unsigned long long*>(ws + p.off_keys_out);
  A.pos_in = ints(p.off_pos_in);
  A.pos_out = ints(p.off_pos_out);
  A.terms = doubles(p.off_terms);
  A.enclosed = doubles(p.off_enclosed);
  A.ctotal = doubles(p.off_ctotal);
  A.cbase = doubles(p.off_cbase);
  A.partials = doubles(p.off_partials);
  A.groups = groups_out_dev;
  A.shells = shells_out_dev;
  A.sorted_members = sorted_members_dev_or_null;
  A.sorted_q = sorted_q_dev_or_null;
  const dim3 block(kGroupThreads);
  NBH_HIP(hipMemsetAsync(A.flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(radial_check_kernel, dim3(p.group_blocks), block, 0, st, A);
  NBH_LAUNCH_CHECK();
  NBH_HIP(radial_scan(ws + p.off_scan_tmp, scan_bytes, A.nchunks, A.chunk_start, p.group_scan_count, st));
  if (p.member_blocks > 0) {
    hipLaunchKernelGGL(radial_key_kernel, dim3(p.member_blocks), block, 0, st, A);
    NBH_LAUNCH_CHECK();
    NBH_HIP(radial_sort(ws + p.off_sort_tmp, sort_bytes, A.keys_in, A.keys_out, A.pos_in, A.pos_out, (size_t)n_members,
                        key_bits, st));
    hipLaunchKernelGGL(radial_first_kernel, dim3(p.member_blocks), block, 0, st, A);
    hipLaunchKernelGGL(radial_terms_kernel, dim3(p.member_blocks), block, 0, st, A);
  }
  hipLaunchKernelGGL(radial_small_kernel, dim3((unsigned)((n_groups + kGroupThreads - 1) / kGroupThreads)), block, 0, st, A);
  if (p.chunk_blocks > 0) {
    hipLaunchKernelGGL(radial_scan_kernel, dim3(p.chunk_blocks), block, 0, st, A);
    hipLaunchKernelGGL(radial_base_kernel, dim3(p.combine_blocks), block, 0, st, A);
    hipLaunchKernelGGL(radial_cut_kernel, dim3(p.chunk_blocks), block, 0, st, A);
  }
  hipLaunchKernelGGL(radial_row_kernel, dim3(p.group_blocks), block, 0, st, A);
  NBH_LAUNCH_CHECK();
  NBH_HIP(radial_scan(ws + p.off_scan_tmp, scan_bytes, A.snchunks, A.schunk_start, p.row_scan_count, st));
  hipLaunchKernelGGL(radial_shell_small_kernel, dim3((unsigned)((p.n_rows + kGroupThreads - 1) / kGroupThreads)), block, 0,
                     st, A);
  if (p.chunk_blocks > 0) {
    hipLaunchKernelGGL(radial_shell_chunk_kernel, dim3(p.chunk_blocks), block, 0, st, A);
    hipLaunchKernelGGL(radial_shell_combine_kernel, dim3(p.combine_blocks), block, 0, st, A);
  }
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}

}  // namespace nbh

using namespace nbh;

extern "C" int nbody_hip_groups_radial_profile(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev,
                                               const int* members_dev_or_null, long long n_groups, long long n_members,
                                               const double* centres_dev, const double* vels_dev_or_null,
                                               const double* cuts_host, int n_cuts, int mode,
                                               nbody_hip_radial_group* groups_out_dev, nbody_hip_radial_shell* shells_out_dev,
                                               int* sorted_members_dev_or_null, float* sorted_q_dev_or_null) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  return radial_profile_launch(ctx, d, offsets_dev, members_dev_or_null, n_groups, n_members, centres_dev, vels_dev_or_null,
                               cuts_host, n_cuts, mode, groups_out_dev, shells_out_dev, sorted_members_dev_or_null,
                               sorted_q_dev_or_null);
}
