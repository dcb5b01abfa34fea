// neighbours_common.h -- the arithmetic of the k nearest neighbours, the local density and the density centre
// (include/nbody_hip_neighbours.h: the model) as plain inline functions: the key packing, the
// sorted insertion, the K choice, the argument rule, the status rule, the density, and the terms and merges of the
// density centre.  No HIP intrinsics: grid_neighbours.inc and density_centre.hip run these on the device,
// neighbours_check.cpp on the host under the sanitizers, so both evaluate the same expressions.  The fp64 expressions
// below hold no product that feeds an add except in the density centre's terms, and every translation unit that
// evaluates THOSE (density_centre.hip, neighbours_check.cpp) is built with -ffp-contract=off.
#pragma once

#include <cmath>

#include "nbody_hip_neighbours.h"

#ifndef NBH_HD
#if defined(__HIPCC__)
#define NBH_HD __host__ __device__
#else
#define NBH_HD
#endif
#endif

// (g++ knows no `#pragma unroll`; it needs none: on the host the arrays are memory)
#if defined(__clang__)
#define NBH_UNROLL _Pragma("unroll")
#else
#define NBH_UNROLL
#endif

namespace nbh {

// ---- keys ---------------------------------------------------------------------------------------------------------------
typedef unsigned long long NeighKey;
// an empty slot: above every key of a candidate (the high word is a NaN's pattern, and a NaN is never taken); its low
// word reads as index -1
constexpr NeighKey kNeighEmpty = ~0ull;

NBH_HD inline unsigned int neigh_bits(float d2) { return __builtin_bit_cast(unsigned int, d2); }
NBH_HD inline bool neigh_takes(float d2) { return d2 >= 0.0f; }  // false for a NaN alone: d2 is a sum of squares
NBH_HD inline NeighKey neigh_key(float d2, int index) {
  return ((NeighKey)neigh_bits(d2) << 32) | (NeighKey)(unsigned int)index;
}
NBH_HD inline int neigh_key_index(NeighKey key) { return (int)(unsigned int)(key & 0xffffffffull); }
NBH_HD inline float neigh_key_dist2(NeighKey key) {
  return key == kNeighEmpty ? INFINITY : __builtin_bit_cast(float, (unsigned int)(key >> 32));
}

// K sorted keys, ascending, and -- MASS -- the mass of the body of each.  Every index below is a compile-time constant
// once the loops are unrolled, so the arrays live in registers.
template <int K, bool MASS>
struct NeighList {
  NeighKey a[K];
  float m[MASS ? K : 1];
};

template <int K, bool MASS>
NBH_HD inline void neigh_clear(NeighList<K, MASS>& L) {
NBH_UNROLL
  for (int s = 0; s < K; s++) L.a[s] = kNeighEmpty;
NBH_UNROLL
  for (int s = 0; s < (MASS ? K : 1); s++) L.m[s] = 0.0f;
}

// the cheap test: only a key below the last one enters
template <int K, bool MASS>
NBH_HD inline bool neigh_accepts(const NeighList<K, MASS>& L, NeighKey key) {
  return key < L.a[K - 1];
}

// the insertion of an ACCEPTED key: it replaces the last one and sinks by K - 1 compare-and-swap steps
template <int K, bool MASS>
NBH_HD inline void neigh_insert(NeighList<K, MASS>& L, NeighKey key, float mass) {
  L.a[K - 1] = key;
  if (MASS) L.m[K - 1] = mass;
NBH_UNROLL
  for (int s = K - 1; s > 0; s--) {
    const NeighKey lo = L.a[s - 1], hi = L.a[s];
    const bool swap = hi < lo;
    L.a[s - 1] = swap ? hi : lo;
    L.a[s] = swap ? lo : hi;
    if (MASS) {
      const float mlo = L.m[s - 1], mhi = L.m[s];
      L.m[s - 1] = swap ? mhi : mlo;
      L.m[s] = swap ? mlo : mhi;
    }
  }
}

// slot k - 1 (1 <= k <= K) without a run-time register index
template <int K, bool MASS>
NBH_HD inline NeighKey neigh_kth(const NeighList<K, MASS>& L, int k) {
  NeighKey key = kNeighEmpty;
NBH_UNROLL
  for (int s = 0; s < K; s++) key = (s == k - 1) ? L.a[s] : key;
  return key;
}

// the masses of the slots 0 .. k - 2, in that order, from +0
template <int K>
NBH_HD inline double neigh_msum(const NeighList<K, true>& L, int k) {
  double msum = 0.0;
NBH_UNROLL
  for (int s = 0; s < K; s++)
    if (s < k - 1) msum = msum + (double)L.m[s];
  return msum;
}

// ---- the host's decisions ---------------------------------------------------------------------------------------------
// the list length a call of k runs with: the smallest of {4, 8, 16, 32} that is >= k (0: k is out of range)
NBH_HD inline int neigh_pick_K(int k) {
  if (k < 1 || k > NBODY_HIP_NEIGHBOURS_MAX_K) return 0;
  return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32;
}

enum NeighArgs { kNeighArgsOk = 0, kNeighArgsK = 1, kNeighArgsNoOutput = 2, kNeighArgsRefine = 3 };
// the argument rule of nbody_hip_grid_neighbours, in the order the refusals are reported
NBH_HD inline NeighArgs neigh_args(int k, bool has_index, bool has_dist2, bool has_rho, bool has_status, int refine) {
  if (neigh_pick_K(k) == 0) return kNeighArgsK;
  if (!has_index && !has_dist2 && !has_rho && !has_status) return kNeighArgsNoOutput;
  if (refine != 0 && !has_status) return kNeighArgsRefine;
  return kNeighArgsOk;
}

// at most 2 cells along every axis: every body is in every window
NBH_HD inline bool neigh_whole_grid(int gx, int gy, int gz) { return gx <= 2 && gy <= 2 && gz <= 2; }
NBH_HD inline float neigh_cell2(float cell) { return cell * cell; }

// ---- status and density ---------------------------------------------------------------------------------------------
// kth: slot k - 1 of the finished list
NBH_HD inline int neigh_status(NeighKey kth, float cell2, bool whole_grid) {
  if (kth == kNeighEmpty) return 2;
  const float d2k = neigh_key_dist2(kth);
  if (d2k == 0.0f) return 3;
  return (whole_grid || d2k < cell2) ? 0 : 1;
}

NBH_HD inline double neigh_density(double msum, NeighKey kth, int status) {
  if (status == 2 || status == 3) return 0.0;
  const double r = sqrt((double)neigh_key_dist2(kth));
  return msum / (NBODY_HIP_SPHERE_4PI_3 * ((r * r) * r));
}

// ---- the density centre -----------------------------------------------------------------------------------------------
constexpr int kCentreSmall = 32;      // at most this many bodies: one lane, in turn
constexpr int kCentreChunk = 1024;    // positions per chunk of a larger set
constexpr int kCentreThreads = 256;   // sums per chunk
constexpr int kCentrePerThread = kCentreChunk / kCentreThreads;
constexpr int kCentreSums = 4;        // pass 1: S1, Px, Py, Pz;  pass 2: S2, R, -, -

struct CentreSums {
  double v[kCentreSums];
};
NBH_HD inline void centre_zero(CentreSums& s) {
  for (int a = 0; a < kCentreSums; a++) s.v[a] = 0.0;
}
// a <- a + b: the one way two partial sums are ever combined (a is the one of the EARLIER positions)
NBH_HD inline void centre_merge(CentreSums& a, const CentreSums& b) {
  for (int c = 0; c < kCentreSums; c++) a.v[c] = a.v[c] + b.v[c];
}
NBH_HD inline void centre_add1(CentreSums& s, double rho, float x, float y, float z) {
  s.v[0] = s.v[0] + rho;
  s.v[1] = s.v[1] + rho * (double)x;
  s.v[2] = s.v[2] + rho * (double)y;
  s.v[3] = s.v[3] + rho * (double)z;
}
struct CentrePoint {
  double x[3], s1;
};
NBH_HD inline CentrePoint centre_point(const CentreSums& s) {
  CentrePoint c;
  c.s1 = s.v[0];
  const bool zero = s.v[0] == 0.0;
  for (int a = 0; a < 3; a++) c.x[a] = zero ? 0.0 : s.v[1 + a] / s.v[0];
  return c;
}
NBH_HD inline void centre_add2(CentreSums& s, double rho, float x, float y, float z, const CentrePoint& c) {
  const double dx = (double)x - c.x[0], dy = (double)y - c.x[1], dz = (double)z - c.x[2];
  const double r2 = ((dx * dx) + (dy * dy)) + (dz * dz);
  const double w = rho * rho;
  s.v[0] = s.v[0] + w;
  s.v[1] = s.v[1] + w * r2;
}
NBH_HD inline nbody_hip_density_centre_t centre_bad() {
  nbody_hip_density_centre_t o = {};
  o.status = 1;
  return o;
}
NBH_HD inline nbody_hip_density_centre_t centre_finish(const CentrePoint& c, const CentreSums& s2, int n) {
  nbody_hip_density_centre_t o = {};
  o.n = n;
  if (c.s1 == 0.0) return o;
  for (int a = 0; a < 3; a++) o.centre[a] = c.x[a];
  o.rho_sum = c.s1;
  o.rho2_sum = s2.v[0];
  o.core_radius = s2.v[0] == 0.0 ? 0.0 : sqrt(s2.v[1] / s2.v[0]);
  return o;
}
// chunks of a set of n > kCentreSmall bodies
NBH_HD inline long long centre_chunks(long long n) { return (n + kCentreChunk - 1) / kCentreChunk; }

}  // namespace nbh
