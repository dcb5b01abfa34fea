// radial_common.h -- the per-member arithmetic of the radial profiles (include/nbody_hip_radial.h; DESIGN.md section
// 4.28) as plain inline functions: the distance and the four terms of a member, the sort key, the three cut rules, the
// in-turn enclosed mass of a small group and the finished structs.  No HIP intrinsics: radial_profile.hip runs these on
// the device, radial_check.cpp on the host under the sanitizers, so the two evaluate the same expressions.  Everything is
// fp64 with correctly rounded / and sqrt.  Every translation unit that includes this file is built with
// -ffp-contract=off: a product and the add that takes it are TWO roundings, whatever the compiler could fuse.
#pragma once

#include <cmath>

#include "nbody_hip_radial.h"

#ifndef NBH_HD
#if defined(__HIPCC__)
#define NBH_HD __host__ __device__
#else
#define NBH_HD
#endif
#endif

namespace nbh {

struct RadialCentre {
  double c[3], v[3];  // the group's centre and bulk velocity
};

// q = (float)r2, round to nearest; a finite r2 beyond the floats gives +inf (stated here, not left to the conversion)
NBH_HD inline float radial_q(double r2) {
  return r2 >= 3.4028235677973366e38 ? (float)INFINITY : (float)r2;  // (FLT_MAX + half an ulp: the tie goes to the even
                                                                     // side, +inf; below it the cast rounds to FLT_MAX)
}
NBH_HD inline unsigned int radial_q_bits(float q) {
  unsigned int b;
  __builtin_memcpy(&b, &q, sizeof b);
  return b;
}
NBH_HD inline float radial_q_from_bits(unsigned int b) {
  float q;
  __builtin_memcpy(&q, &b, sizeof q);
  return q;
}
// r2 of a member about the centre; a NaN when any of it is
NBH_HD inline double radial_r2(double x, double y, double z, const RadialCentre& c) {
  const double dx = x - c.c[0], dy = y - c.c[1], dz = z - c.c[2];
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}
// the key that orders a whole call: the group's ordinal above the bits of q (q >= +0: its bits order as it does)
NBH_HD inline unsigned long long radial_key(long long ordinal, unsigned int q_bits) {
  return ((unsigned long long)ordinal << 32) | (unsigned long long)q_bits;
}

struct RadialTerms {
  double t[4];  // m, m*vr, m*vr2, m*vt2
};
NBH_HD inline RadialTerms radial_terms(double x, double y, double z, double vx, double vy, double vz, double m,
                                       const RadialCentre& c) {
  const double dx = x - c.c[0], dy = y - c.c[1], dz = z - c.c[2];
  const double ux = vx - c.v[0], uy = vy - c.v[1], uz = vz - c.v[2];
  const double r2 = ((dx * dx) + (dy * dy)) + (dz * dz);
  const double s = ((ux * dx) + (uy * dy)) + (uz * dz);
  const double u2 = ((ux * ux) + (uy * uy)) + (uz * uz);
  const double r = sqrt(r2);
  const double vr = r2 > 0.0 ? s / r : 0.0;
  const double vr2 = vr * vr;
  const double vt2 = u2 - vr2;
  RadialTerms o;
  o.t[0] = m;
  o.t[1] = m * vr;
  o.t[2] = m * vr2;
  o.t[3] = m * vt2;
  return o;
}

// ---- the cuts ---------------------------------------------------------------------------------------------------------------
// number fraction f of n >= 1 ranks
NBH_HD inline int radial_k_number(double f, int n) {
  long long k = (long long)ceil(f * (double)n);
  if (k < 1) k = 1;
  if (k > n) k = n;
  return (int)k;
}
// the mass rule's threshold: one rounding
NBH_HD inline double radial_mass_threshold(double f, double M) { return f * M; }
// rank s (0-based) is a candidate of the mass rule: K = s + 1 satisfies E(K - 1) >= T.  K_c is the least candidate's K.
NBH_HD inline bool radial_mass_candidate(double E_s, double T) { return E_s >= T; }
// every reported radius: one correctly rounded root of the widened q, so non-decreasing in the rank
NBH_HD inline double radial_radius(float q) { return sqrt((double)q); }
// rank s lies inside radius R: its REPORTED radius does
NBH_HD inline bool radial_inside(float q, double R) { return radial_radius(q) <= R; }

// K_c of a group whose E and q are at hand in rank order, serially: what the kernels compute by integer minimum
NBH_HD inline int radial_k_serial(int mode, double cut, const double* E, const float* q, int n) {
  if (mode == NBODY_HIP_RADIAL_NUMBER) return radial_k_number(cut, n);
  if (mode == NBODY_HIP_RADIAL_MASS) {
    const double T = radial_mass_threshold(cut, E[n - 1]);
    for (int s = 0; s < n; s++)
      if (radial_mass_candidate(E[s], T)) return s + 1;
    return n;
  }
  int k = n;  // the first rank outside: q ascends with the rank
  for (int s = 0; s < n; s++)
    if (!radial_inside(q[s], cut)) {
      k = s;
      break;
    }
  return k;
}

// the enclosed mass of a group of n <= 32 ranks, in turn
NBH_HD inline void radial_enclosed_small(const double* m, int n, double* E) {
  double e = m[0];
  E[0] = e;
  for (int s = 1; s < n; s++) {
    e = e + m[s];
    E[s] = e;
  }
}

// ---- the finished structs -----------------------------------------------------------------------------------------------------
NBH_HD inline nbody_hip_radial_group radial_group_bad(int status) {
  nbody_hip_radial_group o = {};
  o.status = status;
  return o;
}
// what the two raised bits of a group's bad word say: bit 0 catalogue / range / member index, bit 1 a NaN distance
NBH_HD inline int radial_status(int bad_bits) { return (bad_bits & 1) ? 1 : ((bad_bits & 2) ? 2 : 0); }
NBH_HD inline nbody_hip_radial_group radial_group_finish(double M, float q_last, int n) {
  nbody_hip_radial_group o = {};
  o.mass = M;
  o.r_max = radial_radius(q_last);
  o.n = n;
  o.status = 0;
  return o;
}
// the head of a shell row (everything but the four sums, which are zero here): K raised to k_prev, E_at = E(K - 1) and
// q_at = q of rank K - 1 (neither is looked at when K == 0)
NBH_HD inline nbody_hip_radial_shell radial_shell_head(int mode, double cut, int k_prev, int k, double E_at, float q_at) {
  nbody_hip_radial_shell o = {};
  o.radius = mode == NBODY_HIP_RADIAL_RADIUS ? cut : (k > 0 ? radial_radius(q_at) : 0.0);
  o.enclosed_mass = k > 0 ? E_at : 0.0;
  o.count = k - k_prev;
  o.enclosed_count = k;
  return o;
}

}  // namespace nbh
