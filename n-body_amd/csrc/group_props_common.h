// group_props_common.h -- the per-member arithmetic of the group properties (include/nbody_hip_group_props.h:
// nbody_hip_group_props) as plain inline functions.  No HIP intrinsics: group_props.hip runs
// these on the device, group_props_check.cpp on the host under the sanitizers, so the two evaluate the same
// expressions.  Everything is fp64 with correctly rounded / and sqrt.  Every translation unit that includes this file is
// built with -ffp-contract=off: a product and the add that takes it are TWO roundings, whatever the compiler could fuse.
#pragma once

#include <cmath>

#include "nbody_hip_group_props.h"

#ifndef NBH_HD
#if defined(__HIPCC__)
#define NBH_HD __host__ __device__
#else
#define NBH_HD
#endif
#endif

namespace nbh {

struct GroupBody {
  double x, y, z, vx, vy, vz, m;  // the seven floats of a body, widened (exact)
};

NBH_HD inline GroupBody group_body(float x, float y, float z, float vx, float vy, float vz, float m) {
  return GroupBody{(double)x, (double)y, (double)z, (double)vx, (double)vy, (double)vz, (double)m};
}

// PASS 1: mass, sum m x, sum m v
constexpr int kGroupSums1 = 7;
struct GroupSums1 {
  double v[kGroupSums1];  // 0 mass, 1-3 m x, 4-6 m v
};

NBH_HD inline void group_sums1_zero(GroupSums1& s) {
  for (int k = 0; k < kGroupSums1; k++) s.v[k] = 0.0;
}
NBH_HD inline void group_sums1_add(GroupSums1& s, const GroupBody& b) {
  s.v[0] = s.v[0] + b.m;
  s.v[1] = s.v[1] + b.m * b.x;
  s.v[2] = s.v[2] + b.m * b.y;
  s.v[3] = s.v[3] + b.m * b.z;
  s.v[4] = s.v[4] + b.m * b.vx;
  s.v[5] = s.v[5] + b.m * b.vy;
  s.v[6] = s.v[6] + b.m * b.vz;
}
// a <- a + b, the one way two partial sums are ever combined (a is the one of the EARLIER members)
NBH_HD inline void group_sums1_merge(GroupSums1& a, const GroupSums1& b) {
  for (int k = 0; k < kGroupSums1; k++) a.v[k] = a.v[k] + b.v[k];
}

// X = (sum m x) / mass and V = (sum m v) / mass, one division each; zeros when the mass is 0
struct GroupCentre {
  double mass, x[3], v[3];
};
NBH_HD inline GroupCentre group_centre(const GroupSums1& s) {
  GroupCentre c;
  c.mass = s.v[0];
  const bool zero = s.v[0] == 0.0;
  for (int a = 0; a < 3; a++) {
    c.x[a] = zero ? 0.0 : s.v[1 + a] / s.v[0];
    c.v[a] = zero ? 0.0 : s.v[4 + a] / s.v[0];
  }
  return c;
}

// PASS 2: the central sums about the rounded X and V, and the two extrema with their bodies
constexpr int kGroupSums2 = 11;
struct GroupSums2 {
  double v[kGroupSums2];  // 0-2 L, 3 sum m |u|^2 (twice the kinetic energy), 4-9 I xx yy zz xy xz yz, 10 sum m phi
  double r2;              // max |d|^2, -1 before the first member
  double phi;             // min phi (widened), +inf before the first member
  int r2_body, phi_body;  // their bodies, ties to the lowest index; INT_MAX before the first member
};

constexpr int kGroupNoBody = 0x7fffffff;

NBH_HD inline void group_sums2_zero(GroupSums2& s) {
  for (int k = 0; k < kGroupSums2; k++) s.v[k] = 0.0;
  s.r2 = -1.0;
  s.phi = (double)INFINITY;
  s.r2_body = kGroupNoBody;
  s.phi_body = kGroupNoBody;
}
// (value, body) extrema: the larger r2 / the smaller phi wins, equal values go to the lower body index -- a total order on
// the pairs, so the result does not depend on the order of the takes.  A NaN is never taken.
NBH_HD inline void group_take_r2(GroupSums2& s, double r2, int body) {
  if (r2 > s.r2 || (r2 == s.r2 && body < s.r2_body)) {
    s.r2 = r2;
    s.r2_body = body;
  }
}
NBH_HD inline void group_take_phi(GroupSums2& s, double phi, int body) {
  if (phi < s.phi || (phi == s.phi && body < s.phi_body)) {
    s.phi = phi;
    s.phi_body = body;
  }
}

// One member: d = x - X and u = v - V, then every term as m * (a product or a sum of products), parenthesised as written.
// has_phi false: phi plays no part (the sum stays 0, the minimum stays empty).
NBH_HD inline void group_sums2_add(GroupSums2& s, const GroupBody& b, int body, const GroupCentre& c, bool has_phi, float phi) {
  const double dx = b.x - c.x[0], dy = b.y - c.x[1], dz = b.z - c.x[2];
  const double ux = b.vx - c.v[0], uy = b.vy - c.v[1], uz = b.vz - c.v[2];
  s.v[0] = s.v[0] + b.m * ((dy * uz) - (dz * uy));
  s.v[1] = s.v[1] + b.m * ((dz * ux) - (dx * uz));
  s.v[2] = s.v[2] + b.m * ((dx * uy) - (dy * ux));
  s.v[3] = s.v[3] + b.m * (((ux * ux) + (uy * uy)) + (uz * uz));
  s.v[4] = s.v[4] + b.m * (dx * dx);
  s.v[5] = s.v[5] + b.m * (dy * dy);
  s.v[6] = s.v[6] + b.m * (dz * dz);
  s.v[7] = s.v[7] + b.m * (dx * dy);
  s.v[8] = s.v[8] + b.m * (dx * dz);
  s.v[9] = s.v[9] + b.m * (dy * dz);
  group_take_r2(s, ((dx * dx) + (dy * dy)) + (dz * dz), body);
  if (has_phi) {
    s.v[10] = s.v[10] + b.m * (double)phi;
    group_take_phi(s, (double)phi, body);
  }
}
NBH_HD inline void group_sums2_merge(GroupSums2& a, const GroupSums2& b) {
  for (int k = 0; k < kGroupSums2; k++) a.v[k] = a.v[k] + b.v[k];
  group_take_r2(a, b.r2, b.r2_body);
  group_take_phi(a, b.phi, b.phi_body);
}

// the struct of a bad group: status 1, n 0, nothing else
NBH_HD inline nbody_hip_group_props group_props_bad() {
  nbody_hip_group_props o = {};
  o.status = 1;
  return o;
}

// the struct of a good group of n >= 1 members (the halves are exact: a multiplication by 1/2)
NBH_HD inline nbody_hip_group_props group_props_finish(const GroupCentre& c, const GroupSums2& s, int n, int label, bool has_phi) {
  nbody_hip_group_props o = {};
  o.mass = c.mass;
  for (int a = 0; a < 3; a++) {
    o.com[a] = c.x[a];
    o.vel[a] = c.v[a];
    o.ang_mom[a] = s.v[a];
  }
  o.kinetic = 0.5 * s.v[3];
  for (int a = 0; a < 6; a++) o.inertia[a] = s.v[4 + a];
  o.r_max = sqrt(s.r2 > 0.0 ? s.r2 : 0.0);
  o.r_max_body = s.r2_body == kGroupNoBody ? -1 : s.r2_body;  // (every |d|^2 a NaN: no body)
  o.potential = has_phi ? 0.5 * s.v[10] : 0.0;
  o.phi_min = has_phi && s.phi_body != kGroupNoBody ? s.phi : 0.0;
  o.phi_min_body = has_phi && s.phi_body != kGroupNoBody ? s.phi_body : -1;
  o.n = n;
  o.label = label;
  o.status = 0;
  return o;
}

}  // namespace nbh
