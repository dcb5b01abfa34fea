// hop_common.h -- the arithmetic of the density-peak (HOP) groups (hop_groups.hip; the model is in
// include/nbody_hip_hop.h) as plain C++: the order `better`, live and viable, the boundary value
// of a pair and its bits, the edge key, and the status rule.  No HIP include: hop_check.cpp runs all of it on a CPU under
// AddressSanitizer and UBSan (make hop_check).  Both this file's users are built with -ffp-contract=off.
#pragma once

#include <cstring>

#ifdef __HIPCC__
#define HOP_HD __host__ __device__ inline
#else
#define HOP_HD inline
#endif

namespace nbh {

// better(j, b): j is a better hop target than b.  fp64 compares: a NaN density is never better and is never beaten;
// -0 and +0 are equal densities (the lower index wins).
HOP_HD bool hop_better(double rho_j, int j, double rho_b, int b) {
  return rho_j > rho_b || (rho_j == rho_b && j < b);
}

// live(i): false for a NaN
HOP_HD bool hop_live(double rho, double delta_outer) { return rho >= delta_outer; }
// viable(P) of a peak
HOP_HD bool hop_viable(double rho, double delta_outer, double delta_peak) {
  return hop_live(rho, delta_outer) && rho >= delta_peak;
}

// A slot of a row: 0 no neighbour (negative), 1 a neighbour, 2 an index at or past count (the call's status becomes 1)
HOP_HD int hop_slot(int j, int count) { return j < 0 ? 0 : (j < count ? 1 : 2); }

// b(i, j) = (rho_i + rho_j) * 0.5: two roundings, nothing fused (the files that include this are not contracted)
HOP_HD double hop_boundary(double rho_i, double rho_j) {
  const double s = rho_i + rho_j;
  return s * 0.5;
}

// The bits of a boundary value, ordered as unsigned integers the way the values are ordered as doubles: live densities are
// >= delta_outer >= 0, so b >= 0 (+inf included) and is no NaN; a -0 (two live -0 densities at delta_outer = 0) counts as
// the +0 it equals.
HOP_HD unsigned long long hop_boundary_bits(double b) {
  unsigned long long u;
#ifdef __HIP_DEVICE_COMPILE__
  u = (unsigned long long)__double_as_longlong(b);
#else
  std::memcpy(&u, &b, sizeof u);
#endif
  return u == 0x8000000000000000ull ? 0ull : u;
}
HOP_HD double hop_boundary_from_bits(unsigned long long u) {
#ifdef __HIP_DEVICE_COMPILE__
  return __longlong_as_double((long long)u);
#else
  double b;
  std::memcpy(&b, &u, sizeof b);
  return b;
#endif
}

// bits needed to tell the values 0 .. v - 1 apart (v >= 1): 0 for 1, 1 for 2, 2 for 3 and 4
HOP_HD int hop_bits_for(long long v) {
  int b = 0;
  while (b < 62 && (1LL << b) < v) b++;
  return b;
}
// The key of a directed boundary record (P, Q), both body indices below count: (P << qbits) | Q with
// qbits = hop_bits_for(count) <= 30.  One stable sort of bits [0, 2 qbits) puts the records of a peak P side by side, in
// ascending Q.
HOP_HD unsigned long long hop_edge_key(int P, int Q, int qbits) {
  return ((unsigned long long)(unsigned int)P << qbits) | (unsigned long long)(unsigned int)Q;
}
HOP_HD int hop_key_p(unsigned long long key, int qbits) { return (int)(key >> qbits); }
HOP_HD int hop_key_q(unsigned long long key, int qbits) { return (int)(key & ((1ull << qbits) - 1ull)); }

// the status of a call: 0, or 1 when a read slot held an index at or past count (then: no group, every label and peak -1)
HOP_HD int hop_status(int bad_index_flag) { return bad_index_flag ? 1 : 0; }

// One attachment choice: among a peak's edges {Q, S} with Q anchored before the round, the greatest S, ties to the
// lowest Q.  Fed in ascending Q (the order of the sorted edges), the result is true when (S, Q) replaces the choice so
// far; S as hop_boundary_bits, which order as the values do.
HOP_HD bool hop_attach_take(bool have, unsigned long long s_best, unsigned long long s) { return !have || s > s_best; }

}  // namespace nbh
