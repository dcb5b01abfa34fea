// hermite_batch_mergers_common.h -- the arithmetic of the ensemble mergers (include/nbody_hip.h: "ensemble MERGERS",
// nbody_hip_batch_merger_t) as plain inline functions, after the pattern of
// hermite_batch_outcomes_common.h.  No HIP intrinsics: hermite_batch.hip runs these on the device,
// hermite_batch_mergers_check.cpp on the host under the sanitizers, so the two evaluate the same expressions: which
// record merges, the slots, the merged body and what is stored of it, the radius rule, the kinetic delta and the pair
// terms of the potential delta.  Everything is fp64 with correctly rounded sqrt and /; no product is fused into a sum
// (the one freedom the model grants, the contraction of ma Xa + mb Xb, is not taken).
#pragma once

#include <cmath>

#include "hermite_batch_outcomes_common.h"

namespace nbh {

constexpr unsigned int kMergerNone = 0xffffffffu;

// ---- the slot bookkeeping -----------------------------------------------------------------------------------------------
// what one pass does to the slots of a system of n live bodies whose record names the pair (ci, cj)
struct MergerSlots {
  bool valid;               // two different slots, both below n
  unsigned int lo, hi;      // min and max of the pair: the merged body takes lo, hi is refilled or dies
  unsigned int moved_from;  // n - 1 when the last live body moves into hi, kMergerNone when hi is the last
  unsigned int dead;        // n - 1: the slot that leaves the live range
};

NBH_HD inline MergerSlots merger_slots(unsigned int ci, unsigned int cj, unsigned int n) {
  MergerSlots s{false, kMergerNone, kMergerNone, kMergerNone, kMergerNone};
  if (ci == cj || ci >= n || cj >= n) return s;  // (n >= 2 follows; "none" is 0xFFFFFFFF and fails here too)
  s.valid = true;
  s.lo = ci < cj ? ci : cj;
  s.hi = ci < cj ? cj : ci;
  s.dead = n - 1u;
  s.moved_from = s.hi == s.dead ? kMergerNone : s.dead;
  return s;
}

// a pass acts on a system iff it stopped on contact (stop word 1), its status word is 0 and the record is valid
NBH_HD inline bool merger_concerned(unsigned int stopped, unsigned int status) { return stopped == 1u && status == 0u; }

// ---- the merged body ----------------------------------------------------------------------------------------------------
// the radius of the merged body: the volume rule, rounded to fp32
NBH_HD inline float merger_radius(float ra, float rb) {
  NBH_NO_CONTRACT
  const double a = (double)ra, b = (double)rb;
  return (float)cbrt(a * a * a + b * b * b);
}

// what is stored of one component: hi = (float)v and, in extended state precision, lo = (float)(v - hi); else lo = 0
struct MergerSplit {
  float hi, lo;
};
NBH_HD inline MergerSplit merger_split(double v, bool ext) {
  MergerSplit s;
  s.hi = (float)v;
  s.lo = ext ? (float)(v - (double)s.hi) : 0.0f;
  return s;
}

struct MergerBody {
  double M;                               // (double)ma + (double)mb
  float mass;                             // (float)M, the stored mass
  MergerSplit x, y, z, vx, vy, vz;        // the stored state
};

// a (slot lo) and b (slot hi) as the full fp64 state (hi + lo).  M == 0: the plain mean of positions and velocities.
NBH_HD inline MergerBody merger_merge(const DiagBody& a, const DiagBody& b, bool ext) {
  NBH_NO_CONTRACT
  MergerBody o;
  o.M = a.m + b.m;
  o.mass = (float)o.M;
  double X[6];
  if (o.M == 0.0) {
    X[0] = 0.5 * (a.x + b.x);   X[1] = 0.5 * (a.y + b.y);   X[2] = 0.5 * (a.z + b.z);
    X[3] = 0.5 * (a.vx + b.vx); X[4] = 0.5 * (a.vy + b.vy); X[5] = 0.5 * (a.vz + b.vz);
  } else {
    X[0] = (a.m * a.x + b.m * b.x) / o.M;   X[1] = (a.m * a.y + b.m * b.y) / o.M;   X[2] = (a.m * a.z + b.m * b.z) / o.M;
    X[3] = (a.m * a.vx + b.m * b.vx) / o.M; X[4] = (a.m * a.vy + b.m * b.vy) / o.M; X[5] = (a.m * a.vz + b.m * b.vz) / o.M;
  }
  o.x = merger_split(X[0], ext);  o.y = merger_split(X[1], ext);  o.z = merger_split(X[2], ext);
  o.vx = merger_split(X[3], ext); o.vy = merger_split(X[4], ext); o.vz = merger_split(X[5], ext);
  return o;
}

// the merged body as the diagnostics will read it back: from the values as stored
NBH_HD inline DiagBody merger_stored(const MergerBody& o) {
  return diag_body(o.x.hi, o.y.hi, o.z.hi, o.x.lo, o.y.lo, o.z.lo, o.vx.hi, o.vy.hi, o.vz.hi, o.vx.lo, o.vy.lo, o.vz.lo,
                   o.mass);
}

// ---- the energy deltas, from the values as stored ------------------------------------------------------------------------
NBH_HD inline double merger_kinetic(const DiagBody& b) {
  NBH_NO_CONTRACT
  return 0.5 * (b.m * (b.vx * b.vx + b.vy * b.vy + b.vz * b.vz));  // (the diagnostics: half of sum m |V|^2)
}

// delta_ke = 1/2 M |V|^2 - 1/2 ma |Va|^2 - 1/2 mb |Vb|^2
NBH_HD inline double merger_delta_ke(const DiagBody& merged, const DiagBody& a, const DiagBody& b) {
  NBH_NO_CONTRACT
  return (merger_kinetic(merged) - merger_kinetic(a)) - merger_kinetic(b);
}

// what another live body k adds to the pair sum (the diagnostics' sum of m_i m_j / sqrt(|d|^2 + eps2)): its new term with
// the merged body minus its two old terms
NBH_HD inline double merger_pair_delta(const DiagBody& merged, const DiagBody& a, const DiagBody& b, const DiagBody& k,
                                       double eps2) {
  NBH_NO_CONTRACT
  return (diag_pair(merged, k, 0.0, eps2).term - diag_pair(a, k, 0.0, eps2).term) - diag_pair(b, k, 0.0, eps2).term;
}

// delta_pe = -G (sum over the others of merger_pair_delta  -  the pair's own term)
NBH_HD inline double merger_delta_pe(double others, const DiagBody& a, const DiagBody& b, double G, double eps2) {
  NBH_NO_CONTRACT
  return -G * (others - diag_pair(a, b, 0.0, eps2).term);
}

// The sum over the others in the model's order, as one sequential program: `lanes` workers of which worker t starts from
// 0 and adds the terms of k = t, t + lanes, ... (k != lo, hi; k < n); then inside every wave of `wave` workers lane l
// takes lane l + off for off = wave / 2 ... 1; then the waves' sums in rising order.  The device runs the same three
// stages on 256 threads; this form is for the host check.  scratch: lanes entries.
template <class TermAt>
inline double merger_others_model(int n, int lo, int hi, int lanes, int wave, double* scratch, TermAt term) {
  for (int t = 0; t < lanes; t++) {
    scratch[t] = 0.0;
    for (int k = t; k < n; k += lanes)
      if (k != lo && k != hi) scratch[t] += term(k);
  }
  for (int w0 = 0; w0 < lanes; w0 += wave)
    for (int off = wave / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; l++) scratch[w0 + l] += scratch[w0 + l + off];
  double total = scratch[0];
  for (int w0 = wave; w0 < lanes; w0 += wave) total += scratch[w0];
  return total;
}

}  // namespace nbh
