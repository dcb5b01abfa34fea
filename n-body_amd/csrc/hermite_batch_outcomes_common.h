// hermite_batch_outcomes_common.h -- the per-body arithmetic of the ensemble outcomes (include/nbody_hip.h: "ensemble
// OUTCOMES", nbody_hip_batch_outcome_t) as plain inline functions, after the pattern of
// system_diag_common.h.  No HIP intrinsics: hermite_batch.hip runs these on the device, hermite_batch_outcomes_check.cpp
// on the host under the sanitizers, so the two evaluate the same expressions.  Everything is fp64 with correctly rounded
// sqrt and / (no fast-math, no rsq, no fp32), and no product is fused into a sum: every operation rounds once, which is
// what the numpy restatement of the tests does.
#pragma once

#include <cmath>

#include "system_diag_common.h"

#if defined(__clang__)
#define NBH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NBH_NO_CONTRACT  // (g++ for the host check: built without -ffp-contract=fast and without FMA code generation)
#endif

namespace nbh {

// the sums over the bodies of a system: 0 mass, 1-3 m X, 4-6 m V
constexpr int kOutcomeSums = 7;
struct OutcomeSums {
  double v[kOutcomeSums];
};

NBH_HD inline void outcome_sums_zero(OutcomeSums& s) {
  for (int k = 0; k < kOutcomeSums; k++) s.v[k] = 0.0;
}

NBH_HD inline void outcome_body_add(OutcomeSums& s, const DiagBody& b) {
  NBH_NO_CONTRACT
  s.v[0] += b.m;
  s.v[1] += b.m * b.x;
  s.v[2] += b.m * b.y;
  s.v[3] += b.m * b.z;
  s.v[4] += b.m * b.vx;
  s.v[5] += b.m * b.vy;
  s.v[6] += b.m * b.vz;
}

// a += b, component by component (a lane taking another lane's sums, a wave's sums joining the total)
NBH_HD inline void outcome_sums_add(OutcomeSums& a, const OutcomeSums& b) {
  for (int k = 0; k < kOutcomeSums; k++) a.v[k] += b.v[k];
}

// one body against the centre of mass of all the rest
struct OutcomeBody {
  double r, vr, e, rest_mass;  // all 0 when the rest has no mass
  double dw;                   // d.w: the sign the test looks at (vr = dw / r)
  bool escapes;
};

NBH_HD inline OutcomeBody outcome_body(const OutcomeSums& S, const DiagBody& b, double G, double r_esc) {
  NBH_NO_CONTRACT
  OutcomeBody o{0.0, 0.0, 0.0, 0.0, 0.0, false};
  const double mr = S.v[0] - b.m;
  if (!(mr > 0.0)) return o;  // (the rest is massless, or NaN: never an escape)
  const double Rx = (S.v[1] - b.m * b.x) / mr, Ry = (S.v[2] - b.m * b.y) / mr, Rz = (S.v[3] - b.m * b.z) / mr;
  const double Ux = (S.v[4] - b.m * b.vx) / mr, Uy = (S.v[5] - b.m * b.vy) / mr, Uz = (S.v[6] - b.m * b.vz) / mr;
  const double dx = b.x - Rx, dy = b.y - Ry, dz = b.z - Rz;
  const double wx = b.vx - Ux, wy = b.vy - Uy, wz = b.vz - Uz;
  const double r = sqrt(dx * dx + dy * dy + dz * dz);
  const double dw = dx * wx + dy * wy + dz * wz;
  o.rest_mass = mr;
  o.r = r;
  o.dw = dw;
  o.vr = dw / r;
  o.e = 0.5 * (wx * wx + wy * wy + wz * wz) - (G * S.v[0]) / r;
  o.escapes = r > r_esc && dw > 0.0 && o.e > 0.0;  // (a NaN anywhere: false)
  return o;
}

// The sums of a system in the model's order, as one sequential program: `lanes` workers of which worker t starts from 0
// and adds the bodies t, t + lanes, ...; then inside every wave of `wave` workers lane l takes lane l + off for
// off = wave / 2 ... 1; then the waves' sums in rising order.  body(i) returns the DiagBody of body i.  The device runs
// the same three stages on 512 threads; this form is for the host check.  scratch: lanes entries.
template <class BodyAt>
inline OutcomeSums outcome_sums_model(int n, int lanes, int wave, OutcomeSums* scratch, BodyAt body) {
  for (int t = 0; t < lanes; t++) {
    outcome_sums_zero(scratch[t]);
    for (int i = t; i < n; i += lanes) outcome_body_add(scratch[t], body(i));
  }
  for (int w0 = 0; w0 < lanes; w0 += wave)
    for (int off = wave / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; l++) outcome_sums_add(scratch[w0 + l], scratch[w0 + l + off]);
  OutcomeSums total = scratch[0];
  for (int w0 = wave; w0 < lanes; w0 += wave) outcome_sums_add(total, scratch[w0]);
  return total;
}

}  // namespace nbh
