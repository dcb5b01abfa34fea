// system_diag_common.h -- the per-body and per-pair arithmetic of the ensemble diagnostics (include/nbody_hip.h:
// nbody_hip_system_diag) as plain inline functions.  No HIP intrinsics: system_diag.hip runs
// these on the device, system_diag_check.cpp on the host under the sanitizers, so the two evaluate the same
// expressions.  Everything is fp64 with correctly rounded sqrt and / (no fast-math, no rsq, no fp32).
#pragma once

#include <cmath>

#include "nbody_hip.h"

#if defined(__HIPCC__)
#define NBH_HD __host__ __device__
#else
#define NBH_HD
#endif

namespace nbh {

// the state of one body: X = hi + lo and V = hi + lo as exact fp64 sums, m widened
struct DiagBody {
  double x, y, z, vx, vy, vz, m;
};

NBH_HD inline DiagBody diag_body(float px, float py, float pz, float plx, float ply, float plz, float vx, float vy, float vz,
                                 float vlx, float vly, float vlz, float m) {
  // (a float has 24 bits and the two halves overlap by at most their ordering: hi + lo is exact in fp64)
  return DiagBody{(double)px + (double)plx, (double)py + (double)ply, (double)pz + (double)plz,
                  (double)vx + (double)vlx, (double)vy + (double)vly, (double)vz + (double)vlz, (double)m};
}

// the sums over the bodies: mass, sum m X, sum m V, sum m X x V, sum m |V|^2 (kinetic = half of it), and the pair sum
// sum_{i<j} m_i m_j / sqrt(|d|^2 + eps2) (potential = -G times it)
constexpr int kDiagSums = 12;
struct DiagSums {
  double v[kDiagSums];  // 0 mass, 1-3 m X, 4-6 m V, 7-9 m X x V, 10 m |V|^2, 11 the pair sum
};

NBH_HD inline void diag_sums_zero(DiagSums& s) {
  for (int k = 0; k < kDiagSums; k++) s.v[k] = 0.0;
}

NBH_HD inline void diag_body_add(DiagSums& s, const DiagBody& b) {
  s.v[0] += b.m;
  s.v[1] += b.m * b.x;
  s.v[2] += b.m * b.y;
  s.v[3] += b.m * b.z;
  s.v[4] += b.m * b.vx;
  s.v[5] += b.m * b.vy;
  s.v[6] += b.m * b.vz;
  s.v[7] += b.m * (b.y * b.vz - b.z * b.vy);
  s.v[8] += b.m * (b.z * b.vx - b.x * b.vz);
  s.v[9] += b.m * (b.x * b.vy - b.y * b.vx);
  s.v[10] += b.m * (b.vx * b.vx + b.vy * b.vy + b.vz * b.vz);
}

// a minimum over pairs with its pair: ties go to the lexicographically smallest (i, j); i < 0: no candidate yet.  A
// NaN value is never taken.
struct DiagMin {
  double v;
  int i, j;
};

NBH_HD inline DiagMin diag_min_none(double v) { return DiagMin{v, -1, -1}; }

NBH_HD inline void diag_min_take(DiagMin& m, double v, int i, int j) {
  if (!(v == v)) return;
  const bool first = m.i < 0;
  const bool smaller = v < m.v;
  const bool tie = v == m.v && (i < m.i || (i == m.i && j < m.j));
  if (first || smaller || tie) {
    m.v = v;
    m.i = i;
    m.j = j;
  }
}

NBH_HD inline void diag_min_merge(DiagMin& m, const DiagMin& o) {
  if (o.i >= 0) diag_min_take(m, o.v, o.i, o.j);
}

// one pair i < j, d = X_j - X_i, w = V_j - V_i
struct DiagPair {
  double term;    // m_i m_j / sqrt(|d|^2 + eps2); 0 when |d|^2 + eps2 == 0
  double r;       // |d|, unsoftened
  double eb;      // 1/2 mu |w|^2 - G m_i m_j / r, mu = m_i m_j / (m_i + m_j); meaningful only when bindable
  bool bindable;  // r > 0 and m_i + m_j > 0
};

NBH_HD inline double diag_binding_energy(const DiagBody& a, const DiagBody& b, double r, double G) {
  const double wx = b.vx - a.vx, wy = b.vy - a.vy, wz = b.vz - a.vz;
  const double mm = a.m * b.m;
  const double mu = mm / (a.m + b.m);
  return 0.5 * mu * (wx * wx + wy * wy + wz * wz) - G * mm / r;
}

NBH_HD inline DiagPair diag_pair(const DiagBody& a, const DiagBody& b, double G, double eps2) {
  const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  const double r2 = dx * dx + dy * dy + dz * dz;
  const double h = r2 + eps2;
  DiagPair p;
  p.term = h == 0.0 ? 0.0 : a.m * b.m / sqrt(h);
  p.r = sqrt(r2);
  p.bindable = p.r > 0.0 && a.m + b.m > 0.0;
  p.eb = p.bindable ? diag_binding_energy(a, b, p.r, G) : 0.0;
  return p;
}

// the two-body (Kepler) elements of a pair with binding energy eb < 0: a = -G m_i m_j / (2 eb), h = d x w,
// e = sqrt(max(0, 1 + 2 (eb / mu) |h|^2 / (G (m_i + m_j))^2))
NBH_HD inline void diag_elements(const DiagBody& a, const DiagBody& b, double G, double eb, double* semi, double* ecc) {
  const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  const double wx = b.vx - a.vx, wy = b.vy - a.vy, wz = b.vz - a.vz;
  const double hx = dy * wz - dz * wy, hy = dz * wx - dx * wz, hz = dx * wy - dy * wx;
  const double mm = a.m * b.m, ms = a.m + b.m;
  const double mu = mm / ms;
  const double gm = G * ms;
  const double q = 1.0 + 2.0 * (eb / mu) * (hx * hx + hy * hy + hz * hz) / (gm * gm);
  *semi = -G * mm / (2.0 * eb);
  *ecc = sqrt(q > 0.0 ? q : 0.0);
}

// The pairs of a system of n bodies as a rectangle of R = ceil(n / 2) rows and C = n - 1 columns.  Cell (r, c) is
//   c <  C - r:  the pair (r, r + 1 + c)                 (row r of the triangle, its n - 1 - r pairs)
//   c >= C - r:  the pair (n - 1 - r, c + 1)             (row n - 1 - r, its r pairs)
// and, for odd n, the second half of the middle row r = (n - 1) / 2 is empty (it would repeat the first).  Every pair
// i < j appears once.  The cells are dealt to T workers in contiguous runs of q = ceil(R C / T): worker t takes the
// cells [t q, (t + 1) q) in index order, so no worker adds more than q pair terms.
struct DiagCells {
  int n, C, R, M, q;
};

NBH_HD inline DiagCells diag_cells(int n, int workers) {
  DiagCells s;
  s.n = n;
  s.C = n - 1;
  s.R = (n + 1) / 2;
  s.M = s.R * s.C;
  s.q = (s.M + workers - 1) / workers;
  return s;
}

NBH_HD inline int diag_imin(int a, int b) { return a < b ? a : b; }
NBH_HD inline int diag_imax(int a, int b) { return a > b ? a : b; }

// the cells [a, b) of worker t, and the rows [r0, r1) they touch
NBH_HD inline void diag_worker_cells(const DiagCells& s, int t, int* a, int* b, int* r0, int* r1) {
  *a = diag_imin(t * s.q, s.M);
  *b = diag_imin(*a + s.q, s.M);
  *r0 = *r1 = 0;
  if (*b > *a) {  // (then C >= 1)
    *r0 = *a / s.C;
    *r1 = (*b - 1) / s.C + 1;
  }
}

// The pairs that the cells [a, b) hold in row r with their second body in the source tile [t0, t1): two runs
// (i, j), jlo <= j < jhi, one per half of the row; a run with jlo >= jhi is empty.  Every j is in [i + 1, n).
struct DiagRun {
  int i, jlo, jhi;
};

NBH_HD inline void diag_row_runs(const DiagCells& s, int a, int b, int r, int t0, int t1, DiagRun* first, DiagRun* second) {
  const int base = r * s.C;
  const int c_lo = diag_imax(a - base, 0), c_hi = diag_imin(b - base, s.C);
  const int split = s.C - r;  // the cells of the pair (r, .) end here
  first->i = r;
  first->jlo = diag_imax(r + 1 + c_lo, t0);
  first->jhi = diag_imin(r + 1 + diag_imin(c_hi, split), t1);
  const int i2 = s.n - 1 - r;
  second->i = i2;
  second->jlo = diag_imax(diag_imax(c_lo, split) + 1, t0);
  second->jhi = i2 == r ? second->jlo : diag_imin(c_hi + 1, t1);
}

// The struct of one legal system from its reduced sums and minima.  bi / bj: the bodies of bind (read only when it has a
// pair with eb < 0).
NBH_HD inline void diag_finish(const DiagSums& s, const DiagMin& sep, const DiagMin& bind, const DiagBody& bi,
                               const DiagBody& bj, double G, int n, nbody_hip_system_diag* o) {
  const double mass = s.v[0];
  o->mass = mass;
  for (int c = 0; c < 3; c++) {
    o->com[c] = mass == 0.0 ? 0.0 : s.v[1 + c] / mass;
    o->momentum[c] = s.v[4 + c];
    o->ang_mom[c] = s.v[7 + c];
  }
  o->kinetic = 0.5 * s.v[10];
  o->potential = -G * s.v[11];
  o->min_sep = sep.i < 0 ? INFINITY : sep.v;
  o->min_i = sep.i;
  o->min_j = sep.j;
  o->bind_energy = o->bind_a = o->bind_e = 0.0;
  o->bind_i = o->bind_j = -1;
  if (bind.i >= 0 && bind.v < 0.0) {
    o->bind_energy = bind.v;
    o->bind_i = bind.i;
    o->bind_j = bind.j;
    diag_elements(bi, bj, G, bind.v, &o->bind_a, &o->bind_e);
  }
  o->n = n;
  o->status = 0;
}

}  // namespace nbh
