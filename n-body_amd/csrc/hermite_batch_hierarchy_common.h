// hermite_batch_hierarchy_common.h -- the arithmetic of the ensemble hierarchies (include/nbody_hip.h: "ensemble
// HIERARCHIES", nbody_hip_batch_hierarchy_t, nbody_hip_batch_node_t) as plain inline functions,
// after the pattern of hermite_batch_outcomes_common.h.  No HIP intrinsics: hermite_batch.hip runs these on the device,
// hermite_batch_hierarchy_check.cpp on the host under the sanitizers, so the two evaluate the same expressions.
// Everything is fp64 with correctly rounded sqrt and /, no product is fused into a sum, sums of three terms go left to
// right: every operation rounds once, which is what the restatement of the tests does.
#pragma once

#include <cmath>

#include "hermite_batch_outcomes_common.h"

namespace nbh {

constexpr int kHierMax = NBODY_HIP_BATCH_HIERARCHY_MAX;  // bodies of an examined system
constexpr int kHierNodes = 2 * kHierMax;                 // slots of its table (2 n - 1 are ever used)
constexpr unsigned int kHierNone = 0xffffffffu;

// a node is a body: {m, X, V} (a composite: the sum of the masses and the centre of mass)
typedef DiagBody HierNode;

// one pair p < q of the top set: d = X_q - X_p, w = V_q - V_p
struct HierPair {
  double M, r, eps, dw, a;  // a: only of a candidate, else 0
  bool candidate;           // M > 0 and r > 0 and eps < 0
};

NBH_HD inline HierPair hier_pair(const HierNode& p, const HierNode& q, double G) {
  NBH_NO_CONTRACT
  const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
  const double wx = q.vx - p.vx, wy = q.vy - p.vy, wz = q.vz - p.vz;
  HierPair o;
  o.M = p.m + q.m;
  o.r = sqrt(dx * dx + dy * dy + dz * dz);
  const double v2 = wx * wx + wy * wy + wz * wz;
  o.eps = 0.5 * v2 - (G * o.M) / o.r;
  o.dw = dx * wx + dy * wy + dz * wz;
  o.candidate = o.M > 0.0 && o.r > 0.0 && o.eps < 0.0;  // (a NaN anywhere: false)
  o.a = o.candidate ? (G * o.M) / (-2.0 * o.eps) : 0.0;
  return o;
}

// the eccentricity of a pair from its eps and M: h = d x w
NBH_HD inline double hier_ecc(const HierNode& p, const HierNode& q, double G, double M, double eps) {
  NBH_NO_CONTRACT
  const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
  const double wx = q.vx - p.vx, wy = q.vy - p.vy, wz = q.vz - p.vz;
  const double hx = dy * wz - dz * wy, hy = dz * wx - dx * wz, hz = dx * wy - dy * wx;
  const double h2 = hx * hx + hy * hy + hz * hz;
  const double gm = G * M;
  const double t = 1.0 + ((2.0 * eps) * h2) / (gm * gm);
  return sqrt(t > 0.0 ? t : 0.0);
}

// the composite of p and q: both products rounded, then the sum, then the quotient
NBH_HD inline HierNode hier_composite(const HierNode& p, const HierNode& q, double M) {
  NBH_NO_CONTRACT
  HierNode c;
  c.m = M;
  c.x = (p.m * p.x + q.m * q.x) / M;
  c.y = (p.m * p.y + q.m * q.y) / M;
  c.z = (p.m * p.z + q.m * q.z) / M;
  c.vx = (p.m * p.vx + q.m * q.vx) / M;
  c.vy = (p.m * p.vy + q.m * q.vy) / M;
  c.vz = (p.m * p.vz + q.m * q.vz) / M;
  return c;
}

// a (1 + e) of a composite, 0 of a leaf
NBH_HD inline double hier_apo(double a, double e) {
  NBH_NO_CONTRACT
  return a * (1.0 + e);
}

// the four criteria of one top pair
NBH_HD inline bool hier_pair_resolved(const HierPair& o, double apo_p, double apo_q, double r_sep, double kappa) {
  NBH_NO_CONTRACT
  return o.r > r_sep && o.dw > 0.0 && o.eps > 0.0 && o.r > kappa * (apo_p + apo_q);
}

// The order of the reductions: a minimum of integer keys (value bits, then p, then q), so it depends on no lane, wave or
// thread order.  The value is a > 0 of a candidate or r >= 0 of a top pair: the bits of a non-negative double order as
// unsigned integers.  None: above every key.
struct HierKey {
  unsigned long long bits;
  unsigned int pq;  // p << 8 | q, node ids below 128
};

NBH_HD inline HierKey hier_key_none() { return HierKey{~0ull, kHierNone}; }
NBH_HD inline HierKey hier_key(double v, unsigned int p, unsigned int q) {
  HierKey k;
  __builtin_memcpy(&k.bits, &v, sizeof(double));
  k.pq = (p << 8) | q;
  return k;
}
NBH_HD inline bool hier_key_less(const HierKey& a, const HierKey& b) {
  return a.bits < b.bits || (a.bits == b.bits && a.pq < b.pq);
}
NBH_HD inline bool hier_key_is_none(const HierKey& k) { return k.pq == kHierNone; }
NBH_HD inline double hier_key_value(const HierKey& k) {
  double v;
  __builtin_memcpy(&v, &k.bits, sizeof(double));
  return v;
}

// pair t of the K (K - 1) / 2 pairs i < j of a list of K entries, in the order (0,1), (0,2), (1,2), (0,3), ...:
// j is the largest integer with j (j - 1) / 2 <= t.  t < 2,016: the fp32 root is off by at most one, which the two
// corrections take back.
NBH_HD inline void hier_pair_index(int t, int* i, int* j) {
  int jj = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
  if (jj * (jj - 1) / 2 > t) jj--;
  if ((jj + 1) * jj / 2 <= t) jj++;
  *j = jj;
  *i = t - jj * (jj - 1) / 2;
}

NBH_HD inline void hier_node_leaf(nbody_hip_batch_node_t* s, double m) {
  s->left = s->right = s->parent = kHierNone;
  s->bodies = 1u;
  s->mass = m;
  s->a = s->e = s->r = s->energy = s->reserved = 0.0;
}

NBH_HD inline void hier_record_none(nbody_hip_batch_hierarchy_t* rec) {
  rec->resolved = rec->top_count = 0u;
  rec->macro = 0ull;
  rec->node_count = rec->largest = 0u;
  rec->min_sep = INFINITY;
  rec->min_p = rec->min_q = kHierNone;
  rec->reserved[0] = rec->reserved[1] = rec->reserved[2] = 0.0;
}

// The whole decomposition of one system of 2 <= n <= kHierMax bodies as one sequential program, for the host check: the
// device runs the same functions with the pairs dealt over 512 threads and the keys reduced by minima.  body(i): the
// HierNode of body i.  table: 2 n slots, all written (those at and above node_count with zeros).
template <class BodyAt>
inline void hierarchy_model(int n, BodyAt body, double G, double r_sep, double kappa, unsigned long long macro,
                            nbody_hip_batch_hierarchy_t* rec, nbody_hip_batch_node_t* table) {
  HierNode node[kHierNodes];
  int top[kHierMax];
  for (int i = 0; i < 2 * n; i++) {
    table[i] = nbody_hip_batch_node_t{};
  }
  for (int i = 0; i < n; i++) {
    node[i] = body(i);
    top[i] = i;
    hier_node_leaf(&table[i], node[i].m);
  }
  int K = n, count = n;
  for (int k = 0; k < n - 1; k++) {
    HierKey best = hier_key_none();
    for (int i = 0; i < K; i++)
      for (int j = i + 1; j < K; j++) {
        const HierPair o = hier_pair(node[top[i]], node[top[j]], G);
        if (!o.candidate) continue;
        const HierKey key = hier_key(o.a, (unsigned int)top[i], (unsigned int)top[j]);
        if (hier_key_less(key, best)) best = key;
      }
    if (hier_key_is_none(best)) break;
    const int p = (int)(best.pq >> 8), q = (int)(best.pq & 0xffu), c = count++;
    const HierPair o = hier_pair(node[p], node[q], G);
    node[c] = hier_composite(node[p], node[q], o.M);
    nbody_hip_batch_node_t* s = &table[c];
    s->left = (unsigned int)p;
    s->right = (unsigned int)q;
    s->parent = kHierNone;
    s->bodies = table[p].bodies + table[q].bodies;
    s->mass = o.M;
    s->a = o.a;
    s->e = hier_ecc(node[p], node[q], G, o.M, o.eps);
    s->r = o.r;
    s->energy = o.eps;
    s->reserved = 0.0;
    table[p].parent = table[q].parent = (unsigned int)c;
    int K2 = 0;
    for (int i = 0; i < K; i++)
      if (top[i] != p && top[i] != q) top[K2++] = top[i];
    top[K2++] = c;  // (the largest id: the list stays in rising order)
    K = K2;
  }
  HierKey sep = hier_key_none();
  unsigned int failed = 0u, largest = 0u;
  for (int i = 0; i < K; i++) {
    if (table[top[i]].bodies > largest) largest = table[top[i]].bodies;
    for (int j = i + 1; j < K; j++) {
      const int p = top[i], q = top[j];
      const HierPair o = hier_pair(node[p], node[q], G);
      if (!hier_pair_resolved(o, hier_apo(table[p].a, table[p].e), hier_apo(table[q].a, table[q].e), r_sep, kappa)) failed++;
      if (o.r == o.r) {  // (a NaN separation is never the smallest)
        const HierKey key = hier_key(o.r, (unsigned int)p, (unsigned int)q);
        if (hier_key_less(key, sep)) sep = key;
      }
    }
  }
  hier_record_none(rec);
  rec->resolved = K >= 2 && failed == 0u ? 1u : 0u;
  rec->top_count = (unsigned int)K;
  rec->macro = macro;
  rec->node_count = (unsigned int)count;
  rec->largest = largest;
  if (!hier_key_is_none(sep)) {
    rec->min_sep = hier_key_value(sep);
    rec->min_p = sep.pq >> 8;
    rec->min_q = sep.pq & 0xffu;
  }
}

}  // namespace nbh
