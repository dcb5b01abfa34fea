// group_props_check.cpp -- the arithmetic of the group properties (group_props_common.h) on a CPU, under
// AddressSanitizer and UBSan and without contraction (make group_props_check).  group_struct() below sums a group in
// the ORDER OF THE MODEL (include/nbody_hip_group_props.h: serially up to S members; else chunks of C, 256 sums per chunk
// folded 32, 16, .., 1 in runs of 64 and the runs in order, the chunk sums folded the same way) with the very functions
// the kernels call.  It is held against
//   * known answers on an exact lattice (mirrored pairs about an integer centre: every sum exact, so any order must give
//     the same struct as a plain loop in integers), at every size at which the order changes;
//   * a long double restatement in plain member order on random data, within (n + 8) 2^-53 of the absolute sums;
//   * the rules of the extrema: ties to the lowest body index whatever the member order, NaN never taken;
//   * the special cases: mass 0, no phi, one member, the bad struct.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "group_props_common.h"
#include "group_props_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
#define EXPECT(cond, ...)              \
  do {                                 \
    checked++;                         \
    if (!(cond)) {                     \
      if (failures++ < 40) {           \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

struct Bodies {
  std::vector<float> x, y, z, vx, vy, vz, m, phi;
  std::vector<int> index;  // the body index of every member (the order of the list is the order of the sums)
  size_t n() const { return m.size(); }
  GroupBody body(size_t p) const { return group_body(x[p], y[p], z[p], vx[p], vy[p], vz[p], m[p]); }
};

template <class S>
static void merge(S& a, const S& b);
template <>
void merge(GroupSums1& a, const GroupSums1& b) { group_sums1_merge(a, b); }
template <>
void merge(GroupSums2& a, const GroupSums2& b) { group_sums2_merge(a, b); }
static void zero(GroupSums1& s) { group_sums1_zero(s); }
static void zero(GroupSums2& s) { group_sums2_zero(s); }

// 64 sums folded as a wave folds them: s[l] += s[l + off] for l < off, off = 32, 16, .., 1
template <class S>
static S fold64(std::vector<S> s) {
  for (int off = 32; off > 0; off >>= 1)
    for (int l = 0; l < off; l++) merge(s[l], s[l + off]);
  return s[0];
}

// the sum of a group in the order of the model; add(s, p) adds member p
template <class S, class Add>
static S model_sum(size_t n, Add add) {
  S total;
  zero(total);
  if (n <= (size_t)kGroupSmall) {
    for (size_t p = 0; p < n; p++) add(total, p);
    return total;
  }
  const size_t chunks = (size_t)group_chunks((long long)n);
  std::vector<S> chunk_sum(chunks);
  for (size_t k = 0; k < chunks; k++) {
    const size_t base = k * kGroupChunk, end = std::min(base + kGroupChunk, n);
    std::vector<S> t(kGroupThreads);
    for (int i = 0; i < kGroupThreads; i++) {
      zero(t[i]);
      for (int j = 0; j < kGroupPerThread; j++) {
        const size_t p = base + (size_t)j * kGroupThreads + i;
        if (p < end) add(t[i], p);
      }
    }
    S c;
    for (int w = 0; w < kGroupThreads / 64; w++) {
      const S run = fold64(std::vector<S>(t.begin() + 64 * w, t.begin() + 64 * (w + 1)));
      if (w == 0) c = run; else merge(c, run);
    }
    chunk_sum[k] = c;
  }
  std::vector<S> lane(64);
  for (int l = 0; l < 64; l++) {
    zero(lane[l]);
    for (size_t k = l; k < chunks; k += 64) merge(lane[l], chunk_sum[k]);
  }
  return fold64(lane);
}

static nbody_hip_group_props group_struct(const Bodies& b, bool has_phi) {
  const GroupSums1 s1 = model_sum<GroupSums1>(b.n(), [&](GroupSums1& s, size_t p) { group_sums1_add(s, b.body(p)); });
  const GroupCentre c = group_centre(s1);
  const GroupSums2 s2 = model_sum<GroupSums2>(b.n(), [&](GroupSums2& s, size_t p) {
    group_sums2_add(s, b.body(p), b.index[p], c, has_phi, has_phi ? b.phi[p] : 0.0f);
  });
  return group_props_finish(c, s2, (int)b.n(), b.index[0], has_phi);
}

// the lattice of the tests: n / 2 mirrored pairs about an integer centre, one body at the centre when n is odd
static Bodies lattice(size_t n, std::mt19937_64& rng, int c[3], int V[3]) {
  Bodies b;
  auto draw = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned long long)(hi - lo + 1)); };
  for (int a = 0; a < 3; a++) {
    c[a] = draw(-512, 512);
    V[a] = draw(-16, 16);
  }
  const float masses[4] = {0.5f, 1.0f, 2.0f, 4.0f};
  auto push = [&](int ox, int oy, int oz, int wx, int wy, int wz, float m) {
    b.x.push_back((float)(c[0] + ox)); b.y.push_back((float)(c[1] + oy)); b.z.push_back((float)(c[2] + oz));
    b.vx.push_back((float)(V[0] + wx)); b.vy.push_back((float)(V[1] + wy)); b.vz.push_back((float)(V[2] + wz));
    b.m.push_back(m);
    b.phi.push_back((float)draw(-512, 0) / 8.0f);
  };
  for (size_t k = 0; k + 1 < n; k += 2) {
    const int o[3] = {draw(-32, 32), draw(-32, 32), draw(-32, 32)}, w[3] = {draw(-8, 8), draw(-8, 8), draw(-8, 8)};
    const float m = masses[rng() % 4];
    push(o[0], o[1], o[2], w[0], w[1], w[2], m);
    push(-o[0], -o[1], -o[2], -w[0], -w[1], -w[2], m);
  }
  if (n % 2) push(0, 0, 0, 0, 0, 0, masses[rng() % 4]);
  // body indices: a seeded shuffle of 1000 .. 1000 + n - 1, so that the lowest index is anywhere in the list
  b.index.resize(n);
  for (size_t p = 0; p < n; p++) b.index[p] = 1000 + (int)p;
  for (size_t p = n; p > 1; p--) std::swap(b.index[p - 1], b.index[rng() % p]);
  return b;
}

static void check_lattice(size_t n, std::mt19937_64& rng) {
  int c[3], V[3];
  const Bodies b = lattice(n, rng, c, V);
  const nbody_hip_group_props o = group_struct(b, true);
  // the same in exact arithmetic: everything times 16 is an integer (masses in halves, phi in eighths)
  long long M2 = 0, L2[3] = {0, 0, 0}, T2 = 0, I2[6] = {0, 0, 0, 0, 0, 0}, W16 = 0, r2max = -1, phi8min = 1;
  int r2body = 0, phibody = 0;
  for (size_t p = 0; p < n; p++) {
    const long long m2 = (long long)(2 * b.m[p]);
    const long long d[3] = {(long long)b.x[p] - c[0], (long long)b.y[p] - c[1], (long long)b.z[p] - c[2]};
    const long long u[3] = {(long long)b.vx[p] - V[0], (long long)b.vy[p] - V[1], (long long)b.vz[p] - V[2]};
    M2 += m2;
    for (int a = 0; a < 3; a++) L2[a] += m2 * (d[(a + 1) % 3] * u[(a + 2) % 3] - d[(a + 2) % 3] * u[(a + 1) % 3]);
    T2 += m2 * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
    for (int k = 0; k < 6; k++) I2[k] += m2 * d[pa[k]] * d[pb[k]];
    const long long phi8 = (long long)(8 * b.phi[p]);
    W16 += m2 * phi8;
    const long long r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (r2 > r2max || (r2 == r2max && b.index[p] < r2body)) { r2max = r2; r2body = b.index[p]; }
    if (phi8min > 0 || phi8 < phi8min || (phi8 == phi8min && b.index[p] < phibody)) { phi8min = phi8; phibody = b.index[p]; }
  }
  EXPECT(o.status == 0 && o.n == (int)n && o.label == b.index[0], "n %zu: head", n);
  EXPECT(o.mass == M2 / 2.0, "n %zu: mass %g", n, o.mass);
  for (int a = 0; a < 3; a++) {
    EXPECT(o.com[a] == c[a] && o.vel[a] == V[a], "n %zu: centre axis %d: %g %g", n, a, o.com[a], o.vel[a]);
    EXPECT(o.ang_mom[a] == L2[a] / 2.0, "n %zu: ang_mom %d: %g", n, a, o.ang_mom[a]);
  }
  EXPECT(o.kinetic == T2 / 4.0, "n %zu: kinetic %g", n, o.kinetic);
  for (int k = 0; k < 6; k++) EXPECT(o.inertia[k] == I2[k] / 2.0, "n %zu: inertia %d: %g", n, k, o.inertia[k]);
  EXPECT(o.potential == W16 / 32.0, "n %zu: potential %g", n, o.potential);
  EXPECT(o.r_max == std::sqrt((double)r2max) && o.r_max_body == r2body, "n %zu: r_max %g body %d (want %d)", n, o.r_max,
         o.r_max_body, r2body);
  EXPECT(o.phi_min == phi8min / 8.0 && o.phi_min_body == phibody, "n %zu: phi_min %g body %d (want %d)", n, o.phi_min,
         o.phi_min_body, phibody);
  EXPECT(o.reserved[0] == 0 && o.reserved[1] == 0 && o.reserved[2] == 0, "reserved");
  const nbody_hip_group_props q = group_struct(b, false);
  EXPECT(q.potential == 0.0 && q.phi_min == 0.0 && q.phi_min_body == -1 && q.kinetic == o.kinetic && q.r_max_body == o.r_max_body,
         "n %zu: without phi", n);
}

static void check_random(size_t n, std::mt19937_64& rng) {
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> um(0.5, 1.5);
  Bodies b;
  for (size_t p = 0; p < n; p++) {
    b.x.push_back((float)(3.0 + g(rng))); b.y.push_back((float)(-7.0 + g(rng))); b.z.push_back((float)g(rng));
    b.vx.push_back((float)(0.3 * g(rng))); b.vy.push_back((float)(1.0 + 0.3 * g(rng))); b.vz.push_back((float)(0.3 * g(rng)));
    b.m.push_back((float)um(rng));
    b.phi.push_back((float)(-1.0 - um(rng)));
    b.index.push_back((int)p);
  }
  const nbody_hip_group_props o = group_struct(b, true);
  typedef long double LD;
  LD M = 0, P[3] = {0, 0, 0}, Q[3] = {0, 0, 0}, aP[3] = {0, 0, 0}, aQ[3] = {0, 0, 0};
  for (size_t p = 0; p < n; p++) {
    const LD m = b.m[p], x[3] = {b.x[p], b.y[p], b.z[p]}, v[3] = {b.vx[p], b.vy[p], b.vz[p]};
    M += m;
    for (int a = 0; a < 3; a++) {
      P[a] += m * x[a]; Q[a] += m * v[a];
      aP[a] += fabsl(m * x[a]); aQ[a] += fabsl(m * v[a]);
    }
  }
  const double e = ((double)n + 8.0) * std::ldexp(1.0, -53);
  EXPECT(std::fabs(o.mass - (double)M) <= e * (double)M, "n %zu: mass", n);
  for (int a = 0; a < 3; a++) {
    const double bx = (e * (double)aP[a] + std::fabs(o.com[a]) * e * (double)M) / (double)M * 1.000001 + 2 * std::ldexp(std::fabs(o.com[a]), -53);
    const double bv = (e * (double)aQ[a] + std::fabs(o.vel[a]) * e * (double)M) / (double)M * 1.000001 + 2 * std::ldexp(std::fabs(o.vel[a]), -53);
    EXPECT(std::fabs(o.com[a] - (double)(P[a] / M)) <= bx, "n %zu: com %d off by %g (bound %g)", n, a,
           std::fabs(o.com[a] - (double)(P[a] / M)), bx);
    EXPECT(std::fabs(o.vel[a] - (double)(Q[a] / M)) <= bv, "n %zu: vel %d", n, a);
  }
  // the central sums about the SAME rounded X and V as the struct's (the effect of their rounding is not arithmetic of
  // pass 2), in long double and plain member order
  LD L[3] = {0, 0, 0}, aL[3] = {0, 0, 0}, T = 0, I[6] = {0, 0, 0, 0, 0, 0}, aI[6] = {0, 0, 0, 0, 0, 0}, W = 0, aW = 0, r2max = -1;
  for (size_t p = 0; p < n; p++) {
    const LD m = b.m[p];
    const LD d[3] = {(LD)b.x[p] - o.com[0], (LD)b.y[p] - o.com[1], (LD)b.z[p] - o.com[2]};
    const LD u[3] = {(LD)b.vx[p] - o.vel[0], (LD)b.vy[p] - o.vel[1], (LD)b.vz[p] - o.vel[2]};
    for (int a = 0; a < 3; a++) {
      const int i = (a + 1) % 3, j = (a + 2) % 3;
      L[a] += m * (d[i] * u[j] - d[j] * u[i]);
      aL[a] += m * (fabsl(d[i] * u[j]) + fabsl(d[j] * u[i]));
    }
    T += m * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
    for (int k = 0; k < 6; k++) {
      I[k] += m * d[pa[k]] * d[pb[k]];
      aI[k] += fabsl(m * d[pa[k]] * d[pb[k]]);
    }
    W += m * (LD)b.phi[p];
    aW += fabsl(m * (LD)b.phi[p]);
    const LD r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (r2 > r2max) r2max = r2;
  }
  for (int a = 0; a < 3; a++)
    EXPECT(std::fabs(o.ang_mom[a] - (double)L[a]) <= e * (double)aL[a], "n %zu: ang_mom %d off by %g (bound %g)", n, a,
           std::fabs(o.ang_mom[a] - (double)L[a]), e * (double)aL[a]);
  EXPECT(std::fabs(o.kinetic - (double)(T / 2)) <= e * (double)(T / 2), "n %zu: kinetic", n);
  for (int k = 0; k < 6; k++) EXPECT(std::fabs(o.inertia[k] - (double)I[k]) <= e * (double)aI[k], "n %zu: inertia %d", n, k);
  EXPECT(std::fabs(o.potential - (double)(W / 2)) <= e * (double)(aW / 2), "n %zu: potential", n);
  EXPECT(std::fabs(o.r_max - (double)sqrtl(r2max)) <= 8 * std::ldexp(o.r_max, -53), "n %zu: r_max", n);
}

static void check_rules() {
  // ties go to the lowest body index, whatever the order of the takes; NaN is never taken
  const int bodies[4] = {9, 3, 7, 5};
  int order[4] = {0, 1, 2, 3};
  do {
    GroupSums2 s;
    group_sums2_zero(s);
    for (int k = 0; k < 4; k++) {
      group_take_r2(s, bodies[order[k]] == 9 ? 1.0 : 4.0, bodies[order[k]]);
      group_take_phi(s, bodies[order[k]] == 9 ? -1.0 : -2.5, bodies[order[k]]);
      group_take_r2(s, std::nan(""), 1);
      group_take_phi(s, std::nan(""), 1);
    }
    EXPECT(s.r2 == 4.0 && s.r2_body == 3 && s.phi == -2.5 && s.phi_body == 3, "ties: %g %d %g %d", s.r2, s.r2_body, s.phi, s.phi_body);
    // ... and through a merge, in both directions
    GroupSums2 a, b;
    group_sums2_zero(a);
    group_sums2_zero(b);
    group_take_r2(a, 4.0, bodies[order[0]]);
    group_take_r2(b, 4.0, bodies[order[1]]);
    group_sums2_merge(a, b);
    EXPECT(a.r2_body == std::min(bodies[order[0]], bodies[order[1]]), "merge tie");
  } while (std::next_permutation(order, order + 4));
  // an empty partial sum changes nothing
  GroupSums2 s, z;
  group_sums2_zero(s);
  group_sums2_zero(z);
  group_take_r2(s, 0.0, 5);
  group_take_phi(s, (double)INFINITY, 6);
  group_sums2_merge(s, z);
  EXPECT(s.r2 == 0.0 && s.r2_body == 5 && s.phi_body == 6, "empty merge");
  // mass 0: the centre is the origin, not a NaN
  Bodies b;
  for (int p = 0; p < 3; p++) {
    b.x.push_back(1.0f + p); b.y.push_back(2.0f); b.z.push_back(3.0f);
    b.vx.push_back(1.0f); b.vy.push_back(0.0f); b.vz.push_back(-1.0f);
    b.m.push_back(0.0f);
    b.phi.push_back(-1.0f);
    b.index.push_back(10 + p);
  }
  const nbody_hip_group_props o = group_struct(b, true);
  EXPECT(o.mass == 0.0 && o.com[0] == 0.0 && o.vel[2] == 0.0 && o.kinetic == 0.0 && o.status == 0 && o.n == 3, "mass 0");
  EXPECT(o.r_max == std::sqrt(9.0 + 4.0 + 9.0) && o.r_max_body == 12 && o.phi_min == -1.0 && o.phi_min_body == 10, "mass 0: extrema");
  // every phi a NaN: no body
  b.phi.assign(3, std::nanf(""));
  const nbody_hip_group_props q = group_struct(b, true);
  EXPECT(q.phi_min_body == -1 && q.phi_min == 0.0, "NaN phi");
  // the bad struct
  const nbody_hip_group_props bad = group_props_bad();
  nbody_hip_group_props want;
  std::memset(&want, 0, sizeof want);
  want.status = 1;
  EXPECT(std::memcmp(&bad, &want, sizeof want) == 0 && sizeof want == 192, "the bad struct");
}

int main() {
  std::mt19937_64 rng(2026);
  const size_t S = kGroupSmall, C = kGroupChunk;
  const size_t sizes[] = {1, 2, 3, 4, 5, 9, S - 1, S, S + 1, 63, 64, 65, 255, 256, 257, 511, 513, C - 1, C, C + 1,
                          2 * C, 2 * C + 1, 63 * C + 5, 64 * C, 64 * C + 3, 130 * C + 77};
  for (size_t n : sizes) {
    check_lattice(n, rng);
    check_random(n, rng);
  }
  check_rules();
  if (failures) {
    std::printf("group_props_check: %d FAILURES in %lld checks\n", failures, checked);
    return 1;
  }
  std::printf("group_props_check: ok, %lld checks\n", checked);
  return 0;
}
