// radial_check.cpp -- the arithmetic of the radial profiles (radial_common.h) on a CPU, under AddressSanitizer and UBSan and
// without contraction (make radial_check): the member's distance, q, key and four terms on known-answer cases and against
// a long double restatement; the order the keys give (ties in q, r2 == 0, q overflowing to +inf, the NaN that no key is
// made of); the three cut rules at K = 1, K = n, with E not monotone, and two cuts with an empty shell between them; the
// finished structs.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "radial_common.h"
#include "radial_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    checked++;                                                   \
    if (!(cond) && failures++ < 40) std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
  } while (0)

struct Body {
  float x, y, z, vx, vy, vz, m;
};

// one group by the functions of the header, as the kernels use them: keys, a stable sort, E in turn, K, the heads
struct Profile {
  std::vector<int> order;
  std::vector<float> q;
  std::vector<double> E;
  std::vector<RadialTerms> terms;
  std::vector<int> K;
  std::vector<nbody_hip_radial_shell> shells;
  nbody_hip_radial_group group;
};

static Profile profile(const std::vector<Body>& b, const RadialCentre& c, const std::vector<double>& cuts, int mode) {
  const int n = (int)b.size();
  Profile P;
  std::vector<unsigned long long> key(n);
  int bad = 0;
  for (int p = 0; p < n; p++) {
    const double r2 = radial_r2(b[p].x, b[p].y, b[p].z, c);
    if (r2 != r2) bad |= 2;
    key[p] = radial_key(0, r2 != r2 ? 0u : radial_q_bits(radial_q(r2)));
  }
  if (bad) {
    P.group = radial_group_bad(radial_status(bad));
    return P;
  }
  P.order.resize(n);
  for (int p = 0; p < n; p++) P.order[p] = p;
  std::stable_sort(P.order.begin(), P.order.end(), [&](int a, int b2) { return key[a] < key[b2]; });
  std::vector<double> m(n);
  for (int s = 0; s < n; s++) {
    const Body& o = b[P.order[s]];
    P.q.push_back(radial_q_from_bits((unsigned int)key[P.order[s]]));
    P.terms.push_back(radial_terms(o.x, o.y, o.z, o.vx, o.vy, o.vz, o.m, c));
    m[s] = P.terms.back().t[0];
  }
  P.E.resize(n);
  radial_enclosed_small(m.data(), n, P.E.data());
  P.group = radial_group_finish(P.E[n - 1], P.q[n - 1], n);
  int prev = 0;
  for (double cut : cuts) {
    int K = radial_k_serial(mode, cut, P.E.data(), P.q.data(), n);
    if (K < prev) K = prev;
    P.K.push_back(K);
    P.shells.push_back(radial_shell_head(mode, cut, prev, K, K > 0 ? P.E[K - 1] : 0.0, K > 0 ? P.q[K - 1] : 0.0f));
    prev = K;
  }
  return P;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  static_assert(sizeof(nbody_hip_radial_group) == 32 && sizeof(nbody_hip_radial_shell) == 64, "the structs");
  const RadialCentre origin = {{0, 0, 0}, {0, 0, 0}};

  // ---- known answers of a member: (3, 4, 0) about the origin with u = (1, 2, 3), m = 2
  {
    const RadialTerms t = radial_terms(3, 4, 0, 1, 2, 3, 2, origin);
    CHECK(radial_r2(3, 4, 0, origin) == 25.0 && radial_q(25.0) == 25.0f && radial_radius(25.0f) == 5.0);
    CHECK(t.t[0] == 2.0 && t.t[1] == 2.0 * (11.0 / 5.0) && t.t[2] == 2.0 * ((11.0 / 5.0) * (11.0 / 5.0)));
    CHECK(t.t[3] == 2.0 * (14.0 - (11.0 / 5.0) * (11.0 / 5.0)));
    // on the centre: vr = 0, all of u is tangential
    const RadialTerms z = radial_terms(1, 1, 1, 1, 2, 3, 4, RadialCentre{{1, 1, 1}, {0, 0, 0}});
    CHECK(z.t[0] == 4.0 && z.t[1] == 0.0 && z.t[2] == 0.0 && z.t[3] == 4.0 * 14.0);
    CHECK(radial_q_bits(radial_q(0.0)) == 0u);
    // a bulk velocity and a centre: d and u are differences
    const RadialTerms w = radial_terms(5, 0, 0, 7, 0, 0, 1, RadialCentre{{2, 0, 0}, {3, 0, 0}});
    CHECK(w.t[1] == 4.0 && w.t[2] == 16.0 && w.t[3] == 0.0);
  }
  // ---- q: rounding to nearest, the overflow, the bit order
  {
    CHECK(radial_q(1.0 + std::ldexp(1.0, -24)) == 1.0f);              // a tie goes to the even side
    CHECK(radial_q(1.0 + std::ldexp(1.5, -24)) == 1.0f + std::ldexp(1.0f, -23));
    CHECK(radial_q(3.4028234663852886e38) == std::numeric_limits<float>::max());
    CHECK(radial_q(3.4028235e38) == std::numeric_limits<float>::max());  // below the half ulp above FLT_MAX
    CHECK(std::isinf(radial_q(3.4028235677973366e38)) && std::isinf(radial_q(1e300)) && std::isinf(radial_q(inf)));
    CHECK(radial_q_bits(radial_q(inf)) == 0x7f800000u);
    const double r2s[] = {0.0, 1e-300, 1e-45, 1e-38, 0.5, 1.0, 1.0000001, 2.0, 1e30, 3.4e38, 1e300, inf};
    for (size_t i = 1; i < sizeof(r2s) / sizeof(r2s[0]); i++)
      CHECK(radial_q_bits(radial_q(r2s[i - 1])) <= radial_q_bits(radial_q(r2s[i])));
    CHECK(radial_key(3, 0xffffffffu) < radial_key(4, 0u) && radial_key(0x7ffffffeLL, 5u) >> 32 == 0x7ffffffeULL);
    CHECK(radial_q_from_bits(radial_q_bits(1.5f)) == 1.5f);
  }
  // ---- the order, E and K of a hand-made group: ties in q (the earlier position first), a member on the centre
  {
    const std::vector<Body> b = {{2, 0, 0, 0, 0, 0, 1}, {0, 1, 0, 0, 0, 0, 2}, {0, 0, -1, 0, 0, 0, 4}, {0, 0, 0, 0, 0, 0, 8},
                                 {-1, 0, 0, 0, 0, 0, 16}, {0, -2, 0, 0, 0, 0, 32}};
    const Profile P = profile(b, origin, {0.125, 0.25, 0.5, 1.0}, NBODY_HIP_RADIAL_MASS);
    const int order[] = {3, 1, 2, 4, 0, 5};
    const double E[] = {8, 10, 14, 30, 31, 63};
    for (int s = 0; s < 6; s++) CHECK(P.order[s] == order[s] && P.E[s] == E[s]);
    // T = 7.875, 15.75, 31.5, 63: K = 1, 4, 6, 6 -- K = 1, K = n, and an empty last shell
    const int K[] = {1, 4, 6, 6};
    for (int c = 0; c < 4; c++) CHECK(P.K[c] == K[c] && P.shells[c].enclosed_count == K[c] && P.shells[c].enclosed_mass == E[K[c] - 1]);
    CHECK(P.shells[0].radius == 0.0 && P.shells[1].radius == 1.0 && P.shells[2].radius == 2.0 && P.shells[3].count == 0);
    CHECK(P.shells[1].count == 3 && P.group.mass == 63.0 && P.group.r_max == 2.0 && P.group.n == 6 && P.group.status == 0);
    const Profile N = profile(b, origin, {0.01, 0.5, 0.51, 1.0}, NBODY_HIP_RADIAL_NUMBER);
    CHECK(N.K[0] == 1 && N.K[1] == 3 && N.K[2] == 4 && N.K[3] == 6);
    const Profile R = profile(b, origin, {0.0, 0.5, 1.0, 1.5, inf}, NBODY_HIP_RADIAL_RADIUS);
    CHECK(R.K[0] == 1 && R.K[1] == 1 && R.K[2] == 4 && R.K[3] == 4 && R.K[4] == 6);
    CHECK(R.shells[1].count == 0 && R.shells[3].count == 0 && R.shells[1].radius == 0.5 && std::isinf(R.shells[4].radius));
    CHECK(R.shells[1].mass == 0.0 && R.shells[1].enclosed_mass == 8.0);
    // nobody inside: K = 0, zeros
    const Profile R0 = profile({{1, 0, 0, 0, 0, 0, 1}}, origin, {0.5}, NBODY_HIP_RADIAL_RADIUS);
    CHECK(R0.K[0] == 0 && R0.shells[0].enclosed_mass == 0.0 && R0.shells[0].count == 0 && R0.shells[0].radius == 0.5);
  }
  // ---- q overflow: the far members tie at +inf in position order; the NaN: status 2 and zeros
  {
    const std::vector<Body> b = {{3e19f, 0, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 0, 0, 1}, {-3e19f, 3e19f, 0, 0, 0, 0, 1}};
    const Profile P = profile(b, origin, {1.0}, NBODY_HIP_RADIAL_MASS);
    CHECK(P.order[0] == 1 && P.order[1] == 0 && P.order[2] == 2 && std::isinf(P.q[1]) && std::isinf(P.q[2]));
    CHECK(std::isinf(P.group.r_max) && P.group.mass == 3.0 && P.K[0] == 3);
    std::vector<Body> c = b;
    c[1].y = std::nanf("");
    const Profile Q = profile(c, origin, {1.0}, NBODY_HIP_RADIAL_MASS);
    CHECK(Q.group.status == 2 && Q.group.n == 0 && Q.group.mass == 0.0 && Q.group.r_max == 0.0);
    const nbody_hip_radial_group one = radial_group_bad(1);
    CHECK(one.status == 1 && one.n == 0 && one.reserved[0] == 0 && one.reserved[1] == 0);
    CHECK(radial_status(0) == 0 && radial_status(1) == 1 && radial_status(2) == 2 && radial_status(3) == 1);
  }
  // ---- the mass rule says SMALLEST: an E that is not monotone (a negative mass)
  {
    const double E[] = {5, 3, 4, 6};
    const float q[] = {0, 1, 2, 3};
    CHECK(radial_k_serial(NBODY_HIP_RADIAL_MASS, 0.75, E, q, 4) == 1);  // T = 4.5: rank 0 passes, ranks 1 and 2 do not
    CHECK(radial_k_serial(NBODY_HIP_RADIAL_MASS, 1.0, E, q, 4) == 4);
    const double Eneg[] = {-1, -2};
    CHECK(radial_k_serial(NBODY_HIP_RADIAL_MASS, 0.5, Eneg, q, 2) == 1);  // T = -1
    CHECK(radial_k_number(1.0, 7) == 7 && radial_k_number(1e-9, 7) == 1 && radial_k_number(0.5, 7) == 4 && radial_k_number(0.5, 8) == 4);
    // 0.1 as a double is above one tenth, but the product 0.1 * 10.0 rounds once, to 1.0, and the ceil sees 1
    CHECK(0.1 * 10.0 == 1.0 && radial_k_number(0.1, 10) == 1 && radial_k_number(0.3, 10) == 3 && radial_k_number(0.7, 10) == 7 &&
          radial_k_number(0.30000000000000004, 10) == 4);
  }

  // ---- random groups against a long double restatement
  std::mt19937_64 rng(97531);
  std::uniform_real_distribution<float> U(-2.0f, 2.0f), M(0.5f, 1.5f);
  for (int trial = 0; trial < 3000; trial++) {
    const int n = 1 + (int)(rng() % 32);
    std::vector<Body> b(n);
    for (auto& o : b) o = {U(rng), U(rng), U(rng), U(rng), U(rng), U(rng), M(rng)};
    if (n > 3) b[2] = b[0], b[2].m = M(rng);  // an exact tie in q
    const RadialCentre c = {{U(rng) * 0.1, U(rng) * 0.1, U(rng) * 0.1}, {U(rng) * 0.1, U(rng) * 0.1, U(rng) * 0.1}};
    const std::vector<double> cuts = {0.1, 0.5, 0.9, 1.0};
    const Profile P = profile(b, c, cuts, NBODY_HIP_RADIAL_MASS);
    long double cum = 0;
    for (int s = 0; s < n; s++) {
      const Body& o = b[P.order[s]];
      const long double dx = (long double)o.x - c.c[0], dy = (long double)o.y - c.c[1], dz = (long double)o.z - c.c[2];
      const long double ux = (long double)o.vx - c.v[0], uy = (long double)o.vy - c.v[1], uz = (long double)o.vz - c.v[2];
      const long double r2 = dx * dx + dy * dy + dz * dz, u2 = ux * ux + uy * uy + uz * uz;
      const long double vr = r2 > 0 ? (ux * dx + uy * dy + uz * dz) / sqrtl(r2) : 0;
      CHECK(fabsl((long double)P.q[s] - r2) <= r2 * 6.1e-8L);  // half an ulp of a float, and the fp64 roundings below it
      if (s) CHECK(P.q[s - 1] < P.q[s] || (P.q[s - 1] == P.q[s] && P.order[s - 1] < P.order[s]));
      const long double tol = 16 * 1.2e-16L;
      CHECK(P.terms[s].t[0] == (double)o.m);
      CHECK(fabsl(P.terms[s].t[1] - o.m * vr) <= tol * o.m * sqrtl(u2));
      CHECK(fabsl(P.terms[s].t[2] - o.m * vr * vr) <= tol * o.m * u2);
      CHECK(fabsl(P.terms[s].t[3] - o.m * (u2 - vr * vr)) <= tol * o.m * 2 * u2);
      cum += o.m;
      CHECK(fabsl(P.E[s] - cum) <= (s + 1) * 1.2e-16L * cum);
    }
    for (size_t k = 0; k < cuts.size(); k++) {  // K against the rule on the header's own E, written out again
      const double T = cuts[k] * P.E[n - 1];
      int K = n;
      for (int s = n - 1; s >= 0; s--)
        if (P.E[s] >= T) K = s + 1;
      CHECK(P.K[k] == K && P.shells[k].radius == std::sqrt((double)P.q[K - 1]));
      CHECK(K == 1 || P.E[K - 2] < T);
    }
    CHECK(P.K.back() == n && P.group.r_max == std::sqrt((double)P.q[n - 1]));
  }
  if (failures) {
    std::printf("radial_check: %d FAILURES in %lld checks\n", failures, checked);
    return 1;
  }
  std::printf("radial_check: ok, %lld checks\n", checked);
  return 0;
}
