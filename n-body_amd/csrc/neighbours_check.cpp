// neighbours_check.cpp -- the arithmetic of the neighbour search and the density centre (neighbours_common.h) on a CPU,
// under AddressSanitizer and UBSan (make neighbours_check): plain g++ with -ffp-contract=off, no HIP.
//   * the sorted insertion, driven as the kernel drives it, against std::sort of the keys for every list length K and
//     every k, with ties, coincident bodies, +inf and NaN among the candidates; the result for k is the same for every K
//   * the K choice, the argument rule, the status rule at both neighbours of fl(cell * cell), the density
//   * the density centre in the model's summation order: exact on integer data, and against a long double sum within
//     (n + 8) u sum|t| on general data
// `neighbours_check cases` prints the density centres of seeded sets (hex floats) for the numpy restatement of the tests.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "neighbours_common.h"

using namespace nbh;

static int g_fail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      g_fail++;                                                       \
    }                                                                 \
  } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

struct Cand {
  float d2, m;
  int index;
};

// the candidate loop of grid_neighbours_kernel
template <int K>
static NeighList<K, true> run_list(const std::vector<Cand>& c) {
  NeighList<K, true> L;
  neigh_clear(L);
  for (const Cand& e : c) {
    if (!neigh_takes(e.d2) || neigh_bits(e.d2) > (unsigned int)(L.a[K - 1] >> 32)) continue;
    const NeighKey key = neigh_key(e.d2, e.index);
    if (neigh_accepts(L, key)) neigh_insert(L, key, e.m);
  }
  return L;
}

template <int K>
static void check_insertion(const std::vector<Cand>& c, std::vector<NeighKey>& first32) {
  const NeighList<K, true> L = run_list<K>(c);
  std::vector<std::pair<NeighKey, float>> want;
  for (const Cand& e : c)
    if (e.d2 == e.d2) want.push_back({neigh_key(e.d2, e.index), e.m});
  std::sort(want.begin(), want.end());
  for (int s = 0; s < K; s++) {
    const bool have = s < (int)want.size();
    CHECK(L.a[s] == (have ? want[s].first : kNeighEmpty));
    if (have) CHECK(L.m[s] == want[s].second);
    CHECK(neigh_key_index(L.a[s]) == (have ? neigh_key_index(want[s].first) : -1));
    if (!have) CHECK(neigh_key_dist2(L.a[s]) == INFINITY);
    // a prefix: the same keys whatever K
    if (first32.size() == 32) CHECK(first32[s] == L.a[s]);
  }
  for (int k = 1; k <= K; k++) {
    CHECK(neigh_kth(L, k) == L.a[k - 1]);
    double msum = 0.0;
    for (int s = 0; s < k - 1; s++) msum = msum + (double)L.m[s];
    CHECK(neigh_msum(L, k) == msum);
  }
  if (K == 32) first32.assign(L.a, L.a + 32);
}

static void insertion() {
  const float values[] = {0.0f, 1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 0.25f, 1e-38f, 1e-45f, 3e38f, INFINITY};
  for (int trial = 0; trial < 400; trial++) {
    const int n = trial < 70 ? trial : (int)(rnd() % 200u);
    std::vector<Cand> c;
    std::vector<int> perm(n);
    for (int i = 0; i < n; i++) perm[i] = i;
    for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[rnd() % (unsigned)(i + 1)]);
    for (int i = 0; i < n; i++) {
      Cand e;
      const unsigned pick = rnd() % 16u;
      if (pick < 11) e.d2 = values[pick];
      else if (pick == 11) e.d2 = std::numeric_limits<float>::quiet_NaN();
      else e.d2 = (float)(rnd() % 1000u) / 64.0f;
      if (trial % 5 == 0) e.d2 = (float)(rnd() % 4u);  // massive ties
      e.m = (float)(1 + rnd() % 1000u) / 8.0f;
      e.index = trial % 7 == 0 ? perm[i] + 0x7fffff00 - n : perm[i];  // distinct; the largest indices too
      c.push_back(e);
    }
    std::vector<NeighKey> first32;
    check_insertion<32>(c, first32);
    check_insertion<16>(c, first32);
    check_insertion<8>(c, first32);
    check_insertion<4>(c, first32);
  }
  // the bit pattern orders as the float does, and the index breaks ties
  CHECK(neigh_key(0.0f, 5) < neigh_key(1e-45f, 0));
  CHECK(neigh_key(1.0f, 7) < neigh_key(1.0f, 8));
  CHECK(neigh_key(1.0f, 0x7fffffff) < neigh_key(std::nextafter(1.0f, 2.0f), 0));
  CHECK(neigh_key(INFINITY, 0x7fffffff) < kNeighEmpty);
  CHECK(!neigh_takes(std::numeric_limits<float>::quiet_NaN()) && neigh_takes(0.0f) && neigh_takes(INFINITY));
  CHECK(neigh_key_index(neigh_key(2.0f, 123456)) == 123456 && neigh_key_dist2(neigh_key(2.0f, 123456)) == 2.0f);
}

static void decisions() {
  for (int k = -3; k <= 40; k++) {
    int want = 0;
    if (k >= 1 && k <= 32) {
      want = 4;
      while (want < k) want *= 2;
    }
    CHECK(neigh_pick_K(k) == want);
  }
  // the argument rule: k first, then the outputs, then refine
  for (int k = -1; k <= 34; k++)
    for (int mask = 0; mask < 16; mask++)
      for (int refine = 0; refine < 3; refine++) {
        const bool i = mask & 1, d = mask & 2, r = mask & 4, s = mask & 8;
        const NeighArgs want = (k < 1 || k > 32) ? kNeighArgsK : mask == 0 ? kNeighArgsNoOutput
                               : (refine && !s) ? kNeighArgsRefine : kNeighArgsOk;
        CHECK(neigh_args(k, i, d, r, s, refine) == want);
      }
  CHECK(neigh_whole_grid(1, 2, 2) && neigh_whole_grid(2, 2, 2) && !neigh_whole_grid(3, 1, 1) && !neigh_whole_grid(1, 1, 3));
}

static void status_and_density() {
  const float cells[] = {1.0f, 1.5f, 0.1f, 3.0f, 1.0000001f, 7.3e-5f, 1234.5f};
  for (float cell : cells) {
    const float c2 = neigh_cell2(cell);
    CHECK(c2 == cell * cell);
    const float below = std::nextafter(c2, 0.0f), above = std::nextafter(c2, INFINITY);
    CHECK(neigh_status(neigh_key(below, 3), c2, false) == 0);
    CHECK(neigh_status(neigh_key(c2, 3), c2, false) == 1);
    CHECK(neigh_status(neigh_key(above, 3), c2, false) == 1);
    CHECK(neigh_status(neigh_key(c2, 3), c2, true) == 0);
    CHECK(neigh_status(neigh_key(above, 3), c2, true) == 0);
    CHECK(neigh_status(neigh_key(INFINITY, 3), c2, true) == 0 && neigh_status(neigh_key(INFINITY, 3), c2, false) == 1);
    CHECK(neigh_status(kNeighEmpty, c2, false) == 2 && neigh_status(kNeighEmpty, c2, true) == 2);
    CHECK(neigh_status(neigh_key(0.0f, 3), c2, false) == 3 && neigh_status(neigh_key(0.0f, 0), c2, true) == 3);
  }
  // the density: known answers, and the stated expression
  CHECK(neigh_density(5.0, neigh_key(4.0f, 1), 0) == 5.0 / (NBODY_HIP_SPHERE_4PI_3 * 8.0));
  CHECK(neigh_density(5.0, neigh_key(4.0f, 1), 1) == 5.0 / (NBODY_HIP_SPHERE_4PI_3 * 8.0));
  CHECK(neigh_density(0.0, neigh_key(4.0f, 1), 0) == 0.0);
  CHECK(neigh_density(5.0, kNeighEmpty, 2) == 0.0 && neigh_density(5.0, neigh_key(0.0f, 1), 3) == 0.0);
  CHECK(neigh_density(5.0, neigh_key(INFINITY, 1), 1) == 0.0);
  for (int trial = 0; trial < 1000; trial++) {
    const float d2 = (float)(1 + rnd() % 100000u) / 777.0f;
    const double msum = (double)(rnd() % 1000u) / 3.0;
    const double r = sqrt((double)d2);
    CHECK(neigh_density(msum, neigh_key(d2, 9), 0) == msum / (NBODY_HIP_SPHERE_4PI_3 * ((r * r) * r)));
  }
  CHECK(NBODY_HIP_SPHERE_4PI_3 == 4.0 * 3.14159265358979323846 / 3.0);
}

// ---- the density centre in the model's order ---------------------------------------------------------------------------
// add(s, p): the term of position p into s
template <class Add>
static CentreSums ordered(long long n, Add add) {
  CentreSums total;
  centre_zero(total);
  if (n <= kCentreSmall) {
    for (long long p = 0; p < n; p++) add(total, p);
    return total;
  }
  const long long chunks = centre_chunks(n);
  CentreSums c[64];
  for (int l = 0; l < 64; l++) centre_zero(c[l]);
  for (long long ch = 0; ch < chunks; ch++) {
    const long long base = ch * kCentreChunk, end = std::min<long long>(base + kCentreChunk, n);
    CentreSums s[kCentreThreads];
    for (int t = 0; t < kCentreThreads; t++) {
      centre_zero(s[t]);
      for (int j = 0; j < kCentrePerThread; j++) {
        const long long p = base + (long long)j * kCentreThreads + t;
        if (p < end) add(s[t], p);
      }
    }
    for (int w = 0; w < kCentreThreads / 64; w++)
      for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; l++) centre_merge(s[64 * w + l], s[64 * w + l + off]);
    for (int w = 1; w < kCentreThreads / 64; w++) centre_merge(s[0], s[64 * w]);
    centre_merge(c[ch % 64], s[0]);
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int l = 0; l < off; l++) centre_merge(c[l], c[l + off]);
  return c[0];
}

struct Set {
  std::vector<double> rho;
  std::vector<float> x, y, z;
};
// seeded data both this program and the numpy restatement can make: integers only
static Set seeded(long long n, bool lattice) {
  Set s;
  for (long long p = 0; p < n; p++) {
    const uint64_t a = (uint64_t)p * 2654435761ull + 12345ull, b = (uint64_t)p * 40503ull + 977ull;
    if (lattice) {
      s.rho.push_back((double)(1 + a % 4u));
      s.x.push_back((float)((int)(b % 129u) - 64));
      s.y.push_back((float)((int)((b / 129u) % 129u) - 64));
      s.z.push_back((float)((int)((b / 16641u) % 129u) - 64));
    } else {
      s.rho.push_back((double)(1 + a % 1000003u) / 4099.0);
      s.x.push_back((float)((int)(b % 100003u) - 50000) / 1021.0f);
      s.y.push_back((float)((int)((b / 7u) % 100003u) - 50000) / 2039.0f + 3.0f);
      s.z.push_back((float)((int)((b / 13u) % 100003u) - 50000) / 4093.0f - 2.0f);
    }
  }
  return s;
}

static nbody_hip_density_centre_t centre_of(const Set& s, CentreSums* s1_out = nullptr, CentreSums* s2_out = nullptr) {
  const long long n = (long long)s.rho.size();
  const CentreSums s1 = ordered(n, [&](CentreSums& a, long long p) { centre_add1(a, s.rho[p], s.x[p], s.y[p], s.z[p]); });
  const CentrePoint c = centre_point(s1);
  const CentreSums s2 = ordered(n, [&](CentreSums& a, long long p) { centre_add2(a, s.rho[p], s.x[p], s.y[p], s.z[p], c); });
  if (s1_out) *s1_out = s1;
  if (s2_out) *s2_out = s2;
  return centre_finish(c, s2, (int)n);
}

static const long long kSizes[] = {1, 2, 31, 32, 33, 64, 1023, 1024, 1025, 2048, 5000, 65537, 70001};

static void density_centre() {
  const double u = std::ldexp(1.0, -53);
  for (long long n : kSizes) {
    // integer data: every sum is exact whatever its order
    const Set L = seeded(n, true);
    double S1 = 0, P[3] = {0, 0, 0};
    for (long long p = 0; p < n; p++) {
      S1 += L.rho[p];
      P[0] += L.rho[p] * L.x[p];
      P[1] += L.rho[p] * L.y[p];
      P[2] += L.rho[p] * L.z[p];
    }
    CentreSums s1, s2;
    nbody_hip_density_centre_t o = centre_of(L, &s1, &s2);
    CHECK(s1.v[0] == S1 && s1.v[1] == P[0] && s1.v[2] == P[1] && s1.v[3] == P[2]);
    CHECK(o.n == (int)n && o.status == 0 && o.rho_sum == S1 && o.centre[0] == P[0] / S1 && o.centre[2] == P[2] / S1);
    double S2 = 0;
    for (long long p = 0; p < n; p++) S2 += L.rho[p] * L.rho[p];
    CHECK(o.rho2_sum == S2);
    // general data against long double sums: each sum within (n + 8) u sum|t| -- n - 1 additions in any order, each at
    // most u times the running absolute sum; at most 6 roundings inside a term (d, its square, two additions, rho * rho,
    // the product); the long double sum's own (n + 6) 2^-64 sum|t| and its rounding to fp64 are below 2 u sum|t|
    const Set G = seeded(n, false);
    o = centre_of(G, &s1, &s2);
    long double w[4] = {0, 0, 0, 0}, aw[4] = {0, 0, 0, 0};
    for (long long p = 0; p < n; p++) {
      const long double t[4] = {(long double)G.rho[p], (long double)G.rho[p] * G.x[p], (long double)G.rho[p] * G.y[p],
                                (long double)G.rho[p] * G.z[p]};
      for (int a = 0; a < 4; a++) {
        w[a] += t[a];
        aw[a] += fabsl(t[a]);
      }
    }
    for (int a = 0; a < 4; a++) CHECK(fabsl((long double)s1.v[a] - w[a]) <= (long double)((double)(n + 8) * u) * aw[a]);
    long double W2 = 0, R = 0;
    for (long long p = 0; p < n; p++) {
      const long double dx = (long double)G.x[p] - o.centre[0], dy = (long double)G.y[p] - o.centre[1],
                        dz = (long double)G.z[p] - o.centre[2];
      const long double ww = (long double)G.rho[p] * G.rho[p];
      W2 += ww;
      R += ww * (dx * dx + dy * dy + dz * dz);
    }
    CHECK(fabsl((long double)s2.v[0] - W2) <= (long double)((double)(n + 8) * u) * W2);
    CHECK(fabsl((long double)s2.v[1] - R) <= (long double)((double)(n + 8) * u) * R);
    CHECK(o.core_radius == sqrt(s2.v[1] / s2.v[0]) && o.rho_sum == s1.v[0] && o.rho2_sum == s2.v[0]);
    for (int a = 0; a < 3; a++) CHECK(o.centre[a] == s1.v[1 + a] / s1.v[0]);
  }
  // no weight at all: zeros, n kept
  Set Z = seeded(40, false);
  for (double& r : Z.rho) r = 0.0;
  const nbody_hip_density_centre_t o = centre_of(Z);
  CHECK(o.n == 40 && o.status == 0 && o.rho_sum == 0.0 && o.rho2_sum == 0.0 && o.core_radius == 0.0);
  CHECK(o.centre[0] == 0.0 && o.centre[1] == 0.0 && o.centre[2] == 0.0);
  const nbody_hip_density_centre_t b = centre_bad();
  CHECK(b.status == 1 && b.n == 0 && b.rho_sum == 0.0 && b.core_radius == 0.0 && b.centre[1] == 0.0);
  CHECK(sizeof(nbody_hip_density_centre_t) == 64);
}

static void print_cases() {
  printf("sizes S %d C %d T %d\n", kCentreSmall, kCentreChunk, kCentreThreads);
  for (long long n : kSizes) {
    const nbody_hip_density_centre_t o = centre_of(seeded(n, false));
    printf("centre %lld %a %a %a %a %a %a\n", n, o.centre[0], o.centre[1], o.centre[2], o.core_radius, o.rho_sum, o.rho2_sum);
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "cases")) {
    print_cases();
    return 0;
  }
  insertion();
  decisions();
  status_and_density();
  density_centre();
  if (g_fail) {
    printf("neighbours_check: %d FAILED\n", g_fail);
    return 1;
  }
  printf("neighbours_check: ok\n");
  return 0;
}
