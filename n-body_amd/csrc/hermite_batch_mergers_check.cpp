// hermite_batch_mergers_check.cpp -- the arithmetic of the ensemble mergers on a CPU, under AddressSanitizer and UBSan
// (make mergers_check; plain g++, no device, nothing loaded into another process).  It includes
// hermite_batch_mergers_common.h, the file the merge kernel of hermite_batch.hip is written in, and runs
//   (a) the slot bookkeeping against its statement in include/nbody_hip.h for every record of every n <= 6, with the
//       compaction carried out on arrays of exactly n slots (an index out of range is an error of the sanitizer);
//   (b) known answers: two equal bodies head-on (V exactly 0, X exactly the midpoint), two massless bodies (the plain
//       mean), the volume rule at 3-4-5-like radii, the split of a value into hi + lo;
//   (c) the merged body and the deltas of drawn systems against a long double restatement;
//   (d) the same drawn systems printed, inputs and results as hexadecimal floats ("case ..." / "body ..." / "out ..."
//       lines), for tests/test_hermite_batch_mergers_cpu.py to compare with the numpy restatement bit for bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>

#include "hermite_batch_mergers_common.h"

using namespace nbh;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);                 \
      failures++;                                                      \
    }                                                                  \
  } while (0)

struct Rng {  // a 64-bit LCG: the same draws on every machine
  uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0 - 0.5;
  }
};

struct Body {
  float x[3], lx[3], v[3], lv[3], m, r;
};

static DiagBody full(const Body& b) {
  return diag_body(b.x[0], b.x[1], b.x[2], b.lx[0], b.lx[1], b.lx[2], b.v[0], b.v[1], b.v[2], b.lv[0], b.lv[1], b.lv[2], b.m);
}

// ---- (a) the slots, and the compaction on arrays of exactly n entries ------------------------------------------------------
static void check_slots() {
  for (unsigned int n = 0; n <= 6; n++) {
    const unsigned int cand[] = {0, 1, 2, 3, 4, 5, 6, 7, kMergerNone};
    for (unsigned int ci : cand)
      for (unsigned int cj : cand) {
        const MergerSlots s = merger_slots(ci, cj, n);
        const bool valid = ci != cj && ci < n && cj < n;
        CHECK(s.valid == valid);
        if (!valid) continue;
        CHECK(s.lo == (ci < cj ? ci : cj) && s.hi == (ci < cj ? cj : ci) && s.dead == n - 1);
        CHECK(s.moved_from == (s.hi == n - 1 ? kMergerNone : n - 1));
        // the compaction as the kernel carries it out, on ids
        std::vector<unsigned int> ids(n);
        for (unsigned int k = 0; k < n; k++) ids[k] = k;
        if (s.moved_from != kMergerNone) ids[s.hi] = ids[s.moved_from];
        ids[s.dead] = kMergerNone;
        unsigned int alive = 0;
        for (unsigned int k = 0; k + 1 < n; k++) {
          CHECK(ids[k] != kMergerNone && ids[k] != s.hi);
          alive++;
        }
        CHECK(alive == n - 1 && ids[s.lo] == s.lo);
      }
  }
  CHECK(merger_concerned(1u, 0u) && !merger_concerned(0u, 0u) && !merger_concerned(2u, 0u) && !merger_concerned(3u, 0u) &&
        !merger_concerned(4u, 0u) && !merger_concerned(1u, 1u) && !merger_concerned(1u, 2u));
}

// ---- (b) known answers -------------------------------------------------------------------------------------------------------
static void check_known() {
  for (int ext = 0; ext < 2; ext++) {
    const DiagBody a{-0.5, 0.25, 1.0, 0.25, -0.125, 0.0, 0.5}, b{0.5, 0.75, 3.0, -0.25, 0.125, 0.0, 0.5};
    const MergerBody o = merger_merge(a, b, ext != 0);
    CHECK(o.M == 1.0 && o.mass == 1.0f);
    CHECK(o.x.hi == 0.0f && o.y.hi == 0.5f && o.z.hi == 2.0f && o.x.lo == 0.0f && o.y.lo == 0.0f && o.z.lo == 0.0f);
    CHECK(o.vx.hi == 0.0f && o.vy.hi == 0.0f && o.vz.hi == 0.0f && o.vx.lo == 0.0f);
    const DiagBody g = merger_stored(o);
    CHECK(merger_delta_ke(g, a, b) == -2.0 * (0.5 * (0.5 * (0.0625 + 0.015625))));
    // two massless bodies: the plain mean
    const DiagBody za{1.0, 2.0, 3.0, 1.0, 0.0, -1.0, 0.0}, zb{3.0, 2.0, -3.0, 0.0, 1.0, 1.0, 0.0};
    const MergerBody z = merger_merge(za, zb, ext != 0);
    CHECK(z.M == 0.0 && z.mass == 0.0f && z.x.hi == 2.0f && z.y.hi == 2.0f && z.z.hi == 0.0f && z.vx.hi == 0.5f &&
          z.vy.hi == 0.5f && z.vz.hi == 0.0f);
    // the split: hi + lo restores 48 bits in extended mode, lo is 0 otherwise
    const double v = 1.0 + std::ldexp(1.0, -30);
    const MergerSplit s = merger_split(v, ext != 0);
    CHECK(s.hi == 1.0f && s.lo == (ext ? std::ldexp(1.0f, -30) : 0.0f));
  }
  CHECK(merger_radius(0.0f, 0.0f) == 0.0f && merger_radius(2.0f, 0.0f) == 2.0f && merger_radius(0.0f, 0.5f) == 0.5f);
  CHECK(merger_radius(3.0f, 4.0f) == (float)std::cbrt(91.0) && merger_radius(1.0f, 1.0f) == (float)std::cbrt(2.0));
  // the pair's own term leaves, nobody else is there: delta_pe = +G ma mb / sqrt(d2 + eps2)
  const DiagBody a{0, 0, 0, 0, 0, 0, 2.0}, b{3.0, 4.0, 0, 0, 0, 0, 0.5};
  CHECK(merger_delta_pe(0.0, a, b, 2.0, 0.0) == 2.0 * (1.0 / 5.0));
  CHECK(merger_delta_pe(0.0, a, b, 2.0, 144.0) == 2.0 * (1.0 / 13.0));
  CHECK(merger_delta_pe(0.0, a, a, 1.0, 0.0) == 0.0);  // (coincident and unsoftened: the diagnostics' term is 0)
}

// ---- (c), (d) drawn systems ---------------------------------------------------------------------------------------------------
static void hex(const char* tag, double v) { std::printf(" %s %a", tag, v); }

static void drawn_case(const char* name, int n, int ci, int cj, bool ext, double G, float eps, Rng& rng) {
  std::vector<Body> B(n);
  for (Body& b : B) {
    for (int c = 0; c < 3; c++) {
      b.x[c] = (float)(4.0 * rng.next());
      b.v[c] = (float)rng.next();
      b.lx[c] = ext ? (float)(std::ldexp(rng.next(), -25) * std::fabs(b.x[c])) : 0.0f;
      b.lv[c] = ext ? (float)(std::ldexp(rng.next(), -25) * std::fabs(b.v[c])) : 0.0f;
    }
    b.m = (float)(0.6 + rng.next());
    b.r = (float)(0.3 + 0.5 * rng.next());
  }
  const double eps2 = (double)(eps * eps);  // the fp32 product, as the handle's
  const MergerSlots s = merger_slots((unsigned int)ci, (unsigned int)cj, (unsigned int)n);
  CHECK(s.valid);
  if (!s.valid) return;
  const DiagBody a = full(B[s.lo]), b = full(B[s.hi]);
  const MergerBody o = merger_merge(a, b, ext);
  const DiagBody g = merger_stored(o);
  std::vector<double> scratch(256);
  const double others = merger_others_model(n, (int)s.lo, (int)s.hi, 256, 64, scratch.data(),
                                            [&](int k) { return merger_pair_delta(g, a, b, full(B[k]), eps2); });
  const double dke = merger_delta_ke(g, a, b), dpe = merger_delta_pe(others, a, b, G, eps2);
  const float radius = merger_radius(B[s.lo].r, B[s.hi].r);

  // (c) long double: the merged body to 2 ulp of fp64 before the rounding to what is stored, the deltas to a bound on
  // the rounding of their sums
  const long double M = (long double)a.m + (long double)b.m;
  const double A6[6] = {a.x, a.y, a.z, a.vx, a.vy, a.vz}, B6[6] = {b.x, b.y, b.z, b.vx, b.vy, b.vz};
  const MergerSplit* S6[6] = {&o.x, &o.y, &o.z, &o.vx, &o.vy, &o.vz};
  CHECK(o.M == (double)M && o.mass == (float)(double)M);
  for (int c = 0; c < 6; c++) {
    const long double X = ((long double)a.m * A6[c] + (long double)b.m * B6[c]) / M;
    const double scale = (std::fabs(a.m * A6[c]) + std::fabs(b.m * B6[c])) / (double)M;
    const double got = (double)S6[c]->hi + (double)S6[c]->lo;
    const double tol = ext ? std::ldexp(scale, -46) : std::ldexp(std::fabs((double)X), -24) + std::ldexp(scale, -50);
    CHECK(std::fabs((double)((long double)got - X)) <= tol);
    CHECK(ext || S6[c]->lo == 0.0f);
  }
  const long double r3 = (long double)B[s.lo].r * B[s.lo].r * B[s.lo].r + (long double)B[s.hi].r * B[s.hi].r * B[s.hi].r;
  CHECK(std::fabs((double)((long double)radius - cbrtl(r3))) <= std::ldexp((double)radius, -23));
  auto ke = [](const DiagBody& q) { return 0.5L * q.m * ((long double)q.vx * q.vx + (long double)q.vy * q.vy + (long double)q.vz * q.vz); };
  auto term = [&](const DiagBody& p, const DiagBody& q) {
    const long double dx = (long double)q.x - p.x, dy = (long double)q.y - p.y, dz = (long double)q.z - p.z;
    const long double h = dx * dx + dy * dy + dz * dz + eps2;
    return h == 0.0L ? 0.0L : (long double)p.m * q.m / sqrtl(h);
  };
  long double sum = 0.0L, mag = (long double)std::fabs((double)term(a, b));
  for (int k = 0; k < n; k++)
    if (k != (int)s.lo && k != (int)s.hi) {
      const DiagBody q = full(B[k]);
      sum += term(g, q) - term(a, q) - term(b, q);
      mag += term(g, q) + term(a, q) + term(b, q);
    }
  CHECK(std::fabs((double)((long double)dke - (ke(g) - ke(a) - ke(b)))) <= std::ldexp((double)(ke(g) + ke(a) + ke(b)), -48));
  CHECK(std::fabs((double)((long double)dpe - (-(long double)G * (sum - term(a, b))))) <=
        std::fabs(G) * (double)mag * (n + 16) * std::ldexp(1.0, -52));

  // (d) printed
  std::printf("case %s n %d ext %d i %d j %d", name, n, ext ? 1 : 0, ci, cj);
  hex("G", G);
  hex("eps", (double)eps);
  std::printf("\n");
  for (int k = 0; k < n; k++) {
    std::printf("body %d", k);
    for (int c = 0; c < 3; c++) hex("x", B[k].x[c]);
    for (int c = 0; c < 3; c++) hex("lx", B[k].lx[c]);
    for (int c = 0; c < 3; c++) hex("v", B[k].v[c]);
    for (int c = 0; c < 3; c++) hex("lv", B[k].lv[c]);
    hex("m", B[k].m);
    hex("r", B[k].r);
    std::printf("\n");
  }
  std::printf("out lo %u hi %u moved %" PRId64 " dead %u", s.lo, s.hi, s.moved_from == kMergerNone ? (int64_t)-1 : (int64_t)s.moved_from,
              s.dead);
  hex("M", o.M);
  hex("mass", o.mass);
  for (int c = 0; c < 6; c++) {
    hex("hi", S6[c]->hi);
    hex("lo", S6[c]->lo);
  }
  hex("radius", radius);
  hex("dke", dke);
  hex("others", others);
  hex("dpe", dpe);
  std::printf("\n");
}

int main() {
  check_slots();
  check_known();
  Rng rng{20231u};
  const struct { const char* name; int n, i, j; } cases[] = {
      {"pair", 2, 1, 0},      {"triple01", 3, 0, 1},    {"triple02", 3, 2, 0},       {"triple12", 3, 1, 2},
      {"five", 5, 3, 1},      {"tile", 257, 3, 255},    {"block", 1025, 255, 3},     {"last", 300, 299, 7},
  };
  for (const auto& c : cases)
    for (int ext = 0; ext < 2; ext++)
      for (int soft = 0; soft < 2; soft++) drawn_case(c.name, c.n, c.i, c.j, ext != 0, soft ? 1.0 : 0.75, soft ? 0.05f : 0.0f, rng);
  if (failures) {
    std::printf("hermite_batch_mergers_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("hermite_batch_mergers_check: ok\n");
  return 0;
}
