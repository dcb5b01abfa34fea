// hermite_batch_outcomes_check.cpp -- the arithmetic of the ensemble outcomes on a CPU, under AddressSanitizer and UBSan
// (make outcomes_check; plain g++, no device, nothing loaded into another process).  It includes
// hermite_batch_outcomes_common.h, the file the escape test of hermite_batch.hip is written in, and runs
//   (a) known-answer cases of the model in include/nbody_hip.h ("ensemble OUTCOMES"): two bodies on an analytic
//       hyperbola, a bound pair beyond r_esc, an approaching body beyond r_esc, a rest without mass, a massless escaper,
//       NaN input, n = 1;
//   (b) the sums in the kernel's order (512 workers, waves of 64, distances 32 .. 1, eight waves in rising order) against
//       a long double sum in index order, to (ceil(n / 512) + 13) 2^-53 sum |t_k|, for sizes on both sides of every edge
//       of that order, with every index checked to be inside the system;
//   (c) the per-body quantities against a long double restatement of the formulas on random systems.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hermite_batch_outcomes_common.h"

using namespace nbh;

namespace {

constexpr int kThreads = 512, kWaveLanes = 64;
const double U = std::ldexp(1.0, -53);
int failures = 0;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      failures++;                                          \
    }                                                      \
  } while (0)

struct System {
  std::vector<float> p, pl, v, vl, m;  // [n][3] hi and lo, [n]
  int n() const { return (int)m.size(); }
  DiagBody body(int i) const {
    if (i < 0 || i >= n()) {
      std::printf("FAIL: body index %d outside [0, %d)\n", i, n());
      std::exit(1);
    }
    return diag_body(p[3 * i], p[3 * i + 1], p[3 * i + 2], pl[3 * i], pl[3 * i + 1], pl[3 * i + 2], v[3 * i], v[3 * i + 1],
                     v[3 * i + 2], vl[3 * i], vl[3 * i + 1], vl[3 * i + 2], m[i]);
  }
};

// rows: {x, y, z, vx, vy, vz, m} in fp64, split hi + lo as the engine does
System make(const std::vector<std::vector<double>>& rows) {
  System s;
  for (const auto& r : rows) {
    for (int c = 0; c < 6; c++) {
      const float hi = (float)r[c], lo = (float)(r[c] - (double)hi);
      (c < 3 ? s.p : s.v).push_back(hi);
      (c < 3 ? s.pl : s.vl).push_back(lo);
    }
    s.m.push_back((float)r[6]);
  }
  return s;
}

OutcomeSums sums_of(const System& s) {
  std::vector<OutcomeSums> scratch(kThreads);
  return outcome_sums_model(s.n(), kThreads, kWaveLanes, scratch.data(), [&](int i) { return s.body(i); });
}

// what the kernel records of a system at one boundary: the count, the lowest index, that body's values
struct Verdict {
  unsigned int count, lowest;
  OutcomeBody first;
};

Verdict verdict(const System& s, double G, double r_esc) {
  Verdict v{0u, 0xffffffffu, OutcomeBody{0, 0, 0, 0, 0, false}};
  if (s.n() < 2 || !(r_esc > 0.0)) return v;
  const OutcomeSums S = sums_of(s);
  for (int i = s.n() - 1; i >= 0; i--) {  // (any order: a count and a minimum)
    const OutcomeBody o = outcome_body(S, s.body(i), G, r_esc);
    if (o.escapes) {
      v.count++;
      if ((unsigned int)i < v.lowest) {
        v.lowest = (unsigned int)i;
        v.first = o;
      }
    }
  }
  return v;
}

void known_answers() {
  // two equal bodies receding radially: r = 4, |w| = 1, G M = 1: e = 1/2 - 1/4 = 1/4 = v_inf^2 / 2 exactly, vr = 1
  {
    const System s = make({{2, 0, 0, 0.5, 0, 0, 0.5}, {-2, 0, 0, -0.5, 0, 0, 0.5}});
    const Verdict v = verdict(s, 1.0, 3.0);
    CHECK(v.count == 2u && v.lowest == 0u, "hyperbola: count %u lowest %u", v.count, v.lowest);
    CHECK(v.first.r == 4.0 && v.first.vr == 1.0 && v.first.e == 0.25 && v.first.rest_mass == 0.5,
          "hyperbola: r %.17g vr %.17g e %.17g M_r %.17g", v.first.r, v.first.vr, v.first.e, v.first.rest_mass);
    // ... inside the escape radius: nobody
    CHECK(verdict(s, 1.0, 4.0).count == 0u, "hyperbola at r == r_esc: the comparison is strict");
    CHECK(verdict(s, 1.0, 0.0).count == 0u, "r_esc = 0: no test");
    // a general hyperbola: v_inf = 0.3 at r = 10 with G M = 1, 0.7 rad off the radius: e = v_inf^2 / 2 (the state is
    // hi + lo of two floats: 2^-48 relative)
    const double vinf = 0.3, r = 10.0, w = std::sqrt(vinf * vinf + 2.0 / r), c = std::cos(0.7), sn = std::sin(0.7);
    const System h = make({{0.25 * r, 0, 0, 0.25 * w * c, 0.25 * w * sn, 0, 0.75}, {-0.75 * r, 0, 0, -0.75 * w * c, -0.75 * w * sn, 0, 0.25}});
    const Verdict vh = verdict(h, 1.0, 5.0);
    CHECK(vh.count == 2u && vh.lowest == 0u, "general hyperbola: count %u", vh.count);
    CHECK(std::fabs(vh.first.e - 0.5 * vinf * vinf) < 1e-13, "general hyperbola: e %.17g", vh.first.e);
    CHECK(std::fabs(vh.first.r - r) < 1e-12 && std::fabs(vh.first.vr - w * c) < 1e-13, "general hyperbola: r, vr");
  }
  // a bound pair beyond r_esc, moving outward: e < 0
  {
    const System s = make({{0.875, 0, 0, 0.125, 0.125, 0, 0.5}, {-0.875, 0, 0, -0.125, -0.125, 0, 0.5}});
    const OutcomeBody o = outcome_body(sums_of(s), s.body(0), 1.0, 1.5);
    CHECK(o.r == 1.75 && o.dw > 0.0 && o.e < 0.0 && !o.escapes, "bound pair: r %.17g dw %.17g e %.17g", o.r, o.dw, o.e);
    CHECK(verdict(s, 1.0, 1.5).count == 0u, "bound pair beyond r_esc");
  }
  // an unbound body beyond r_esc that APPROACHES: d.w < 0
  {
    const System s = make({{2, 0, 0, -0.5, 0, 0, 0.5}, {-2, 0, 0, 0.5, 0, 0, 0.5}});
    const OutcomeBody o = outcome_body(sums_of(s), s.body(0), 1.0, 3.0);
    CHECK(o.e == 0.25 && o.dw < 0.0 && o.vr == -1.0 && !o.escapes, "approaching: e %.17g dw %.17g", o.e, o.dw);
    CHECK(verdict(s, 1.0, 3.0).count == 0u, "approaching body");
  }
  // the whole mass in body 0: body 0 has M_r = 0 and never escapes; the massless body 1 can
  {
    const System s = make({{0, 0, 0, 0, 0, 0, 1.0}, {4, 0, 0, 1, 0, 0, 0.0}});
    const OutcomeSums S = sums_of(s);
    const OutcomeBody o0 = outcome_body(S, s.body(0), 1.0, 3.0), o1 = outcome_body(S, s.body(1), 1.0, 3.0);
    CHECK(!o0.escapes && o0.rest_mass == 0.0 && o0.r == 0.0 && o0.e == 0.0, "M_r = 0");
    CHECK(o1.escapes && o1.r == 4.0 && o1.vr == 1.0 && o1.e == 0.25 && o1.rest_mass == 1.0, "massless escaper: e %.17g", o1.e);
    const Verdict v = verdict(s, 1.0, 3.0);
    CHECK(v.count == 1u && v.lowest == 1u, "massless escaper: count %u lowest %u", v.count, v.lowest);
    // all bodies massless: nobody
    const System z = make({{0, 0, 0, 0, 0, 0, 0.0}, {4, 0, 0, 1, 0, 0, 0.0}});
    CHECK(verdict(z, 1.0, 3.0).count == 0u, "massless system");
  }
  // NaN input: every comparison is false
  {
    const System s = make({{2, 0, 0, 0.5, 0, 0, 0.5}, {-2, NAN, 0, -0.5, 0, 0, 0.5}});
    CHECK(verdict(s, 1.0, 3.0).count == 0u, "NaN position");
    const System t = make({{2, 0, 0, 0.5, 0, 0, 0.5}, {-2, 0, 0, -0.5, 0, 0, NAN}});
    CHECK(verdict(t, 1.0, 3.0).count == 0u, "NaN mass");
    const System c = make({{2, 0, 0, 0.5, 0, 0, 0.5}, {-2, 0, 0, -0.5, 0, 0, 0.5}});
    CHECK(verdict(c, NAN, 3.0).count == 0u, "NaN G");
  }
  // n = 1: M_r = m - m = 0
  {
    const System s = make({{5, 0, 0, 3, 0, 0, 1.0}});
    CHECK(!outcome_body(sums_of(s), s.body(0), 1.0, 1.0).escapes && verdict(s, 1.0, 1.0).count == 0u, "n = 1");
  }
}

System random_system(int n, unsigned seed) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> N(0.0, 1.0);
  std::uniform_real_distribution<double> M(0.5, 1.5);
  std::vector<std::vector<double>> rows;
  for (int i = 0; i < n; i++) rows.push_back({N(g), N(g), N(g), N(g), N(g), N(g), M(g) / n});
  return make(rows);
}

void sums_in_kernel_order() {
  for (int n : {1, 2, 5, 63, 64, 65, 511, 512, 513, 1024, 1025, 4095, 4096}) {
    const System s = random_system(n, 100u + (unsigned)n);
    const OutcomeSums S = sums_of(s);
    long double ref[kOutcomeSums] = {0}, mag[kOutcomeSums] = {0};
    for (int i = 0; i < n; i++) {
      const DiagBody b = s.body(i);
      const long double t[kOutcomeSums] = {(long double)b.m, (long double)b.m * b.x, (long double)b.m * b.y, (long double)b.m * b.z,
                                           (long double)b.m * b.vx, (long double)b.m * b.vy, (long double)b.m * b.vz};
      for (int k = 0; k < kOutcomeSums; k++) {
        ref[k] += t[k];
        mag[k] += std::fabs(t[k]);
      }
    }
    const double ops = (double)((n + kThreads - 1) / kThreads + 6 + 7 + 1);  // additions on the longest path, + the product
    for (int k = 0; k < kOutcomeSums; k++)
      CHECK(std::fabs((double)((long double)S.v[k] - ref[k])) <= ops * U * (double)mag[k], "n %d sum %d: %.17g against %.17Lg", n,
            k, S.v[k], ref[k]);
  }
}

void bodies_against_long_double() {
  for (int n : {2, 3, 64, 600}) {
    const System s = random_system(n, 7u + (unsigned)n);
    const OutcomeSums S = sums_of(s);
    const double G = 1.0;
    for (int i = 0; i < n; i++) {
      const DiagBody b = s.body(i);
      const OutcomeBody o = outcome_body(S, b, G, 0.5);
      const long double mr = (long double)S.v[0] - b.m;
      const long double X[3] = {b.x, b.y, b.z}, V[3] = {b.vx, b.vy, b.vz};
      long double r2 = 0, w2 = 0, dw = 0;
      for (int c = 0; c < 3; c++) {
        const long double d = X[c] - ((long double)S.v[1 + c] - (long double)b.m * X[c]) / mr;
        const long double w = V[c] - ((long double)S.v[4 + c] - (long double)b.m * V[c]) / mr;
        r2 += d * d;
        w2 += w * w;
        dw += d * w;
      }
      const long double r = sqrtl(r2), e = 0.5L * w2 - (long double)G * S.v[0] / r;
      // (well conditioned by construction: masses of one size, no body near the rest's centre of mass on the scale 1e-3)
      const double tol = 1e-12;
      CHECK(std::fabs((double)(o.r - r)) <= tol * (double)r, "n %d body %d: r", n, i);
      CHECK(std::fabs((double)(o.vr - dw / r)) <= tol * (double)(sqrtl(w2)), "n %d body %d: vr", n, i);
      CHECK(std::fabs((double)(o.e - e)) <= tol * (double)(0.5L * w2 + (long double)G * S.v[0] / r), "n %d body %d: e", n, i);
      CHECK(std::fabs((double)(o.rest_mass - mr)) <= U * (double)mr, "n %d body %d: M_r", n, i);
      CHECK(o.escapes == (r > 0.5L && dw > 0 && e > 0), "n %d body %d: the decision", n, i);
    }
  }
}

}  // namespace

int main() {
  known_answers();
  sums_in_kernel_order();
  bodies_against_long_double();
  if (failures) {
    std::printf("hermite_batch_outcomes_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("hermite_batch_outcomes_check: ok\n");
  return 0;
}
