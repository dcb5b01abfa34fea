// hermite_batch_hierarchy_check.cpp -- the arithmetic of the ensemble hierarchies on a CPU, under AddressSanitizer and
// UBSan (make hierarchy_check; plain g++, no device, nothing loaded into another process).  It includes
// hermite_batch_hierarchy_common.h, the file the examination of hermite_batch.hip is written in, and runs
//   (a) known-answer cases of the model in include/nbody_hip.h ("ensemble HIERARCHIES") whose arithmetic is exact: a
//       circular binary with a far single (receding, approaching, inside r_sep, failing the isolation criterion,
//       permuted), a hierarchical triple, two mirrored binaries with bitwise equal a, three singles, n = 2 bound and
//       unbound, massless bodies, the cold chain of 64;
//   (b) the triangular pair index on every t < 2,016 and the key order;
//   (c) the pair function, the elements and the composite against a long double restatement on random nodes, and the
//       sequential decomposition against one in long double on random systems, with the structure of every table checked.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "hermite_batch_hierarchy_common.h"

using namespace nbh;

namespace {

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

typedef std::vector<HierNode> Bodies;  // {x, y, z, vx, vy, vz, m}

struct Result {
  nbody_hip_batch_hierarchy_t rec;
  std::vector<nbody_hip_batch_node_t> table;
};

Result run(const Bodies& b, double G, double r_sep, double kappa) {
  Result r;
  const int n = (int)b.size();
  r.table.resize(2 * (size_t)n);
  hierarchy_model(n, [&](int i) {
    if (i < 0 || i >= n) {
      std::printf("FAIL: body index %d outside [0, %d)\n", i, n);
      std::exit(1);
    }
    return b[(size_t)i];
  }, G, r_sep, kappa, 7ull, &r.rec, r.table.data());
  return r;
}

// the canonical string of a forest (the rule of hierarchy_string in the Python package)
int lowest(const std::vector<nbody_hip_batch_node_t>& t, unsigned int k) {
  return t[k].left == kHierNone ? (int)k : std::min(lowest(t, t[k].left), lowest(t, t[k].right));
}
std::string text(const std::vector<nbody_hip_batch_node_t>& t, unsigned int k) {
  if (t[k].left == kHierNone) return std::to_string(k);
  unsigned int a = t[k].left, b = t[k].right;
  if (lowest(t, b) < lowest(t, a)) std::swap(a, b);
  return "[" + text(t, a) + " " + text(t, b) + "]";
}
std::string forest(const Result& r) {
  std::vector<std::pair<int, std::string>> tops;
  for (unsigned int k = 0; k < r.rec.node_count; k++)
    if (r.table[k].parent == kHierNone) tops.push_back({lowest(r.table, k), text(r.table, k)});
  std::sort(tops.begin(), tops.end());
  std::string s;
  for (size_t i = 0; i < tops.size(); i++) s += (i ? " " : "") + tops[i].second;
  return s;
}

// what every table must satisfy
void structure(const Result& r, int n) {
  const auto& t = r.table;
  const unsigned int count = r.rec.node_count;
  CHECK(count >= (unsigned int)n && count <= 2u * (unsigned int)n - 1u, "node_count %u of n = %d", count, n);
  unsigned int tops = 0, largest = 0;
  for (unsigned int k = 0; k < 2u * (unsigned int)n; k++) {
    const nbody_hip_batch_node_t& s = t[k];
    if (k >= count) {
      CHECK(s.left == 0 && s.right == 0 && s.parent == 0 && s.bodies == 0 && s.mass == 0 && s.a == 0 && s.e == 0 &&
            s.r == 0 && s.energy == 0 && s.reserved == 0, "slot %u above node_count is not zero", k);
      continue;
    }
    if (k < (unsigned int)n) {
      CHECK(s.left == kHierNone && s.right == kHierNone && s.bodies == 1 && s.a == 0 && s.e == 0 && s.r == 0 && s.energy == 0,
            "leaf %u", k);
    } else {
      CHECK(s.left < s.right && s.right < k, "composite %u of (%u, %u)", k, s.left, s.right);
      if (s.left < s.right && s.right < k) {
        CHECK(t[s.left].parent == k && t[s.right].parent == k, "children of %u do not point back", k);
        CHECK(s.bodies == t[s.left].bodies + t[s.right].bodies, "bodies of %u", k);
        CHECK(s.mass == t[s.left].mass + t[s.right].mass, "mass of %u", k);
      }
      CHECK(s.a > 0 && s.energy < 0 && s.r > 0 && s.e >= 0, "elements of composite %u", k);
    }
    if (s.parent == kHierNone) {
      tops++;
      largest = std::max(largest, s.bodies);
    } else {
      CHECK(s.parent > k && s.parent < count, "parent of %u", k);
    }
  }
  CHECK(tops == r.rec.top_count && tops + (count - (unsigned int)n) == (unsigned int)n, "top_count %u", r.rec.top_count);
  CHECK(largest == r.rec.largest, "largest %u", r.rec.largest);
  CHECK(r.rec.macro == 7ull && r.rec.reserved[0] == 0 && r.rec.reserved[1] == 0 && r.rec.reserved[2] == 0, "record");
  if (tops < 2) CHECK(std::isinf(r.rec.min_sep) && r.rec.min_p == kHierNone && r.rec.min_q == kHierNone && !r.rec.resolved, "K < 2");
}

HierNode B(double x, double y, double z, double vx, double vy, double vz, double m) { return HierNode{x, y, z, vx, vy, vz, m}; }

void known_answers() {
  // a circular binary of two masses 2 at distance 1 (G = 1: w = 2, eps = -2, a = 1, h = 2, e = 0, all exact) and a
  // single of mass 1 at x = 100
  const Bodies bin = {B(-0.5, 0, 0, 0, -1, 0, 2), B(0.5, 0, 0, 0, 1, 0, 2)};
  auto with = [&](HierNode third) { Bodies b = bin; b.push_back(third); return b; };
  {
    const Result r = run(with(B(100, 0, 0, 5, 0, 0, 1)), 1.0, 10.0, 5.0);
    structure(r, 3);
    CHECK(forest(r) == "[0 1] 2", "forest %s", forest(r).c_str());
    const nbody_hip_batch_node_t& c = r.table[3];
    CHECK(c.left == 0 && c.right == 1 && c.mass == 4.0 && c.a == 1.0 && c.e == 0.0 && c.r == 1.0 && c.energy == -2.0, "binary");
    CHECK(r.rec.resolved == 1 && r.rec.top_count == 2 && r.rec.node_count == 4 && r.rec.largest == 2, "record");
    CHECK(r.rec.min_sep == 100.0 && r.rec.min_p == 2 && r.rec.min_q == 3, "min_sep %g", r.rec.min_sep);
  }
  CHECK(run(with(B(100, 0, 0, -5, 0, 0, 1)), 1.0, 10.0, 5.0).rec.resolved == 0, "an approaching single");
  CHECK(run(with(B(100, 0, 0, 5, 0, 0, 1)), 1.0, 150.0, 0.0).rec.resolved == 0, "a single inside r_sep");
  CHECK(run(with(B(100, 0, 0, 5, 0, 0, 1)), 1.0, 100.0, 0.0).rec.resolved == 0, "r = r_sep is not beyond");
  CHECK(run(with(B(100, 0, 0, 5, 0, 0, 1)), 1.0, 10.0, 100.0).rec.resolved == 0, "r = kappa apo is not isolated");
  CHECK(run(with(B(100, 0, 0, 5, 0, 0, 1)), 1.0, 10.0, 99.0).rec.resolved == 1, "kappa 99");
  {
    const Bodies b = {bin[0], B(100, 0, 0, 5, 0, 0, 1), bin[1]};
    const Result r = run(b, 1.0, 10.0, 5.0);
    structure(r, 3);
    CHECK(forest(r) == "[0 2] 1" && r.table[3].left == 0 && r.table[3].right == 2 && r.rec.resolved == 1 &&
          r.rec.min_p == 1 && r.rec.min_q == 3, "permuted: %s", forest(r).c_str());
  }
  {  // a hierarchical triple: the third body bound to the pair
    const Result r = run(with(B(20, 0, 0, 0, 0.3, 0, 1)), 1.0, 10.0, 0.0);
    structure(r, 3);
    CHECK(forest(r) == "[[0 1] 2]" && r.rec.top_count == 1 && r.rec.node_count == 5 && r.rec.resolved == 0 &&
          r.rec.largest == 3 && r.table[4].left == 2 && r.table[4].right == 3, "triple: %s", forest(r).c_str());
  }
  {  // two mirrored binaries receding along x: bitwise equal a, the ids decide
    const Bodies b = {B(-10.5, 0, 0, -3, -1, 0, 2), B(-9.5, 0, 0, -3, 1, 0, 2), B(9.5, 0, 0, 3, -1, 0, 2), B(10.5, 0, 0, 3, 1, 0, 2)};
    const Result r = run(b, 1.0, 5.0, 2.0);
    structure(r, 4);
    CHECK(r.table[4].a == r.table[5].a && r.table[4].left == 0 && r.table[4].right == 1 && r.table[5].left == 2 &&
          r.table[5].right == 3, "the tie");
    CHECK(forest(r) == "[0 1] [2 3]" && r.rec.resolved == 1 && r.rec.top_count == 2 && r.rec.min_sep == 20.0 &&
          r.rec.min_p == 4 && r.rec.min_q == 5, "2+2: %s", forest(r).c_str());
  }
  {  // three mutually unbound receding singles
    const Bodies b = {B(-10, 0, 0, -4, 0, 0, 1), B(10, 0, 0, 4, 0, 0, 1), B(0, 10, 0, 0, 4, 0, 1)};
    const Result r = run(b, 1.0, 5.0, 3.0);
    structure(r, 3);
    CHECK(forest(r) == "0 1 2" && r.rec.top_count == 3 && r.rec.resolved == 1 && r.rec.node_count == 3 && r.rec.largest == 1, "ionisation");
    CHECK(r.rec.min_p == 0 && r.rec.min_q == 2 && r.rec.min_sep == std::sqrt(200.0), "the tie of the separations goes to (0, 2)");
  }
  {
    const Result r = run(bin, 1.0, 10.0, 0.0);
    structure(r, 2);
    CHECK(forest(r) == "[0 1]" && r.rec.top_count == 1 && r.rec.resolved == 0, "n = 2 bound");
    const Result u = run({B(-1, 0, 0, -3, 0, 0, 1), B(1, 0, 0, 3, 0, 0, 1)}, 1.0, 1.0, 0.0);
    structure(u, 2);
    CHECK(forest(u) == "0 1" && u.rec.top_count == 2 && u.rec.resolved == 1 && u.rec.min_sep == 2.0, "n = 2 unbound");
  }
  {  // a massless body bound to a massive one; two massless bodies are never a candidate
    const Result r = run({B(0, 0, 0, 0, 0, 0, 4), B(1, 0, 0, 0, 2, 0, 0)}, 1.0, 1.0, 0.0);
    structure(r, 2);
    CHECK(forest(r) == "[0 1]" && r.table[2].mass == 4.0 && r.table[2].a == 1.0 && r.table[2].e == 0.0, "massless bound");
    const Result z = run({B(0, 0, 0, 0, 0, 0, 0), B(1, 0, 0, 0, 0, 0, 0)}, 1.0, 0.5, 0.0);
    structure(z, 2);
    CHECK(forest(z) == "0 1" && z.rec.resolved == 0 && z.rec.min_sep == 1.0, "two massless bodies at rest");
  }
  {  // the cold chain x_i = 3^i: 63 nested composites, e = 1
    Bodies b;
    for (int i = 0; i < 64; i++) b.push_back(B(std::pow(3.0, i), 0, 0, 0, 0, 0, 1));
    const Result r = run(b, 1.0, 1.0, 0.0);
    structure(r, 64);
    CHECK(r.rec.node_count == 127 && r.rec.top_count == 1 && r.rec.largest == 64, "chain");
    for (unsigned int k = 64; k < 127; k++)
      CHECK(r.table[k].e == 1.0 && r.table[k].bodies == k - 62 && r.table[k].left == (k == 64 ? 0 : k - 63) &&
            r.table[k].right == (k == 64 ? 1 : k - 1), "chain node %u: (%u, %u)", k, r.table[k].left, r.table[k].right);
  }
  // NaN input: never a candidate, never resolved
  {
    const Result r = run({B(NAN, 0, 0, 0, 0, 0, 1), B(1, 0, 0, 0, 0, 0, 1)}, 1.0, 0.5, 0.0);
    CHECK(r.rec.top_count == 2 && r.rec.resolved == 0 && std::isinf(r.rec.min_sep) && r.rec.min_p == kHierNone, "NaN");
  }
}

void index_and_keys() {
  int t = 0;
  for (int j = 1; j < 64; j++)
    for (int i = 0; i < j; i++, t++) {
      int a, b;
      hier_pair_index(t, &a, &b);
      CHECK(a == i && b == j, "pair %d: (%d, %d), expected (%d, %d)", t, a, b, i, j);
    }
  CHECK(t == 2016, "2,016 pairs");
  const HierKey none = hier_key_none();
  CHECK(hier_key_is_none(none) && !hier_key_is_none(hier_key(INFINITY, 126, 127)), "none");
  CHECK(hier_key_less(hier_key(INFINITY, 126, 127), none) && hier_key_less(hier_key(1.0, 5, 6), hier_key(1.0000000000000002, 0, 1)), "value first");
  CHECK(hier_key_less(hier_key(1.0, 0, 7), hier_key(1.0, 1, 2)) && hier_key_less(hier_key(1.0, 1, 2), hier_key(1.0, 1, 3)), "then p, then q");
  CHECK(hier_key_less(hier_key(0.0, 3, 4), hier_key(5e-324, 0, 1)) && hier_key_value(hier_key(2.5, 1, 2)) == 2.5, "bits order");
}

// ---- the long double restatement -------------------------------------------------------------------------------------
struct LNode { long double x[3], v[3], m; };
struct LPair { long double M, r, eps, dw, a, e, kin, pot; };
LNode widen(const HierNode& b) { return LNode{{b.x, b.y, b.z}, {b.vx, b.vy, b.vz}, b.m}; }
LPair lpair(const LNode& p, const LNode& q, long double G) {
  long double d[3], w[3], r2 = 0, v2 = 0, dw = 0;
  for (int c = 0; c < 3; c++) {
    d[c] = q.x[c] - p.x[c];
    w[c] = q.v[c] - p.v[c];
    r2 += d[c] * d[c];
    v2 += w[c] * w[c];
    dw += d[c] * w[c];
  }
  LPair o;
  o.M = p.m + q.m;
  o.r = sqrtl(r2);
  o.kin = 0.5L * v2;
  o.pot = G * o.M / o.r;
  o.eps = o.kin - o.pot;
  o.dw = dw;
  o.a = G * o.M / (-2.0L * o.eps);
  const long double h[3] = {d[1] * w[2] - d[2] * w[1], d[2] * w[0] - d[0] * w[2], d[0] * w[1] - d[1] * w[0]};
  const long double t = 1.0L + 2.0L * o.eps * (h[0] * h[0] + h[1] * h[1] + h[2] * h[2]) / (G * o.M * G * o.M);
  o.e = sqrtl(t > 0 ? t : 0);
  return o;
}

void against_long_double() {
  std::mt19937_64 gen(20);
  std::uniform_real_distribution<double> pos(-4.0, 4.0), vel(-0.7, 0.7), mass(0.2, 2.0);
  auto body = [&] { return B(pos(gen), pos(gen), pos(gen), vel(gen), vel(gen), vel(gen), mass(gen)); };
  const double G = 1.3;
  for (int k = 0; k < 4000; k++) {
    const HierNode p = body(), q = body();
    const HierPair o = hier_pair(p, q, G);
    const LPair l = lpair(widen(p), widen(q), G);
    // eps: two terms of a handful of roundings each, with cancellation between them
    const double scale = (double)(l.kin + l.pot);
    CHECK(std::fabs(o.r - (double)l.r) <= 4 * U * (double)l.r, "r");
    CHECK(std::fabs(o.eps - (double)l.eps) <= 8 * U * scale, "eps %a against %La", o.eps, l.eps);
    CHECK(o.M == (double)l.M || std::fabs(o.M - (double)l.M) <= U * (double)l.M, "M");
    if (o.candidate && -l.eps > 1e-6L * scale) {
      const double amp = scale / (double)-l.eps;  // the relative error of eps enters a
      CHECK(std::fabs(o.a - (double)l.a) <= (8 * amp + 4) * U * (double)l.a, "a");
      const double e = hier_ecc(p, q, G, o.M, o.eps);
      // e^2 = 1 + t: absolute error of t about (8 amp + 12) u |t|, |t| <= 1 when e is real
      CHECK(std::fabs(e * e - (double)(l.e * l.e)) <= (8 * amp + 16) * U * 2.0, "e %a against %La", e, l.e);
    }
    const HierNode c = hier_composite(p, q, o.M);
    const long double cx = (p.m * (long double)p.x + q.m * (long double)q.x) / l.M;
    CHECK(std::fabs(c.x - (double)cx) <= 4 * U * (std::fabs(p.x) + std::fabs(q.x)), "composite");
  }
  // whole systems: the structure, and the forest of a decomposition in long double wherever every choice has a margin
  int compared = 0;
  for (int k = 0; k < 600; k++) {
    const int n = 2 + (int)(gen() % 9);
    Bodies b;
    for (int i = 0; i < n; i++) b.push_back(body());
    const Result r = run(b, G, 1.0, 0.5);
    structure(r, n);
    std::vector<LNode> node;
    std::vector<int> top;
    for (int i = 0; i < n; i++) { node.push_back(widen(b[(size_t)i])); top.push_back(i); }
    std::vector<std::pair<int, int>> made;
    bool clear = true;
    while (top.size() >= 2) {
      long double best = -1, second = -1;
      int bp = -1, bq = -1;
      for (size_t i = 0; i < top.size(); i++)
        for (size_t j = i + 1; j < top.size(); j++) {
          const LPair o = lpair(node[(size_t)top[i]], node[(size_t)top[j]], G);
          if (fabsl(o.eps) < 1e-9L * (o.kin + o.pot)) clear = false;
          if (!(o.M > 0 && o.r > 0 && o.eps < 0)) continue;
          if (best < 0 || o.a < best) { second = best; best = o.a; bp = top[i]; bq = top[j]; }
          else if (second < 0 || o.a < second) second = o.a;
        }
      if (bp < 0) break;
      if (second >= 0 && second - best < 1e-9L * second) clear = false;
      const LNode &p = node[(size_t)bp], &q = node[(size_t)bq];
      LNode c;
      c.m = p.m + q.m;
      for (int d = 0; d < 3; d++) {
        c.x[d] = (p.m * p.x[d] + q.m * q.x[d]) / c.m;
        c.v[d] = (p.m * p.v[d] + q.m * q.v[d]) / c.m;
      }
      made.push_back({bp, bq});
      std::vector<int> next;
      for (int id : top) if (id != bp && id != bq) next.push_back(id);
      next.push_back((int)node.size());
      node.push_back(c);
      top = next;
    }
    if (!clear) continue;
    compared++;
    CHECK(r.rec.node_count == (unsigned int)n + made.size(), "system %d: %u nodes against %zu composites", k, r.rec.node_count, made.size());
    for (size_t c = 0; c < made.size() && (unsigned int)n + c < r.rec.node_count; c++)
      CHECK((int)r.table[(size_t)n + c].left == made[c].first && (int)r.table[(size_t)n + c].right == made[c].second,
            "system %d, composite %zu", k, c);
  }
  CHECK(compared > 500, "only %d systems had clear choices", compared);
}

}  // namespace

int main() {
  known_answers();
  index_and_keys();
  against_long_double();
  if (failures) {
    std::printf("hierarchy_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("hierarchy_check: ok\n");
  return 0;
}
