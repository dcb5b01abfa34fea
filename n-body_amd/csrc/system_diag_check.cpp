// system_diag_check.cpp -- the arithmetic of the ensemble diagnostics on a CPU, under AddressSanitizer and UBSan (make
// diag_check; plain g++, no device, nothing loaded into another process).  It includes system_diag_common.h, the file
// the kernel of system_diag.hip is written in, and evaluates nbody_hip_system_diag for the edge systems of the model
//   (a) by a straightforward loop over the shared functions: bodies in index order, pairs i < j in index order;
//   (b) in the KERNEL'S order: 256 workers, the cells of diag_cells per worker, sources in tiles of 512 held in a buffer
//       of exactly 512 entries, the wave reduction at distances 32 .. 1 and the four waves in order -- checking on the way
//       that every pair i < j is visited exactly once and every index is inside the system and the tile;
//   (c) by a long double restatement of the formulas in include/nbody_hip.h.
// (a) and (b) must agree exactly in every index and minimum and to the summation bound in the sums; both must agree
// with (c) to the bound (terms + 32) 2^-53 sum |t_k| per sum and 64 2^-53 relative in the pair quantities.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "system_diag_common.h"

using namespace nbh;

namespace {

constexpr int kThreads = 256, kWaveLanes = 64, kTile = 512;
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
  const char* name;
  std::vector<float> p, pl, v, vl, m;  // [n][3] hi and lo, [n]
  double G, eps2;
  int n() const { return (int)m.size(); }
  DiagBody body(int i) const {
    return diag_body(p[3 * i], p[3 * i + 1], p[3 * i + 2], pl[3 * i], pl[3 * i + 1], pl[3 * i + 2], v[3 * i], v[3 * i + 1],
                     v[3 * i + 2], vl[3 * i], vl[3 * i + 1], vl[3 * i + 2], m[i]);
  }
};

System make(const char* name, const std::vector<std::vector<double>>& rows, double G, float eps) {
  // rows: {x, y, z, vx, vy, vz, m} in fp64, split hi + lo as the engine does
  System s;
  s.name = name;
  s.G = G;
  s.eps2 = (double)(eps * eps);
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

// (a)
nbody_hip_system_diag straightforward(const System& s) {
  const int n = s.n();
  DiagSums sums;
  diag_sums_zero(sums);
  DiagMin sep = diag_min_none(INFINITY), bind = diag_min_none(0.0);
  for (int i = 0; i < n; i++) diag_body_add(sums, s.body(i));
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      const DiagPair p = diag_pair(s.body(i), s.body(j), s.G, s.eps2);
      sums.v[kDiagSums - 1] += p.term;
      diag_min_take(sep, p.r, i, j);
      if (p.bindable) diag_min_take(bind, p.eb, i, j);
    }
  nbody_hip_system_diag o{};
  const bool bound = bind.i >= 0 && bind.v < 0.0;
  diag_finish(sums, sep, bind, bound ? s.body(bind.i) : DiagBody{}, bound ? s.body(bind.j) : DiagBody{}, s.G, n, &o);
  return o;
}

// (b); arithmetic == false: the enumeration alone (the large sizes)
nbody_hip_system_diag kernel_order(const System& s, int n, bool arithmetic) {
  const DiagCells cells = diag_cells(n, kThreads);
  std::vector<DiagSums> sums(kThreads);
  std::vector<DiagMin> sep(kThreads, diag_min_none(INFINITY)), bind(kThreads, diag_min_none(0.0));
  for (auto& x : sums) diag_sums_zero(x);
  std::vector<unsigned char> seen((size_t)n * n, 0);
  std::vector<long long> per_worker(kThreads, 0);
  for (int t0 = 0; t0 < n; t0 += kTile) {
    const int t1 = diag_imin(t0 + kTile, n);
    std::vector<DiagBody> tile((size_t)(t1 - t0));  // exactly the tile: an index outside it is an ASan report
    for (int tid = 0; tid < kThreads; tid++)
      for (int k = t0 + tid; k < t1; k += kThreads) {
        if (!arithmetic) continue;
        tile[(size_t)(k - t0)] = s.body(k);
        diag_body_add(sums[tid], tile[(size_t)(k - t0)]);
      }
    for (int tid = 0; tid < kThreads; tid++) {
      int a, b, r0, r1;
      diag_worker_cells(cells, tid, &a, &b, &r0, &r1);
      CHECK(b - a <= cells.q && a <= b, "n %d worker %d: cells [%d, %d) exceed q %d", n, tid, a, b, cells.q);
      for (int r = r0; r < r1; r++) {
        CHECK(r >= 0 && r < cells.R, "n %d worker %d: row %d of %d", n, tid, r, cells.R);
        DiagRun run[2];
        diag_row_runs(cells, a, b, r, t0, t1, &run[0], &run[1]);
        for (int h = 0; h < 2; h++) {
          if (run[h].jlo >= run[h].jhi) continue;
          const int i = run[h].i;
          CHECK(i >= 0 && i < n, "n %d: target %d", n, i);
          for (int j = run[h].jlo; j < run[h].jhi; j++) {
            CHECK(j > i && j < n && j >= t0 && j < t1, "n %d: pair (%d, %d) in tile [%d, %d)", n, i, j, t0, t1);
            if (!(j > i && j < n && i >= 0)) continue;
            seen[(size_t)i * n + j]++;
            per_worker[tid]++;
            if (!arithmetic) continue;
            const DiagPair p = diag_pair(s.body(i), tile.at((size_t)(j - t0)), s.G, s.eps2);
            sums[tid].v[kDiagSums - 1] += p.term;
            diag_min_take(sep[tid], p.r, i, j);
            if (p.bindable) diag_min_take(bind[tid], p.eb, i, j);
          }
        }
      }
    }
  }
  long long bad = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) bad += seen[(size_t)i * n + j] != (j > i ? 1 : 0);
  CHECK(bad == 0, "n %d: %lld pairs not visited exactly once", n, bad);
  for (int tid = 0; tid < kThreads; tid++)
    CHECK(per_worker[tid] <= cells.q, "n %d worker %d: %lld pairs, q = %d", n, tid, per_worker[tid], cells.q);
  // q + 9 <= n^2 / 512 + 64: the chain length DESIGN.md section 4.14 states
  CHECK((double)cells.q + 9.0 <= (double)n * n / 512.0 + 64.0, "n %d: q = %d", n, cells.q);
  nbody_hip_system_diag o{};
  if (!arithmetic) return o;
  for (int off = kWaveLanes / 2; off > 0; off >>= 1)
    for (int w = 0; w < kThreads / kWaveLanes; w++)
      for (int l = 0; l < kWaveLanes; l++) {  // (ascending: lane l reads lane l + off before that one changes)
        const int t = w * kWaveLanes + l;
        if (l + off >= kWaveLanes) continue;  // (the shuffle hands such a lane its own value; lane 0 never reads it)
        for (int k = 0; k < kDiagSums; k++) sums[t].v[k] += sums[t + off].v[k];
        diag_min_merge(sep[t], sep[t + off]);
        diag_min_merge(bind[t], bind[t + off]);
      }
  for (int w = 1; w < kThreads / kWaveLanes; w++) {
    for (int k = 0; k < kDiagSums; k++) sums[0].v[k] += sums[w * kWaveLanes].v[k];
    diag_min_merge(sep[0], sep[w * kWaveLanes]);
    diag_min_merge(bind[0], bind[w * kWaveLanes]);
  }
  const bool bound = bind[0].i >= 0 && bind[0].v < 0.0;
  diag_finish(sums[0], sep[0], bind[0], bound ? s.body(bind[0].i) : DiagBody{}, bound ? s.body(bind[0].j) : DiagBody{}, s.G,
              n, &o);
  return o;
}

// (c)
struct Ref {
  long double mass, com[3], mom[3], ang[3], ke, pe, min_sep, eb, a, e;
  long double abs_sum[12];  // sum |t_k| of: mass, m X (3), m V (3), m X x V (3), KE, PE
  int min_i, min_j, bind_i, bind_j;
};

Ref restate(const System& s) {
  typedef long double ld;
  const int n = s.n();
  Ref r{};
  r.min_i = r.min_j = r.bind_i = r.bind_j = -1;
  r.min_sep = INFINITY;
  std::vector<ld> X(3 * (size_t)n), V(3 * (size_t)n), M((size_t)n);
  for (int i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) {
      X[3 * i + c] = (ld)s.p[3 * i + c] + (ld)s.pl[3 * i + c];
      V[3 * i + c] = (ld)s.v[3 * i + c] + (ld)s.vl[3 * i + c];
    }
    M[i] = (ld)s.m[i];
  }
  ld sm[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    const ld *x = &X[3 * i], *v = &V[3 * i], m = M[i];
    r.mass += m;
    r.abs_sum[0] += fabsl(m);
    const ld l[3] = {x[1] * v[2] - x[2] * v[1], x[2] * v[0] - x[0] * v[2], x[0] * v[1] - x[1] * v[0]};
    // (the cross product cancels: its terms are bounded by the products, not by the result)
    const ld la[3] = {fabsl(x[1] * v[2]) + fabsl(x[2] * v[1]), fabsl(x[2] * v[0]) + fabsl(x[0] * v[2]),
                      fabsl(x[0] * v[1]) + fabsl(x[1] * v[0])};
    for (int c = 0; c < 3; c++) {
      sm[c] += m * x[c];
      r.abs_sum[1 + c] += fabsl(m * x[c]);
      r.mom[c] += m * v[c];
      r.abs_sum[4 + c] += fabsl(m * v[c]);
      r.ang[c] += m * l[c];
      r.abs_sum[7 + c] += fabsl(m) * la[c];
    }
    const ld k = 0.5L * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    r.ke += k;
    r.abs_sum[10] += fabsl(k);
  }
  for (int c = 0; c < 3; c++) r.com[c] = r.mass == 0 ? 0 : sm[c] / r.mass;
  bool any = false;
  ld best = 0;
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      ld d[3], w[3], r2 = 0, w2 = 0;
      for (int c = 0; c < 3; c++) {
        d[c] = X[3 * j + c] - X[3 * i + c];
        w[c] = V[3 * j + c] - V[3 * i + c];
        r2 += d[c] * d[c];
        w2 += w[c] * w[c];
      }
      const ld h = r2 + (ld)s.eps2;
      if (h != 0) {
        const ld t = (ld)s.G * M[i] * M[j] / sqrtl(h);
        r.pe -= t;
        r.abs_sum[11] += fabsl(t);
      }
      const ld sep = sqrtl(r2);
      if (sep < r.min_sep) {
        r.min_sep = sep;
        r.min_i = i;
        r.min_j = j;
      }
      const ld ms = M[i] + M[j];
      if (sep > 0 && ms > 0) {
        const ld mu = M[i] * M[j] / ms;
        const ld eb = 0.5L * mu * w2 - (ld)s.G * M[i] * M[j] / sep;
        if (!any || eb < best) {
          any = true;
          best = eb;
          if (eb < 0) {
            const ld hx = d[1] * w[2] - d[2] * w[1], hy = d[2] * w[0] - d[0] * w[2], hz = d[0] * w[1] - d[1] * w[0];
            const ld gm = (ld)s.G * ms;
            const ld q = 1 + 2 * (eb / mu) * (hx * hx + hy * hy + hz * hz) / (gm * gm);
            r.eb = eb;
            r.a = -(ld)s.G * M[i] * M[j] / (2 * eb);
            r.e = sqrtl(q > 0 ? q : 0);
            r.bind_i = i;
            r.bind_j = j;
          }
        }
      }
    }
  return r;
}

void compare(const System& s, const char* how, const nbody_hip_system_diag& o, const Ref& r, double terms_pairs) {
  const int n = s.n();
  auto sum_ok = [&](double got, long double want, long double abs_sum, double terms, const char* what) {
    const long double bound = (terms + 32.0) * U * abs_sum;
    CHECK(fabsl((long double)got - want) <= bound, "%s (%s) %s: got %.17g, want %.17Lg, bound %.3Lg", s.name, how, what, got,
          want, bound);
  };
  sum_ok(o.mass, r.mass, r.abs_sum[0], n, "mass");
  for (int c = 0; c < 3; c++) {
    // com = (sum m X) / mass: the sum's bound over the mass, and one rounding
    if (r.mass != 0) {
      const long double bound = (n + 34.0) * U * r.abs_sum[1 + c] / fabsl(r.mass);
      CHECK(fabsl((long double)o.com[c] - r.com[c]) <= bound, "%s (%s) com[%d]: got %.17g want %.17Lg", s.name, how, c,
            o.com[c], r.com[c]);
    } else {
      CHECK(o.com[c] == 0.0, "%s (%s) com[%d] with mass 0: %g", s.name, how, c, o.com[c]);
    }
    sum_ok(o.momentum[c], r.mom[c], r.abs_sum[4 + c], n, "momentum");
    sum_ok(o.ang_mom[c], r.ang[c], r.abs_sum[7 + c], n, "ang_mom");
  }
  sum_ok(o.kinetic, r.ke, r.abs_sum[10], n, "kinetic");
  sum_ok(o.potential, r.pe, r.abs_sum[11], terms_pairs, "potential");
  CHECK(o.n == n && o.status == 0, "%s (%s): n %d status %d", s.name, how, o.n, o.status);
  CHECK(o.min_i == r.min_i && o.min_j == r.min_j, "%s (%s): min pair (%d, %d), want (%d, %d)", s.name, how, o.min_i, o.min_j,
        r.min_i, r.min_j);
  CHECK(o.bind_i == r.bind_i && o.bind_j == r.bind_j, "%s (%s): bound pair (%d, %d), want (%d, %d)", s.name, how, o.bind_i,
        o.bind_j, r.bind_i, r.bind_j);
  auto rel_ok = [&](double got, long double want, const char* what) {
    const bool ok = std::isinf((double)want) ? got == (double)want : fabsl((long double)got - want) <= 64.0 * U * fabsl(want);
    CHECK(ok, "%s (%s) %s: got %.17g, want %.17Lg", s.name, how, what, got, want);
  };
  rel_ok(o.min_sep, r.min_sep, "min_sep");
  rel_ok(o.bind_energy, r.eb, "bind_energy");
  rel_ok(o.bind_a, r.a, "bind_a");
  if (r.bind_i >= 0 && r.e > 0)
    CHECK(fabsl((long double)o.bind_e - r.e) <= 64.0 * U / r.e, "%s (%s) bind_e: got %.17g, want %.17Lg", s.name, how, o.bind_e,
          r.e);
  else
    CHECK(o.bind_e == 0.0 || r.bind_i >= 0, "%s (%s) bind_e without a pair: %g", s.name, how, o.bind_e);
}

void same(const System& s, const nbody_hip_system_diag& a, const nbody_hip_system_diag& b) {
  CHECK(a.mass == b.mass && a.min_sep == b.min_sep && a.bind_energy == b.bind_energy && a.bind_a == b.bind_a &&
            a.bind_e == b.bind_e && a.min_i == b.min_i && a.min_j == b.min_j && a.bind_i == b.bind_i && a.bind_j == b.bind_j &&
            a.n == b.n && a.status == b.status,
        "%s: the two orders differ in an index or a minimum", s.name);
}

void run(const System& s) {
  const int n = s.n();
  const Ref r = restate(s);
  const nbody_hip_system_diag a = straightforward(s), b = kernel_order(s, n, true);
  compare(s, "index order", a, r, 0.5 * n * (n - 1));
  compare(s, "kernel order", b, r, diag_cells(n, kThreads).q + 9);
  same(s, a, b);
  std::printf("%-28s n %4d  KE %.17g  PE %.17g  min (%d, %d) %.17g  bound (%d, %d) E_b %.17g a %.17g e %.17g\n", s.name, n,
              b.kinetic, b.potential, b.min_i, b.min_j, b.min_sep, b.bind_i, b.bind_j, b.bind_energy, b.bind_a, b.bind_e);
}

}  // namespace

int main() {
  static_assert(sizeof(nbody_hip_system_diag) == 152, "nbody_hip_system_diag is 152 bytes");
  // 1. the edge systems of the model
  const System one = make("one body", {{1, 2, 3, 0.1, 0.2, 0.3, 2}}, 1.0, 0.05f);
  run(one);
  {
    const nbody_hip_system_diag o = straightforward(one);
    CHECK(std::isinf(o.min_sep) && o.min_sep > 0 && o.min_i == -1 && o.min_j == -1 && o.bind_i == -1 && o.bind_j == -1 &&
              o.potential == 0.0,
          "one body: min_sep %g pair (%d, %d) PE %g", o.min_sep, o.min_i, o.min_j, o.potential);
  }
  const System tie = make("min_sep tie", {{0, 0, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 3, 0, 1}, {0, 1, 0, 3, 0, 0, 1}}, 1.0, 0.f);
  run(tie);
  {
    const nbody_hip_system_diag o = kernel_order(tie, 3, true);
    CHECK(o.min_i == 0 && o.min_j == 1 && o.min_sep == 1.0, "tie: (%d, %d) %g", o.min_i, o.min_j, o.min_sep);
  }
  const std::vector<std::vector<double>> coincident = {{0.5, 0.25, 0, 0, 0, 0, 1}, {0.5, 0.25, 0, 0.1, 0, 0, 2}, {4, 0, 0, 0, 9, 0, 1}};
  const System c0 = make("coincident pair, eps = 0", coincident, 1.0, 0.f);
  run(c0);
  {
    const nbody_hip_system_diag o = kernel_order(c0, 3, true);
    CHECK(o.min_sep == 0.0 && o.min_i == 0 && o.min_j == 1 && o.bind_i == -1 && std::isfinite(o.potential),
          "coincident, eps 0: min %g (%d, %d) bound %d PE %g", o.min_sep, o.min_i, o.min_j, o.bind_i, o.potential);
  }
  const System c1 = make("coincident pair, eps = 1/4", {{0.5, 0.25, 0, 0, 0, 0, 1}, {0.5, 0.25, 0, 0.1, 0, 0, 2}}, 1.5, 0.25f);
  run(c1);
  {
    const nbody_hip_system_diag o = kernel_order(c1, 2, true);
    CHECK(o.potential == -1.5 * 1 * 2 / 0.25 && o.bind_i == -1, "coincident, eps 1/4: PE %.17g", o.potential);
  }
  const System massless = make("all masses 0", {{1, 0, 0, 0, 1, 0, 0}, {-1, 0, 0, 0, -1, 0, 0}, {0, 2, 0, 1, 0, 0, 0}}, 1.0, 0.f);
  run(massless);
  {
    const nbody_hip_system_diag o = kernel_order(massless, 3, true);
    CHECK(o.com[0] == 0 && o.com[1] == 0 && o.com[2] == 0 && o.bind_i == -1 && o.mass == 0, "all masses 0");
  }
  const System hyper = make("hyperbolic pair", {{-1, 0, 0, 0, -2, 0, 1}, {1, 0, 0, 0, 2, 0, 1}}, 1.0, 0.f);
  run(hyper);
  CHECK(kernel_order(hyper, 2, true).bind_i == -1, "a hyperbolic pair is not bound");
  // two bound pairs with exactly equal E_b: the second is the first mirrored (x -> -x, v -> -v) and shifted by a power of two
  const System twins = make("two equal bound pairs",
                            {{64.5, 0, 0, 0, 0.5, 0, 1}, {65.5, 0, 0, 0, -0.5, 0, 1}, {-64.5, 0, 0, 0, -0.5, 0, 1},
                             {-65.5, 0, 0, 0, 0.5, 0, 1}},
                            1.0, 0.f);
  run(twins);
  {
    const nbody_hip_system_diag o = kernel_order(twins, 4, true);
    CHECK(o.bind_i == 0 && o.bind_j == 1 && o.min_i == 0 && o.min_j == 1 && o.bind_energy < 0, "twins: bound (%d, %d)", o.bind_i,
          o.bind_j);
  }
  // 2. clusters with residuals that matter, at sizes on both sides of a worker, a row and a tile
  std::mt19937_64 gen(20);
  std::normal_distribution<double> g(0.0, 1.0);
  std::uniform_real_distribution<double> um(0.5, 2.0);
  for (int n : {2, 5, 63, 65, 257, 513, 1025}) {
    std::vector<std::vector<double>> rows;
    for (int i = 0; i < n; i++)
      rows.push_back({64 + 0.01 * g(gen), -32 + 0.01 * g(gen), 16 + 0.01 * g(gen), 3 * g(gen), 3 * g(gen), 3 * g(gen), um(gen) / n});
    rows[1] = rows[0];  // a tight, bound pair: its separation is far below the fp32 spacing at 64
    rows[1][0] += 1e-7;
    rows[1][4] += 0.01;
    const std::string name = "cluster of " + std::to_string(n);
    run(make(name.c_str(), rows, 1.7, 1e-4f));
  }
  // 3. the enumeration alone at every size class up to the largest system
  const System none{};
  for (int n : {1, 2, 3, 4, 64, 255, 256, 511, 512, 1024, 2047, 2048, 3000, 4095, 4096}) (void)kernel_order(none, n, false);
  if (failures) {
    std::printf("system_diag_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("system_diag_check: ok\n");
  return 0;
}
