// slab_plan_check.cpp -- the host arithmetic of the sharded spatial hash's exchange (slab_plan.h) on a CPU, under
// AddressSanitizer and UBSan (make plan_check): the owner formula against its written-out definition, the slab map's
// invariants, the balancing rule on histograms whose answer can be seen by eye, the adoption rule at its edge, and the
// exchange plan against a written-out restatement of the loops sharded_hash.hip used to carry -- BOTH derivations of
// every offset that it held, the RCCL receive offsets and the peer-copy destination offsets.
#include <cstdio>
#include <random>
#include <vector>

#include "slab_plan.h"

using namespace nbh;

static int failures = 0;
#define EXPECT(cond, ...)              \
  do {                                 \
    if (!(cond)) {                     \
      if (failures++ < 40) {           \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

// rank r owns the layers z with r gz / W <= z < (r + 1) gz / W (integer division)
static void check_owner_formula() {
  for (int W = 1; W <= 32; W++)
    for (int gz = 1; gz <= 4096; gz++) {
      int covered = 0;
      for (int r = 0; r < W; r++)
        for (int z = (int)((long long)r * gz / W); z < (int)((long long)(r + 1) * gz / W); z++, covered++)
          if (slab_owner(z, gz, W) != r) EXPECT(false, "slab_owner(%d, %d, %d) = %d, the definition says %d", z, gz, W, slab_owner(z, gz, W), r);
      EXPECT(covered == gz, "W %d gz %d: the definition covers %d layers", W, gz, covered);
    }
}

static void check_map(const char* what, int W, const float* cuts, float lo_z, float cell, int gz) {
  SlabMap m;
  slab_map(m, W, cuts, lo_z, cell, gz);
  EXPECT((int)m.owner.size() == gz, "%s: %zu owners for %d layers", what, m.owner.size(), gz);
  for (int z = 0; z < gz; z++) {
    const int o = m.owner[(size_t)z];
    EXPECT(o >= 0 && o < W, "%s: layer %d has owner %d of %d", what, z, o, W);
    EXPECT(z == 0 || m.owner[(size_t)(z - 1)] <= o, "%s: the owners descend at layer %d", what, z);
    EXPECT(m.lo[o] <= z && z < m.hi[o], "%s: layer %d outside [%d, %d) of its owner %d", what, z, m.lo[o], m.hi[o], o);
    if (cuts) {  // the number of cuts at or below the layer's centre
      int want = 0;
      for (int k = 0; k + 1 < W; k++) want += cuts[k] <= fmaf((float)z + 0.5f, cell, lo_z) ? 1 : 0;
      EXPECT(o == want, "%s: layer %d has owner %d, %d cuts lie at or below its centre", what, z, o, want);
    }
  }
  int at = 0;  // [lo, hi) of the ranks tile [0, gz); a rank without layers has lo == hi
  for (int r = 0; r < W; r++) {
    EXPECT(m.lo[r] == at && m.hi[r] >= m.lo[r], "%s: rank %d owns [%d, %d), the ranks before it end at %d", what, r, m.lo[r], m.hi[r], at);
    at = m.hi[r];
  }
  EXPECT(at == gz, "%s: the slabs end at %d of %d layers", what, at, gz);
}

static void check_maps() {
  for (int W = 1; W <= 32; W++)
    for (int gz : {1, 2, 3, W - 1, W, W + 1, 2 * W, 2 * W + 1, 97, 4096})
      if (gz >= 1) check_map("equal layer counts", W, nullptr, -3.f, 0.5f, gz);
  const float ascending[7] = {-2.1f, -1.f, 0.25f, 0.5f, 2.f, 2.5f, 3.f};
  const float coincide[7] = {-1.f, -1.f, -1.f, 0.5f, 0.5f, 2.f, 2.f};
  const float outside[7] = {-50.f, -40.f, 0.f, 0.f, 30.f, 40.f, 50.f};  // cuts below and above the grid: ranks without layers
  for (int W : {1, 2, 3, 8})
    for (int gz : {1, 2, 5, 12, 40})
      for (const float* cuts : {ascending, coincide, outside}) {
        check_map("cuts", W, cuts, -3.f, 0.5f, gz);
        check_map("cuts", W, cuts, -3.001f, 1.0f, gz);
      }
}

static void expect_cuts(const char* what, int W, const std::vector<int>& hist, size_t n, std::vector<int> want_layers) {
  std::vector<float> cuts;
  const float lo_z = -2.f, cell = 0.5f;
  balanced_cuts(W, cell, hist.data(), (int)hist.size(), lo_z, n, cuts);
  EXPECT(cuts.size() == want_layers.size(), "%s: %zu cuts", what, cuts.size());
  for (size_t k = 0; k < cuts.size() && k < want_layers.size(); k++)
    EXPECT(cuts[k] == lo_z + (float)want_layers[k] * cell, "%s: cut %zu at %g, expected the lower edge of layer %d", what, k, cuts[k],
           want_layers[k]);
}

static void check_balanced_cuts() {
  expect_cuts("one rank", 1, {5, 5}, 10, {});
  // all 12 bodies in layer 2: the first cut (want 4: less than half of the layer) stays below it, the second (want 8: more
  // than half) goes above it
  expect_cuts("all bodies in one layer", 3, {0, 0, 12, 0}, 12, {2, 3});
  expect_cuts("equal layers", 4, {5, 5, 5, 5, 5, 5, 5, 5}, 40, {2, 4, 6});
  expect_cuts("equal layers, two ranks", 2, {7, 7, 7, 7}, 28, {2});
  expect_cuts("an empty grid", 3, {0, 0, 0, 0}, 0, {4, 4});  // nothing to balance: every cut runs to the top
  // want = 10 of {4, 10, 6}: layer 1 holds bodies 5..14; 6 of its 10 lie below the mark -> the cut goes above it
  expect_cuts("the crossing body late in its layer", 2, {4, 10, 6}, 20, {2});
  // want = 10 of {6, 10, 4}: 4 of its 10 lie below the mark -> the cut stays below it
  expect_cuts("the crossing body early in its layer", 2, {6, 10, 4}, 20, {1});
  expect_cuts("exactly half", 2, {5, 10, 5}, 20, {1});  // (want - run) 2 == hist: not more than half, the cut stays below
}

// two ranks, two layers, the current map gives rank 0 both layers' worth (100); the candidate's largest slab is `cand`
static void check_adoption() {
  SlabMap cur, cand;
  const float none[1] = {100.f}, mid[1] = {0.f};
  slab_map(cur, 2, none, -1.f, 1.f, 2);  // both layers to rank 0
  slab_map(cand, 2, mid, -1.f, 1.f, 2);  // one layer each
  for (int most : {94, 95, 96}) {
    const int hist[2] = {most, 100 - most};
    EXPECT(largest_slab(hist, 2, cur) == 100 && largest_slab(hist, 2, cand) == most, "largest slabs %lld, %lld",
           largest_slab(hist, 2, cur), largest_slab(hist, 2, cand));
    EXPECT(adopt_cuts(hist, 2, cur, cand) == (most < 95), "a candidate at %d %% of the largest slab", most);
  }
  const int zero[2] = {0, 0};
  EXPECT(!adopt_cuts(zero, 2, cur, cand), "an empty grid adopts nothing");
}

// ---- the exchange plan against the loops of the former hash_force_phase, written out -----------------------------
struct Seen {
  int cases = 0, no_bodies = 0, no_layers = 0, one_layer_both = 0, all_migrate = 0, none_migrate = 0, zero_at_boundary = 0, sparse = 0;
};

static void check_plan(int W, const std::vector<int>& M, const std::vector<int>& hist, long long layer_cells, const SlabMap& map,
                       Seen& seen) {
  const int gz = (int)hist.size();
  ExchangePlan p;
  exchange_plan(p, W, M.data(), hist.data(), gz, layer_cells, map);
  EXPECT((int)p.rank.size() == W, "%zu rank plans for %d ranks", p.rank.size(), W);
  seen.cases++;
  unsigned long long migrated = 0, halo_bodies = 0;
  bool all_dense = true, any_off = false, all_off = true;
  for (int r = 0; r < W; r++) {
    const RankPlan& a = p.rank[(size_t)r];
    // "5: migration", first loop
    size_t n_new = 0, n_leave = 0, n_arrive = 0, n_row = 0;
    for (int q = 0; q < W; q++) {
      n_new += (size_t)M[q * W + r];
      n_row += (size_t)M[r * W + q];
      if (q != r) { n_leave += (size_t)M[r * W + q]; n_arrive += (size_t)M[q * W + r]; }
    }
    migrated += n_leave;
    any_off = any_off || n_leave;
    all_off = all_off && M[r * W + r] == 0;
    if (n_new == 0) seen.no_bodies++;
    EXPECT(a.n_new == n_new && a.n_leave == n_leave && a.n_arrive == n_arrive, "W %d rank %d: counts %zu %zu %zu, the loops say %zu %zu %zu",
           W, r, a.n_new, a.n_leave, a.n_arrive, n_new, n_leave, n_arrive);
    EXPECT(a.n_new == n_row - a.n_leave + a.n_arrive, "W %d rank %d: n_new %zu is not n - n_leave + n_arrive", W, r, a.n_new);
    // the sends: rows grouped by new owner, ascending, own rank absent; destination offset as the peer copies derived it
    size_t soff = 0, k = 0;
    for (int q = 0; q < W; q++) {
      if (q == r) continue;
      const size_t cnt = (size_t)M[r * W + q];
      if (cnt) {
        size_t doff = 0;  // arrivals are ordered by source rank
        for (int s = 0; s < r; s++)
          if (s != q) doff += (size_t)M[s * W + q];
        const bool have = k < a.sends.size();
        EXPECT(have && a.sends[k].peer == q && a.sends[k].rows_off == soff && a.sends[k].got_off == doff && a.sends[k].count == cnt,
               "W %d rank %d: send %zu to %d is not {rows %zu, got %zu, count %zu}", W, r, k, q, soff, doff, cnt);
        if (have) {  // exactly one matching arrival at the peer, with the same count
          int matches = 0;
          for (const RowTransfer& t : p.rank[(size_t)q].arrivals)
            matches += t.peer == r && t.count == cnt && t.got_off == a.sends[k].got_off && t.rows_off == soff ? 1 : 0;
          EXPECT(matches == 1, "W %d: the send %d -> %d has %d matching arrivals", W, r, q, matches);
        }
        k++;
      }
      soff += cnt;
    }
    EXPECT(k == a.sends.size() && soff == a.n_leave, "W %d rank %d: %zu sends tile %zu of %zu rows", W, r, a.sends.size(), soff, a.n_leave);
    // the arrivals: receive offsets as the RCCL form derived them; they tile [0, n_arrive) in source order
    size_t doff = 0;
    k = 0;
    for (int s = 0; s < W; s++) {
      if (s == r) continue;
      const size_t cnt = (size_t)M[s * W + r];
      if (cnt) {
        EXPECT(k < a.arrivals.size() && a.arrivals[k].peer == s && a.arrivals[k].got_off == doff && a.arrivals[k].count == cnt,
               "W %d rank %d: arrival %zu from %d is not {got %zu, count %zu}", W, r, k, s, doff, cnt);
        k++;
      }
      doff += cnt;
    }
    EXPECT(k == a.arrivals.size() && doff == a.n_arrive, "W %d rank %d: %zu arrivals tile %zu of %zu rows", W, r, a.arrivals.size(), doff,
           a.n_arrive);
    // "6, 7": the halo plan
    int z_lo = map.lo[r], z_hi = map.hi[r], lower = -1, upper = -1;
    size_t n_head = 0, n_tail = 0, in_lower = 0, in_upper = 0;
    if (W > 1 && z_hi > z_lo) {
      if (z_lo > 0) {
        lower = map.owner[(size_t)(z_lo - 1)];
        n_head = (size_t)hist[z_lo];
        in_lower = (size_t)hist[z_lo - 1];
        if (!hist[z_lo] || !hist[z_lo - 1]) seen.zero_at_boundary++;
      }
      if (z_hi < gz) {
        upper = map.owner[(size_t)z_hi];
        n_tail = (size_t)hist[z_hi - 1];
        in_upper = (size_t)hist[z_hi];
      }
      if (z_hi == z_lo + 1 && lower >= 0 && upper >= 0 && n_head) seen.one_layer_both++;
    }
    if (z_hi == z_lo) seen.no_layers++;
    halo_bodies += in_lower + in_upper;
    EXPECT(a.z_lo == z_lo && a.z_hi == z_hi && a.lower == lower && a.upper == upper, "W %d rank %d: slab [%d, %d) between %d and %d", W, r,
           a.z_lo, a.z_hi, a.lower, a.upper);
    EXPECT(a.n_head == n_head && a.n_tail == n_tail && a.in_lower == in_lower && a.in_upper == in_upper,
           "W %d rank %d: halo counts %zu %zu %zu %zu, the loops say %zu %zu %zu %zu", W, r, a.n_head, a.n_tail, a.in_lower, a.in_upper, n_head,
           n_tail, in_lower, in_upper);
    if (lower >= 0) EXPECT(n_head == p.rank[(size_t)lower].in_upper, "W %d rank %d: n_head is not the in_upper of rank %d", W, r, lower);
    if (upper >= 0) EXPECT(n_tail == p.rank[(size_t)upper].in_lower, "W %d rank %d: n_tail is not the in_lower of rank %d", W, r, upper);
    // the layers that leave: RCCL sent the head then the tail; the peer copies wrote the head BEHIND the receiver's lower
    // halo (hist[dz_lo - 1] bodies) into start-array slot 1, the tail to the front into slot 0
    int n_out = 0;
    if (n_head) {
      const int dz_lo = map.lo[lower];
      const size_t d_in_lower = dz_lo > 0 ? (size_t)hist[dz_lo - 1] : 0;
      const LayerTransfer& t = a.out[n_out++];
      EXPECT(a.n_out >= n_out && t.peer == lower && t.out_off == 0 && t.count == n_head && t.in_off == d_in_lower && t.out_slot == 0 &&
                 t.in_slot == 1 && t.in_off == p.rank[(size_t)lower].in_lower,
             "W %d rank %d: the head goes to %d at %zu, slot %d", W, r, t.peer, t.in_off, t.in_slot);
    }
    if (n_tail) {
      const LayerTransfer& t = a.out[n_out++];
      EXPECT(a.n_out >= n_out && t.peer == upper && t.out_off == n_head && t.count == n_tail && t.in_off == 0 && t.out_slot == 1 &&
                 t.in_slot == 0,
             "W %d rank %d: the tail goes to %d at %zu, slot %d", W, r, t.peer, t.in_off, t.in_slot);
    }
    EXPECT(a.n_out == n_out, "W %d rank %d: %d layers leave, the loops say %d", W, r, a.n_out, n_out);
    // the layers that arrive, as RCCL received them: from below at 0 into slot 0, from above at in_lower into slot 1
    int n_in = 0;
    if (in_lower) {
      const LayerTransfer& t = a.in[n_in++];
      EXPECT(a.n_in >= n_in && t.peer == lower && t.in_off == 0 && t.count == in_lower && t.in_slot == 0 && t.out_slot == 1 &&
                 t.out_off == p.rank[(size_t)lower].n_head,
             "W %d rank %d: the lower halo comes from %d to %zu, slot %d", W, r, t.peer, t.in_off, t.in_slot);
    }
    if (in_upper) {
      const LayerTransfer& t = a.in[n_in++];
      EXPECT(a.n_in >= n_in && t.peer == upper && t.in_off == in_lower && t.count == in_upper && t.in_slot == 1 && t.out_slot == 0 &&
                 t.out_off == 0,
             "W %d rank %d: the upper halo comes from %d to %zu, slot %d", W, r, t.peer, t.in_off, t.in_slot);
    }
    EXPECT(a.n_in == n_in, "W %d rank %d: %d layers arrive, the loops say %d", W, r, a.n_in, n_in);
    // the form of the force phase
    long long n_r = 0;
    for (int q = 0; q < W; q++) n_r += M[q * W + r];
    if (n_r > 0 && (long long)(map.hi[r] - map.lo[r]) * layer_cells > 4LL * n_r + 4096) all_dense = false;
  }
  EXPECT(p.all_dense == all_dense, "W %d: all_dense %d, the loops say %d", W, (int)p.all_dense, (int)all_dense);
  EXPECT(p.migrated == migrated && p.halo_bodies == halo_bodies, "W %d: totals %llu %llu, the loops say %llu %llu", W, p.migrated,
         p.halo_bodies, migrated, halo_bodies);
  if (!all_dense) seen.sparse++;
  if (W > 1 && !any_off) seen.none_migrate++;
  if (W > 1 && all_off && any_off) seen.all_migrate++;
}

static void check_plans() {
  std::mt19937 gen(20240611u);
  auto below = [&](int n) { return (int)(gen() % (unsigned)n); };
  Seen seen;
  for (int W : {1, 2, 3, 4, 5, 6, 7, 8, 16, 32})
    for (int c = 0; c < 64; c++) {
      const int shape = c % 8;
      // grid: fewer layers than ranks (shape 3), one layer per rank (4), else up to a few layers per rank
      const int gz = shape == 3 ? 1 + below(W) : shape == 4 ? W : 1 + below(5 * W);
      std::vector<int> hist((size_t)gz);
      for (int& h : hist) h = below(4) == 0 || shape == 6 ? (below(2) ? 0 : below(50)) : 1 + below(1000);
      // map: equal layer counts, or cuts (shape 7: coinciding ones)
      const float lo_z = -4.f, cell = 0.5f;
      std::vector<float> cuts((size_t)(W - 1));
      float at = lo_z;
      for (float& v : cuts) v = at = at + (shape == 7 && below(2) ? 0.f : 0.25f * (float)below(2 * 5 + 1));
      SlabMap map;
      slab_map(map, W, c % 2 && W > 1 ? cuts.data() : nullptr, lo_z, cell, gz);
      // send matrix: nobody migrates (1), everybody does (2), ranks without bodies (5)
      std::vector<int> M((size_t)W * W);
      const int idle = below(W);
      for (int s = 0; s < W; s++)
        for (int d = 0; d < W; d++) {
          int v = below(3) == 0 ? 0 : below(s == d ? 100000 : 300);
          if (shape == 1 && s != d) v = 0;
          if (shape == 2 && s == d) v = 0;
          if (shape == 2 && s != d) v += 1;
          if (shape == 5 && (s == idle || d == idle || s == W - 1 || d == W - 1)) v = 0;
          M[(size_t)(s * W + d)] = v;
        }
      check_plan(W, M, hist, c % 4 == 3 ? 1000000 : 1 + below(400), map, seen);
    }
  EXPECT(seen.cases == 640, "%d cases", seen.cases);
  EXPECT(seen.no_bodies > 0 && seen.no_layers > 0 && seen.one_layer_both > 0 && seen.all_migrate > 0 && seen.none_migrate > 0 &&
             seen.zero_at_boundary > 0 && seen.sparse > 0,
         "edge shapes seen: ranks without bodies %d, without layers %d, one-layer slabs between two neighbours %d, everybody migrating %d, "
         "nobody %d, empty layers at a slab boundary %d, sparse grids %d",
         seen.no_bodies, seen.no_layers, seen.one_layer_both, seen.all_migrate, seen.none_migrate, seen.zero_at_boundary, seen.sparse);
}

int main() {
  check_owner_formula();
  check_maps();
  check_balanced_cuts();
  check_adoption();
  check_plans();
  if (failures) {
    std::printf("slab_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("slab_plan_check: ok\n");
  return 0;
}
