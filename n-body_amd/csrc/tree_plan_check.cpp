// tree_plan_check.cpp -- the host decisions of the Barnes-Hut tree (tree_plan.h) on a CPU, under AddressSanitizer and
// UBSan (make tree_plan_check): the walk plan against a written-out restatement of the if-chain tree_walk used to
// carry, the size table and the two node bounds against the expressions they replace, the invariants that tie a
// build's and a walk's decisions to the arrays sized at create time, the array replacement with an allocator that
// fails at every position, and the compaction and decode of a hand-made tree against values worked out by hand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tree_plan.h"

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

// the body counts at which a decision changes
static std::vector<int> body_counts() {
  std::vector<int> c = {1, 63, 64, 65, kPairFrom - 1, kPairFrom, kPairFrom + 1, 131071, 131072, kPrefixMax, kPrefixMax + 1,
                        0x07ffffff};
  for (int K = 1; K <= kMaxReplicas; K *= 2)
    for (int d = -1; d <= 1; d++) {
      c.push_back(kSplitAuto / (2 * K) + d);
      c.push_back(kSplitBudget / (2 * K) + d);
    }
  return c;
}

// ---------------------------------------------------------------------------------------
// what tree_walk did, statement by statement, before the plan existed: which kernel, on which grid, with which
// arguments, and what it left in the handle
// ---------------------------------------------------------------------------------------
struct Did {
  int kernel = 0;  // 0 nothing, 1 plain, 2 counting, 3 replicas + combine, 4 pair, -1 the pair-on-plain-ids error
  bool quad = false, waited = false, ordered = false, planned = false;
  int K = 1, unit_max = 1, grid_x = 0, grid_y = 1, plan_waves = 0, plan_cap = 0;
  int cost_first, cost_n;
  bool plan_pending;
};

static Did restated_walk(int first, int count, const WalkState& g) {
  Did d;
  d.cost_first = g.cost_first; d.cost_n = g.cost_n; d.plan_pending = g.plan_pending;
  const int n = count;
  const int blocks = (n + 256 - 1) / 256;
  const bool visits = g.count_visits;
  if (g.plan_pending && !g.capturing) d.waited = true;
  if (n == 0) return d;
  int K = 1;
  while (K < 16 && (size_t)(2 * K) * (size_t)n <= (size_t)327680) K *= 2;
  if (n >= 98304) K = 1;
  if (g.tune_replicas > 0) {
    K = 1;
    while (K < g.tune_replicas && K < 16 && (size_t)(2 * K) * (size_t)n <= (size_t)2097152) K *= 2;
  }
  const size_t units = g.tune_split_level > 0 ? (size_t)g.tune_split_level * (size_t)K : 96;
  int unit_max = (int)(g.built_count / units);
  if (unit_max < 1) unit_max = 1;
  d.K = K; d.unit_max = unit_max;
  if (g.built_order == 2) {
    d.quad = true;
    if (K == 1 && visits) { d.kernel = 2; d.grid_x = blocks; }
    else if (K == 1) { d.kernel = 1; d.grid_x = blocks; }
    else { d.kernel = 3; d.grid_x = blocks; d.grid_y = K; }
    return d;
  }
  int form = g.tune_form > 0 ? g.tune_form : 2;
  if (!g.aligned) {
    if (g.tune_form == 2) { d.kernel = -1; return d; }
    form = 1;
  }
  if (K == 1 && visits && g.tune_form != 2) form = 1;
  if (K == 1 && visits && form == 1) {
    d.kernel = 2; d.grid_x = blocks;
  } else if (K == 1 && form == 2) {
    const int waves = (n + 63) / 64;
    int grid = waves;
    if (g.tune_schedule && g.cost_first == first && g.cost_n == n && waves >= 2048) {
      const int cap = waves / 8 + waves / 32 + 8;
      if (g.plan_pending && first == 0 && g.plan_n == n && g.plan_cap == cap && !g.capturing) {
      } else {
        d.planned = true; d.plan_waves = waves; d.plan_cap = cap;
      }
      d.ordered = true;
      grid = 8 * cap;
    }
    d.plan_pending = false;
    d.kernel = 4; d.grid_x = grid;
    d.cost_first = first;
    d.cost_n = n;
  } else if (K == 1) {
    d.kernel = 1; d.grid_x = blocks;
  } else {
    d.kernel = 3; d.grid_x = blocks; d.grid_y = K;
  }
  return d;
}

static Did plan_as_did(const WalkPlan& p) {
  Did d;
  d.quad = p.quad; d.waited = p.wait_plan; d.K = p.K; d.unit_max = p.unit_max;
  d.cost_first = p.cost_first; d.cost_n = p.cost_n; d.plan_pending = p.plan_pending;
  if (p.pair_on_plain_ids) { d.kernel = -1; return d; }
  switch (p.form) {
    case WalkForm::None: d.quad = false; break;
    case WalkForm::Plain: d.kernel = 1; d.grid_x = p.blocks; break;
    case WalkForm::Count: d.kernel = 2; d.grid_x = p.blocks; break;
    case WalkForm::Split: d.kernel = 3; d.grid_x = p.blocks; d.grid_y = p.K; break;
    case WalkForm::Pair:
      d.kernel = 4; d.grid_x = p.grid; d.ordered = p.scheduled; d.planned = p.scheduled && p.plan_now;
      if (d.planned) { d.plan_waves = p.waves; d.plan_cap = p.cap; }
      break;
  }
  return d;
}

static long check_walk_plan(size_t* max_order_slots) {
  long cases = 0;
  for (int built : body_counts()) {
    const int ranges[4][2] = {{0, built}, {built / 2, built - built / 2}, {built > 1 ? 1 : 0, 0}, {built / 3 + 1 < built ? built / 3 + 1 : 0, built / 2}};
    for (const auto& r : ranges) {
      const int first = r[0], n = r[1];
      if (first + n > built) continue;
      const int cap = (int)schedule_cap((size_t)((n + 63) / 64));
      for (int replicas = 0; replicas <= 16; replicas++)
      for (int split : {0, 1, 1024})
      for (int form = 0; form <= 2; form++)
      for (int schedule = 0; schedule <= 1; schedule++)
      for (int order = 1; order <= 2; order++)
      for (int flags = 0; flags < 8; flags++)
      for (int pending = 0; pending < 4; pending++)  // none; queued for this walk; for another count; with another cap
      for (int cost = 0; cost < 4; cost++) {         // none; of this range; of the full range; of another count
        WalkState s{};
        s.built_count = (size_t)built; s.built_order = order;
        s.aligned = flags & 1; s.count_visits = flags & 2; s.capturing = flags & 4;
        s.tune_replicas = replicas; s.tune_split_level = split; s.tune_form = form; s.tune_schedule = schedule;
        s.cost_first = cost == 0 ? -1 : cost == 2 ? 0 : first;
        s.cost_n = cost == 0 ? -1 : cost == 2 ? built : cost == 3 ? n - 1 : n;
        s.plan_pending = pending != 0;
        s.plan_n = pending == 2 ? n + 1 : n;
        s.plan_cap = pending == 3 ? cap + 1 : cap;
        const WalkPlan p = walk_plan(first, n, 0.0f, s);
        const Did a = plan_as_did(p), b = restated_walk(first, n, s);
        cases++;
        const bool same = a.kernel == b.kernel && a.quad == (b.kernel > 0 && b.quad) && a.waited == b.waited &&
                          a.ordered == b.ordered && a.planned == b.planned && (a.kernel <= 0 || (a.K == b.K && a.unit_max == b.unit_max)) &&
                          a.grid_x == b.grid_x && a.grid_y == b.grid_y && a.plan_waves == b.plan_waves &&
                          a.plan_cap == b.plan_cap && a.cost_first == b.cost_first && a.cost_n == b.cost_n &&
                          a.plan_pending == b.plan_pending;
        EXPECT(same, "built %d walk [%d, +%d) replicas %d split %d form %d schedule %d order %d flags %d pending %d cost %d: "
               "plan kernel %d grid %d x %d K %d unit %d, restatement kernel %d grid %d x %d K %d unit %d",
               built, first, n, replicas, split, form, schedule, order, flags, pending, cost, a.kernel, a.grid_x, a.grid_y,
               a.K, a.unit_max, b.kernel, b.grid_x, b.grid_y, b.K, b.unit_max);
        // what nothing checked: the replicas' partial sums fit their buffer, the schedule fits the arrays of a tree
        // created for at least `built` bodies
        if (p.form == WalkForm::Split) EXPECT((size_t)p.K * (size_t)n <= (size_t)kSplitBudget, "K %d x n %d", p.K, n);
        EXPECT(p.K >= 1 && p.K <= kMaxReplicas && (p.K & (p.K - 1)) == 0, "K %d", p.K);
        if (p.form == WalkForm::Pair) {
          const TreeSizes z = tree_sizes((size_t)built, 20, 1, 0);
          EXPECT((size_t)p.waves <= z.cost, "%d waves, %zu costs", p.waves, z.cost);
          if (p.scheduled) EXPECT((size_t)p.grid <= z.order && p.grid == 8 * p.cap, "grid %d, %zu slots", p.grid, z.order);
          if ((size_t)p.grid > *max_order_slots) *max_order_slots = (size_t)p.grid;
        }
      }
    }
  }
  // the guard rule, once: eps^2 below 1e-12 cannot keep rsq of a zero distance finite
  EXPECT(walk_guard(0.0f) && walk_guard(9.9e-13f) && !walk_guard(1e-12f) && !walk_guard(1e-6f), "guard rule");
  EXPECT(walk_plan(0, 100, 0.0f, WalkState{}).guard && !walk_plan(0, 100, 1e-6f, WalkState{}).guard, "guard in the plan");
  // the build queues a schedule exactly when the next full-range walk would use one
  for (int n : body_counts())
    for (int schedule = 0; schedule <= 1; schedule++)
      for (int cost = 0; cost < 3; cost++) {
        const int cf = cost == 0 ? -1 : 0, cn = cost == 1 ? n : cost == 2 ? n - 1 : -1;
        const bool want = schedule && cf == 0 && cn == n && (n + 63) / 64 >= 2048;
        EXPECT(walk_scheduled(schedule, cf, cn, 0, n) == want, "n %d schedule %d cost %d", n, schedule, cost);
      }
  return cases;
}

// ---------------------------------------------------------------------------------------
// the size table against the expressions of create / tree_alloc_nodes / set_params, and every build against the table
// ---------------------------------------------------------------------------------------
static long check_sizes() {
  long cases = 0;
  const std::vector<int> counts = body_counts();
  for (int maxp : counts)
    for (int depth : {1, 4, 10, 11, 20, 21})
      for (int leaf : {1, 8, 1024})
        for (int limit : {0, 16, 100000}) {
          const size_t n = (size_t)maxp;
          const TreeSizes s = tree_sizes(n, depth, leaf, limit);
          size_t cap = n + 2 * (size_t)(depth + 1) * (n / (size_t)(leaf + 1) + 1) + 16;
          if (cap > 0x0fffffffu) cap = 0x0fffffffu;
          if (limit > 0 && (size_t)limit < cap) cap = (size_t)limit;
          const size_t rank_G = (n + 64) / 64, nrank = 2 * (size_t)(depth + 1) * rank_G;
          const size_t waves = n / 64 + 1, ocap = waves / 8 + waves / 32 + 8;
          const size_t pcap = (n < 1572864 ? n : (size_t)1572864) + 8;
          EXPECT(s.capacity == cap && s.capacity <= 0x0fffffffu && s.capacity >= 16, "capacity %zu", s.capacity);
          EXPECT(s.wide == (depth > 10) && s.key_bytes == n * (depth > 10 ? 8 : 4), "keys");
          EXPECT((size_t)s.rank_G == rank_G && s.plane == nrank + nrank / 2 && s.rank_off == nrank, "ranks");
          EXPECT(s.rec == cap + 8 && s.pair_words == (cap / 2 + 8) * 12, "records");
          EXPECT(s.quad64 == cap * 10 && s.quad == 2 * cap + 16, "moments");
          EXPECT(s.bodies == n && s.partial == (size_t)3 * 2097152, "bodies");
          EXPECT(s.prefix_cap == pcap && s.prefix == pcap + 2 * (1572864 / 1024 + 2), "prefix");
          EXPECT(s.cost == waves && s.order == 8 * ocap && s.bounds == 16, "schedule");
          // the bound set_params refuses by: nodes, without the padding ids -- and only for the deep trees
          const bool refused = depth > 10 && n + (size_t)(depth + 1) * (n / (size_t)(leaf + 1) + 1) + 16 > 0x0fffffffu;
          EXPECT(tree_params_fit(n, depth, leaf) == !refused, "set_params bound: %d bodies depth %d leaf %d", maxp, depth, leaf);
          EXPECT(tree_id_bound(n, depth, leaf) >= tree_node_bound(n, depth, leaf), "the id bound is the wider one");
          for (int ni : counts) {
            if (ni > maxp) continue;
            for (int form = 0; form <= 2; form++)
              for (int order = 1; order <= 2; order++) {
                const BuildLayout b = build_layout(ni, depth, form, order, s.prefix_cap);
                cases++;
                EXPECT(b.G == (ni + 64) / 64 && b.tbl == (size_t)(depth + 1) * (size_t)b.G && b.levels == depth + 1, "ranks of %d", ni);
                EXPECT(b.odd_plane == b.tbl && b.cum_plane == 2 * b.tbl && b.odd_off == b.tbl, "regions of %d", ni);
                EXPECT(3 * b.tbl <= s.plane && 2 * b.tbl <= s.rank_off, "%d of %d bodies: planes", ni, maxp);
                EXPECT(b.aligned == (ni >= 98304 || (form == 2 && order == 1)), "aligned");
                EXPECT(b.clear_words == (b.aligned ? 2 * b.tbl : 0) && b.clear_words * 4 <= 2 * b.tbl * 8, "cleared words");
                EXPECT(b.fused == (ni <= 1572864), "fused");
                EXPECT(b.pblocks == ni / 1024 + 1 && b.btot == s.prefix_cap && b.boff == b.btot + 1572864 / 1024 + 2, "prefix blocks");
                if (b.fused) {
                  EXPECT((size_t)ni + 1 <= s.prefix_cap, "%d + 1 prefix entries of %zu", ni, s.prefix_cap);
                  EXPECT((size_t)b.pblocks <= s.prefix_blocks && b.boff + (size_t)b.pblocks <= s.prefix, "%d block totals", b.pblocks);
                }
                EXPECT(b.wide == (depth > 10) && b.key_bits == (b.wide ? 63 : 30) && b.first_bit == (b.wide ? 63 - 3 * depth : 0), "key bits");
                EXPECT(b.first_bit >= 0 && b.key_bits - b.first_bit == 3 * (b.wide ? depth : 10), "bits that shape the tree");
                EXPECT(b.top == (depth < 4 ? depth : 4) && b.blocks == (ni + 255) / 256, "levels");
                const size_t want = (2 * (size_t)ni + 255) / 256;
                EXPECT(b.monopole_grid == (want < 1 ? 1 : want > 16384 ? 16384 : want), "monopole grid");
              }
          }
        }
  return cases;
}

// ---------------------------------------------------------------------------------------
// replace_arrays with malloc and a stub that fails at the k-th allocation (or the k-th clear), for every k
// ---------------------------------------------------------------------------------------
static int fail_at = -1, calls = 0, live = 0;
static int stub_alloc(void** p, size_t bytes) {
  if (calls++ == fail_at) return 2;  // (what an out-of-memory allocation returns: an error code, *p untouched)
  *p = std::malloc(bytes);
  std::memset(*p, 0xa5, bytes);
  live++;
  return 0;
}
static void stub_free(void* p) { std::free(p); live--; }
static int stub_zero(void* p, size_t bytes) {
  if (calls++ == fail_at) return 3;
  std::memset(p, 0, bytes);
  return 0;
}

static void check_replace() {
  int *a = nullptr, *b = nullptr;
  double* c = nullptr;
  void* d = nullptr;
  NodeRec* e = nullptr;
  int capacity = 0;
  const auto table = [&](ArraySlot* s, size_t n) {
    s[0] = array_slot(&a, n);
    s[1] = array_slot(&b, n, true);
    s[2] = array_slot(&c, 3 * n);
    s[3] = ArraySlot{&d, 0, false};  // (an empty scratch array still gets an allocation)
    s[4] = array_slot(&e, n + 8, true);
    return 5;
  };
  ArraySlot s[8];
  const int steps = 5 + 2;  // five allocations, two clears
  for (int round = 0; round < 2; round++)  // from nothing, then over a live set (which must be freed first, once)
    for (int k = 0; k <= steps; k++) {
      if (round == 1) {
        fail_at = -1;
        EXPECT(replace_arrays(s, table(s, 10), &capacity, 10, stub_alloc, stub_free, stub_zero) == 0 && capacity == 10, "set-up");
      }
      fail_at = k; calls = 0;
      const int rc = replace_arrays(s, table(s, 100), &capacity, 100, stub_alloc, stub_free, stub_zero);
      if (k < steps) {
        EXPECT(rc != 0, "step %d fails, the routine returned 0", k);
        EXPECT(!a && !b && !c && !d && !e && capacity == 0 && live == 0, "after a failure at step %d: %p %p %p %p %p capacity %d live %d",
               k, (void*)a, (void*)b, (void*)c, d, (void*)e, capacity, live);
      } else {
        EXPECT(rc == 0 && a && b && c && d && e && capacity == 100 && live == 5, "success: rc %d capacity %d live %d", rc, capacity, live);
        bool cleared = true, untouched = true;
        for (int i = 0; i < 100; i++) cleared = cleared && b[i] == 0 && e[i].child == 0u;
        for (int i = 0; i < 100; i++) untouched = untouched && a[i] == (int)0xa5a5a5a5;
        EXPECT(cleared && untouched, "only the arrays marked so are cleared");
        a[99] = 1; c[299] = 1.0; e[107].count = 1;  // (the full extents are there: ASan checks)
        release_arrays(s, table(s, 0), &capacity, stub_free);
        EXPECT(!a && !b && !c && !d && !e && capacity == 0 && live == 0, "after the release");
        release_arrays(s, table(s, 0), &capacity, stub_free);  // (a second release frees nothing)
        EXPECT(live == 0, "released twice");
      }
    }
  fail_at = -1;
}

// ---------------------------------------------------------------------------------------
// a three-level tree of five bodies, by hand.  ids: 0 root | 1 padding hole, 2 3 4 the root's children (octants 0, 5, 6)
// | 5 padding hole, 6 7 the children of node 2 (octants 0, 7), 8 the first child node 4 would have had: node 4 holds
// two bodies and was CUT at the capacity -- it is a leaf of two bodies, its children do not exist.
// Root cube lo = (-1, -2, -4), half 4.
// ---------------------------------------------------------------------------------------
static void check_decode(bool wide) {
  const int max_depth = wide ? 11 : 2;  // (63-bit keys come with the deep trees; levels 3 .. 11 are empty)
  const int top = wide ? 60 : 27;       // bit of the first octant digit
  const auto key = [&](unsigned long long d1, unsigned long long d2) { return d1 << top | d2 << (top - 3); };
  const unsigned long long keys[5] = {key(0, 0), key(0, 7), key(5, 3), key(6, 1), key(6, 2)};
  const int idx[5] = {4, 2, 0, 3, 1};
  const int first_of[9] = {0, -1, 0, 2, 3, -1, 0, 1, -1};
  int id_base[kMaxDepth + 3];
  for (int k = 0; k < kMaxDepth + 3; k++) id_base[k] = k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 5 : 9;
  int compact[9];
  EXPECT(compact_ids(first_of, 9, compact) == 6 && compact_ids(first_of, 9, nullptr) == 6, "six nodes");
  EXPECT(compact_ids(first_of, 5, nullptr) == 4 && compact_ids(first_of, 0, nullptr) == 0, "a prefix of the ids");
  const int want_compact[9] = {0, -1, 1, 2, 3, -1, 4, 5, -1};
  for (int k = 0; k < 9; k++) EXPECT(compact[k] == want_compact[k], "id %d -> %d", k, compact[k]);
  NodeRec rec[9] = {};
  const auto node = [&](int id, float x, float y, float z, float m, int first, int count, unsigned child) {
    rec[id].cx = x; rec[id].cy = y; rec[id].cz = z; rec[id].mass = m; rec[id].first = first; rec[id].count = count; rec[id].child = child;
  };
  node(0, 0.5f, 0.25f, 0.125f, 5.f, 0, 5, 2u | 3u << 28);
  node(2, 1.f, 1.5f, 2.f, 2.f, 0, 2, 6u | 2u << 28);
  node(3, 3.f, 3.5f, 4.f, 1.f, 2, 1, 0u);
  node(4, 5.f, 5.5f, 6.f, 2.f, 3, 2, 0u);
  node(6, 7.f, 7.5f, 8.f, 1.f, 0, 1, 0u);
  node(7, 9.f, 9.5f, 10.f, 1.f, 1, 1, 0u);
  TreeRoot root{};
  root.lo[0] = -1.f; root.lo[1] = -2.f; root.lo[2] = -4.f; root.half = 4.f;
  RefOctreeNode out[7];
  std::memset(out, 0x5a, sizeof(out));
  decode_nodes(rec, keys, idx, root, id_base, max_depth, compact, 9, out);
  struct Want { float c[3], h, com[3], m; int child[8], particle; bool leaf; int count; };
  const Want want[6] = {
      {{3.f, 2.f, 0.f}, 4.f, {0.5f, 0.25f, 0.125f}, 5.f, {1, -1, -1, -1, -1, 2, 3, -1}, -1, false, 5},
      {{1.f, 0.f, -2.f}, 2.f, {1.f, 1.5f, 2.f}, 2.f, {4, -1, -1, -1, -1, -1, -1, 5}, -1, false, 2},
      {{5.f, 0.f, 2.f}, 2.f, {3.f, 3.5f, 4.f}, 1.f, {-1, -1, -1, -1, -1, -1, -1, -1}, 0, true, 1},
      {{5.f, 4.f, -2.f}, 2.f, {5.f, 5.5f, 6.f}, 2.f, {-1, -1, -1, -1, -1, -1, -1, -1}, 3, true, 2},
      {{0.f, -1.f, -3.f}, 1.f, {7.f, 7.5f, 8.f}, 1.f, {-1, -1, -1, -1, -1, -1, -1, -1}, 4, true, 1},
      {{2.f, 1.f, -1.f}, 1.f, {9.f, 9.5f, 10.f}, 1.f, {-1, -1, -1, -1, -1, -1, -1, -1}, 2, true, 1},
  };
  for (int k = 0; k < 6; k++) {
    const RefOctreeNode& o = out[k];
    const Want& w = want[k];
    EXPECT(o.center[0] == w.c[0] && o.center[1] == w.c[1] && o.center[2] == w.c[2] && o.half_size == w.h,
           "%s node %d: centre %g %g %g half %g", wide ? "63-bit" : "30-bit", k, o.center[0], o.center[1], o.center[2], o.half_size);
    EXPECT(o.com[0] == w.com[0] && o.com[1] == w.com[1] && o.com[2] == w.com[2] && o.total_mass == w.m, "node %d: monopole", k);
    for (int c = 0; c < 8; c++) EXPECT(o.children[c] == w.child[c], "%s node %d: child %d is %d", wide ? "63-bit" : "30-bit", k, c, o.children[c]);
    EXPECT(o.particle_index == w.particle && o.is_leaf == w.leaf && o.particle_count == w.count, "node %d: particle %d leaf %d count %d",
           k, o.particle_index, (int)o.is_leaf, o.particle_count);
  }
  unsigned char untouched[sizeof(RefOctreeNode)];
  std::memset(untouched, 0x5a, sizeof(untouched));
  EXPECT(std::memcmp(&out[6], untouched, sizeof(untouched)) == 0, "six nodes are written, no seventh");
}

int main() {
  size_t max_order = 0;
  const long walks = check_walk_plan(&max_order);
  const long builds = check_sizes();
  check_replace();
  check_decode(false);
  check_decode(true);
  // the node capacity never exceeds 28 bits, whatever is asked
  EXPECT(tree_sizes(0x07ffffff, 21, 1, 0).capacity == 0x0fffffffu && tree_sizes(0x07ffffff, 21, 1, 0x7fffffff).capacity == 0x0fffffffu,
         "the 2^28 clamp");
  EXPECT(!tree_params_fit(0x07ffffff, 21, 1) && tree_params_fit(0x07ffffff, 10, 1) && tree_params_fit(1u << 20, 21, 1), "set_params bound");
  if (failures) {
    std::printf("tree_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("tree_plan_check: ok (%ld walk plans, %ld build layouts, largest schedule %zu slots)\n", walks, builds, max_order);
  return 0;
}
