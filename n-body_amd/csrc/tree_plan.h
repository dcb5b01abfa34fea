// tree_plan.h -- the host decisions of the Barnes-Hut tree (barnes_hut.hip) as plain arithmetic: the size of every
// array of a tree, the layout of one build, the plan of one walk, and the decode of the built tree into the
// reference's node layout (the routine that replaces a set of device arrays: device_arrays.h).  Plain C++17, no HIP include: tree_plan_check.cpp runs
// all of it on a CPU under AddressSanitizer and UBSan (make tree_plan_check).
//
// barnes_hut.hip derives each of these ONCE per create / build / walk and issues allocations and launches from the
// result; nothing here launches, allocates by itself or reads device memory.
#pragma once

#include <cmath>
#include <cstddef>

#include "device_arrays.h"  // ArraySlot, replace_arrays, release_arrays

namespace nbh {

constexpr int kMaxDepth = 21;      // 63-bit Morton keys (the reference caps its insertion at depth 20, :363)
constexpr int kDepth32 = 10;       // up to here 30-bit keys in 32-bit words (the faster sort)
constexpr int kSplitBudget = 2097152;  // capacity of the partial-sum buffer: replicas * n
constexpr int kSplitAuto = 327680;     // automatic choice: replicas * n up to here (= 5120 waves; tools/bh_k_small.py)
constexpr int kMaxReplicas = 16;
constexpr int kPairFrom = 98304;       // bodies from which the walk runs without replicas (tools/bh_split_vs_pair.py)

struct TreeRoot {
  float lo[3];
  float half;
  float scale;  // 1024 / (2 half)
  int pad[3];
};

// 32-byte traversal record: one s_load_dwordx8 per node, eight siblings = 256 contiguous bytes
struct __attribute__((aligned(32))) NodeRec {
  float cx, cy, cz, mass;  // centre of mass, mass
  float size2;             // (2 half)^2
  int first, count;        // range of the Morton-sorted body list
  unsigned int child;      // first child id | child count << 28 ; 0 = leaf
};

constexpr int kPairWords = 12;
#ifndef NBH_BH_PREFIX_MAX
#define NBH_BH_PREFIX_MAX 1572864
#endif
constexpr int kPrefixMax = NBH_BH_PREFIX_MAX;
constexpr int kPrefixBlock = 1024;
constexpr int kQuadWords = 10;

constexpr int kTreeBlock = 256;          // threads of a walk / build workgroup (kBlock of common.h; asserted there)
constexpr size_t kMaxNodeId = 0x0fffffffu;  // child ids are 28-bit
constexpr int kScheduleFromWaves = 2048;    // the pair walk takes a cost-ordered schedule from this many waves

// ---------------------------------------------------------------------------------------
// SIZES
// ---------------------------------------------------------------------------------------
// Two bounds on the node count of a tree over n bodies stand side by side, and they DIFFER:
//   tree_node_bound  counts NODES: the leaves (<= n) and, per level, the internal nodes (<= n / (leaf_max + 1) + 1).
//                    nbody_hip_tree_set_params REJECTS a deep tree (63-bit keys) whose bound passes the 28-bit ids.
//   tree_id_bound    counts IDS: every internal node may add one padding id for its children (even-aligned sibling
//                    groups), hence the factor 2 on the internal nodes.  The allocation CLAMPS it to 28 bits (and to
//                    nbody_hip_tree_limit_nodes): a tree that needs more is cut where the numbering passes the capacity.
// So parameters that set_params accepts may still have an id bound above 2^28; such a tree is allocated at the clamp
// and, if it ever needs the ids beyond, cut -- slower, never wrong.
inline size_t tree_node_bound(size_t n, int max_depth, int leaf_max) {
  return n + (size_t)(max_depth + 1) * (n / (size_t)(leaf_max + 1) + 1) + 16;
}
inline size_t tree_id_bound(size_t n, int max_depth, int leaf_max) {
  return n + 2 * (size_t)(max_depth + 1) * (n / (size_t)(leaf_max + 1) + 1) + 16;
}
inline bool tree_params_fit(size_t n, int max_depth, int leaf_max) {
  return max_depth <= kDepth32 || tree_node_bound(n, max_depth, leaf_max) <= kMaxNodeId;
}

// slots of one XCD's share of the pair walk's schedule (walk_plan_kernel) for this many waves
constexpr size_t schedule_cap(size_t waves) { return waves / 8 + waves / 32 + 8; }

// element counts (bytes where the name says so) of every array of a tree handle
struct TreeSizes {
  // fixed at create time, from max_particles alone
  size_t bodies;        // d_idx_a, d_idx_b, d_sorted
  size_t partial;       // d_partial: 3 sums x kSplitBudget (replicas x bodies)
  size_t prefix_cap;    // prefix entries of d_prefix ...
  size_t prefix_blocks; // ... followed by this many block totals and as many block offsets
  size_t prefix;        // d_prefix in all
  size_t cost;          // d_cost: one per wave
  size_t order;         // d_order: 8 XCDs x schedule_cap
  size_t bounds;        // d_bounds
  // replaced by set_params / limit_nodes
  bool wide;            // 63-bit keys in 64-bit words
  size_t capacity;      // node ids
  size_t key_bytes;     // d_keys_a, d_keys_b
  int rank_G;           // groups of 64 over the positions 0 .. n (a marker may sit one past the last body)
  size_t plane;         // d_plane: node flags, odd-group markers, cumulative flags of every level
  size_t rank_off;      // d_rank_off: node and odd-group offsets of every level
  size_t rec;           // t.rec: + 8, sibling-group prefetch reads ahead
  size_t pair_words;    // t.pb: + 8 blocks, group fetches read ahead
  // allocated by the first order-2 build
  size_t quad64;        // d_quad64
  size_t quad;          // d_quad: + 16, sibling groups read ahead
};

inline TreeSizes tree_sizes(size_t max_particles, int max_depth, int leaf_max, int node_limit) {
  TreeSizes s{};
  const size_t n = max_particles;
  s.bodies = n;
  s.partial = (size_t)3 * kSplitBudget;
  s.prefix_cap = (n < (size_t)kPrefixMax ? n : (size_t)kPrefixMax) + 8;
  s.prefix_blocks = kPrefixMax / kPrefixBlock + 2;
  s.prefix = s.prefix_cap + 2 * s.prefix_blocks;
  s.cost = n / 64 + 1;
  s.order = 8 * schedule_cap(s.cost);
  s.bounds = 16;
  s.wide = max_depth > kDepth32;
  size_t cap = tree_id_bound(n, max_depth, leaf_max);
  // 28-bit child ids.  A tree that would need more nodes than the arrays hold is cut where the numbering passes the
  // capacity: the nodes beyond do not exist, their parents become leaves of several bodies (exact body-by-body
  // interactions; tree_fill_kernel / store_node flag them from the UNCLAMPED node total) -- slower, never wrong.
  if (cap > kMaxNodeId) cap = kMaxNodeId;
  if (node_limit > 0 && (size_t)node_limit < cap) cap = (size_t)node_limit;
  s.capacity = cap;
  s.key_bytes = n * (s.wide ? sizeof(unsigned long long) : sizeof(unsigned int));
  s.rank_G = (int)((n + 64) / 64);
  const size_t tbl = (size_t)(max_depth + 1) * (size_t)s.rank_G;
  s.plane = 3 * tbl;
  s.rank_off = 2 * tbl;
  s.rec = cap + 8;
  s.pair_words = (cap / 2 + 8) * kPairWords;
  s.quad64 = cap * kQuadWords;
  s.quad = 2 * cap + 16;
  return s;
}

// ---------------------------------------------------------------------------------------
// ONE BUILD of ni bodies
// ---------------------------------------------------------------------------------------
struct BuildLayout {
  int ni, blocks, levels;
  int G;              // the ranks are laid out for THIS build's body count: G groups of 64 over the positions 0 .. ni
  size_t tbl;         // levels x G: one plane / one offset table
  size_t odd_plane, cum_plane;  // offsets into d_plane: odd-group markers, cumulative flags (plane 0: node flags)
  size_t odd_off;     // offset into d_rank_off
  size_t clear_words; // 32-bit words of the odd plane AND the cumulative plane that the key kernel clears (aligned only)
  bool wide, aligned, fused;
  int first_bit, key_bits;  // the key bits that shape the tree
  int pblocks;        // workgroups of the prefix sums (fused)
  size_t btot, boff;  // offsets into d_prefix: block totals, block offsets
  unsigned monopole_grid;
  int top;            // bottom-up passes: levels max_depth .. top + 1 one launch each, the narrow top in one workgroup
};

// even-aligned sibling groups are what the pair walk needs: trees it will walk (from kPairFrom bodies, or when that
// walk form is forced) get them, smaller trees keep plain ids and save three launches
// (order 2 always walks with the plain walk: a forced pair form does not change its ids)
inline bool build_aligned(int ni, int tune_form, int order) { return ni >= kPairFrom || (tune_form == 2 && order == 1); }

inline BuildLayout build_layout(int ni, int max_depth, int tune_form, int order, size_t prefix_cap) {
  BuildLayout b{};
  b.ni = ni;
  b.blocks = (ni + kTreeBlock - 1) / kTreeBlock;
  b.levels = max_depth + 1;
  b.G = (ni + 64) / 64;
  b.tbl = (size_t)b.levels * (size_t)b.G;
  b.odd_plane = b.tbl;
  b.cum_plane = 2 * b.tbl;
  b.odd_off = b.tbl;
  b.wide = max_depth > kDepth32;
  b.aligned = build_aligned(ni, tune_form, order);
  b.clear_words = b.aligned ? 2 * b.tbl : 0;
  // trees of <= kPrefixMax bodies: every node's monopole from the double-double prefix sums of the sorted bodies
  // (ni + 1 prefix entries: entry ni, the total, is thread ni's "sum before")
  b.fused = ni <= kPrefixMax;
  // only the 3 * max_depth leading bits of the 63 shape the tree (bodies that share them share a leaf of the
  // deepest level, where the order is immaterial: such a leaf interacts body by body)
  b.first_bit = b.wide ? 63 - 3 * max_depth : 0;
  b.key_bits = b.wide ? 63 : 30;
  b.pblocks = ni / kPrefixBlock + 1;
  b.btot = prefix_cap;
  b.boff = prefix_cap + kPrefixMax / kPrefixBlock + 2;
  // (about two ids per body in practice; a fixed grid strides over whatever the numbering arrived at)
  const size_t want = (2 * (size_t)ni + kTreeBlock - 1) / kTreeBlock;
  b.monopole_grid = (unsigned)(want < 1 ? 1 : want > 16384 ? 16384 : want);
  b.top = max_depth < 4 ? max_depth : 4;
  return b;
}

// ---------------------------------------------------------------------------------------
// ONE WALK
// ---------------------------------------------------------------------------------------
// GUARD instantiations (a pair at distance 0 is left out) when the softening cannot keep rsq finite
inline bool walk_guard(float eps2) { return eps2 < 1e-12f; }

// "is there a schedule": the previous walk of this very range recorded every wave's node visits, and there are enough
// waves for an order to matter.  The walk asks it of its range, the build of the full range (to queue the schedule on
// the side stream).
inline bool walk_scheduled(bool tune_schedule, int cost_first, int cost_n, int first, int n) {
  return tune_schedule && cost_first == first && cost_n == n && (n + 63) / 64 >= kScheduleFromWaves;
}

enum class WalkForm : int {
  None = 0,  // empty range: nothing is launched
  Plain,     // bh_traverse_kernel
  Count,     // ... its visit-histogram instantiation
  Split,     // ... K replicas + bh_combine_kernel
  Pair,      // bh_traverse_pair_kernel
};

struct WalkState {  // what a walk reads of the handle
  size_t built_count;
  int built_order;
  bool aligned;
  int tune_replicas, tune_split_level, tune_form;
  bool tune_schedule, count_visits;
  int cost_first, cost_n;
  bool plan_pending;
  int plan_n, plan_cap;
  bool capturing;
};

struct WalkPlan {
  WalkForm form;
  bool quad;        // order 2: the quadrupole instantiation of form (never Pair)
  bool guard;
  bool pair_on_plain_ids;  // error: the pair walk was asked for after a build with plain node ids
  bool wait_plan;   // the stream waits for the schedule queued beside the build (whatever the form, before anything else)
  int K, unit_max;
  int blocks;       // Plain / Count: grid (blocks); Split: grid (blocks, K), combine (blocks)
  int grid;         // Pair: workgroups of one wave
  bool scheduled;   // Pair: walks in the order of d_order ...
  bool plan_now;    // ... which this walk computes first (false: queued beside the build)
  int waves, cap;   // arguments of walk_plan_kernel / walk_order_kernel
  int cost_first, cost_n;  // the handle's state after the walk
  bool plan_pending;
};

inline WalkPlan walk_plan(int first, int n, float eps2, const WalkState& s) {
  WalkPlan p{};
  p.guard = walk_guard(eps2);
  p.quad = s.built_order == 2;
  p.wait_plan = s.plan_pending && !s.capturing;
  p.K = 1;
  p.unit_max = 1;
  p.cost_first = s.cost_first;
  p.cost_n = s.cost_n;
  p.plan_pending = s.plan_pending;
  if (n == 0) return p;
  p.blocks = (n + kTreeBlock - 1) / kTreeBlock;
  // replicas of the walk when there are too few waves to hide the fetch latency (see the kernel)
  int K = 1;
  while (K < kMaxReplicas && (size_t)(2 * K) * (size_t)n <= (size_t)kSplitAuto) K *= 2;
  if (n >= kPairFrom) K = 1;  // the pair walk (8 waves per SIMD, scheduled) overtakes two replicas from here
  if (s.tune_replicas > 0) {
    K = 1;
    while (K < s.tune_replicas && K < kMaxReplicas && (size_t)(2 * K) * (size_t)n <= (size_t)kSplitBudget) K *= 2;
  }
  p.K = K;
  // ownership units of at most n_total / 96 bodies (of the whole tree, not of the walked range): measured
  // best at K x (units per replica) ~ 64..128 for every K (tools/bh_split_sweep.py)
  const size_t units = s.tune_split_level > 0 ? (size_t)s.tune_split_level * (size_t)K : 96;
  p.unit_max = (int)(s.built_count / units);
  if (p.unit_max < 1) p.unit_max = 1;
  if (p.quad) {
    // multipole order 2: the plain walk whatever the walk form (the pair walk has no SGPRs for the moments); replicas
    // and visit counting as at order 1.  The pair walk's schedule state is left alone.
    p.form = K > 1 ? WalkForm::Split : s.count_visits ? WalkForm::Count : WalkForm::Plain;
    return p;
  }
  // walk without replicas: the pair walk unless the plain one is asked for -- or the tree was built with plain ids
  // (fewer than kPairFrom bodies and the pair form not forced when it was built): its pair blocks are not group-aligned
  int form = s.tune_form > 0 ? s.tune_form : 2;
  if (!s.aligned) {
    if (s.tune_form == 2) {
      p.pair_on_plain_ids = true;
      return p;
    }
    form = 1;
  }
  // counting on: the diagnostics instantiation of the plain walk (the pair walk visits the same nodes)
  if (K == 1 && s.count_visits && s.tune_form != 2) form = 1;
  if (K > 1) {
    p.form = WalkForm::Split;
  } else if (form == 1) {
    p.form = s.count_visits ? WalkForm::Count : WalkForm::Plain;
  } else {
    // one wave per workgroup: the dispatcher refills single wave slots (4-wave groups: +1.5 %, 16-wave: +7 %)
    p.form = WalkForm::Pair;
    p.waves = (n + 63) / 64;
    p.grid = p.waves;
    if (walk_scheduled(s.tune_schedule, s.cost_first, s.cost_n, first, n)) {
      // the previous walk of this range recorded every wave's node visits: longest first, equal cost per XCD
      p.cap = (int)schedule_cap((size_t)p.waves);
      p.scheduled = true;
      // queued beside the build (the stream already waits for it: wait_plan), or planned now
      p.plan_now = !(s.plan_pending && first == 0 && s.plan_n == n && s.plan_cap == p.cap && !s.capturing);
      p.grid = 8 * p.cap;
    }
    p.plan_pending = false;  // a second walk of the same build recorded new costs: it plans for itself
    p.cost_first = first;
    p.cost_n = n;
  }
  return p;
}

// ---------------------------------------------------------------------------------------
// THE BUILT TREE ON THE HOST
// ---------------------------------------------------------------------------------------
// The engine's ids have holes (padding of odd sibling groups, nodes cut off by the capacity; first_of < 0 marks both):
// the reference's array has none.  compact[nid] = position among the nodes that exist, or -1 (compact may be null);
// returns the number of nodes.
inline int compact_ids(const int* first_of, int nids, int* compact) {
  int count = 0;
  for (int nid = 0; nid < nids; nid++) {
    const bool real = first_of[nid] >= 0;
    if (compact) compact[nid] = real ? count : -1;
    count += real;
  }
  return count;
}

// ref layout: OctreeNode, include/nbody/barnes_hut_tree.hpp:9-30 (76 bytes)
struct RefOctreeNode {
  float center[3]; float half_size; float com[3]; float total_mass;
  int children[8]; int particle_index; bool is_leaf; int particle_count;
};
static_assert(sizeof(RefOctreeNode) == 76, "OctreeNode layout");

// records, sorted keys (30-bit keys widened), sorted indices and root cube -> the reference's nodes, children indexed
// by octant (x = bit 2, y = bit 1, z = bit 0).  id_base: first id of every level (holes included), nids ids in use.
inline void decode_nodes(const NodeRec* rec, const unsigned long long* keys, const int* idx, const TreeRoot& root,
                         const int* id_base, int max_depth, const int* compact, int nids, RefOctreeNode* out) {
  const int axis_bits = max_depth > kDepth32 ? 21 : 10;
  int level = 0;
  for (int nid = 0; nid < nids; nid++) {
    while (level < max_depth && nid >= id_base[level + 1]) level++;
    if (compact[nid] < 0) continue;
    RefOctreeNode& o = out[compact[nid]];
    const int first = rec[nid].first, cnt = rec[nid].count;
    const unsigned int ci = rec[nid].child;
    const unsigned long long k = keys[first];
    unsigned int q[3] = {0, 0, 0};
    for (int bit = 0; bit < axis_bits; bit++) {
      q[0] |= (unsigned)((k >> (3 * bit + 2)) & 1ull) << bit;
      q[1] |= (unsigned)((k >> (3 * bit + 1)) & 1ull) << bit;
      q[2] |= (unsigned)((k >> (3 * bit + 0)) & 1ull) << bit;
    }
    const float h = ldexpf(root.half, -level);
    for (int ax = 0; ax < 3; ax++)
      o.center[ax] = root.lo[ax] + ((float)(q[ax] >> (axis_bits - level)) + 0.5f) * (2.0f * h);
    o.half_size = h;
    o.com[0] = rec[nid].cx; o.com[1] = rec[nid].cy; o.com[2] = rec[nid].cz;
    o.total_mass = rec[nid].mass;
    for (int c = 0; c < 8; c++) o.children[c] = -1;
    o.is_leaf = ci == 0u;
    o.particle_index = (o.is_leaf && cnt >= 1) ? idx[first] : -1;
    o.particle_count = cnt;
    if (!o.is_leaf) {
      const int c0 = (int)(ci & 0x0fffffffu), nc = (int)(ci >> 28);
      const int shift = 3 * axis_bits - 3 - 3 * level;
      for (int c = c0; c < c0 + nc; c++) o.children[(keys[rec[c].first] >> shift) & 7ull] = compact[c];
    }
  }
}

}  // namespace nbh
