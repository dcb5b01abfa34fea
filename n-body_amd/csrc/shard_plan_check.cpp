// shard_plan_check.cpp -- the host arithmetic of the sharded Direct system (shard_plan.h) on a CPU, under AddressSanitizer
// and UBSan (make shard_plan_check): every pair of bodies in two different shards is evaluated exactly once, the plan
// equals written-out restatements of the schedule and of the derivation of the incoming blocks that sharded.hip used to
// carry, every task's slot is its counterpart on the receiving rank, the order of RCCL's sends matches the order of its
// receives, the finalize kernel's block table has room for every world size, and the shard bounds tile [0, n).
#include <cstdio>
#include <vector>

#include "shard_plan.h"

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

// ---- the code the header replaces, written out ----------------------------------------------------------------------
struct Row {
  size_t i0, i1, sh, j0, j1;
};
// nbody_hip_pair_schedule as sharded.hip defined it
static std::vector<Row> schedule_written_out(int world, int rank, size_t S) {
  std::vector<Row> rows;
  for (int d = 1; d <= (world - 1) / 2; d++) rows.push_back({0, S, (size_t)((rank + d) % world), 0, S});
  if (world % 2 == 0 && world > 1) {
    const int sh = (rank + world / 2) % world;
    const size_t h = S / 2;
    if (rank < world / 2) {
      if (h > 0) rows.push_back({0, h, (size_t)sh, 0, S});
    } else {
      rows.push_back({0, S, (size_t)sh, h, S});
    }
  }
  return rows;
}
// the incoming blocks as nbody_hip_sharded_direct_create derived them: for d = 1 .. W-1, rank r - d's tasks that name r
static std::vector<ShardIncoming> incoming_written_out(int W, int r, size_t S) {
  std::vector<ShardIncoming> in;
  for (int d = 1; d < W; d++) {
    const int q = (r - d + W) % W;
    for (const Row& t : schedule_written_out(W, q, S))
      if ((int)t.sh == r) in.push_back({q, t.j0, t.j1});
  }
  return in;
}

// ---- the plan of one (W, S) ------------------------------------------------------------------------------------------
static void check_plan(int W, size_t S, bool enumerate) {
  ShardedDirectPlan p;
  int a = -1, b = -1;
  const PlanFault fault = sharded_direct_plan(p, W, S, &a, &b);
  EXPECT(fault == kPlanOk, "W %d S %zu: fault %d between ranks %d and %d", W, S, (int)fault, a, b);
  EXPECT(p.W == W && p.S == S && (int)p.rank.size() == W, "W %d S %zu: the plan says W %d S %zu, %zu ranks", W, S, p.W, p.S, p.rank.size());
  if (fault != kPlanOk || (int)p.rank.size() != W) return;

  // the restatements, task by task and block by block; the sizes the kernel argument and the ABI's row buffer hold
  for (int r = 0; r < W; r++) {
    const ShardRankPlan& me = p.rank[(size_t)r];
    const std::vector<Row> rows = schedule_written_out(W, r, S);
    EXPECT(me.tasks.size() == rows.size(), "W %d S %zu rank %d: %zu tasks, the schedule has %zu", W, S, r, me.tasks.size(), rows.size());
    for (size_t k = 0; k < me.tasks.size() && k < rows.size(); k++) {
      const ShardTask& t = me.tasks[k];
      EXPECT(t.i0 == rows[k].i0 && t.i1 == rows[k].i1 && (size_t)t.shard == rows[k].sh && t.j0 == rows[k].j0 && t.j1 == rows[k].j1,
             "W %d S %zu rank %d task %zu: (%zu, %zu, %d, %zu, %zu)", W, S, r, k, t.i0, t.i1, t.shard, t.j0, t.j1);
      EXPECT(t.shard != r && t.i0 < t.i1 && t.i1 <= S && t.j0 < t.j1 && t.j1 <= S, "W %d S %zu rank %d task %zu is empty or out of range", W, S, r, k);
    }
    size_t got = 0;
    const int n = pair_schedule(W, r, S, [&](size_t, size_t, int, size_t, size_t) { got++; });
    EXPECT((size_t)n == rows.size() && got == rows.size(), "W %d S %zu rank %d: pair_schedule returns %d after %zu tasks", W, S, r, n, got);
    const std::vector<ShardIncoming> in = incoming_written_out(W, r, S);
    EXPECT(me.incoming.size() == in.size(), "W %d S %zu rank %d: %zu incoming blocks, create derived %zu", W, S, r, me.incoming.size(), in.size());
    for (size_t k = 0; k < me.incoming.size() && k < in.size(); k++)
      EXPECT(me.incoming[k].from == in[k].from && me.incoming[k].j0 == in[k].j0 && me.incoming[k].j1 == in[k].j1,
             "W %d S %zu rank %d block %zu: from %d [%zu, %zu)", W, S, r, k, me.incoming[k].from, me.incoming[k].j0, me.incoming[k].j1);
    EXPECT(me.incoming.size() <= (size_t)kShardMaxBlocks && me.tasks.size() <= (size_t)kShardMaxBlocks,
           "W %d S %zu rank %d: %zu tasks, %zu blocks, room for %d", W, S, r, me.tasks.size(), me.incoming.size(), kShardMaxBlocks);
    const InRanges ranges = in_ranges(me);
    EXPECT(ranges.n == (int)me.incoming.size(), "W %d S %zu rank %d: %d ranges of %zu blocks", W, S, r, ranges.n, me.incoming.size());
    for (int k = 0; k < ranges.n; k++)
      EXPECT(ranges.j0[k] == me.incoming[(size_t)k].j0 && ranges.j1[k] == me.incoming[(size_t)k].j1, "W %d S %zu rank %d range %d: [%u, %u)", W,
             S, r, k, ranges.j0[k], ranges.j1[k]);
  }

  // every task's slot is its counterpart: it exists, names the sender, spans the same rows; no slot twice, none left over
  std::vector<std::vector<int>> matched((size_t)W);
  for (int r = 0; r < W; r++) matched[(size_t)r].assign(p.rank[(size_t)r].incoming.size(), 0);
  for (int r = 0; r < W; r++)
    for (const ShardTask& t : p.rank[(size_t)r].tasks) {
      if (t.shard < 0 || t.shard >= W) continue;  // (reported above)
      const std::vector<ShardIncoming>& in = p.rank[(size_t)t.shard].incoming;
      EXPECT(t.slot >= 0 && (size_t)t.slot < in.size(), "W %d S %zu: rank %d -> %d names slot %d of %zu", W, S, r, t.shard, t.slot, in.size());
      if (t.slot < 0 || (size_t)t.slot >= in.size()) continue;
      const ShardIncoming& s = in[(size_t)t.slot];
      EXPECT(s.from == r && s.j0 == t.j0 && s.j1 == t.j1, "W %d S %zu: rank %d -> %d [%zu, %zu) lands in the slot of rank %d [%zu, %zu)", W, S, r,
             t.shard, t.j0, t.j1, s.from, s.j0, s.j1);
      matched[(size_t)t.shard][(size_t)t.slot]++;
    }
  for (int r = 0; r < W; r++)
    for (size_t k = 0; k < matched[(size_t)r].size(); k++)
      EXPECT(matched[(size_t)r][k] == 1, "W %d S %zu: slot %zu of rank %d is filled by %d tasks", W, S, k, r, matched[(size_t)r][k]);

  // RCCL matches the messages between two ranks by order: what a sends to b, in task order, is what b receives from a, in
  // incoming order -- and that is at most one message
  for (int x = 0; x < W; x++)
    for (int y = 0; y < W; y++) {
      std::vector<size_t> sent, received;
      for (const ShardTask& t : p.rank[(size_t)x].tasks)
        if (t.shard == y) sent.push_back(t.j1 - t.j0);
      for (const ShardIncoming& s : p.rank[(size_t)y].incoming)
        if (s.from == x) received.push_back(s.j1 - s.j0);
      EXPECT(sent == received, "W %d S %zu: rank %d sends %zu messages to rank %d, which receives %zu", W, S, x, sent.size(), y, received.size());
      EXPECT(sent.size() <= 1, "W %d S %zu: rank %d sends %zu messages to rank %d", W, S, x, sent.size(), y);
      EXPECT(x != y || sent.empty(), "W %d S %zu: rank %d sends to itself", W, S, x);
    }

  // every pair of bodies in two different shards lies in exactly one rectangle of exactly one rank.  By arithmetic: the
  // rectangles of a pair of shards {x, y}, in (row of x, row of y) coordinates, lie inside S x S, do not overlap and have
  // S^2 bodies between them
  struct Rect {
    size_t u0, u1, v0, v1;
  };
  for (int x = 0; x < W; x++)
    for (int y = x + 1; y < W; y++) {
      std::vector<Rect> rects;
      for (const ShardTask& t : p.rank[(size_t)x].tasks)
        if (t.shard == y) rects.push_back({t.i0, t.i1, t.j0, t.j1});
      for (const ShardTask& t : p.rank[(size_t)y].tasks)
        if (t.shard == x) rects.push_back({t.j0, t.j1, t.i0, t.i1});
      unsigned long long area = 0;
      for (size_t k = 0; k < rects.size(); k++) {
        area += (unsigned long long)(rects[k].u1 - rects[k].u0) * (rects[k].v1 - rects[k].v0);
        for (size_t m = k + 1; m < rects.size(); m++) {
          const bool apart = rects[k].u1 <= rects[m].u0 || rects[m].u1 <= rects[k].u0 || rects[k].v1 <= rects[m].v0 || rects[m].v1 <= rects[k].v0;
          EXPECT(apart, "W %d S %zu: two rectangles of the shards %d and %d overlap", W, S, x, y);
        }
      }
      EXPECT(area == (unsigned long long)S * S, "W %d S %zu: the shards %d and %d have %llu of %llu pairs evaluated", W, S, x, y, area,
             (unsigned long long)S * S);
    }
  // ... and by enumeration: bodies by global index, pad rows included
  if (enumerate) {
    const size_t N = (size_t)W * S;
    std::vector<int> seen(N * N, 0);
    for (int r = 0; r < W; r++)
      for (const ShardTask& t : p.rank[(size_t)r].tasks)
        for (size_t i = t.i0; i < t.i1; i++)
          for (size_t j = t.j0; j < t.j1; j++) seen[((size_t)r * S + i) * N + (size_t)t.shard * S + j]++;
    for (size_t i = 0; i < N; i++)
      for (size_t j = 0; j < N; j++) {
        const int both = seen[i * N + j] + seen[j * N + i];
        if (i / S == j / S)
          EXPECT(both == 0, "W %d S %zu: the bodies %zu and %zu of one shard are in %d rectangles", W, S, i, j, both);
        else
          EXPECT(both == 1, "W %d S %zu: the bodies %zu and %zu are in %d rectangles", W, S, i, j, both);
      }
  }

  // balance: the ranks' rectangle areas are equal, but for the half row that an odd S leaves to the upper rank of an
  // antipodal pair (S bodies: less than half a rectangle)
  unsigned long long least = ~0ull, most = 0;
  for (int r = 0; r < W; r++) {
    unsigned long long work = 0;
    for (const ShardTask& t : p.rank[(size_t)r].tasks) work += (unsigned long long)(t.i1 - t.i0) * (t.j1 - t.j0);
    least = work < least ? work : least;
    most = work > most ? work : most;
  }
  const unsigned long long uneven = (W % 2 == 0 && S % 2 == 1) ? S : 0;
  EXPECT(most - least == uneven, "W %d S %zu: the ranks' work spans [%llu, %llu]", W, S, least, most);
  EXPECT(2 * (most - least) <= (unsigned long long)S * S + 1, "W %d S %zu: the ranks' work differs by more than half a rectangle", W, S);

  // S = 1 at even W: the lower rank of an antipodal pair has no antipodal task (h = 0), the upper rank takes the rectangle
  if (S == 1 && W % 2 == 0)
    for (int r = 0; r < W; r++) {
      const int partner = (r + W / 2) % W;
      const ShardTask* anti = nullptr;
      for (const ShardTask& t : p.rank[(size_t)r].tasks)
        if (t.shard == partner) anti = &t;
      if (r < W / 2)
        EXPECT(!anti && (int)p.rank[(size_t)r].tasks.size() == (W - 1) / 2, "W %d S 1: the lower rank %d has an antipodal task", W, r);
      else
        EXPECT(anti && anti->i0 == 0 && anti->i1 == 1 && anti->j0 == 0 && anti->j1 == 1, "W %d S 1: the upper rank %d lacks the whole rectangle", W, r);
    }
}

// shards are contiguous and cover [0, n); an empty rank has lo == hi == n; S W >= n
static void check_bounds(size_t n, int W) {
  size_t at = 0;
  const size_t S = (n + (size_t)W - 1) / (size_t)W;
  for (int r = 0; r < W; r++) {
    const ShardBounds b = shard_bounds(n, W, r);
    EXPECT(b.shard == S, "n %zu W %d rank %d: shard %zu, ceil(n / W) is %zu", n, W, r, b.shard, S);
    EXPECT(b.lo == at && b.hi >= b.lo && b.hi - b.lo <= S, "n %zu W %d rank %d: [%zu, %zu) after %zu", n, W, r, b.lo, b.hi, at);
    EXPECT(b.lo == ((size_t)r * S < n ? (size_t)r * S : n), "n %zu W %d rank %d: lo %zu", n, W, r, b.lo);
    if (b.lo == b.hi) EXPECT(b.lo == n, "n %zu W %d: the empty rank %d sits at %zu", n, W, r, b.lo);
    if (b.hi < n) EXPECT(b.hi - b.lo == S, "n %zu W %d rank %d: a short shard [%zu, %zu) before the end", n, W, r, b.lo, b.hi);
    at = b.hi;
  }
  EXPECT(at == n, "n %zu W %d: the shards end at %zu", n, W, at);
  EXPECT(S * (size_t)W >= n && S * (size_t)W < n + (size_t)W, "n %zu W %d: S %zu", n, W, S);
}

int main() {
  for (int W = 1; W <= kShardMaxRanks; W++) {
    for (size_t S : {1, 2, 3, 7, 8}) check_plan(W, S, true);
    for (size_t S : {131072, 12500000}) check_plan(W, S, false);
    for (long long n : {1LL, 2LL, (long long)W - 1, (long long)W, (long long)W + 1, 2LL * W + 1, 1048576LL, 100000000LL})
      if (n >= 1) check_bounds((size_t)n, W);
  }
  if (failures) {
    std::printf("shard_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("shard_plan_check: ok\n");
  return 0;
}
