// shard_plan.h -- the host arithmetic of the sharded Direct system (sharded.hip): the index-range shards, the schedule that
// evaluates every pair of shards exactly once, and the exchange of the reaction blocks that follows from it.  Plain C++17,
// no HIP include: shard_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make shard_plan_check).
//
// From (W, S) alone -- integers every process holds alike -- sharded_direct_plan derives, ONCE at create, every rank's tasks, the
// reaction blocks it receives, and for every task the slot of the receiver's block that it fills.  The RCCL executor
// issues Send / Recv from the plan's entries, the peer-copy executor hipMemcpyAsync from the same entries; neither
// searches for its counterpart.
#pragma once

#include <cstddef>
#include <vector>

namespace nbh {

constexpr int kShardMaxRanks = 32;                  // = NBODY_HIP_MAX_RANKS (sharded.hip asserts it)
constexpr int kShardMaxBlocks = kShardMaxRanks / 2;  // tasks per rank, and reaction blocks a rank receives, at most

// rank r holds the bodies [lo, hi) of n in a shard of S = ceil(n / W) rows (the rest is padding); a rank past the end of
// the bodies has lo == hi == n
struct ShardBounds {
  size_t shard, lo, hi;
};
inline ShardBounds shard_bounds(size_t n, int world, int rank) {
  const size_t s = (n + (size_t)world - 1) / (size_t)world;
  const size_t l = (size_t)rank * s < n ? (size_t)rank * s : n;
  const size_t h = l + s < n ? l + s : n;
  return {s, l, h};
}

// Rank r takes the ring neighbours r+1 .. r+(W-1)/2 whole; for even W the antipodal rectangle is cut in half: the
// lower rank takes its first half x the whole partner, the upper rank its whole shard x the partner's second half.
// put(i0, i1, shard, j0, j1) receives the tasks in order: own rows [i0, i1) x rows [j0, j1) of `shard`.  Returns their number.
template <class Put>
inline int pair_schedule(int world, int rank, size_t S, Put put) {
  int k = 0;
  auto task = [&](size_t i0, size_t i1, int sh, size_t j0, size_t j1) {
    put(i0, i1, sh, j0, j1);
    k++;
  };
  for (int d = 1; d <= (world - 1) / 2; d++) task(0, S, (rank + d) % world, 0, S);
  if (world % 2 == 0 && world > 1) {
    const int sh = (rank + world / 2) % world;
    const size_t h = S / 2;
    if (rank < world / 2) {
      if (h > 0) task(0, h, sh, 0, S);
    } else {
      task(0, S, sh, h, S);
    }
  }
  return k;
}

// own bodies [i0, i1) x rows [j0, j1) of shard `shard`; the reactions on those rows (row 0 = body j0) go to block `slot`
// of rank `shard`'s incoming list.  The sender and the receiver read THE SAME two entries: tasks[k] here, incoming[slot] there.
struct ShardTask {
  size_t i0, i1, j0, j1;
  int shard, slot;
};
struct ShardIncoming {  // reactions on my rows [j0, j1) computed by rank `from`
  int from;
  size_t j0, j1;
};
struct ShardRankPlan {
  std::vector<ShardTask> tasks;         // in schedule order
  std::vector<ShardIncoming> incoming;  // in ring distance d = 1 .. W-1 of the sender r - d: the finalize kernel's summation order
};
struct ShardedDirectPlan {
  int W = 0;
  size_t S = 0;
  std::vector<ShardRankPlan> rank;  // [W]: every rank's, not only the local ones'
};

// what must hold of a plan before anything is issued from it (it does, for every W <= kShardMaxRanks: the check proves it)
enum PlanFault { kPlanOk = 0, kPlanMismatch, kPlanTooManyBlocks };

// Fills p in place.  On kPlanMismatch *a / *b are the sender and the receiver whose entries do not match.
inline PlanFault sharded_direct_plan(ShardedDirectPlan& p, int W, size_t S, int* a = nullptr, int* b = nullptr) {
  p.W = W;
  p.S = S;
  p.rank.assign((size_t)W, ShardRankPlan());
  for (int r = 0; r < W; r++)
    pair_schedule(W, r, S, [&](size_t i0, size_t i1, int sh, size_t j0, size_t j1) {
      p.rank[(size_t)r].tasks.push_back({i0, i1, j0, j1, sh, -1});
    });
  // who sends me what: rank q's tasks that name me, in order of ring distance (a fixed summation order); the task learns
  // its slot here
  for (int r = 0; r < W; r++)
    for (int d = 1; d < W; d++) {
      const int q = (r - d + W) % W;
      for (ShardTask& t : p.rank[(size_t)q].tasks)
        if (t.shard == r) {
          if (t.slot >= 0) {  // (a task names one rank: it cannot be found twice)
            if (a) *a = q;
            if (b) *b = r;
            return kPlanMismatch;
          }
          t.slot = (int)p.rank[(size_t)r].incoming.size();
          p.rank[(size_t)r].incoming.push_back({q, t.j0, t.j1});
        }
    }
  for (int r = 0; r < W; r++) {
    for (const ShardTask& t : p.rank[(size_t)r].tasks) {
      const bool in_world = t.shard >= 0 && t.shard < W && t.shard != r;
      const std::vector<ShardIncoming>* in = in_world ? &p.rank[(size_t)t.shard].incoming : nullptr;
      if (!in || t.slot < 0 || (size_t)t.slot >= in->size() || (*in)[(size_t)t.slot].from != r ||
          (*in)[(size_t)t.slot].j1 - (*in)[(size_t)t.slot].j0 != t.j1 - t.j0) {
        if (a) *a = r;
        if (b) *b = t.shard;
        return kPlanMismatch;
      }
    }
    if (p.rank[(size_t)r].incoming.size() > (size_t)kShardMaxBlocks) return kPlanTooManyBlocks;
  }
  return kPlanOk;
}

// the row ranges of a rank's incoming blocks as the finalize kernel takes them (the device pointers join them once the
// blocks are allocated).  Only for a plan that sharded_direct_plan found kPlanOk.
struct InRanges {
  int n;
  unsigned int j0[kShardMaxBlocks], j1[kShardMaxBlocks];
};
inline InRanges in_ranges(const ShardRankPlan& r) {
  InRanges in = {};
  for (const ShardIncoming& b : r.incoming) {
    if (in.n == kShardMaxBlocks) break;
    in.j0[in.n] = (unsigned)b.j0;
    in.j1[in.n] = (unsigned)b.j1;
    in.n++;
  }
  return in;
}

}  // namespace nbh
