// slab_plan.h -- the host arithmetic of one exchange of the z-slab sharded spatial hash (sharded_hash.hip), and the two
// owner functions that the partition pass on the device (slab.hip) and every rank's host must evaluate alike.  Plain
// C++17, no HIP include: slab_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make plan_check).
//
// From integers that every process holds alike after the step's one host synchronisation -- the summed W x W send matrix,
// the bodies per layer, the grid -- exchange_plan derives, ONCE, where every migrating row and every halo layer goes.
// The RCCL executor issues Send / Recv from the plan's entries, the peer-copy executor hipMemcpyAsync from the same
// entries; neither recomputes an offset.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define NBH_SLAB_HD __host__ __device__
#else
#define NBH_SLAB_HD
#endif

namespace nbh {

constexpr int kMaxRanks = 64;  // what slab.hip accepts (the sharded systems stop at NBODY_HIP_MAX_RANKS = 32)

// padded box and grid dims exactly as SpatialHashGrid::build derives them (force_spatial_hash.cu:225-246)
inline void grid_from_box(const float raw[6], float cell, float bounds[6], int dims[3]) {
  for (int a = 0; a < 3; a++) {
    bounds[a] = raw[a] - 0.001f;
    bounds[3 + a] = raw[3 + a] + 0.001f;
    const float cells = ceilf((bounds[3 + a] - bounds[a]) / cell);
    dims[a] = (cells < 1.0e9f && cells >= 0.0f) ? (int)cells + 1 : 0x40000000;
  }
}

// owner of layer z when rank r owns [r gz / W, (r+1) gz / W): r = ceil((z+1) W / gz) - 1
// (z >= floor(r gz / W)  <=>  z + 1 > r gz / W  <=>  (z + 1) W - 1 >= r gz: the largest such r is the quotient)
NBH_SLAB_HD inline int slab_owner(int z, int gz, int world) {
  return (int)((((long long)z + 1) * world - 1) / gz);
}

// ... or, with cuts (n >= 0): the ranks' slabs are bounded by PHYSICAL z coordinates (chosen by the host so that the
// slabs hold about the same number of bodies): the owner of layer z is the number of cuts at or below the layer's
// centre, lo_z + (z + 1/2) cell -- formed with ONE fma on the device and on the host (nbody_hip_slab_layer_owner), so
// that both sides and all ranks assign every layer alike.  Monotone in z: a rank's layers are contiguous.
struct SlabCuts {
  float z[kMaxRanks];
  int n;  // world - 1 cuts, ascending; < 0: equal layer counts (slab_owner)
};
NBH_SLAB_HD inline int slab_owner_cuts(int z, float lo_z, float cell, const SlabCuts& c) {
  const float zc = fmaf((float)z + 0.5f, cell, lo_z);
  int r = 0;
  for (int k = 0; k < c.n; k++) r += c.z[k] <= zc ? 1 : 0;
  return r;
}

// owner of every layer of a grid and the ranks' layer ranges [lo, hi), as the partition pass on the device assigns them
// (a rank without layers has lo == hi)
struct SlabMap {
  std::vector<int> owner;  // [gz]
  int lo[kMaxRanks], hi[kMaxRanks];
};
// cuts: W - 1 ascending z coordinates, or nullptr for equal layer counts.  Fills m in place (its storage is reused).
inline void slab_map(SlabMap& m, int W, const float* cuts, float lo_z, float cell, int gz) {
  SlabCuts c;
  c.n = cuts ? W - 1 : -1;
  for (int k = 0; k < c.n; k++) c.z[k] = cuts[k];
  m.owner.resize((size_t)gz);
  for (int z = 0; z < gz; z++) m.owner[(size_t)z] = cuts ? slab_owner_cuts(z, lo_z, cell, c) : slab_owner(z, gz, W);
  for (int r = 0, z = 0; r < W; r++) {  // owners ascend with z: a rank's layers are contiguous
    while (z < gz && m.owner[(size_t)z] < r) z++;
    m.lo[r] = z;
    while (z < gz && m.owner[(size_t)z] == r) z++;
    m.hi[r] = z;
  }
}

// cuts that give every rank about n / W bodies, from the bodies per layer of a grid with lower bound lo_z: the k-th cut is
// the lower edge of the first layer at which the running count reaches k n / W
inline void balanced_cuts(int W, float cell, const int* hist, int gz, float lo_z, size_t n, std::vector<float>& cuts) {
  cuts.assign((size_t)(W > 1 ? W - 1 : 0), 0.f);
  long long run = 0;
  int z = 0;
  for (int k = 1; k < W; k++) {
    const long long want = (long long)((double)n * k / W);
    while (z < gz && run + hist[z] <= want) run += hist[z++];
    // layer z holds the body that crosses k n / W: it goes to the side that leaves the smaller error
    int b = z;
    if (z < gz && (want - run) * 2 > hist[z]) b = z + 1;
    cuts[(size_t)(k - 1)] = lo_z + (float)b * cell;
  }
}

inline long long largest_slab(const int* hist, int W, const SlabMap& m) {
  long long most = 0;
  for (int r = 0; r < W; r++) {
    long long c = 0;
    for (int z = m.lo[r]; z < m.hi[r]; z++) c += hist[z];
    most = c > most ? c : most;
  }
  return most;
}
// candidate cuts are adopted when they would take 5 % off the largest slab (a moved cut sends a layer of bodies to another
// rank: not for every wobble)
inline bool adopt_cuts(const int* hist, int W, const SlabMap& cur, const SlabMap& cand) {
  return largest_slab(hist, W, cand) * 100 < largest_slab(hist, W, cur) * 95;
}

// one group of migrating rows, in rows of 16 floats.  The sender and the receiver hold THE SAME entry: `rows_off` is the
// offset in the sender's `rows`, `got_off` the offset in the receiver's `got`, `peer` the other side.
struct RowTransfer {
  int peer;
  size_t rows_off, got_off, count;
};
// one boundary layer on its way, in bodies.  Again the same entry on both sides: `out_off` / `out_slot` are the offset in
// the sender's halo_out and the slot of its start-array pair, `in_off` / `in_slot` those of the receiver's halo_in.
struct LayerTransfer {
  int peer;
  size_t out_off, in_off, count;
  int out_slot, in_slot;
};
struct RankPlan {
  size_t n_new = 0, n_leave = 0, n_arrive = 0;
  std::vector<RowTransfer> sends, arrivals;  // sends ascending by destination, arrivals ascending by source; none empty
  // halo: my layers [z_lo, z_hi); the owners of the layer below and above them (-1: none); bodies of my lowest / highest
  // layer (they leave) and of the layer below / above my slab (they arrive: the lower one first, the upper one behind it)
  int z_lo = 0, z_hi = 0, lower = -1, upper = -1;
  size_t n_head = 0, n_tail = 0, in_lower = 0, in_upper = 0;
  LayerTransfer out[2], in[2];  // out: head, then tail; in: from below, then from above; none empty
  int n_out = 0, n_in = 0;
};
struct ExchangePlan {
  std::vector<RankPlan> rank;  // [W]
  bool all_dense = true;       // every rank's slab carries per-cell start arrays: the two-grid form
  unsigned long long migrated = 0, halo_bodies = 0;
};

// M[src * W + dst]: bodies that rank src holds and rank dst owns next; hist[z]: bodies in layer z, all ranks;
// layer_cells = gx gy.  Fills p in place (its storage is reused from step to step).
inline void exchange_plan(ExchangePlan& p, int W, const int* M, const int* hist, int gz, long long layer_cells,
                          const SlabMap& map) {
  p.rank.resize((size_t)W);
  p.all_dense = true;
  p.migrated = p.halo_bodies = 0;
  for (int r = 0; r < W; r++) {
    RankPlan& a = p.rank[(size_t)r];
    a.sends.clear();
    a.arrivals.clear();
    a.n_new = a.n_leave = a.n_arrive = 0;
  }
  // migration: rows leave grouped by new owner, ascending, own rank absent; arrivals are ordered by source rank
  for (int q = 0; q < W; q++) {
    RankPlan& dst = p.rank[(size_t)q];
    dst.n_new += (size_t)M[q * W + q];
    for (int s = 0; s < W; s++) {
      if (s == q) continue;
      RankPlan& src = p.rank[(size_t)s];
      const size_t cnt = (size_t)M[s * W + q];
      if (cnt) {
        src.sends.push_back({q, src.n_leave, dst.n_arrive, cnt});
        dst.arrivals.push_back({s, src.n_leave, dst.n_arrive, cnt});
      }
      src.n_leave += cnt;
      dst.n_arrive += cnt;
      dst.n_new += cnt;
    }
  }
  // halo: what arrives, per rank ...
  for (int r = 0; r < W; r++) {
    RankPlan& a = p.rank[(size_t)r];
    p.migrated += a.n_leave;
    a.z_lo = map.lo[r];
    a.z_hi = map.hi[r];
    a.lower = a.upper = -1;
    a.n_head = a.n_tail = a.in_lower = a.in_upper = 0;
    if (W > 1 && a.z_hi > a.z_lo) {
      if (a.z_lo > 0) {
        a.lower = map.owner[(size_t)(a.z_lo - 1)];
        a.n_head = (size_t)hist[a.z_lo];
        a.in_lower = (size_t)hist[a.z_lo - 1];
      }
      if (a.z_hi < gz) {
        a.upper = map.owner[(size_t)a.z_hi];
        a.n_tail = (size_t)hist[a.z_hi - 1];
        a.in_upper = (size_t)hist[a.z_hi];
      }
    }
    p.halo_bodies += a.in_lower + a.in_upper;
    // too sparse for the per-cell start arrays of the two-grid kernel: one rank decides for all
    if (a.n_new > 0 && (long long)(a.z_hi - a.z_lo) * layer_cells > 4LL * (long long)a.n_new + 4096) p.all_dense = false;
  }
  // ... and where each layer that leaves lands: my lowest layer is the UPPER halo of the owner of the layer below, behind
  // its lower halo (slot 1); my highest layer is the LOWER halo of the owner of the layer above, at the front (slot 0)
  for (int r = 0; r < W; r++) p.rank[(size_t)r].n_out = p.rank[(size_t)r].n_in = 0;
  for (int r = 0; r < W; r++) {
    RankPlan& a = p.rank[(size_t)r];
    if (a.n_head) {
      RankPlan& d = p.rank[(size_t)a.lower];
      a.out[a.n_out++] = {a.lower, 0, d.in_lower, a.n_head, 0, 1};
    }
    if (a.n_tail) a.out[a.n_out++] = {a.upper, a.n_head, 0, a.n_tail, 1, 0};
  }
  for (int r = 0; r < W; r++) {  // the receiver's view of the same entries: from below (its tail), then from above (its head)
    RankPlan& a = p.rank[(size_t)r];
    if (a.in_lower) {
      const RankPlan& b = p.rank[(size_t)a.lower];
      a.in[a.n_in] = b.out[b.n_out - 1];
      a.in[a.n_in++].peer = a.lower;
    }
    if (a.in_upper) {
      const RankPlan& b = p.rank[(size_t)a.upper];
      a.in[a.n_in] = b.out[0];
      a.in[a.n_in++].peer = a.upper;
    }
  }
}

}  // namespace nbh
