// direct_plan.h -- the host decisions of the single-GPU Direct N^2 family (direct.hip, direct_sym.hip, energy.hip,
// hermite.hip, hermite_block.hip) as plain code: which kernel a force, field, potential or
// force-and-jerk call launches, with which shape and how many workspace bytes, and which kernel a block step takes.
// Plain C++17, no HIP include: direct_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make
// direct_plan_check) against the code it replaces.  Nothing here launches, allocates, reads device memory or reads the
// environment.
#pragma once

#include <cstddef>

namespace nbh {

constexpr int kDirectBlock = 256;  // threads of a workgroup (kBlock of common.h, asserted there)
constexpr int kDirectCU = 256;     // compute units (kNumCU of common.h, asserted there)
constexpr int kDirectTile = 256;   // sources per LDS tile (TS of direct.hip and hermite_common.h, PTS of energy.hip)

inline size_t plan_ceil(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- THE TUNING: what nbody_hip_direct_tuning, _deterministic and _slot_budget leave in the context ----
constexpr size_t kSlotBudgetDefault = (size_t)24 << 30;
constexpr size_t kLargeWorkspace = (size_t)64 << 20;  // a workspace above this is worth giving back (both release rules)

struct DirectTuning {
  int variant = -1, tpl = 0, splits = 0;  // overrides (variant -1 / others 0 = automatic)
  // symmetric kernels: 0 = fp64 atomics; 1 = slot planes + fixed-order sum (bitwise reproducible) when they fit the
  // budget, else atomics; 2 = slot planes REQUIRED (a call that cannot have them fails with NBODY_HIP_ERR_RESOURCE)
  int deterministic = 1;
  size_t det_budget = kSlotBudgetDefault;  // most slot-plane bytes the deterministic form may take
};
// "no tuning": the Hermite sweeps and the field call take the automatic shape whatever the context holds
inline DirectTuning no_tuning() { return DirectTuning{}; }

// m * rsq(eps2)^3 must stay finite for the branch-free self-pair trick: below this softening the one-sided kernels run
// their GUARD form and the symmetric kernels are not taken.  (Two comparisons, not one and its negation: a NaN is
// neither guarded nor fit for pairs, as in the code these replace.)
constexpr float kGuardBelow = 1e-12f;
inline bool direct_guard(float eps2) { return eps2 < kGuardBelow; }
inline bool direct_pairs_ok(float eps2) { return eps2 >= kGuardBelow; }

// ---- THE ONE-SIDED KERNELS: direct_kernel, direct_field_kernel, direct_jerk_kernel ----
struct OneSidedShape {
  int R, splits, src_per_split, blocks_x, n_pad;
  size_t rows() const { return (size_t)splits * n_pad; }  // float4 rows of one [splits][n_pad] partial array
};

inline OneSidedShape one_sided_shape(const DirectTuning& t, size_t n_tgt, size_t n_src) {
  OneSidedShape s;
  // Targets per lane: 4 once every CU still gets >= 4 blocks; small problems prefer more blocks over more ILP.
  // Measured on MI355X (tools/sweep_direct.py): 4 targets per lane wins from N = 2.6e5 up; below ~3e4 targets more
  // blocks matter more than ILP.
  s.R = n_tgt >= 32768 ? 4 : 2;
  if (t.tpl == 1 || t.tpl == 2 || t.tpl == 4) s.R = t.tpl;
  s.blocks_x = (int)plan_ceil(n_tgt, (size_t)kDirectBlock * s.R);
  s.n_pad = s.blocks_x * kDirectBlock * s.R;
  const int tiles = (int)plan_ceil(n_src, kDirectTile);
  // Aim for >= 16 blocks per CU queued so the last wave of blocks is short (measured: 4096 blocks beat 1024/2048 at
  // N = 2^20 by 3-7 %).
  int want = (kDirectCU * 16 + s.blocks_x - 1) / s.blocks_x;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  if (t.splits > 0) want = t.splits;
  if (want > tiles) want = tiles > 0 ? tiles : 1;
  const int tiles_per_split = (tiles + want - 1) / want;
  s.src_per_split = tiles_per_split * kDirectTile;
  s.splits = tiles_per_split > 0 ? (tiles + tiles_per_split - 1) / tiles_per_split : 1;  // (no sources: one empty split)
  if (s.splits < 1) s.splits = 1;
  return s;
}

// what a one-sided force call runs: direct_kernel<R, variant, guard> (variant 1 at R = 1: refused once the workspace is
// reserved, and only when there are sources to sweep)
struct OneSidedPlan {
  OneSidedShape s;
  int variant;  // 0 scalar body, 1 packed body, 2 the third body
  bool guard, refused;
  size_t bytes() const { return s.rows() * 4 * sizeof(float); }
};

inline OneSidedPlan one_sided_plan(const DirectTuning& t, size_t n_tgt, size_t n_src, float eps2) {
  OneSidedPlan p;
  p.s = one_sided_shape(t, n_tgt, n_src);
  p.guard = direct_guard(eps2);
  // automatic choice: the packed body (measured 4.2e12 vs 3.5e12 pairs/s for the scalar body)
  p.variant = t.variant;
  if (p.variant < 0 || p.variant > 2) p.variant = p.s.R >= 2 ? 1 : 0;
  if (p.guard && p.variant == 1) p.variant = 0;
  p.refused = n_src > 0 && p.s.R == 1 && p.variant == 1;
  return p;
}

// the source splits of the potential sweeps (potential_kernel): a function of the two counts alone
struct PotentialSplits { int bx, splits, src_per_split; };

inline PotentialSplits potential_splits(size_t n_tgt, size_t n_src) {
  PotentialSplits p;
  p.bx = (int)plan_ceil(n_tgt, kDirectBlock);
  const int tiles = (int)plan_ceil(n_src, kDirectTile);
  int splits = (kDirectCU * 8 + p.bx - 1) / p.bx;
  if (splits > 64) splits = 64;
  if (splits > tiles) splits = tiles;
  if (splits < 1) splits = 1;
  const int tiles_per_split = tiles > 0 ? (tiles + splits - 1) / splits : 1;
  p.splits = tiles > 0 ? (tiles + tiles_per_split - 1) / tiles_per_split : 0;  // (no sources: nothing to launch)
  p.src_per_split = tiles_per_split * kDirectTile;
  return p;
}

// ---- THE SYMMETRIC KERNELS: direct_sym_kernel, all pairs of one set and two disjoint sets ----
constexpr int kSymBlocksPerCU = 16;  // workgroups aimed at per CU (tools/sweep_mid.py)
constexpr int kSymMinChunks = 4;     // at least 4 chunks (256 J bodies) per workgroup
#ifndef NBH_DET_GEN_R
#define NBH_DET_GEN_R 16
#endif
constexpr int kDetGenR = NBH_DET_GEN_R;  // bodies per lane of the general-mass instantiation in deterministic mode at sizes
                                         // where the equal-mass one takes 16 (round 2: 12 -- the slot kernel spilled into
                                         // AGPRs at 16; with the single loop body of round 3 it does not)

// symmetric kernel worth it from here (measured, tools/sweep_sym_sizes.py): below, the one-sided kernel
inline bool symmetric_pays(const DirectTuning& t, size_t n) {
  if (t.variant == 3 || t.variant == 4) return true;  // (4: 3 with every fp64 sum in LDS)
  return t.variant < 0 && n >= 12288;
}

// bodies per lane R, measured (tools/sweep_sym_sizes.py, profiles/r01_sym_R_sweep.txt): the larger R, the fewer rotations
// per pair but the fewer workgroups; the two-set kernel has NBI x splits workgroups whatever R is, so it takes R = 16
// much earlier than the half-ring all-pairs kernel
inline int sym_R(const DirectTuning& t, size_t n, bool two_sets) {
  if (t.tpl == 2 || t.tpl == 4 || t.tpl == 6 || t.tpl == 8 || t.tpl == 16 || (t.tpl == 12 && !two_sets)) return t.tpl;
  if (two_sets) return n >= 49152 ? 16 : (n >= 16384 ? 8 : 4);
  // (tools/sweep_sym_sizes.py, deterministic slots: 262,144 bodies 10.45 ms at 16 per lane against 10.89 at 8;
  // 131,072: 2.80 ms at 12 -- two workgroups per CU -- against 2.92 at 8)
  return n >= 200000 ? 16 : (n >= 100000 ? 12 : (n >= 28000 ? 8 : 6));  // (6: tools/sweep_mid.py, 12,288 bodies 0.064 vs 0.076 ms at 4)
}

// Accumulator residency RL of direct_sym_kernel: the fp64 I-side sums of a lane's first RL bodies live in LDS.  Below 8
// bodies per lane none, up to 12 all; at 16, 12 -- two workgroups per CU (tools/direct_residency_ab.py, DESIGN.md 4.1;
// N = 2^20: equal masses 155.0 -> 149.5 ms with slots, 154.7 -> 149.4 with atomics; general masses 171.0 -> 168.0 and
// 189.4 -> 165.3; tools/pair_residency_ab.py, 131,072 x 131,072: 4.93 -> 4.70 ms) -- except with tuning variant 4 and in
// the deterministic two-set form (which runs 8 by default), where every sum is in LDS.
constexpr int sym_residency(int R, int variant, bool two_sets, bool det) {
  return R >= 16 ? ((variant == 4 || (two_sets && det)) ? R : 12) : (R >= 8 ? R : 0);
}

// workgroups = blocks x splits; a split is a run of `per` 64-body chunks of the flat (partner, chunk) list of `total`
struct SymSplit { int per, splits; };
inline SymSplit sym_split(const DirectTuning& t, int total, int chunks_per_partner, int blocks, int blocks_per_cu) {
  int splits = t.splits > 0 ? t.splits : (kDirectCU * blocks_per_cu + blocks - 1) / blocks;
  if (splits < 1) splits = 1;
  int per = (total + splits - 1) / splits;
  if (per < kSymMinChunks) per = kSymMinChunks;
  if (per > chunks_per_partner)  // whole partners when there are enough
    per = (per + chunks_per_partner - 1) / chunks_per_partner * chunks_per_partner;
  return SymSplit{per, (total + per - 1) / per};
}

// all pairs of one set: NB superblocks of 256 R bodies, partner offsets 0 .. D
struct SymShape {
  int R, NB, D, per, splits;
  size_t plane;
  // slot planes of the deterministic form: D reaction slots (3 float planes) then `splits` I-side slots (3 double
  // planes), the second block 256-byte aligned; the atomic form: 3 double planes
  size_t reaction_bytes() const { return align256((size_t)D * 3 * plane * sizeof(float)); }
  size_t det_bytes() const { return reaction_bytes() + (size_t)splits * 3 * plane * sizeof(double); }
  size_t atomic_bytes() const { return 3 * plane * sizeof(double); }
};

inline SymShape sym_shape(const DirectTuning& t, size_t n, int R) {
  SymShape c;
  c.R = R;
  const int S = kDirectBlock * R;
  c.NB = (int)plan_ceil(n, S);
  c.D = c.NB / 2;
  const SymSplit sp = sym_split(t, (c.D + 1) * (S / 64), S / 64, c.NB, kSymBlocksPerCU);
  c.per = sp.per;
  c.splits = sp.splits;
  c.plane = (size_t)c.NB * S;
  return c;
}

// Two disjoint sets: NBI x splits workgroups over the NBJ partners.  The deterministic form has a shape of its own: 8
// bodies per lane and half as many workgroups per CU -- every split owns an fp64 I-side slot per body (24 B x splits x
// n_i written and read back), so fewer, longer splits pay: 131,072 x 131,072 bodies: 5.04 ms against 5.47 at 16 bodies per
// lane / 128 splits (atomics: 4.95; tools/pair_det_probe.py)
struct PairShape {
  int R, NBI, NBJ, per, splits;
  size_t plane_i, plane_j;
  bool det;
  // deterministic: `splits` fp64 I-side slots per I body (256-byte aligned), then NBI fp32 reaction slots per J body;
  // atomics: 3 double planes per set, the first block 256-byte aligned
  size_t i_bytes() const { return align256((size_t)(det ? splits : 1) * 3 * plane_i * sizeof(double)); }
  size_t j_bytes() const { return det ? (size_t)NBI * 3 * plane_j * sizeof(float) : plane_j * 3 * sizeof(double); }
  size_t bytes() const { return i_bytes() + j_bytes(); }
};

inline PairShape pair_shape(const DirectTuning& t, size_t ni, size_t nj, bool det_form) {
  PairShape c;
  c.det = det_form;
  c.R = sym_R(t, ni < nj ? ni : nj, true);
  if (det_form && t.tpl == 0 && c.R > 8) c.R = 8;
  const int S = kDirectBlock * c.R;
  c.NBI = (int)plan_ceil(ni, S);
  c.NBJ = (int)plan_ceil(nj, S);
  const SymSplit sp = sym_split(t, c.NBJ * (S / 64), S / 64, c.NBI, det_form ? kSymBlocksPerCU / 2 : kSymBlocksPerCU);
  c.per = sp.per;
  c.splits = sp.splits;
  c.plane_i = (size_t)c.NBI * S;
  c.plane_j = (size_t)c.NBJ * S;
  return c;
}

// May the deterministic form take `bytes` of slot planes?  They must fit the budget and, unless the workspace already
// holds them, a quarter of the memory that is free on the device right now (plus what the workspace would give back) --
// on a shared or smaller GPU the atomic form is the better citizen.  free_bytes == kFreeUnknown: cannot tell -- try, the
// allocation failure path falls back.  *asked (may be null) is set when the answer came from free_bytes: a caller that
// passed kFreeUnknown to spare the query then asks the device and plans again.
constexpr size_t kFreeUnknown = ~(size_t)0;
inline bool slot_budget_allows(size_t bytes, size_t budget, size_t held, size_t free_bytes, bool* asked = nullptr) {
  if (bytes > budget) return false;
  if (bytes <= held) return true;
  if (asked) *asked = true;
  if (free_bytes == kFreeUnknown) return true;
  return bytes <= (free_bytes + held) / 4;
}

// What a force call over all pairs of n bodies runs (nbody_hip_direct_forces, direct_packed with targets == sources):
// one-sided with `one`, or symmetric with the equal-mass and the general-mass shape, slot planes or atomics, and `bytes`
// of workspace.  held: bytes the workspace holds already; free_bytes: free device memory, or kFreeUnknown.
struct DirectPlan {
  bool symmetric = false;        // false: one-sided kernel (direct.hip)
  bool det = false;              // slot planes
  bool required = false;         // deterministic mode 2: without slot planes the call is refused
  bool asked_free = false;       // the budget rule got as far as free_bytes
  OneSidedPlan one{};            // !symmetric
  SymShape eq{}, gen{};          // symmetric: equal-mass / general-mass instantiation
  size_t bytes = 0;              // workspace the call needs
  size_t det_bytes_wanted = 0;   // what the slot planes would need (also when they were refused)
  int kernel() const { return symmetric ? (det ? 2 : 1) : 0; }  // (last_direct_kernel, nbody_hip_direct_info)
  // the slot planes could not be had after all: the atomic form needs 24 bytes per body
  void demote_to_atomics() { det = false, gen = eq, bytes = eq.atomic_bytes(); }
};

inline DirectPlan direct_plan(const DirectTuning& t, size_t n, float eps2, size_t held, size_t free_bytes) {
  DirectPlan p;
  // tiny softening: the guard variant of the one-sided kernel
  p.symmetric = direct_pairs_ok(eps2) && symmetric_pays(t, n);
  if (!p.symmetric) {
    p.one = one_sided_plan(t, n, n, eps2);
    p.bytes = p.one.bytes();
    return p;
  }
  p.required = t.deterministic == 2;
  p.eq = sym_shape(t, n, sym_R(t, n, false));
  p.gen = p.eq;
  if (t.deterministic) {
    // general masses at 16 bodies per lane: the slot stores push the kernel past the 256 architectural registers
    // (191 ms against 170 ms with atomics at N = 2^20); 12 bodies per lane (78 KiB of LDS = two workgroups per CU)
    // run it in 172 ms where 8 take 177 (tools/direct_det_probe.py, same box)
    SymShape gen = (kDetGenR != 16 && p.eq.R == 16 && t.tpl == 0) ? sym_shape(t, n, kDetGenR) : p.eq;
    size_t need = p.eq.det_bytes() > gen.det_bytes() ? p.eq.det_bytes() : gen.det_bytes();
    bool ok = slot_budget_allows(need, t.det_budget, held, free_bytes, &p.asked_free);
    if (!ok && gen.R != p.eq.R) {  // the general-mass shape has more slots: try with the common shape
      gen = p.eq;
      need = p.eq.det_bytes();
      ok = slot_budget_allows(need, t.det_budget, held, free_bytes, &p.asked_free);
    }
    if (ok) {
      p.det = true;
      p.gen = gen;
      p.bytes = need;
    }
    p.det_bytes_wanted = need;
  }
  if (!p.det) p.bytes = p.eq.atomic_bytes();
  return p;
}

// The two-set counterpart (nbody_hip_direct_forces_pair_packed, the sharded pair phase): the shape of the form that
// runs, and the atomic one to fall back to.
struct PairPlan {
  bool det = false, required = false, asked_free = false;
  PairShape s{}, atomics{};
  size_t det_bytes_wanted = 0;
  void demote_to_atomics() { det = false, s = atomics; }
};

inline PairPlan pair_plan(const DirectTuning& t, size_t ni, size_t nj, size_t held, size_t free_bytes) {
  PairPlan p;
  p.required = t.deterministic == 2;
  p.s = p.atomics = pair_shape(t, ni, nj, false);
  if (t.deterministic) {
    const PairShape slots = pair_shape(t, ni, nj, true);
    p.det_bytes_wanted = slots.bytes();
    p.det = slot_budget_allows(slots.bytes(), t.det_budget, held, free_bytes, &p.asked_free);
    if (p.det) p.s = slots;
  }
  return p;
}

// ---- THE BLOCK STEP (hermite_block.hip): which kernel one block step launches, and the narrow form's sizes ----
constexpr int kNarrowSources = 1024;  // sources a block of the narrow form sweeps (kBlock x kNarrowS, hermite_block_common.h)
constexpr int kNarrowTargets = 4;     // targets per block of the narrow form (kNarrowT)
// active sets smaller than this take the narrow form when the choice is automatic.  Measured on the MI355X
// (profiles/r10_hermite_block.txt): the narrow form costs about 3.3 ps per pair on top of a launch, the wide one the
// sweep of one 512-target block whatever the size of the set; at 65,536 bodies they meet at 384 targets, at 4,096 bodies
// the narrow form still leads there by 14 of 67 microseconds (it would lead up to ~1,800).
constexpr int kNarrowBelow = 384;

// direct_jerk_active_narrow_kernel: grid (splits, groups), partial arrays [splits][n_pad]; the resident form sweeps all
// bodies' rows: n_active == n
struct NarrowSizes {
  int splits, groups, n_pad;
  size_t rows() const { return (size_t)splits * n_pad; }
  size_t bytes() const { return 2 * rows() * 4 * sizeof(float); }  // the sums of a and of j
};
inline NarrowSizes narrow_sizes(size_t n, size_t n_active) {
  NarrowSizes z;
  z.splits = (int)plan_ceil(n, kNarrowSources);
  z.groups = (int)plan_ceil(n_active, kNarrowTargets);
  z.n_pad = z.groups * kNarrowTargets;
  return z;
}

// narrow_below: the handle's override (nbody_hip_hermite_block_tuning), 0 = automatic
inline bool block_takes_narrow(int narrow_below, size_t n_active, size_t n) {
  if (narrow_below > 0) return n_active < (size_t)narrow_below;
  return n_active < (size_t)kNarrowBelow && n_active < n;  // (all bodies active: the shared-step shape)
}

// scheduling: 0 host, 1 resident (required), 2 automatic: resident below resident_below bodies and up to resident_max
inline bool block_takes_resident(int scheduling, size_t n, size_t resident_below, size_t resident_max) {
  return scheduling == 1 || (scheduling == 2 && n < resident_below && n <= resident_max);
}

// a schedule read back from the device: the next tick t must lie ahead of the current one and inside the macro step of
// 2^L ticks, with a non-empty active set of at most n bodies.  The fields are what the refusal reports.
struct ScheduleFault {
  unsigned int t, was, end, n_active;
  size_t n;
  bool bad;
};
inline ScheduleFault block_schedule_check(unsigned int t, unsigned int cur_tick, int L, unsigned int n_active, size_t n) {
  const unsigned int end = 1u << L;
  return ScheduleFault{t, cur_tick, end, n_active, n, n_active == 0 || n_active > n || t <= cur_tick || t > end};
}

}  // namespace nbh
