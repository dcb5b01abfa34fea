// direct_plan_check.cpp -- the host decisions of the single-GPU Direct family (direct_plan.h) on a CPU, under
// AddressSanitizer and UBSan (make direct_plan_check): every function of the header against a restatement of the code it
// replaced (copied from direct.hip, direct_sym.hip, energy.hip, hermite_common.h, hermite_block.hip and api.hip as they
// stood before the header), field by field, over both neighbours of every threshold, every tuning
// nbody_hip_direct_tuning accepts, the three deterministic modes, budgets, free-memory answers, held workspaces and
// softenings; then the invariants of the shapes and byte counts over the same enumeration.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "direct_plan.h"

static int failures = 0;
static long long checked = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    checked++;                           \
    if (!(cond)) {                       \
      if (failures++ < 40) {             \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

// ---------------------------------------------------------------------------------------
// the code as it stood before the plan (nothing in this namespace calls into the header)
// ---------------------------------------------------------------------------------------
namespace restated {

constexpr int kBlock = 256, kNumCU = 256, TS = 256, PTS = 256;
constexpr int kSymBlocksPerCU = 16, kSymMinChunks = 4, kDetGenR = 16;
constexpr int kNarrowS = 4, kNarrowT = 4, kNarrowBelow = 384;

// the context's fields the decisions read, and the device's answer to hipMemGetInfo
struct Ctx {
  int tune_variant = -1, tune_tpl = 0, tune_splits = 0;
  int deterministic = 1;
  size_t det_budget = (size_t)24 << 30;
  size_t partial_bytes = 0;
  bool mem_info_fails = false;
  size_t mem_free = 0;
};

// direct.hip
struct Shape { int R; int splits; int src_per_split; int blocks_x; int n_tgt_pad; };
static Shape r_choose_shape(int tune_tpl, int tune_splits, size_t n_tgt, size_t n_src) {
  Shape s;
  int R = n_tgt >= 32768 ? 4 : 2;
  if (tune_tpl == 1 || tune_tpl == 2 || tune_tpl == 4) R = tune_tpl;
  s.R = R;
  s.blocks_x = (int)((n_tgt + (size_t)kBlock * R - 1) / ((size_t)kBlock * R));
  s.n_tgt_pad = s.blocks_x * kBlock * R;
  const int tiles = (int)((n_src + TS - 1) / TS);
  int want = (kNumCU * 16 + s.blocks_x - 1) / s.blocks_x;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  if (tune_splits > 0) want = tune_splits;
  if (want > tiles) want = tiles > 0 ? tiles : 1;
  const int tiles_per_split = (tiles + want - 1) / want;
  s.src_per_split = tiles_per_split * TS;
  s.splits = tiles_per_split > 0 ? (tiles + tiles_per_split - 1) / tiles_per_split : 1;
  if (s.splits < 1) s.splits = 1;
  return s;
}
// hermite_common.h (n_sources > 0: with none it divides by tiles_per_split = 0)
struct JerkShape { int R, splits, src_per_split, blocks_x, n_pad; };
static JerkShape r_jerk_shape(size_t n_targets, size_t n_sources) {
  JerkShape s;
  s.R = n_targets >= 32768 ? 4 : 2;
  s.blocks_x = (int)((n_targets + (size_t)kBlock * s.R - 1) / ((size_t)kBlock * s.R));
  s.n_pad = s.blocks_x * kBlock * s.R;
  const int tiles = (int)((n_sources + TS - 1) / TS);
  int want = (kNumCU * 16 + s.blocks_x - 1) / s.blocks_x;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  if (want > tiles) want = tiles > 0 ? tiles : 1;
  const int tiles_per_split = (tiles + want - 1) / want;
  s.src_per_split = tiles_per_split * TS;
  s.splits = (tiles + tiles_per_split - 1) / tiles_per_split;
  if (s.splits < 1) s.splits = 1;
  return s;
}
// direct_packed's variant rule: the template arguments it launches with (launched: ns > 0), or the refusal
struct Variant { bool refused, launched; int R, V; bool guard; };
static Variant r_variant(const Ctx* ctx, const Shape& s, float eps2, int ns) {
  const bool guard = eps2 < 1e-12f;
  int variant = ctx->tune_variant;
  if (variant < 0 || variant > 2) variant = s.R >= 2 ? 1 : 0;
  if (guard && variant == 1) variant = 0;
  Variant v{false, ns > 0, 0, 0, guard};
  auto dispatch = [&](int RR) {
    if (guard) {
      if (variant == 2) { v.R = RR; v.V = 2; }
      else { v.R = RR; v.V = 0; }
    } else if (variant == 1) {
      v.R = RR < 2 ? 2 : RR; v.V = 1;
    } else if (variant == 2) {
      v.R = RR; v.V = 2;
    } else {
      v.R = RR; v.V = 0;
    }
  };
  if (ns > 0) {
    if (s.R == 4) dispatch(4);
    else if (s.R == 2) dispatch(2);
    else {
      if (variant == 1) { v.refused = true; return v; }
      dispatch(1);
    }
  }
  return v;
}

// energy.hip: nbody_hip_potential_energy_f64, nbody_hip_energies_packed, nbody_hip_direct_potential
struct Pot { int bx, splits, src_per_split; };
static Pot r_potential_energy(size_t n) {
  const int bx = (int)((n + kBlock - 1) / kBlock);
  const int tiles = (int)((n + PTS - 1) / PTS);
  int splits = (kNumCU * 8 + bx - 1) / bx;
  if (splits > 64) splits = 64;
  if (splits > tiles) splits = tiles;
  if (splits < 1) splits = 1;
  const int tiles_per_split = (tiles + splits - 1) / splits;
  splits = (tiles + tiles_per_split - 1) / tiles_per_split;
  return Pot{bx, splits, tiles_per_split * PTS};
}
static Pot r_energies_packed(size_t n_targets, size_t n_sources) {
  const int bx = (int)((n_targets + kBlock - 1) / kBlock);
  const int tiles = (int)((n_sources + PTS - 1) / PTS);
  int splits = (kNumCU * 8 + bx - 1) / bx;
  if (splits > 64) splits = 64;
  if (splits > tiles) splits = tiles;
  if (splits < 1) splits = 1;
  const int tiles_per_split = tiles > 0 ? (tiles + splits - 1) / splits : 1;
  splits = tiles > 0 ? (tiles + tiles_per_split - 1) / tiles_per_split : 0;
  return Pot{bx, splits, tiles_per_split * PTS};
}
static Pot r_direct_potential(size_t n) {
  const int bx = (int)((n + kBlock - 1) / kBlock);
  const int tiles = (int)((n + PTS - 1) / PTS);
  int splits = (kNumCU * 8 + bx - 1) / bx;
  if (splits > 64) splits = 64;
  if (splits > tiles) splits = tiles;
  if (splits < 1) splits = 1;
  const int tiles_per_split = (tiles + splits - 1) / splits;
  splits = (tiles + tiles_per_split - 1) / tiles_per_split;
  return Pot{bx, splits, tiles_per_split * PTS};
}

// direct_sym.hip
static bool r_symmetric_pays(const Ctx* ctx, size_t n) {
  if (ctx->tune_variant == 3 || ctx->tune_variant == 4) return true;
  return ctx->tune_variant < 0 && n >= 12288;
}
static int r_sym_R(const Ctx* ctx, size_t n, bool two_sets) {
  if (ctx->tune_tpl == 2 || ctx->tune_tpl == 4 || ctx->tune_tpl == 6 || ctx->tune_tpl == 8 ||
      ctx->tune_tpl == 16 || (ctx->tune_tpl == 12 && !two_sets))
    return ctx->tune_tpl;
  if (two_sets) return n >= 49152 ? 16 : (n >= 16384 ? 8 : 4);
  return n >= 200000 ? 16 : (n >= 100000 ? 12 : (n >= 28000 ? 8 : 6));
}
static size_t r_align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct SymShape {
  int R, NB, D, per, splits;
  size_t plane;
  size_t reaction_bytes() const { return r_align256((size_t)D * 3 * plane * sizeof(float)); }
  size_t det_bytes() const { return reaction_bytes() + (size_t)splits * 3 * plane * sizeof(double); }
  size_t atomic_bytes() const { return 3 * plane * sizeof(double); }
};
static SymShape r_sym_shape(const Ctx* ctx, size_t n, int R) {
  SymShape c;
  c.R = R;
  const int S = kBlock * R;
  c.NB = (int)((n + S - 1) / S);
  c.D = c.NB / 2;
  const int total = (c.D + 1) * (S / 64);
  int splits = ctx->tune_splits > 0 ? ctx->tune_splits : (kNumCU * kSymBlocksPerCU + c.NB - 1) / c.NB;
  if (splits < 1) splits = 1;
  int per = (total + splits - 1) / splits;
  if (per < kSymMinChunks) per = kSymMinChunks;
  if (per > S / 64) per = (per + S / 64 - 1) / (S / 64) * (S / 64);
  c.per = per;
  c.splits = (total + per - 1) / per;
  c.plane = (size_t)c.NB * S;
  return c;
}
static bool r_hipMemGetInfo(const Ctx* ctx, size_t* free_b) {
  if (ctx->mem_info_fails) return false;
  *free_b = ctx->mem_free;
  return true;
}
static bool r_det_budget_allows(const Ctx* ctx, size_t bytes) {
  if (bytes > ctx->det_budget) return false;
  if (bytes <= ctx->partial_bytes) return true;
  size_t free_b = 0;
  if (!r_hipMemGetInfo(ctx, &free_b)) return true;
  return bytes <= (free_b + ctx->partial_bytes) / 4;
}
struct DirectPlan {
  bool symmetric = false, det = false;
  SymShape eq{}, gen{};
  size_t bytes = 0, det_bytes_wanted = 0;
};
static DirectPlan r_direct_plan(const Ctx* ctx, size_t n, bool query_device) {
  DirectPlan p;
  p.symmetric = r_symmetric_pays(ctx, n);
  p.eq = r_sym_shape(ctx, n, r_sym_R(ctx, n, false));
  p.gen = p.eq;
  p.det = false;
  p.bytes = 0;
  if (!p.symmetric) return p;
  if (ctx->deterministic) {
    SymShape gen = (kDetGenR != 16 && p.eq.R == 16 && ctx->tune_tpl == 0) ? r_sym_shape(ctx, n, kDetGenR) : p.eq;
    size_t need = p.eq.det_bytes() > gen.det_bytes() ? p.eq.det_bytes() : gen.det_bytes();
    bool ok = query_device ? r_det_budget_allows(ctx, need) : need <= ctx->det_budget;
    if (!ok && gen.R != p.eq.R) {
      gen = p.eq;
      need = p.eq.det_bytes();
      ok = query_device ? r_det_budget_allows(ctx, need) : need <= ctx->det_budget;
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
// api.hip, nbody_hip_direct_info: the plan, patched for tiny softening
static DirectPlan r_info_plan(const Ctx* ctx, size_t n, float eps2, bool dev) {
  DirectPlan p = r_direct_plan(ctx, n, dev);
  if (!(eps2 >= 1e-12f)) p.symmetric = false;
  return p;
}
// direct_packed with targets == sources: the gate in front of direct_symmetric
static bool r_force_is_symmetric(const Ctx* ctx, size_t n, float eps2) { return eps2 >= 1e-12f && r_symmetric_pays(ctx, n); }
// direct_symmetric after a failed reservation
static void r_all_pairs_fallback(DirectPlan& plan) {
  plan.det = false;
  plan.gen = plan.eq;
  plan.bytes = plan.eq.atomic_bytes();
}
// residency at 16 bodies per lane: sym_RL, kSymRL16 with launch_all_pairs_R, kPairRL16 with launch_sym
constexpr int r_sym_RL(int R) { return R >= 16 ? 12 : (R >= 8 ? R : 0); }
static int r_all_pairs_RL(const Ctx* ctx, int R) {
  if (R == 16) return ctx->tune_variant == 4 ? 16 : 12;
  return r_sym_RL(R);
}
static int r_pair_RL(const Ctx* ctx, int R, bool DET) {
  if (R == 16 && !DET) {
    if (ctx->tune_variant != 4) return 12;
  }
  return R >= 8 ? R : 0;
}

// direct_symmetric_pair: the shape lambda, then the call's decisions up to the reservation and after a failed one
struct Pair {
  int R = 0, NBI = 0, NBJ = 0, per = 0, splits = 0;
  size_t plane_i = 0, plane_j = 0, det_i = 0, det_j = 0;
  bool det = false, refused = false;
  size_t refused_bytes = 0, reserve = 0, accj_offset = 0;
};
static void r_pair_shape(const Ctx* ctx, size_t ni, size_t nj, bool det_form, Pair& o) {
  const size_t nmin = ni < nj ? ni : nj;
  o.R = r_sym_R(ctx, nmin, true);
  if (det_form && ctx->tune_tpl == 0 && o.R > 8) o.R = 8;
  const int S = kBlock * o.R;
  o.NBI = (int)((ni + S - 1) / S);
  o.NBJ = (int)((nj + S - 1) / S);
  const int total = o.NBJ * (S / 64);
  const int per_cu = det_form ? kSymBlocksPerCU / 2 : kSymBlocksPerCU;
  o.splits = ctx->tune_splits > 0 ? ctx->tune_splits : (kNumCU * per_cu + o.NBI - 1) / o.NBI;
  if (o.splits < 1) o.splits = 1;
  o.per = (total + o.splits - 1) / o.splits;
  if (o.per < kSymMinChunks) o.per = kSymMinChunks;
  if (o.per > S / 64) o.per = (o.per + S / 64 - 1) / (S / 64) * (S / 64);
  o.splits = (total + o.per - 1) / o.per;
  o.plane_i = (size_t)o.NBI * S;
  o.plane_j = (size_t)o.NBJ * S;
  o.det_i = r_align256((size_t)o.splits * 3 * o.plane_i * sizeof(double));
  o.det_j = (size_t)o.NBI * 3 * o.plane_j * sizeof(float);
}
static Pair r_pair_call(const Ctx* ctx, size_t ni, size_t nj, bool reservation_fails) {
  Pair o;
  r_pair_shape(ctx, ni, nj, ctx->deterministic != 0, o);
  bool det = ctx->deterministic != 0 && r_det_budget_allows(ctx, o.det_i + o.det_j);
  if (ctx->deterministic == 2 && !det) {
    o.refused = true;
    o.refused_bytes = o.det_i + o.det_j;
    return o;
  }
  if (!det) r_pair_shape(ctx, ni, nj, false, o);
  size_t bi = r_align256(o.plane_i * 3 * sizeof(double)), bj = o.plane_j * 3 * sizeof(double);
  o.reserve = det ? o.det_i + o.det_j : bi + bj;
  if (reservation_fails && det && ctx->deterministic != 2) {
    det = false;
    r_pair_shape(ctx, ni, nj, false, o);
    bi = r_align256(o.plane_i * 3 * sizeof(double));
    bj = o.plane_j * 3 * sizeof(double);
    o.reserve = bi + bj;
  }
  o.det = det;
  o.accj_offset = det ? o.det_i : bi;
  return o;
}

// hermite_block.hip: block_one_step's narrow sizes, block_resident_run's, the predicates and the range check
struct Narrow { size_t splits, groups, n_pad; };
static Narrow r_narrow_step(size_t n, unsigned int n_active) {
  const int splits = (int)((n + (size_t)kBlock * kNarrowS - 1) / ((size_t)kBlock * kNarrowS));
  const int groups = (int)((n_active + kNarrowT - 1) / kNarrowT);
  const int n_pad = groups * kNarrowT;
  return Narrow{(size_t)splits, (size_t)groups, (size_t)n_pad};
}
static Narrow r_narrow_resident(size_t n, size_t* want_partial) {
  const size_t splits = (n + (size_t)kBlock * kNarrowS - 1) / ((size_t)kBlock * kNarrowS);
  const size_t n_pad = (n + kNarrowT - 1) / kNarrowT * kNarrowT;
  *want_partial = 2 * splits * n_pad * 16;
  return Narrow{splits, n_pad / kNarrowT, n_pad};
}
static bool r_block_takes_narrow(int narrow_below, size_t n_active, size_t n) {
  if (narrow_below > 0) return n_active < (size_t)narrow_below;
  return n_active < (size_t)kNarrowBelow && n_active < n;
}
static int r_block_form(int scheduling, size_t count, size_t resident_below, size_t resident_max) {
  return scheduling == 1 || (scheduling == 2 && count < resident_below && count <= resident_max) ? 1 : 0;
}
static bool r_schedule_bad(unsigned int t, unsigned int cur_tick, int L, unsigned int n_active, size_t n,
                           unsigned int* end_out) {
  const unsigned int end = 1u << L;
  *end_out = end;
  return n_active == 0 || n_active > n || t <= cur_tick || t > end;
}

}  // namespace restated

using namespace nbh;
using restated::Ctx;

static DirectTuning tuning_of(const Ctx& c) {
  DirectTuning t;
  t.variant = c.tune_variant;
  t.tpl = c.tune_tpl;
  t.splits = c.tune_splits;
  t.deterministic = c.deterministic;
  t.det_budget = c.det_budget;
  return t;
}
static size_t free_of(const Ctx& c) { return c.mem_info_fails ? kFreeUnknown : c.mem_free; }

static bool same(const SymShape& a, const restated::SymShape& b) {
  return a.R == b.R && a.NB == b.NB && a.D == b.D && a.per == b.per && a.splits == b.splits && a.plane == b.plane &&
         a.reaction_bytes() == b.reaction_bytes() && a.det_bytes() == b.det_bytes() && a.atomic_bytes() == b.atomic_bytes();
}
static bool same(const SymShape& a, const SymShape& b) {
  return a.R == b.R && a.NB == b.NB && a.D == b.D && a.per == b.per && a.splits == b.splits && a.plane == b.plane;
}

static const size_t kCounts[] = {1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 12287, 12288, 16383, 16384, 27999, 28000,
                                 32767, 32768, 49151, 49152, 99999, 100000, 199999, 200000, (size_t)1 << 20, (size_t)1 << 22,
                                 ((size_t)1 << 30) - 1};
static const int kVariants[] = {-1, 0, 1, 2, 3, 4}, kTpl[] = {0, 1, 2, 4, 6, 8, 12, 16}, kSplits[] = {0, 1, 3, 5, 64, 4096};
static const float kEps2[] = {0.0f, 9.9e-13f, 1e-12f, 1e-6f};
static const size_t kBudgets[] = {1, (size_t)1 << 20, (size_t)24 << 30};

// one-sided shapes, the variant rule and the potential splits
static void check_one_sided(const Ctx& c) {
  const DirectTuning t = tuning_of(c);
  static const size_t kSources[] = {0, 1, 256, 257, 12288, 32768, 100000, (size_t)1 << 20, ((size_t)1 << 30) - 1};
  for (size_t nt : kCounts)
    for (size_t ns : kSources) {
      const restated::Shape o = restated::r_choose_shape(c.tune_tpl, c.tune_splits, nt, ns);
      const OneSidedShape s = one_sided_shape(t, nt, ns);
      EXPECT(s.R == o.R && s.splits == o.splits && s.src_per_split == o.src_per_split && s.blocks_x == o.blocks_x &&
                 s.n_pad == o.n_tgt_pad && s.rows() == (size_t)o.splits * o.n_tgt_pad,
             "choose_shape nt %zu ns %zu tpl %d splits %d", nt, ns, c.tune_tpl, c.tune_splits);
      EXPECT(s.n_pad % (256 * s.R) == 0 && (size_t)s.n_pad >= nt && s.splits >= 1, "one-sided padding nt %zu", nt);
      EXPECT(ns == 0 || (size_t)s.splits * s.src_per_split >= ns, "one-sided splits cover nt %zu ns %zu", nt, ns);
      for (float e : kEps2) {
        const restated::Variant v = restated::r_variant(&c, o, e, (int)ns);
        const OneSidedPlan p = one_sided_plan(t, nt, ns, e);
        // what direct_packed makes of the plan: refused, or (with sources) direct_kernel<R, V, guard>
        const int R = (p.variant == 1 && p.s.R < 2) ? 2 : p.s.R;
        EXPECT(p.refused == v.refused && p.guard == v.guard && (v.refused || !v.launched || (R == v.R && p.variant == v.V)) &&
                   !(p.guard && p.variant == 1) && p.bytes() == (size_t)o.splits * o.n_tgt_pad * 16,
               "variant rule nt %zu ns %zu eps2 %g variant %d tpl %d", nt, ns, (double)e, c.tune_variant, c.tune_tpl);
      }
    }
}
static void check_untuned() {
  std::printf("jerk_shape with no sources divided by zero tiles per split: the header is held to choose_shape's answer there\n");
  for (size_t nt : kCounts)
    for (size_t ns : kCounts) {
      const restated::JerkShape o = restated::r_jerk_shape(nt, ns);
      const OneSidedShape s = one_sided_shape(no_tuning(), nt, ns);
      EXPECT(s.R == o.R && s.splits == o.splits && s.src_per_split == o.src_per_split && s.blocks_x == o.blocks_x &&
                 s.n_pad == o.n_pad, "jerk_shape nt %zu ns %zu", nt, ns);
      const restated::Pot a = restated::r_energies_packed(nt, ns);
      const PotentialSplits p = potential_splits(nt, ns);
      EXPECT(p.bx == a.bx && p.splits == a.splits && p.src_per_split == a.src_per_split, "energies_packed %zu %zu", nt, ns);
      EXPECT(p.splits >= 1 && (size_t)p.splits * p.src_per_split >= ns, "potential splits cover %zu %zu", nt, ns);
    }
  for (size_t n : kCounts) {
    const restated::Pot a = restated::r_potential_energy(n), b = restated::r_direct_potential(n);
    const PotentialSplits p = potential_splits(n, n);
    EXPECT(p.bx == a.bx && p.splits == a.splits && p.src_per_split == a.src_per_split && p.bx == b.bx &&
               p.splits == b.splits && p.src_per_split == b.src_per_split, "potential splits n %zu", n);
    const restated::Shape z = restated::r_choose_shape(0, 0, n, 0);
    const OneSidedShape s = one_sided_shape(no_tuning(), n, 0);
    EXPECT(s.splits == z.splits && s.splits == 1 && s.src_per_split == 0 && s.n_pad == z.n_tgt_pad, "no sources, n %zu", n);
    EXPECT(potential_splits(n, 0).splits == 0 && restated::r_energies_packed(n, 0).splits == 0, "no sources: no splits");
  }
  for (float e : kEps2)
    EXPECT(direct_guard(e) == (e < 1e-12f) && direct_pairs_ok(e) == (e >= 1e-12f) && direct_guard(e) != direct_pairs_ok(e),
           "guard rule %g", (double)e);
  const float nan = __builtin_nanf("");
  EXPECT(!direct_guard(nan) && !direct_pairs_ok(nan), "a NaN is neither guarded nor fit for pairs");
}

static void check_sym_invariants(const SymShape& s, size_t n) {
  const int chunks = (s.D + 1) * (256 * s.R / 64);
  EXPECT(s.splits >= 1 && s.per >= kSymMinChunks && (long long)s.splits * s.per >= chunks, "sym splits n %zu R %d", n, s.R);
  EXPECT(s.plane % (256 * (size_t)s.R) == 0 && s.plane >= n, "sym plane n %zu R %d", n, s.R);
  EXPECT(s.reaction_bytes() % 256 == 0 && s.reaction_bytes() >= (size_t)s.D * 3 * s.plane * 4 &&
             s.reaction_bytes() < (size_t)s.D * 3 * s.plane * 4 + 256 &&
             s.det_bytes() == s.reaction_bytes() + (size_t)s.splits * 3 * s.plane * 8 && s.atomic_bytes() == 24 * s.plane,
         "sym bytes n %zu R %d", n, s.R);
}

// the all-pairs plan: shapes, residency, budget rule, plan, info, fallback
static void check_all_pairs(Ctx c) {
  for (size_t n : kCounts) {
    c.partial_bytes = 0;
    c.mem_info_fails = true;
    const DirectTuning t0 = tuning_of(c);
    EXPECT(symmetric_pays(t0, n) == restated::r_symmetric_pays(&c, n), "symmetric_pays n %zu", n);
    const int R = sym_R(t0, n, false);
    EXPECT(R == restated::r_sym_R(&c, n, false) && sym_R(t0, n, true) == restated::r_sym_R(&c, n, true), "sym_R n %zu", n);
    const SymShape eq = sym_shape(t0, n, R);
    EXPECT(same(eq, restated::r_sym_shape(&c, n, R)), "sym_shape n %zu R %d", n, R);
    check_sym_invariants(eq, n);
    for (int r : {2, 4, 6, 8, 12, 16})
      for (int det = 0; det < 2; det++) {
        EXPECT(sym_residency(r, c.tune_variant, false, det != 0) == restated::r_all_pairs_RL(&c, r), "residency R %d", r);
        if (r != 12) EXPECT(sym_residency(r, c.tune_variant, true, det != 0) == restated::r_pair_RL(&c, r, det != 0), "pair residency R %d", r);
        EXPECT(sym_residency(r, -1, false, false) == restated::r_sym_RL(r), "default residency R %d", r);
      }
    const size_t need = eq.det_bytes();
    const size_t frees[] = {kFreeUnknown, 0, need - 1, 4 * need}, helds[] = {0, need - 1, need};
    for (size_t held : helds)
      for (size_t fr : frees) {
        c.partial_bytes = held;
        c.mem_info_fails = fr == kFreeUnknown;
        c.mem_free = fr == kFreeUnknown ? 0 : fr;
        const DirectTuning t = tuning_of(c);
        for (size_t bytes : {need - 1, need, need + 1, (size_t)1, c.det_budget, c.det_budget + 1})
          EXPECT(slot_budget_allows(bytes, t.det_budget, held, free_of(c)) == restated::r_det_budget_allows(&c, bytes),
                 "budget rule %zu bytes, budget %zu, held %zu, free %zu", bytes, c.det_budget, held, fr);
        for (float e : kEps2) {
          const DirectPlan p = direct_plan(t, n, e, held, free_of(c));
          // the call: direct_packed's gate, then direct_symmetric's plan; the info call: the plan, patched
          const bool sym = restated::r_force_is_symmetric(&c, n, e);
          const restated::DirectPlan o = restated::r_direct_plan(&c, n, true), i = restated::r_info_plan(&c, n, e, true);
          EXPECT(p.symmetric == sym && p.symmetric == i.symmetric, "plan.symmetric n %zu eps2 %g", n, (double)e);
          EXPECT(p.kernel() == (i.symmetric ? (i.det ? 2 : 1) : 0), "plan.kernel n %zu", n);
          if (!sym) {
            const OneSidedPlan q = one_sided_plan(t, n, n, e);
            EXPECT(p.one.s.R == q.s.R && p.one.s.splits == q.s.splits && p.one.s.n_pad == q.s.n_pad && p.one.variant == q.variant &&
                       p.one.guard == q.guard && p.one.refused == q.refused && p.bytes == q.bytes() && !p.det,
                   "the one-sided plan of an all-pairs call n %zu", n);
            continue;
          }
          EXPECT(p.det == o.det && same(p.eq, o.eq) && same(p.gen, o.gen) && p.bytes == o.bytes &&
                     p.det_bytes_wanted == o.det_bytes_wanted && p.required == (c.deterministic == 2),
                 "direct_plan n %zu det %d budget %zu held %zu free %zu", n, c.deterministic, c.det_budget, held, fr);
          EXPECT(p.bytes == (p.det ? (p.eq.det_bytes() > p.gen.det_bytes() ? p.eq.det_bytes() : p.gen.det_bytes())
                                   : p.eq.atomic_bytes()), "plan bytes n %zu", n);
          // asking the device only when the rule gets that far gives the plan that asking always gives
          DirectPlan lazy = direct_plan(t, n, e, held, kFreeUnknown);
          if (lazy.asked_free) lazy = direct_plan(t, n, e, held, free_of(c));
          EXPECT(lazy.det == p.det && lazy.bytes == p.bytes && same(lazy.gen, p.gen), "lazy query n %zu", n);
          // without a device (the info call on a NULL context): the budget alone
          const restated::DirectPlan nodev = restated::r_info_plan(&c, n, e, false);
          const DirectPlan pn = direct_plan(t, n, e, held, kFreeUnknown);
          if (held == 0) EXPECT(pn.det == nodev.det && pn.bytes == nodev.bytes && pn.det_bytes_wanted == nodev.det_bytes_wanted, "no device n %zu", n);
          // the fallback after a failed reservation, and the plan of deterministic mode 0
          DirectPlan d = p;
          restated::DirectPlan od = o;
          d.demote_to_atomics();
          restated::r_all_pairs_fallback(od);
          DirectTuning ta = t;
          ta.deterministic = 0;
          const DirectPlan a = direct_plan(ta, n, e, held, free_of(c));
          EXPECT(d.det == od.det && same(d.gen, od.gen) && same(d.eq, od.eq) && d.bytes == od.bytes, "all-pairs fallback n %zu", n);
          EXPECT(d.kernel() == a.kernel() && same(d.eq, a.eq) && same(d.gen, a.gen) && d.bytes == a.bytes, "demoted plan n %zu", n);
        }
      }
  }
}

// the two-set plan
static void check_pairs(Ctx c) {
  static const size_t kSets[][2] = {{1, 1}, {255, 257}, {1024, 16383}, {16383, 16384}, {16384, 16383}, {16384, 49151},
                                    {49151, 49152}, {49152, 49151}, {49152, 200000}, {100000, 12288}, {131072, 131072},
                                    {(size_t)1 << 20, 1}, {1, (size_t)1 << 20}, {(size_t)1 << 20, ((size_t)1 << 20) + 1}};
  for (const auto& set : kSets) {
    const size_t ni = set[0], nj = set[1];
    restated::Pair probe;
    restated::r_pair_shape(&c, ni, nj, c.deterministic != 0, probe);
    const size_t need = probe.det_i + probe.det_j;
    const size_t frees[] = {kFreeUnknown, 0, need - 1, 4 * need}, helds[] = {0, need - 1, need};
    for (size_t held : helds)
      for (size_t fr : frees) {
        c.partial_bytes = held;
        c.mem_info_fails = fr == kFreeUnknown;
        c.mem_free = fr == kFreeUnknown ? 0 : fr;
        const DirectTuning t = tuning_of(c);
        for (int det_form = 0; det_form < 2; det_form++) {
          restated::Pair o;
          restated::r_pair_shape(&c, ni, nj, det_form != 0, o);
          const PairShape s = pair_shape(t, ni, nj, det_form != 0);
          EXPECT(s.R == o.R && s.NBI == o.NBI && s.NBJ == o.NBJ && s.per == o.per && s.splits == o.splits &&
                     s.plane_i == o.plane_i && s.plane_j == o.plane_j, "pair shape %zu x %zu det %d", ni, nj, det_form);
          if (det_form) EXPECT(s.i_bytes() == o.det_i && s.j_bytes() == o.det_j, "pair slot bytes %zu x %zu", ni, nj);
          EXPECT(s.bytes() == s.i_bytes() + s.j_bytes() && s.i_bytes() % 256 == 0, "pair bytes %zu x %zu", ni, nj);
          EXPECT(s.splits >= 1 && s.per >= kSymMinChunks && (long long)s.splits * s.per >= (long long)s.NBJ * (256 * s.R / 64) &&
                     s.plane_i % (256 * (size_t)s.R) == 0 && s.plane_i >= ni && s.plane_j % (256 * (size_t)s.R) == 0 && s.plane_j >= nj,
                 "pair invariants %zu x %zu", ni, nj);
        }
        for (int fails = 0; fails < 2; fails++) {
          const restated::Pair o = restated::r_pair_call(&c, ni, nj, fails != 0);
          PairPlan p = pair_plan(t, ni, nj, held, free_of(c));
          // what direct_symmetric_pair makes of the plan
          const bool refused = p.required && !p.det;
          EXPECT(refused == o.refused && (!refused || p.det_bytes_wanted == o.refused_bytes), "pair refusal %zu x %zu", ni, nj);
          if (refused) continue;
          if (fails && p.det && !p.required) p.demote_to_atomics();
          EXPECT(p.det == o.det && p.s.det == o.det && p.s.R == o.R && p.s.NBI == o.NBI && p.s.NBJ == o.NBJ && p.s.per == o.per &&
                     p.s.splits == o.splits && p.s.plane_i == o.plane_i && p.s.plane_j == o.plane_j &&
                     p.s.i_bytes() == o.accj_offset && p.s.bytes() == o.reserve,
                 "pair call %zu x %zu det %d held %zu free %zu fails %d", ni, nj, c.deterministic, held, fr, fails);
          if (fails && !p.required) {
            DirectTuning ta = t;
            ta.deterministic = 0;
            const PairPlan a = pair_plan(ta, ni, nj, held, free_of(c));
            EXPECT(!p.det && a.s.R == p.s.R && a.s.splits == p.s.splits && a.s.per == p.s.per && a.s.bytes() == p.s.bytes() &&
                       a.s.det == p.s.det, "demoted pair plan %zu x %zu", ni, nj);
          }
        }
      }
  }
}

static void check_block_step() {
  for (size_t n : kCounts) {
    size_t want = 0;
    const restated::Narrow r = restated::r_narrow_resident(n, &want);
    const NarrowSizes zr = narrow_sizes(n, n);
    EXPECT((size_t)zr.splits == r.splits && (size_t)zr.n_pad == r.n_pad && zr.bytes() == want && zr.rows() == r.splits * r.n_pad,
           "resident sizes n %zu", n);
    for (size_t na : kCounts) {
      if (na > n) continue;
      const restated::Narrow o = restated::r_narrow_step(n, (unsigned int)na);
      const NarrowSizes z = narrow_sizes(n, na);
      EXPECT((size_t)z.splits == o.splits && (size_t)z.groups == o.groups && (size_t)z.n_pad == o.n_pad &&
                 z.bytes() == (size_t)2 * o.splits * o.n_pad * 16, "narrow sizes n %zu active %zu", n, na);
      EXPECT(z.n_pad % 4 == 0 && (size_t)z.n_pad >= na && (size_t)z.splits * 1024 >= n, "narrow padding n %zu active %zu", n, na);
      for (int below : {0, 1, 383, 384, 385, 4096})
        EXPECT(block_takes_narrow(below, na, n) == restated::r_block_takes_narrow(below, na, n), "takes narrow %d %zu %zu", below, na, n);
    }
    for (int sched = 0; sched < 3; sched++)
      for (size_t below : {(size_t)0, (size_t)1024, (size_t)8192})
        EXPECT((block_takes_resident(sched, n, below, 4096) ? 1 : 0) == restated::r_block_form(sched, n, below, 4096),
               "takes resident %d n %zu below %zu", sched, n, below);
  }
  EXPECT(kNarrowBelow == restated::kNarrowBelow, "narrow crossover");
  for (int L : {0, 1, 16, 20})
    for (unsigned int cur : {0u, 1u, (1u << L) - 1u})
      for (unsigned int t : {0u, 1u, 2u, (1u << L) - 1u, 1u << L, (1u << L) + 1u})
        for (unsigned int na : {0u, 1u, 512u, 513u})
          for (size_t n : {(size_t)1, (size_t)512}) {
            unsigned int end = 0;
            const bool bad = restated::r_schedule_bad(t, cur, L, na, n, &end);
            const ScheduleFault f = block_schedule_check(t, cur, L, na, n);
            EXPECT(f.bad == bad && f.t == t && f.was == cur && f.end == end && f.n_active == na && f.n == n, "schedule check");
          }
}

int main() {
  check_untuned();
  check_block_step();
  for (int variant : kVariants)
    for (int tpl : kTpl)
      for (int splits : kSplits) {
        Ctx c;
        c.tune_variant = variant;
        c.tune_tpl = tpl;
        c.tune_splits = splits;
        check_one_sided(c);
        for (int det = 0; det < 3; det++)
          for (size_t budget : kBudgets) {
            c.deterministic = det;
            c.det_budget = budget;
            check_all_pairs(c);
            check_pairs(c);
          }
      }
  if (failures) {
    std::printf("direct_plan_check: %d FAILED of %lld\n", failures, checked);
    return 1;
  }
  std::printf("direct_plan_check: ok (%lld comparisons)\n", checked);
  return 0;
}
