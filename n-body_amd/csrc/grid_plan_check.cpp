// grid_plan_check.cpp -- the host decisions of the spatial hash (grid_plan.h) on a CPU, under AddressSanitizer and UBSan
// (make grid_plan_check): the force plan against a statement-by-statement restatement of the three if-chains and of
// launch_cell_forces as spatial_hash.hip carried them, the start-array plan against the block of grid_build_packed it
// replaces, the grid record, the key bits and the size functions against the expressions they replace, and the array
// replacement over the grid's tables with an allocator that fails at every position.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "grid_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
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

// ---------------------------------------------------------------------------------------
// what a force call did, statement by statement, before the plan existed.  The ONE difference to that code: where it
// read the handle's cell size (of the NEXT build) it reads `cell` here, which the cases set to the cell size AS BUILT.
// ---------------------------------------------------------------------------------------
struct Handle {  // the fields of nbody_hip_grid the force path read
  int tune_kernel;
  bool lb_valid;
  long long lb_base, lb_count;
  GridInfo info;
  size_t built_count;
  float cell;
  double filter_from_inside;
  int split_cnt, use_units;
  bool mapped;
  int hint_words[8];
  unsigned stat_tick;
};

struct Did {
  int err = 0;     // 1 "grid too large", 2 "needs the target grid"
  int kernel = 0;  // 0 nothing, 1 cell runs, 2 two bodies per lane, 3 lane per body, 4 ... split + wave per crowded cell,
                   // 5 wave per cell, 6 two-phase, 7 probe
  bool guard = false, strict = false, units = false, filter = false;
  int R = 0;
  long long c0 = 0, c1 = 0;
  bool list = false, bodies = false, pair_items = false, exported = false;
  int chunk = 0, min_cnt = 0;
  int per_xcd = 0;
  unsigned grid = 0, block = 0, blocks = 0;
  int W = 0;
  unsigned g3[3] = {0, 0, 0};
  long long bound = 0;  // of a unit-form launch
};

static int restated_per_xcd(int hint, long long bound, long long first) {
  long long est = hint > 0 ? (long long)hint + hint / 64 + 64 : first;
  if (est > bound) est = bound;
  long long blocks = (est + 4 * 4 - 1) / (4 * 4);
  if (blocks < 8) blocks = 8;
  return (int)((blocks + 7) / 8);
}

static void restated_list(Did& d, int chunk, int min_cnt = 1, bool bodies = false, bool pair_items = false) {
  d.list = true; d.chunk = chunk; d.min_cnt = min_cnt; d.bodies = bodies; d.pair_items = pair_items;
}

// launch_cell_forces(ctx, tv, sv, gx, gy, gz, cell_first, cell_end, kern, guard, ..., gt, hint_slot) [prebuilt: always null]
static void restated_cell_forces(Did& d, long long cell_first, long long cell_end, int kern, bool guard, Handle* gt, int hint_slot) {
  d.c0 = cell_first; d.c1 = cell_end; d.guard = guard;
  if (cell_end <= cell_first) return;
  const unsigned cblock = 64 * 1;
  auto cgrid = [](int per_xcd) { return (unsigned)(per_xcd * 8 * (4 / 1)); };
  if (kern == 10 && (guard || cell_end - cell_first >= 0x7fffffffLL)) kern = 8;
  if (kern == 10) {
    if (!gt) { d.err = 2; d.kernel = 2; return; }
    restated_list(d, 128, 0x7fffffff, true, true);
    d.blocks = (unsigned)((gt->built_count + 256 - 1) / 256);
    d.kernel = 2;
    return;
  }
  if (kern == 8 || kern == 9) {
    if (!gt) { d.err = 2; d.kernel = 3; return; }
    const bool split = kern == 9 && cell_end - cell_first < 0x7fffffffLL;
    d.blocks = (unsigned)((gt->built_count + 256 - 1) / 256);
    if (split) restated_list(d, 128, gt->split_cnt, true);
    d.kernel = 3;
    if (!split) return;
    const bool uhint = gt->mapped;
    const int hint = uhint ? gt->hint_words[4 * hint_slot] : 0;
    const long long bound = (long long)gt->built_count / gt->split_cnt + (long long)gt->built_count / 128 + 1;
    const int uper = restated_per_xcd(hint, bound, 4096);
    d.kernel = 4; d.R = 2; d.units = true; d.filter = false;
    d.per_xcd = uper; d.grid = cgrid(uper); d.block = cblock; d.bound = bound;
    return;
  }
  const long long nblk = (cell_end - cell_first + 4 * 4 - 1) / (4 * 4);
  int per_xcd = (int)((nblk + 7) / 8);
  const bool can_list = gt && gt->use_units && kern != 5 && cell_end - cell_first < 0x7fffffffLL;
  bool by_units = false;
  const int R = (kern == 2 || kern == 7) ? 1 : (kern == 4 ? 4 : 2);
  if (can_list) {
    const size_t nb = gt->built_count;
    const long long cells = cell_end - cell_first;
    const bool uhint = gt->mapped;
    const int hint = uhint ? gt->hint_words[4 * hint_slot] : 0, crowd = uhint ? gt->hint_words[4 * hint_slot + 1] : 0;
    by_units = gt->use_units == 2 || (hint > 0 && (crowd > 64 || (long long)hint * 10 < cells * 9));
    if (by_units || (uhint && (gt->stat_tick++ & 7) == 0)) {
      restated_list(d, 64 * R);
      if (!by_units) d.exported = true;
    }
    if (by_units) {
      const long long bound = (long long)(cells < (long long)nb ? cells : (long long)nb) + (long long)(nb / (64 * R)) + 1;
      per_xcd = restated_per_xcd(hint, bound, bound);
      d.bound = bound;
    }
  }
  d.per_xcd = per_xcd; d.units = by_units;
  if (kern == 5) {
    d.kernel = 7; d.grid = cgrid(per_xcd); d.block = cblock;
  } else if (kern == 7) {
    d.kernel = 6; d.grid = (unsigned)(per_xcd * 8); d.block = 256;
  } else if (kern == 6) {
    d.kernel = 5; d.R = 2; d.filter = true; d.grid = cgrid(per_xcd); d.block = cblock;
  } else {
    d.kernel = 5; d.R = kern == 2 ? 1 : (kern == 4 ? 4 : 2); d.filter = false; d.grid = cgrid(per_xcd); d.block = cblock;
  }
}

// grid_forces_common
static Did restated_whole(Handle* g, float cutoff, bool hp_guard, bool has_target) {
  Did d;
  const int n = (int)g->built_count;
  const int gx = g->info.dims[0], gy = g->info.dims[1], gz = g->info.dims[2];
  const double rho = (double)n / (double)(g->lb_valid && g->lb_count > 0 ? g->lb_count : g->info.total);
  int W = rho > 0 ? (int)(64.0 / rho + 0.5) : 16;
  if (W < 1) W = 1;
  if (W > 16) W = 16;
  const unsigned grid[3] = {(unsigned)((gx + 4 * W - 1) / (4 * W)), (unsigned)gy, (unsigned)gz};
  if (grid[1] > 65535u || grid[2] > 65535u) { d.err = 1; return d; }
  const bool guard = hp_guard;
  const bool strict = cutoff > g->cell;
  int kern = g->tune_kernel;
  if (kern == 0) {
    if (!g->lb_valid) {
      kern = 1;
    } else if (rho >= 8.0) {
      kern = rho < (strict ? 40.0 : g->filter_from_inside) ? 3 : 6;
    } else {
      kern = n >= 500000 ? 9 : 8;
    }
  }
  if ((kern == 8 || kern == 9 || kern == 10) && !g->lb_valid) kern = 1;
  if (kern == 10 && guard) kern = 8;
  if (kern != 1 && g->lb_valid) {
    restated_cell_forces(d, g->lb_base, g->lb_base + g->lb_count, kern, guard, has_target ? g : nullptr, 0);
    return d;
  }
  d.kernel = 1; d.guard = guard; d.strict = strict; d.W = W;
  d.g3[0] = grid[0]; d.g3[1] = grid[1]; d.g3[2] = grid[2];
  return d;
}

// nbody_hip_grid_forces_pair_packed, after its validation
static Did restated_pair(Handle* gt, int z_first, int z_count, float cutoff, bool hp_guard, int accumulate, bool has_target) {
  Did d;
  const int gx = gt->info.dims[0], gy = gt->info.dims[1], gz = gt->info.dims[2];
  const long long layer = (long long)gx * gy;
  long long z0 = z_first < 0 ? 0 : z_first, z1 = z_count <= 0 ? gz : (long long)z_first + z_count;
  if (z1 > gz) z1 = gz;
  long long c0 = z0 * layer, c1 = z1 * layer;
  if (c0 < gt->lb_base) c0 = gt->lb_base;
  if (c1 > gt->lb_base + gt->lb_count) c1 = gt->lb_base + gt->lb_count;
  const double rho = (double)gt->built_count / (double)(gt->lb_count > 0 ? gt->lb_count : 1);
  int kern = gt->tune_kernel;
  if (kern < 2) kern = rho < 8.0 ? (gt->built_count >= (size_t)500000 ? 9 : 8) : (rho < (cutoff > gt->cell ? 40.0 : gt->filter_from_inside) ? 3 : 6);
  restated_cell_forces(d, c0, c1, kern, hp_guard, has_target ? gt : nullptr, accumulate ? 1 : 0);
  return d;
}

// nbody_hip_grid_forces_layer_packed, after its validation
static Did restated_layer(Handle* gt, int z, float cutoff, bool hp_guard, bool has_target) {
  Did d;
  const int gx = gt->info.dims[0], gy = gt->info.dims[1];
  const long long layer = (long long)gx * gy;
  long long c0 = (long long)z * layer, c1 = c0 + layer;
  if (c0 < gt->lb_base) c0 = gt->lb_base;
  if (c1 > gt->lb_base + gt->lb_count) c1 = gt->lb_base + gt->lb_count;
  const double rho = (double)gt->built_count / (double)(gt->lb_count > 0 ? gt->lb_count : 1);
  int kern = gt->tune_kernel;
  if (kern < 2) kern = rho < 8.0 ? (gt->built_count >= (size_t)500000 ? 9 : 8) : (rho < (cutoff > gt->cell ? 40.0 : gt->filter_from_inside) ? 3 : 6);
  restated_cell_forces(d, c0, c1, kern, hp_guard, has_target ? gt : nullptr, 1);
  return d;
}

static int kernel_of(ForceForm f) {
  switch (f) {
    case ForceForm::None: return 0;
    case ForceForm::CellRun: return 1;
    case ForceForm::Body2: return 2;
    case ForceForm::Body: return 3;
    case ForceForm::BodySplit: return 4;
    case ForceForm::Cell: return 5;
    case ForceForm::TwoPhase: return 6;
    case ForceForm::Probe: return 7;
  }
  return -1;
}

struct Geo {
  size_t n;
  int dims[3];
  long long lb_base, lb_count;  // lb_count < 0: the whole grid
  int z_first, z_count;         // what the two-grid entry asks; the layer entry asks z_first
};

static std::vector<Geo> geometries() {
  std::vector<Geo> g;
  const auto whole = [&](size_t n, int gx, int gy, int gz) { g.push_back(Geo{n, {gx, gy, gz}, 0, -1, 0, 0}); };
  // 1,000 cells: rho = 8, 12 (filter_from_inside overridden), 40, each +- one body; 64 / rho rounding to 0; W above kMaxWv
  for (size_t n : {7999, 8000, 8001, 11999, 12000, 12001, 39999, 40000, 40001, 200000, 10, 1}) whole(n, 10, 10, 10);
  for (size_t n : {kSplitFrom - 1, kSplitFrom, kSplitFrom + 1}) whole(n, 50, 50, 50);  // rho = 4: one lane per body, split or not
  whole(4096, 4, 65535, 2); whole(4096, 4, 65536, 2); whole(4096, 4, 2, 65535); whole(4096, 4, 2, 65536);
  // slabs and asked ranges: clipped below and above, empty, one cell, one layer
  g.push_back(Geo{30000, {10, 10, 10}, 200, 600, 1, 3});
  g.push_back(Geo{30000, {10, 10, 10}, 200, 600, -2, 4});
  g.push_back(Geo{30000, {10, 10, 10}, 200, 600, 7, 0});
  g.push_back(Geo{30000, {10, 10, 10}, 200, 600, 9, 5});   // outside the slab: 0 cells
  g.push_back(Geo{30000, {1, 1, 10}, 3, 1, 3, 1});          // 1 cell
  g.push_back(Geo{30000, {10, 10, 10}, 0, 0, 0, 0});        // a start array of no cells
  // ranges of 0x7fffffff cells +- 1 (no grid is this large -- the arithmetic must hold all the same)
  for (long long c : {0x7ffffffeLL, 0x7fffffffLL, 0x80000000LL}) g.push_back(Geo{600000, {65536, 32768, 1}, 0, c, 0, 0});
  for (long long c : {0x7ffffffeLL, 0x7fffffffLL, 0x80000000LL}) g.push_back(Geo{0x3fffffff, {65536, 32768, 1}, 0, c, 0, 0});
  return g;
}

static void compare(const char* what, const Did& d, const ForcePlan& p, unsigned tick_after, bool has_target, long long id) {
  checked++;
  const int err = p.too_large ? 1 : p.needs_target ? 2 : 0;
  EXPECT(err == d.err, "%s case %lld: error %d, restated %d", what, id, err, d.err);
  if (d.err == 1) return;
  EXPECT(kernel_of(p.form) == d.kernel || (d.err == 2 && kernel_of(p.form) >= 2 && kernel_of(p.form) <= 4),
         "%s case %lld: form %d, restated %d", what, id, kernel_of(p.form), d.kernel);
  if (d.err) return;
  EXPECT(p.stat_tick == tick_after, "%s case %lld: stat_tick %u, restated %u", what, id, p.stat_tick, tick_after);
  EXPECT(p.R == 1 || p.R == 2 || p.R == 4, "%s case %lld: R %d", what, id, p.R);
  EXPECT(!p.make_list || has_target, "%s case %lld: a work list without a target grid", what, id);
  if (d.kernel == 0) {
    EXPECT(!p.make_list, "%s case %lld: a list for nothing", what, id);
    return;
  }
  EXPECT(p.guard == d.guard, "%s case %lld: guard", what, id);
  if (d.kernel == 1) {
    EXPECT(p.strict == d.strict && p.W == d.W && p.run_grid[0] == d.g3[0] && p.run_grid[1] == d.g3[1] && p.run_grid[2] == d.g3[2],
           "%s case %lld: cell runs strict %d W %d grid %u %u %u, restated %d %d %u %u %u", what, id, p.strict, p.W, p.run_grid[0],
           p.run_grid[1], p.run_grid[2], d.strict, d.W, d.g3[0], d.g3[1], d.g3[2]);
    EXPECT(p.run_grid[0] >= 1 && p.run_grid[1] >= 1 && p.run_grid[2] >= 1 && p.run_grid[1] <= 65535u && p.run_grid[2] <= 65535u &&
           p.run_grid[0] <= 0x7fffffffu && p.W >= 1 && p.W <= kMaxWv, "%s case %lld: launch limits of the cell-run kernel", what, id);
    EXPECT(!p.make_list, "%s case %lld: a list for the cell-run kernel", what, id);
    return;
  }
  EXPECT(p.cell_first == d.c0 && p.cell_end == d.c1, "%s case %lld: cells [%lld, %lld), restated [%lld, %lld)", what, id,
         p.cell_first, p.cell_end, d.c0, d.c1);
  EXPECT(p.make_list == d.list && p.export_stats == d.exported, "%s case %lld: list %d export %d, restated %d %d", what, id,
         p.make_list, p.export_stats, d.list, d.exported);
  if (d.list)
    EXPECT(p.chunk == d.chunk && p.min_cnt == d.min_cnt && p.bodies == d.bodies && p.pair_items == d.pair_items,
           "%s case %lld: list chunk %d min_cnt %d bodies %d pairs %d, restated %d %d %d %d", what, id, p.chunk, p.min_cnt, p.bodies,
           p.pair_items, d.chunk, d.min_cnt, d.bodies, d.pair_items);
  if (d.kernel >= 2 && d.kernel <= 4)
    EXPECT(p.body_blocks == d.blocks && p.body_blocks >= 1, "%s case %lld: body blocks %u, restated %u", what, id, p.body_blocks, d.blocks);
  if (d.kernel >= 4) {
    EXPECT(p.per_xcd == d.per_xcd && p.cell_grid == d.grid && p.cell_block == d.block && p.units == d.units,
           "%s case %lld: per_xcd %d grid %u block %u units %d, restated %d %u %u %d", what, id, p.per_xcd, p.cell_grid, p.cell_block,
           p.units, d.per_xcd, d.grid, d.block, d.units);
    EXPECT(p.cell_grid >= 1 && p.cell_grid <= 0x7fffffffu && p.per_xcd >= 1, "%s case %lld: launch limits", what, id);
    if (d.kernel == 4 || d.kernel == 5) EXPECT(p.R == d.R && p.filter == d.filter, "%s case %lld: R %d filter %d, restated %d %d", what, id, p.R, p.filter, d.R, d.filter);
    if (p.units) {  // never larger than the bound allows (in groups of 4 KC units, eight XCDs, at least one group each)
      const long long groups = (d.bound + 4 * kCellsPerWave - 1) / (4 * kCellsPerWave);
      EXPECT(p.per_xcd <= (int)(((groups < 8 ? 8 : groups) + 7) / 8), "%s case %lld: unit launch %d per XCD beyond the bound %lld", what,
             id, p.per_xcd, d.bound);
    }
  }
}

static void check_force_plan() {
  const std::vector<Geo> geos = geometries();
  const float built_cell = 1.0f;
  const float cutoffs[3] = {0.5f, 1.0f, 1.7f};
  long long id = 0;
  for (const Geo& geo : geos) {
    GridInfo info{};
    info.total = 1;
    for (int a = 0; a < 3; a++) { info.dims[a] = geo.dims[a]; info.total = grid_cells_times(info.total, geo.dims[a]); }
    const long long lb_count = geo.lb_count < 0 ? info.total : geo.lb_count;
    const long long hints[5] = {0, 1, lb_count * 9 / 10 - 1, lb_count * 9 / 10 + 1, 0x7fffff00LL};
    for (int tuning = 0; tuning <= 10; tuning++)
      for (int lbv = 0; lbv < 2; lbv++)
        for (int guard = 0; guard < 2; guard++)
          for (float cutoff : cutoffs)
            for (int use_units = 0; use_units <= 2; use_units++)
              for (int mapped = 0; mapped < 2; mapped++)
                for (long long hint : hints)
                  for (int crowd : {0, 64, 65})
                    for (unsigned tick = 0; tick <= 8; tick++)
                      for (double ffi : {kFilterFromInside, 12.0})
                        for (int split_cnt : {kSplitCnt, 2})
                          for (int has_target = 1; has_target >= 0; has_target--) {
                            if (!has_target && (tick || hint)) continue;  // (no entry is without one: the rule alone)
                            if (hint < 0 || hint > INT_MAX) continue;
                            Handle h{};
                            h.tune_kernel = tuning; h.lb_valid = lbv != 0; h.lb_base = geo.lb_base; h.lb_count = lb_count;
                            h.info = info; h.built_count = geo.n; h.cell = built_cell; h.filter_from_inside = ffi;
                            h.split_cnt = split_cnt; h.use_units = use_units; h.mapped = mapped != 0;
                            for (int slot = 0; slot < 2; slot++) { h.hint_words[4 * slot] = (int)hint; h.hint_words[4 * slot + 1] = crowd; }
                            h.stat_tick = tick;
                            ForceState s{};
                            s.tuning = tuning; s.lb_valid = h.lb_valid; s.lb_base = h.lb_base; s.lb_count = h.lb_count; s.info = info;
                            s.built_count = geo.n; s.built_cell = built_cell; s.cutoff = cutoff; s.guard = guard != 0;
                            s.filter_from_inside = ffi; s.split_cnt = split_cnt; s.use_units = use_units; s.has_target = has_target != 0;
                            s.hint_mapped = h.mapped; s.hint = h.mapped ? (int)hint : 0; s.crowd = h.mapped ? crowd : 0; s.stat_tick = tick;
                            id++;
                            {
                              Handle g = h;
                              const Did d = restated_whole(&g, cutoff, guard != 0, has_target != 0);
                              compare("whole", d, force_plan(ForceEntry::Whole, s), g.stat_tick, has_target != 0, id);
                            }
                            if (!h.lb_valid) continue;  // (the other two entries reject a grid without a start array)
                            {
                              Handle g = h;
                              const Did d = restated_pair(&g, geo.z_first, geo.z_count, cutoff, guard != 0, (int)(tick & 1), has_target != 0);
                              const CellRange asked = layer_cells(info, geo.z_first, geo.z_count);
                              ForceState t = s; t.cell_first = asked.first; t.cell_end = asked.end;
                              compare("two grids", d, force_plan(ForceEntry::TwoGrids, t), g.stat_tick, has_target != 0, id);
                            }
                            if (geo.z_first >= 0 && geo.z_first < info.dims[2]) {
                              Handle g = h;
                              const Did d = restated_layer(&g, geo.z_first, cutoff, guard != 0, has_target != 0);
                              const CellRange asked = layer_cells(info, geo.z_first, 1);
                              ForceState t = s; t.cell_first = asked.first; t.cell_end = asked.end;
                              compare("layer", d, force_plan(ForceEntry::Layer, t), g.stat_tick, has_target != 0, id);
                            }
                          }
  }
}

// ---------------------------------------------------------------------------------------
// what grid_build_packed did for the start array, statement by statement
// ---------------------------------------------------------------------------------------
struct Built {
  long long base, count;
  bool dense, grew = false;
  long long cap = 0;
  size_t words = 0;
  int clears = 0;
  int method = 0;  // 1 two-level, 2 by position, 3 per cell
  unsigned ga = 0, gb = 0;
  int cur = 0, next = 0;
  long long lb_capacity;
  bool clean;
  unsigned tick;
};
static Built restated_start(const GridInfo& info, size_t n, bool slab, int slab_z0, int slab_nz, long long lb_capacity,
                            bool lb_by_position, bool clean, unsigned tick) {
  Built b{};
  b.lb_capacity = lb_capacity; b.clean = clean; b.tick = tick;
  const int ni = (int)n;
  long long base = 0, count = info.total;
  if (slab && slab_nz > 0) {
    const long long layer = (long long)info.dims[0] * info.dims[1];
    const long long z0 = slab_z0 < 0 ? 0 : slab_z0;
    long long z1 = (long long)slab_z0 + slab_nz;
    if (z1 > info.dims[2]) z1 = info.dims[2];
    base = z0 * layer;
    count = z1 > z0 ? (z1 - z0) * layer : 0;
  }
  const bool dense = count > 0 && count <= 16LL * (long long)n + 4096;
  if (dense && count + 1 > b.lb_capacity) {
    const long long cap = (count + 1) + (count + 1) / 2;
    const size_t extra = (size_t)(3 * (cap / 64 + 4) + 8);
    b.grew = true; b.cap = cap; b.words = (size_t)cap + extra;
    b.lb_capacity = cap;
    b.clears++;
    b.clean = true;
    b.tick = 0;
  }
  if (dense && count > 2LL * (long long)n) {
    b.clean = false;
    const long long ncoarse = count / 64 + 2;
    b.method = 1;
    b.ga = (unsigned)((ncoarse + 256 - 1) / 256);
    b.gb = (unsigned)((count + 1 + 256 - 1) / 256);
  } else if (dense && lb_by_position) {
    if (!b.clean) { b.clears++; b.clean = true; }
    b.cur = (int)(b.tick & 1); b.next = (int)((b.tick + 1) & 1);
    b.tick++;
    b.method = 2;
    b.ga = (unsigned)((ni + 1 + 256 - 1) / 256);
    b.gb = 512;
  } else if (dense) {
    b.method = 3;
    b.ga = (unsigned)((count + 1 + 256 - 1) / 256);
  }
  b.base = base; b.count = count; b.dense = dense;
  return b;
}

static void check_start_array() {
  for (long long n : {1LL, 63LL, 64LL, 65LL, 4096LL, (1LL << 30) - 1}) {
    std::vector<long long> counts = {1, 2 * n - 1, 2 * n, 2 * n + 1, 16 * n + 4095, 16 * n + 4096, 16 * n + 4097, kMaxCells};
    for (long long layer : counts) {
      if (layer < 1 || layer > kMaxCells) continue;
      // dims {layer, 1, gz}: the whole grid of one layer, and slabs of a grid of eight
      const struct { int gz; bool slab; int z0, nz; } shapes[] = {
          {1, false, 0, 0}, {1, true, 0, 0}, {8, true, 2, 1}, {8, true, -1, 2}, {8, true, 7, 5}, {8, true, 9, 2}, {8, true, 5, -1},
          {8, true, 0, 8}};
      for (const auto& sh : shapes) {
        GridInfo info{};
        info.dims[0] = (int)layer; info.dims[1] = 1; info.dims[2] = sh.gz;
        info.total = layer * sh.gz;
        const Built probe = restated_start(info, (size_t)n, sh.slab, sh.z0, sh.nz, 0, true, false, 0);
        for (long long capacity : {0LL, probe.count, probe.count + 1, probe.count + 2, 2 * probe.count + 7})
          for (int by_position = 0; by_position < 2; by_position++)
            for (int clean = 0; clean < 2; clean++)
              for (unsigned tick : {0u, 1u, 5u, 0xffffffffu}) {
                checked++;
                const Built b = restated_start(info, (size_t)n, sh.slab, sh.z0, sh.nz, capacity, by_position != 0, clean != 0, tick);
                const StartArrayPlan p = start_array_plan(info, (size_t)n, sh.slab, sh.z0, sh.nz, capacity, by_position != 0, clean != 0, tick);
                EXPECT(p.base == b.base && p.count == b.count && p.dense == b.dense, "start array n %lld layer %lld: cells [%lld + %lld] dense %d, restated [%lld + %lld] %d",
                       n, layer, p.base, p.count, p.dense, b.base, b.count, b.dense);
                EXPECT(p.grow == b.grew && p.capacity == b.lb_capacity && (!b.grew || (p.size.capacity == b.cap && p.size.words == b.words)),
                       "start array n %lld count %lld capacity %lld: grow %d to %lld (%zu words), restated %d %lld (%zu)", n, b.count,
                       capacity, p.grow, p.capacity, p.size.words, b.grew, b.lb_capacity, b.words);
                EXPECT((int)p.method == b.method && p.blocks_a == b.ga && p.blocks_b == b.gb, "start array n %lld count %lld: method %d grids %u %u, restated %d %u %u",
                       n, b.count, (int)p.method, p.blocks_a, p.blocks_b, b.method, b.ga, b.gb);
                // (the parent cleared at the growth and, by position with dirty counters, before the launch -- never both)
                EXPECT(b.clears <= 1 && p.clear_counters == (b.clears == 1), "start array: clears %d, plan %d", b.clears, p.clear_counters);
                EXPECT(p.gap_counters_clean == b.clean && p.gap_tick == b.tick, "start array: state after clean %d tick %u, restated %d %u",
                       p.gap_counters_clean, p.gap_tick, b.clean, b.tick);
                if (b.method == 2) EXPECT(p.cur == b.cur && p.next == b.next && p.cur != p.next, "start array: counters %d %d", p.cur, p.next);
                if (!p.dense) continue;
                // every method's launch covers the count + 1 entries (by position: the n + 1 sorted positions that own them)
                const long long lanes_a = (long long)p.blocks_a * kGridBlock, lanes_b = (long long)p.blocks_b * kGridBlock;
                if (p.method == StartMethod::TwoLevel) EXPECT(lanes_a >= p.count / kLbCoarse + 2 && lanes_b >= p.count + 1, "two-level launch");
                if (p.method == StartMethod::ByPosition) EXPECT(lanes_a >= n + 1 && p.blocks_b >= 1, "by-position launch");
                if (p.method == StartMethod::PerCell) EXPECT(lanes_a >= p.count + 1, "per-cell launch");
                // the array this build writes holds count + 1 entries, its tail the coarse level and the gap list
                const StartArraySize size = p.grow ? p.size : start_array_capacity(p.capacity * 2 / 3);  // (any array of this capacity)
                EXPECT(p.capacity >= p.count + 1, "capacity %lld for %lld cells", p.capacity, p.count);
                if (p.grow) {
                  const long long tail = (long long)size.words - size.capacity;
                  EXPECT(tail >= p.count / kLbCoarse + 2, "tail %lld below the coarse level of %lld cells", tail, p.count);
                  EXPECT(tail >= 2 + 3 * ((p.count + 1) / kGapInline + 1), "tail %lld below the gap list of %lld cells", tail, p.count);
                  EXPECT(size.words <= (size_t)INT_MAX && size.capacity <= INT_MAX, "start array of %zu words", size.words);
                }
              }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// the grid record, the key bits, the sizes: against the expressions they replace
// ---------------------------------------------------------------------------------------
static void check_record_and_sizes() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float boxes[][6] = {{0, 0, 0, 1, 1, 1}, {-8, -8, -8, 8, 8, 8}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 3e38f, 1, 1}, {-3e38f, 0, 0, 3e38f, 1, 1},
                            {0, 0, 0, inf, 1, 1}, {0, 0, 0, nan, 1, 1}, {nan, nan, nan, nan, nan, nan}, {0, 0, 0, 1e9f, 1e9f, 1e9f},
                            {0, 0, 0, 463.f, 463.f, 463.f}, {0, 0, 0, 464.f, 464.f, 464.f}, {5, 5, 5, 1, 1, 1}};
  for (const auto& bx : boxes)
    for (float cell : {1.0f, 0.37f, 1e-30f, 3e38f}) {
      checked++;
      GridInfo r{};
      long long total = 1;
      for (int a = 0; a < 3; a++) {
        r.bmin[a] = bx[a];
        r.bmax[a] = bx[3 + a];
        const float cells = ceilf((bx[3 + a] - bx[a]) / cell);
        r.dims[a] = (cells < 1.0e9f && cells >= 0.0f) ? (int)cells + 1 : 0x40000000;
        const long long cap = 0x4000000000000LL;
        total = (r.dims[a] <= 0 || total > cap / r.dims[a]) ? cap : total * r.dims[a];
      }
      r.total = total;
      const GridInfo g = grid_from_bounds(bx, cell);
      EXPECT(std::memcmp(g.dims, r.dims, sizeof r.dims) == 0 && g.total == r.total && g.pad == 0 &&
             std::memcmp(g.bmin, r.bmin, sizeof r.bmin) == 0 && std::memcmp(g.bmax, r.bmax, sizeof r.bmax) == 0,
             "grid_from_bounds: %d %d %d = %lld, restated %d %d %d = %lld", g.dims[0], g.dims[1], g.dims[2], g.total, r.dims[0], r.dims[1], r.dims[2], r.total);
      EXPECT(g.total >= 1 && g.dims[0] >= 1 && g.dims[1] >= 1 && g.dims[2] >= 1, "grid_from_bounds: an axis without cells");
      EXPECT(grid_too_large(g.total) == (g.total > 100000000LL), "grid_too_large");
    }
  EXPECT(grid_from_bounds(boxes[8], 1.0f).total == 0x4000000000000LL, "three axes of 2^30 saturate");
  EXPECT(!grid_too_large(100000000LL) && grid_too_large(100000001LL), "the 1e8 limit");
  for (int b = 0; b <= 50; b++)
    for (long long d = -1; d <= 1; d++) {
      const long long total = (1LL << b) + d;
      int bits = 1;
      while ((1LL << bits) < total && bits < 32) bits++;
      checked++;
      EXPECT(key_bits(total) == bits && bits_for(total) == bits && bits >= 1 && bits <= 32, "key_bits(%lld) = %d, restated %d", total, key_bits(total), bits);
    }
  for (int mode = 0; mode <= 2; mode++)
    for (int last = 0; last <= 32; last++) {
      int spec = 0;
      if (mode && last > 0) spec = mode == 2 ? (last > 10 ? last - 10 : last + 10) : last;
      EXPECT(speculated_bits(mode, last) == spec, "speculated_bits(%d, %d)", mode, last);
      if (mode == 2 && last > 0) EXPECT(spec != last && spec >= 1, "mode 2 is always wrong");
    }
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)4096, (size_t)4194304, (size_t)0x3fffffff}) {
    const GridSizes s = grid_sizes(n);
    EXPECT(s.enc == 8 && s.info == 1 && s.bodies == n && s.unit_count == 8, "grid_sizes(%zu)", n);
    for (size_t built : {(size_t)1, n / 2 + 1, n})
      for (size_t current : {(size_t)0, built + built / 64 + 1023, built + built / 64 + 1024, n + n / 64 + 1024, 4 * n + 4096}) {
        checked++;
        const size_t need = built + built / 64 + 1024;
        size_t want = current;
        if (need > current) {
          const size_t cap = n + n / 64 + 1024;
          want = cap > need ? cap : need;
        }
        EXPECT(unit_list_capacity(built, n, current) == want && want >= need, "unit_list_capacity(%zu, %zu, %zu)", built, n, current);
      }
  }
  for (size_t m : {(size_t)1, (size_t)100, (size_t)3276, (size_t)3277, (size_t)10000, (size_t)0x40000000}) {
    const size_t want = m + m / 4 > 4096 ? m + m / 4 : 4096;
    EXPECT(point_capacity(m) == want && want >= m, "point_capacity(%zu)", m);
  }
  // the group workspace: a quarter more than asked, at least 4,096, at most what the handle holds, never fewer than asked
  for (size_t max_particles : {(size_t)1, (size_t)100, (size_t)4096, (size_t)5000, (size_t)4194304, (size_t)0x3fffffff})
    for (size_t built : {(size_t)1, (size_t)2, (size_t)100, (size_t)3276, (size_t)3277, (size_t)4096, (size_t)4000000, (size_t)0x3fffffff}) {
      if (built > max_particles) continue;
      checked++;
      size_t want = built + built / 4 > 4096 ? built + built / 4 : 4096;
      if (want > max_particles) want = max_particles;
      const size_t cap = group_capacity(built, max_particles);
      EXPECT(cap == want && cap >= built && cap <= max_particles, "group_capacity(%zu, %zu) = %zu", built, max_particles, cap);
      const GroupSizes z = group_sizes(cap);
      EXPECT(z.bodies == cap && z.offsets == cap + 1 && z.counts == 2, "group_sizes(%zu)", cap);
      // every label 0 .. built - 1 and the sentinel `built` fit the sorted bits, and one bit fewer would not hold them
      const int bits = group_key_bits(built);
      EXPECT(bits >= 1 && bits <= 32 && (1LL << bits) > (long long)built && (bits == 1 || (1LL << (bits - 1)) <= (long long)built),
             "group_key_bits(%zu) = %d", built, bits);
    }
  for (long long count : {1LL, 63LL, 64LL, 5832LL, 100000000LL}) {
    const long long cap = (count + 1) + (count + 1) / 2;
    const StartArraySize s = start_array_capacity(count);
    EXPECT(s.capacity == cap && s.words == (size_t)cap + (size_t)(3 * (cap / 64 + 4) + 8), "start_array_capacity(%lld)", count);
  }
  for (long long cells : {1LL, 100LL, 1000000LL})
    for (long long nb : {1LL, 4096LL, 4194304LL}) {
      EXPECT(unit_list_bound(cells, nb, 1, 128) == (cells < nb ? cells : nb) + nb / 128 + 1, "unit_list_bound, every cell");
      EXPECT(unit_list_bound(cells, nb, 6, 128) == nb / 6 + nb / 128 + 1, "unit_list_bound, split");
    }
}

// ---------------------------------------------------------------------------------------
// replace_arrays over tables shaped like the grid's (spatial_hash.hip: fixed_slots -- nine arrays, the last cleared, one
// possibly empty scratch array -- and point_slots), with malloc and a stub that fails at the k-th step, for every k.  The
// grid keeps its capacities itself: it zeroes one before the call and writes it after success (capacity pointer null).
// ---------------------------------------------------------------------------------------
static int fail_at = -1, calls = 0, live = 0;
static int stub_alloc(void** p, size_t bytes) {
  if (calls++ == fail_at) return 2;
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
  unsigned int *enc = nullptr, *keys_a = nullptr, *keys_b = nullptr, *hist = nullptr;
  GridInfo* info = nullptr;
  int *idx = nullptr, *unit_count = nullptr;
  double* sorted = nullptr;
  void* tmp = nullptr;
  void** all[9] = {(void**)&enc, (void**)&info, (void**)&keys_a, (void**)&keys_b, (void**)&idx, (void**)&sorted, &tmp, (void**)&hist,
                   (void**)&unit_count};
  const auto table = [&](ArraySlot* s, size_t n, size_t tmp_bytes) {
    const GridSizes z = grid_sizes(n);
    int k = 0;
    s[k++] = array_slot(&enc, z.enc);
    s[k++] = array_slot(&info, z.info);
    s[k++] = array_slot(&keys_a, z.bodies);
    s[k++] = array_slot(&keys_b, z.bodies);
    s[k++] = array_slot(&idx, z.bodies);
    s[k++] = array_slot(&sorted, 2 * z.bodies);
    s[k++] = ArraySlot{&tmp, tmp_bytes, false};
    s[k++] = array_slot(&hist, 3072);
    s[k++] = array_slot(&unit_count, z.unit_count, true);
    return k;
  };
  const auto none = [&] { for (void** p : all) if (*p) return false; return true; };
  const auto every = [&] { for (void** p : all) if (!*p) return false; return true; };
  ArraySlot s[12];
  const int steps = 9 + 1;  // nine allocations, one clear
  for (int round = 0; round < 2; round++)  // from nothing, then over a live set (which must be freed first, once)
    for (int k = 0; k <= steps; k++) {
      size_t capacity = 0;
      if (round == 1) {
        fail_at = -1;
        EXPECT(replace_arrays(s, table(s, 10, 64), nullptr, 0, stub_alloc, stub_free, stub_zero) == 0 && every(), "set-up");
        capacity = 10;
      }
      fail_at = k; calls = 0;
      capacity = 0;
      const int rc = replace_arrays(s, table(s, 100, 0), nullptr, 0, stub_alloc, stub_free, stub_zero);
      if (rc == 0) capacity = 100;
      checked++;
      if (k < steps) {
        EXPECT(rc != 0 && none() && capacity == 0 && live == 0, "after a failure at step %d: rc %d capacity %zu live %d", k, rc, capacity, live);
      } else {
        EXPECT(rc == 0 && every() && capacity == 100 && live == 9, "success: rc %d live %d", rc, live);
        bool cleared = true;
        for (int i = 0; i < 8; i++) cleared = cleared && unit_count[i] == 0;
        EXPECT(cleared && keys_a[99] == 0xa5a5a5a5u, "only the array marked so is cleared");
        keys_b[99] = 1; idx[99] = 1; sorted[199] = 1.0; hist[3071] = 1; enc[7] = 1; info->total = 1;  // (full extents: ASan checks)
        static_cast<char*>(tmp)[15] = 1;  // (an empty scratch array still gets 16 bytes)
        release_arrays(s, table(s, 0, 0), nullptr, stub_free);
        EXPECT(none() && live == 0, "after the release");
        release_arrays(s, table(s, 0, 0), nullptr, stub_free);  // (a second release frees nothing)
        EXPECT(live == 0, "released twice");
      }
    }
  fail_at = -1;
}

int main() {
  check_record_and_sizes();
  check_start_array();
  check_force_plan();
  check_replace();
  if (failures) {
    std::printf("grid_plan_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("grid_plan_check: ok (%lld cases)\n", checked);
  return 0;
}
