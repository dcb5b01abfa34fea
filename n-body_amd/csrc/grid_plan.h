// grid_plan.h -- the host decisions of the spatial hash (spatial_hash.hip) as plain arithmetic: the grid record and its key
// bits, the size of every array of a grid, the plan of the start array of one build, and the plan of one force call (which
// kernel form, with which template arguments, over which cells, with which launch sizes).  Plain C++17, no HIP include:
// grid_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make grid_plan_check).
//
// spatial_hash.hip derives each of these ONCE per create / build / force call and issues allocations and launches from
// the result; nothing here launches, allocates or reads device memory.  The few functions grid_info_kernel also calls
// carry NBH_GRID_HD, so that the device and the host go on computing the same record.
#pragma once

#include <cmath>
#include <cstddef>

#include "device_arrays.h"  // ArraySlot, replace_arrays, release_arrays

#if defined(__HIPCC__)
#define NBH_GRID_HD __host__ __device__
#else
#define NBH_GRID_HD
#endif

#ifndef NBH_HASH_SPLIT_CNT
#define NBH_HASH_SPLIT_CNT 6
#endif
#ifndef NBH_HASH_KC
#define NBH_HASH_KC 4
#endif
// Waves per workgroup of the wave-per-cell kernel.  The waves of a workgroup share nothing (every wave has its own LDS
// region and its own cells); what the workgroup size decides is when the LDS and the wave slots come back: a workgroup's
// resources are released when its LAST wave ends, and the waves of one workgroup take very different times (four cells
// each, 5 to 25 bodies).
#ifndef NBH_HASH_CELL_WPB
#define NBH_HASH_CELL_WPB 1
#endif

namespace nbh {

// ---------------------------------------------------------------------------------------
// THE GRID RECORD
// ---------------------------------------------------------------------------------------
struct GridInfo {
  float bmin[3];
  float bmax[3];
  int dims[3];
  int pad;
  long long total;
};

// cells per axis (force_spatial_hash.cu:244-246) with the int conversion guarded: NaN / inf / huge
// extents become 2^30 cells, which the "grid too large" check then rejects
NBH_GRID_HD inline int grid_axis_cells(float lo, float hi, float cell) {
  const float cells = ceilf((hi - lo) / cell);
  return (cells < 1.0e9f && cells >= 0.0f) ? (int)cells + 1 : 0x40000000;
}
// running product of the axis sizes, SATURATING at 2^50 (three axes of 2^30 would wrap a 64-bit
// product to 0 and slip under the 1e8 limit)
NBH_GRID_HD inline long long grid_cells_times(long long total, int d) {
  const long long cap = 0x4000000000000LL;
  return (d <= 0 || total > cap / d) ? cap : total * d;
}

inline int bits_for(long long total) {
  int b = 1;
  while ((1LL << b) < total && b < 32) b++;
  return b;
}

constexpr long long kMaxCells = 100000000LL;  // more is "grid too large" (force_spatial_hash.cu:252-254)
inline bool grid_too_large(long long total) { return total > kMaxCells; }

// the host's record for explicit bounds {lo x,y,z, hi x,y,z} (the sharded path): what grid_info_kernel computes from the
// box of the bodies, without the padding
inline GridInfo grid_from_bounds(const float* bounds, float cell) {
  GridInfo gi{};
  long long total = 1;
  for (int a = 0; a < 3; a++) {
    gi.bmin[a] = bounds[a];
    gi.bmax[a] = bounds[3 + a];
    gi.dims[a] = grid_axis_cells(bounds[a], bounds[3 + a], cell);  // :244-246
    total = grid_cells_times(total, gi.dims[a]);
  }
  gi.total = total;
  return gi;
}

// key bits of the sort of a grid of `total` cells
inline int key_bits(long long total) { return bits_for(total); }
// the bit count the key pass is launched on BEFORE the record of this build is back: the previous build's (0: no
// speculation -- switched off, or no previous build); spec_mode 2 is always wrong (tests)
inline int speculated_bits(int spec_mode, int last_bits) {
  if (!spec_mode || last_bits <= 0) return 0;
  return spec_mode == 2 ? (last_bits > 10 ? last_bits - 10 : last_bits + 10) : last_bits;
}

// ---------------------------------------------------------------------------------------
// CONSTANTS OF THE KERNELS THAT THE HOST SIZES LAUNCHES BY
// ---------------------------------------------------------------------------------------
constexpr int kGridBlock = 256;  // threads of a workgroup (kBlock of common.h; asserted in spatial_hash.hip)
// long runs of empty cells (cell_mark_kernel: this many or more go to the gap list) / cells per entry of the coarse level
// of the two-level search (cell_lb_coarse_kernel)
constexpr int kGapInline = 64;
constexpr int kLbCoarse = 64;
static_assert(kGapInline == kLbCoarse, "one scratch area behind the start array serves both");
constexpr int kMaxWv = 16;  // cells per wave of the cell-run kernel, at most
// KC consecutive cells per wave of the wave-per-cell kernel (2 and 3 measured in round 4: 0.635 / 0.639-0.653 against
// 0.634-0.636 ms: no difference)
constexpr int kCellsPerWave = NBH_HASH_KC;
static_assert(kCellsPerWave >= 1 && kCellsPerWave <= 4, "the lookups of a wave's cells are one round of 16 lanes per cell");
constexpr int kCellWPB = NBH_HASH_CELL_WPB;
static_assert(kCellWPB == 1 || kCellWPB == 2 || kCellWPB == 4, "the launch geometry is counted in groups of four waves");
constexpr int kUnitCells = 8;  // consecutive cells per thread of cell_units_kernel (one slot-range atomic per 2,048 cells:
                               // a workgroup per 256 cells made 86,000 atomics on one word at 22 M cells, 0.44 ms)
constexpr int kUnitChunk2 = 64;  // bodies per unit of the two-phase kernel (four passes share one window load)

// the automatic choice
constexpr double kFilterFrom = 40.0;  // bodies per cell from which the filtered form pays when cutoff > cell (see FILTER)
constexpr double kBodyBelow = 8.0;    // bodies per cell below which one lane takes one body (hash_body_force_kernel): 0.72 against
                                      // 0.96 ms at 6.6 per cell, 0.85 against 0.81 at 8.8 (profiles/r04_hash_kernels.txt)
constexpr int kSplitFrom = 500000;   // bodies from which the automatic form below kBodyBelow is the split one
constexpr int kSplitCnt = NBH_HASH_SPLIT_CNT;  // ... except the bodies of cells this crowded: wave per cell (split form)
constexpr double kFilterFromInside = 8.0;  // ... and when cutoff <= cell: everywhere the wave-per-cell form runs at all (with the
                                          // straight-line gather of round 4 the box test pays from ~8 per cell: 0.81 against
                                          // 0.84 ms at 8.8 per cell, 0.78 against 0.86 at 11.2, 0.68 against 0.78 at 14.6,
                                          // 0.52 against 0.93 at cutoff = cell / 2: profiles/r04_hash_kernels.txt)
constexpr long long kListCells = 0x7fffffffLL;  // a work list indexes its cells with an int: ranges below this many

// the run-time switches of a grid and their defaults; read from the environment once, at creation (A/B runs, tests)
struct GridSwitches {
  int split_cnt = kSplitCnt;  // NBH_HASH_SPLIT_CNT: split form, cells from this many bodies take the wave-per-cell kernel
  double filter_from_inside = kFilterFromInside;  // NBH_HASH_FILTER_FROM: bodies per cell from which the filtered form runs
                                                  // when cutoff <= cell
  int use_units = 1;           // NBH_HASH_UNITS: 0 = never the unit list (the cell-range form), 2 = always (tests), 1 = by the
                               // statistics of the previous call
  bool lb_by_position = true;  // NBH_HASH_LB=cell: the per-cell search (cell_lb_kernel) for the start array instead
  int spec_mode = 1;           // NBH_HASH_SPECULATE: 0 = no speculative key pass, 2 = always on wrong key bits (tests)
};

// ---------------------------------------------------------------------------------------
// SIZES
// ---------------------------------------------------------------------------------------
// element counts of the arrays of a grid handle that are fixed at create time, from max_particles alone (the sort's
// temporary storage and its digit counts are sized by the sort front end)
struct GridSizes {
  size_t enc;         // d_enc: 6 ordered-int box words (+ 2)
  size_t info;        // d_info, h_info: one record
  size_t bodies;      // d_keys_a, d_keys_b, d_idx_b, d_sorted; d_light (allocated by the first split-form call)
  size_t unit_count;  // d_unit_count, h_unit_hint: [2][4]
};
inline GridSizes grid_sizes(size_t max_particles) {
  GridSizes s{};
  s.enc = 8;
  s.info = 1;
  s.bodies = max_particles;
  s.unit_count = 8;
  return s;
}

// the start array of `count` cells (+ 1 entry) is allocated with half as much again (grids grow and shrink with the box),
// and behind it the scratch tail: the coarse level of the two-level search, or the two counters and the list of
// cell_mark_kernel's long runs of empty cells (three words each, at most capacity / kGapInline + 1 of them)
struct StartArraySize {
  long long capacity;  // entries of the array proper; the tail starts here
  size_t words;        // ints in all
};
inline StartArraySize start_array_capacity(long long count) {
  StartArraySize s{};
  s.capacity = (count + 1) + (count + 1) / 2;
  s.words = (size_t)s.capacity + (size_t)(3 * (s.capacity / kGapInline + 4) + 8);
  return s;
}

// slots of the work list the next list of a grid is counted against: an occupied cell is at least one unit, chunks hold
// >= 64 bodies.  (`current` when that suffices; otherwise the list is replaced by one for max_particles.)
inline size_t unit_list_capacity(size_t built, size_t max_particles, size_t current) {
  const size_t need = built + built / 64 + 1024;
  if (need <= current) return current;
  const size_t cap = max_particles + max_particles / 64 + 1024;
  return cap > need ? cap : need;
}

// points the field's workspace is (re)allocated for when m are asked
inline size_t point_capacity(size_t m) {
  const size_t cap = m + m / 4;
  return cap > 4096 ? cap : 4096;
}

// bodies the group workspace (nbody_hip_grid_groups) is (re)allocated for when a grid of `built` bodies asks: a quarter
// more than asked, at least 4,096, never more than the handle can be built with -- and never fewer than asked
inline size_t group_capacity(size_t built, size_t max_particles) {
  size_t cap = built + built / 4;
  if (cap < 4096) cap = 4096;
  if (cap > max_particles) cap = max_particles;
  return cap > built ? cap : built;
}
// element counts of the arrays of that workspace, for `cap` bodies (the sort's temporary storage is sized by the sort
// front end, the scan's by the scan)
struct GroupSizes {
  size_t bodies;   // parents, sizes, the two key arrays, the identity payload, the sorted members
  size_t offsets;  // one entry per group and one more: at most bodies + 1
  size_t counts;   // {n_groups, n_members}
};
inline GroupSizes group_sizes(size_t cap) { return GroupSizes{cap, cap + 1, 2}; }
// key bits of the catalogue's sort of n bodies: labels are 0 .. n - 1, the sentinel of the dropped bodies is n
inline int group_key_bits(size_t n) { return bits_for((long long)n + 1); }

// ---------------------------------------------------------------------------------------
// THE START ARRAY OF ONE BUILD
// ---------------------------------------------------------------------------------------
enum class StartMethod : int {
  None = 0,    // not dense (or an empty slab): no start array, the cell-run kernel
  TwoLevel,    // more than two cells per body: cell_lb_coarse_kernel + cell_lb_fine_kernel
  ByPosition,  // cell_mark_kernel + cell_gap_kernel
  PerCell,     // cell_lb_kernel (NBH_HASH_LB=cell)
};

struct StartArrayPlan {
  long long base, count;  // cells [base, base + count] the array covers: the whole grid, or the z layers of a slab
  bool dense;
  bool grow;              // the array is replaced first ...
  StartArraySize size;    // ... by one of this size
  long long capacity;     // entries of the array this build writes (where its scratch tail starts)
  StartMethod method;
  bool clear_counters;    // the two counters at the head of the tail are zeroed before the launches
  unsigned blocks_a, blocks_b;  // TwoLevel: coarse, fine; ByPosition: mark, gap; PerCell: blocks_a
  int cur, next;          // ByPosition: which of the two counters this build counts in / zeroes for the next
  bool gap_counters_clean;  // the handle's state afterwards
  unsigned gap_tick;
};

inline unsigned grid_blocks(long long items) { return (unsigned)((items + kGridBlock - 1) / kGridBlock); }

inline StartArrayPlan start_array_plan(const GridInfo& info, size_t n, bool slab, int z0_in, int nz, long long lb_capacity,
                                       bool lb_by_position, bool gap_counters_clean, unsigned gap_tick) {
  StartArrayPlan p{};
  p.base = 0;
  p.count = info.total;
  if (slab && nz > 0) {
    const long long layer = (long long)info.dims[0] * info.dims[1];
    const long long z0 = z0_in < 0 ? 0 : z0_in;
    long long z1 = (long long)z0_in + nz;
    if (z1 > info.dims[2]) z1 = info.dims[2];
    p.base = z0 * layer;
    p.count = z1 > z0 ? (z1 - z0) * layer : 0;
  }
  // (16 cells per body: a box that has expanded and clumped is still walked cell by cell, with the empty cells skipped by
  // the unit list; beyond that the start array itself -- one search per cell -- costs more than the cell-run kernel's)
  p.dense = p.count > 0 && p.count <= 16LL * (long long)n + 4096;
  p.capacity = lb_capacity;
  p.gap_counters_clean = gap_counters_clean;
  p.gap_tick = gap_tick;
  if (!p.dense) return p;
  if (p.count + 1 > lb_capacity) {
    p.grow = true;
    p.size = start_array_capacity(p.count);
    p.capacity = p.size.capacity;
    p.clear_counters = true;  // both counters of the gap list
    p.gap_counters_clean = true;
    p.gap_tick = 0;
  }
  const int ni = (int)n;
  if (p.count > 2LL * (long long)n) {  // more cells than bodies: two-level search (see cell_lb_coarse_kernel)
    p.method = StartMethod::TwoLevel;
    p.gap_counters_clean = false;  // (the coarse level lies in the same scratch area)
    p.blocks_a = grid_blocks(p.count / kLbCoarse + 2);
    p.blocks_b = grid_blocks(p.count + 1);
  } else if (lb_by_position) {
    p.method = StartMethod::ByPosition;
    if (!p.gap_counters_clean) {
      p.clear_counters = true;
      p.gap_counters_clean = true;
    }
    p.cur = (int)(p.gap_tick & 1);
    p.next = (int)((p.gap_tick + 1) & 1);
    p.gap_tick++;
    p.blocks_a = grid_blocks((long long)ni + 1);
    p.blocks_b = 512;
  } else {
    p.method = StartMethod::PerCell;
    p.blocks_a = grid_blocks(p.count + 1);
  }
  return p;
}

// ---------------------------------------------------------------------------------------
// ONE FORCE CALL
// ---------------------------------------------------------------------------------------
// Launch size of the unit form of the wave-per-cell kernels, in groups of four waves per XCD: one group of KC units per
// wave for the list length the previous call of this kind saw (hint, + 1/64 + 64), `first` on a first call; never more
// than `bound`, what the cells / bodies allow, and at least one group per XCD.  The kernel strides if the list is longer.
inline int unit_list_per_xcd(int hint, long long bound, long long first) {
  long long est = hint > 0 ? (long long)hint + hint / 64 + 64 : first;
  if (est > bound) est = bound;
  long long blocks = (est + 4 * kCellsPerWave - 1) / (4 * kCellsPerWave);
  if (blocks < 8) blocks = 8;
  return (int)((blocks + 7) / 8);
}
// never more units than the cells that make any, plus the further chunks of the crowded ones:
//   min_cnt == 1 (every occupied cell makes units): min(cells, bodies) + bodies / chunk + 1
//   min_cnt >= 2 (the split form: only cells of min_cnt bodies and more):  bodies / min_cnt + bodies / chunk + 1
inline long long unit_list_bound(long long cells, long long bodies, int min_cnt, int chunk) {
  const long long makers = min_cnt > 1 ? bodies / min_cnt : (cells < bodies ? cells : bodies);
  return makers + bodies / chunk + 1;
}

// the cells of the z layers [z_first, z_first + z_count) (z_count <= 0: to the top) of a grid
struct CellRange {
  long long first, end;
};
inline CellRange layer_cells(const GridInfo& info, int z_first, int z_count) {
  const long long layer = (long long)info.dims[0] * info.dims[1];
  long long z0 = z_first < 0 ? 0 : z_first, z1 = z_count <= 0 ? info.dims[2] : (long long)z_first + z_count;
  if (z1 > info.dims[2]) z1 = info.dims[2];
  return CellRange{z0 * layer, z1 * layer};
}

enum class ForceEntry : int {
  Whole = 0,  // nbody_hip_grid_compute_forces / _packed: every cell of one grid
  TwoGrids,   // nbody_hip_grid_forces_pair_packed: targets of one grid, sources of another, a range of z layers
  Layer,      // nbody_hip_grid_forces_layer_packed: targets of one layer, sources an exported layer
};

enum class ForceForm : int {
  None = 0,   // empty range: nothing is launched
  CellRun,    // hash_force_kernel<GUARD, STRICT>: no start array needed
  Body,       // tuning 8: hash_body_force_kernel, every body
  BodySplit,  // tuning 9: ... the bodies of the light cells, then hash_cell_force_kernel<GUARD, 2, false, true, false> over the list
  Body2,      // tuning 10: hash_body2_force_kernel over the pair items of the list
  Cell,       // tunings 2 / 3 / 4 / 6: hash_cell_force_kernel<GUARD, R, false, UNITS, FILTER>
  TwoPhase,   // tuning 7: hash_cell_force2_kernel<GUARD, UNITS>
  Probe,      // tuning 5: the half-shell TIMING PROBE hash_cell_force_kernel<false, 2, true> (not forces)
};

struct ForceState {  // what a force call reads of the target grid's handle and of its arguments
  int tuning;
  bool lb_valid;
  long long lb_base, lb_count;
  GridInfo info;
  size_t built_count;
  float built_cell, cutoff;
  bool guard;
  double filter_from_inside;
  int split_cnt, use_units;
  bool has_target;        // the handle of the target grid is at hand (work list, hints): all three entries have it
  bool hint_mapped;       // the hint words are in mapped host memory ...
  int hint, crowd;        // ... {units, most crowded cell} of the previous call of this kind (0 when not mapped)
  unsigned stat_tick;
  long long cell_first, cell_end;  // TwoGrids / Layer: the cells asked for (Whole: the start array's own)
};

struct ForcePlan {
  ForceForm form;
  bool too_large;     // error: the cell-run kernel's grid passes the launch limits
  bool needs_target;  // error: the form takes a work list and there is no target grid
  bool guard, strict, units, filter;  // template arguments (strict: CellRun; units: Cell, TwoPhase; filter: Cell)
  int R;                              // Cell: targets per lane
  long long cell_first, cell_end;     // clamped to the cells the target's start array covers
  bool make_list;                     // cell_units_kernel over [cell_first, cell_end) ...
  int chunk, min_cnt;
  bool bodies, pair_items;
  bool export_stats;                  // ... for its statistics alone: cell_units_export_kernel
  int per_xcd;                        // groups of four waves per XCD (BodySplit: of its wave-per-cell launch, `uper`)
  unsigned cell_grid, cell_block;     // the wave-per-cell launch
  unsigned body_blocks;               // Body, BodySplit, Body2: workgroups of kGridBlock lanes
  int W;                              // CellRun: cells per wave ...
  unsigned run_grid[3];               // ... and its 3-D grid
  unsigned stat_tick;                 // the handle's state afterwards
};

// THE AUTOMATIC CHOICE, per entry -- the three differ, as they always have:
//   Whole     automatic is tuning == 0 (tuning 1 asks for the cell-run kernel); rho = bodies / cells of the start array,
//             or of the WHOLE GRID where there is none (or it is empty); without a start array every tuning runs the
//             cell-run kernel.
//   TwoGrids  automatic is tuning < 2 (there is no cell-run form over two grids); rho = bodies / max(cells of the start
//   Layer     array, 1).  The start array is a precondition of the entry.
// In all three: below kBodyBelow bodies per cell one lane per body, split from kSplitFrom bodies; from there two targets
// per lane, filtered from kFilterFrom per cell when cutoff > the cell AS BUILT and from filter_from_inside otherwise.
// Which kernel runs is a function of the INPUT alone (body count, grid, cutoff): kernels of different shapes sum in
// different orders, and a choice that hung on statistics arriving asynchronously from earlier calls would make the bits
// depend on timing.  Between the cell range and the unit list of ONE shape the previous call's statistics do decide:
// those two are bit-identical.
inline int force_auto_tuning(double rho, size_t built_count, bool strict, double filter_from_inside) {
  if (rho < kBodyBelow) return built_count >= (size_t)kSplitFrom ? 9 : 8;
  return rho < (strict ? kFilterFrom : filter_from_inside) ? 3 : 6;
}

inline ForcePlan force_plan(ForceEntry entry, const ForceState& s) {
  ForcePlan p{};
  p.guard = s.guard;
  p.strict = s.cutoff > s.built_cell;  // judged on the grid AS BUILT: a pending set_cell_size only reaches the next build
  p.R = 2;
  p.stat_tick = s.stat_tick;
  p.cell_block = 64 * kCellWPB;
  int kern = s.tuning;
  long long c0 = s.cell_first, c1 = s.cell_end;
  if (entry == ForceEntry::Whole) {
    // cells per wave of the cell-run kernel: ~64 targets per wave at the mean occupancy
    const double rho = (double)(int)s.built_count / (double)(s.lb_valid && s.lb_count > 0 ? s.lb_count : s.info.total);
    int W = rho > 0 ? (int)(64.0 / rho + 0.5) : kMaxWv;
    if (W < 1) W = 1;
    if (W > kMaxWv) W = kMaxWv;
    p.W = W;
    p.run_grid[0] = (unsigned)((s.info.dims[0] + 4 * W - 1) / (4 * W));
    p.run_grid[1] = (unsigned)s.info.dims[1];
    p.run_grid[2] = (unsigned)s.info.dims[2];
    if (p.run_grid[1] > 65535u || p.run_grid[2] > 65535u) {  // (whatever the form: the parent's order)
      p.too_large = true;
      return p;
    }
    if (kern == 0) kern = s.lb_valid ? force_auto_tuning(rho, s.built_count, p.strict, s.filter_from_inside) : 1;
    if (kern == 1 || !s.lb_valid) {  // (no start arrays: the cell-run kernel)
      p.form = ForceForm::CellRun;
      return p;
    }
    c0 = s.lb_base;
    c1 = s.lb_base + s.lb_count;
  } else {
    // only cells the target grid's start array covers can hold targets
    if (c0 < s.lb_base) c0 = s.lb_base;
    if (c1 > s.lb_base + s.lb_count) c1 = s.lb_base + s.lb_count;
    if (kern < 2) {
      const double rho = (double)s.built_count / (double)(s.lb_count > 0 ? s.lb_count : 1);
      kern = force_auto_tuning(rho, s.built_count, p.strict, s.filter_from_inside);
    }
  }
  p.cell_first = c0;
  p.cell_end = c1;
  if (c1 <= c0) return p;
  const long long cells = c1 - c0;
  const long long nb = (long long)s.built_count;
  const bool listable = cells < kListCells;
  const auto cell_grid = [](int per_xcd) { return (unsigned)(per_xcd * 8 * (4 / kCellWPB)); };
  if (kern == 10 && (s.guard || !listable)) kern = 8;  // (eps ~ 0: the compare + select forms)
  if (kern == 10 || kern == 8 || kern == 9) {
    // 8: one lane per body for every body.  9 (the automatic form below kBodyBelow bodies per cell), SPLIT by cell: bodies
    // of cells with fewer than split_cnt bodies take one lane each; the cells of split_cnt and more -- the clumps of a
    // box that has clumped: cells of hundreds of bodies and windows of a thousand entries -- go on a work list and the
    // wave-per-cell kernel (two targets per lane) takes them.  The split is a function of the cell alone, so the result
    // is a function of the input alone; the list's length reaches the host one call late and only sizes the launch.
    // 10: two bodies of one cell per lane, every cell (see hash_body2_force_kernel).
    // (use_units does not reach the split: it chooses between two bit-identical forms, this is a kernel shape)
    p.form = kern == 10 ? ForceForm::Body2 : (kern == 8 || !listable) ? ForceForm::Body : ForceForm::BodySplit;
    if (!s.has_target) {
      p.needs_target = true;
      return p;
    }
    p.body_blocks = grid_blocks(nb);  // (Body2: at most one item per body)
    if (p.form == ForceForm::Body) return p;
    if (p.form == ForceForm::Body2) {
      p.make_list = true;
      p.chunk = 128; p.min_cnt = 0x7fffffff; p.bodies = true; p.pair_items = true;
      return p;
    }
    p.make_list = true;  // the crowded cells' units and the light cells' bodies, one pass over the cells
    p.chunk = 128; p.min_cnt = s.split_cnt; p.bodies = true;
    p.units = true;
    // (FILTER = false: the crowded cells take the unfiltered two-targets form.  The filtered one there: measured, not kept
    // -- 1.90 / 1.70 against 1.82 / 1.61 ms per step at 2,000 / 4,000 steps of the clumping box)
    p.per_xcd = unit_list_per_xcd(s.hint_mapped ? s.hint : 0, unit_list_bound(cells, nb, s.split_cnt, 128), 4096);  // (first call: a guess)
    p.cell_grid = cell_grid(p.per_xcd);
    return p;
  }
  p.form = kern == 5 ? ForceForm::Probe : kern == 7 ? ForceForm::TwoPhase : ForceForm::Cell;
  p.filter = kern == 6;
  p.R = (kern == 2 || kern == 7) ? 1 : (kern == 4 ? 4 : 2);  // (3, 6: two; 7: units of kUnitChunk2 = 64 bodies)
  static_assert(kUnitChunk2 == 64, "the two-phase kernel's units are the 64-body chunks of the one-body-per-lane list");
  const long long nblk = (cells + 4 * kCellsPerWave - 1) / (4 * kCellsPerWave);
  p.per_xcd = (int)((nblk + 7) / 8);
  // The unit list (occupied cells in chunks of 64 R bodies) is what the kernel takes when the previous call of this
  // kind saw crowded cells (> 64 bodies) or many empty ones; while the bodies are spread evenly it takes the cell range
  // itself and the list is only made every eighth call, for its statistics (list + export are 19 us at 4.2 M bodies).
  if (s.has_target && s.use_units && kern != 5 && listable) {
    const int hint = s.hint_mapped ? s.hint : 0, crowd = s.hint_mapped ? s.crowd : 0;
    p.units = s.use_units == 2 || (hint > 0 && (crowd > 64 || (long long)hint * 10 < cells * 9));
    if (p.units || (s.hint_mapped && (p.stat_tick++ & 7) == 0)) {
      p.make_list = true;
      p.chunk = 64 * p.R; p.min_cnt = 1;
      p.export_stats = !p.units;
    }
    if (p.units) {
      const long long bound = unit_list_bound(cells, nb, 1, 64 * p.R);
      p.per_xcd = unit_list_per_xcd(hint, bound, bound);
    }
  }
  // (two-phase form: workgroups of kGridBlock threads, four waves)
  p.cell_grid = p.form == ForceForm::TwoPhase ? (unsigned)(p.per_xcd * 8) : cell_grid(p.per_xcd);
  if (p.form == ForceForm::TwoPhase) p.cell_block = kGridBlock;
  return p;
}

// workgroups of cell_units_kernel over this many cells
inline unsigned unit_list_blocks(long long cells) {
  return (unsigned)((cells + kGridBlock * kUnitCells - 1) / (kGridBlock * kUnitCells));
}

}  // namespace nbh
