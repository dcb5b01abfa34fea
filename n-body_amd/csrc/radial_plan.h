// radial_plan.h -- the host decisions of the radial profile pass (radial_profile.hip; the model is in
// include/nbody_hip_radial.h) as plain arithmetic: the key bits the sort has to order, the bound
// on the chunks of groups and of shells that the host can know without reading anything back, the launch sizes, the
// table of the workspace, and the validation of the cuts and the mode.  Plain C++17, no HIP include:
// radial_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make radial_plan_check).
//
// radial_profile.hip derives a RadialPlan ONCE per call and issues its launches from it; nothing here launches,
// allocates or reads device memory.  The two forms (S = 32, C = 1,024), the chunks of a range and the chunk bound are
// those of group_props_plan.h: a shell is a group of the sorted list.
#pragma once

#include <cmath>
#include <cstddef>

#include "group_props_plan.h"

namespace nbh {

constexpr int kRadialMaxCuts = 16;  // NBODY_HIP_RADIAL_MAX_CUTS
constexpr int kRadialModeMass = 0, kRadialModeNumber = 1, kRadialModeRadius = 2;  // NBODY_HIP_RADIAL_*
constexpr long long kRadialMaxRows = 0x7fffffffLL;  // shell rows of a call: n_groups * n_cuts, counted in an int
// doubles of one shell chunk's partial record: the four sums
constexpr int kRadialSums = 4;

// bits needed to tell the values 0 .. v - 1 apart (v >= 1): bits_for(1) = 0, bits_for(2) = 1, bits_for(3) = 2
inline int radial_bits_for(long long v) {
  int b = 0;
  while (b < 63 && (1LL << b) < v) b++;
  return b;
}
// The key of a position is (group ordinal << 32) | bits(q); the ordinals are 0 .. n_groups, n_groups being the key of a
// position in no group: n_groups + 1 values.  The sort orders bits [0, radial_key_bits).
inline int radial_key_bits(long long n_groups) { return 32 + radial_bits_for(n_groups + 1); }

// What the host knows of the chunks of a call.  The groups of an ORDERED catalogue are disjoint ranges of the n_members
// positions, and the shells of a group are disjoint ranges of its ranks: either way ranges of more than S entries that
// hold at most n_members entries between them, so group_chunk_bound holds for the groups' chunks and for the shells'.
// (A catalogue that is not ordered never reaches a chunk: every group of the call is bad.)
inline long long radial_chunk_bound(long long n_members) { return group_chunk_bound(n_members); }

// 0: the cuts and the mode are legal; else why not (1 n_cuts, 2 mode, 3 a cut out of range, 4 not strictly ascending)
inline int radial_cuts_check(const double* cuts, int n_cuts, int mode) {
  if (n_cuts < 1 || n_cuts > kRadialMaxCuts) return 1;
  if (mode != kRadialModeMass && mode != kRadialModeNumber && mode != kRadialModeRadius) return 2;
  for (int c = 0; c < n_cuts; c++) {
    const double v = cuts[c];
    if (mode == kRadialModeRadius) {
      if (!(v >= 0.0)) return 3;  // (a NaN too; +inf is legal)
    } else {
      if (!(v > 0.0 && v <= 1.0)) return 3;
    }
    if (c > 0 && !(cuts[c - 1] < v)) return 4;
  }
  return 0;
}
inline const char* radial_cuts_message(int why) {
  switch (why) {
    case 1: return "n_cuts must be 1 .. 16";
    case 2: return "unknown radial mode";
    case 3: return "a cut is out of range: fractions lie in (0, 1], radii are >= 0";
    case 4: return "the cuts must be strictly ascending";
    default: return "";
  }
}

struct RadialPlan {
  long long n_groups = 0, n_members = 0, n_rows = 0;
  int n_cuts = 0;
  int key_bits = 0;               // the sort orders bits [0, key_bits) of the 64-bit keys
  long long chunk_cap = 0;        // records allocated per chunk table: no chunk number at or above it is ever touched
  unsigned group_blocks = 0;      // one lane per entry of the group scan (n_groups + 1)
  unsigned member_blocks = 0;     // one lane per position of members (0: no position)
  unsigned row_blocks = 0;        // one lane per entry of the shell scan (n_rows + 1)
  unsigned chunk_blocks = 0;      // workgroups of the chunk kernels (0: nothing can be in the chunked form)
  unsigned combine_blocks = 0;    // one WAVE per chunk number
  size_t group_scan_count = 0;    // n_groups + 1
  size_t row_scan_count = 0;      // n_rows + 1
  // the workspace, byte offsets from its (256-byte aligned) start
  size_t off_flag = 0;                                                     // one int: the catalogue is not ordered
  size_t off_bad = 0, off_nchunks = 0, off_chunk_start = 0, off_first = 0;  // per group (+ 1)
  size_t off_k = 0, off_snchunks = 0, off_schunk_start = 0;                 // per shell row (+ 1)
  size_t off_keys_in = 0, off_keys_out = 0, off_pos_in = 0, off_pos_out = 0;  // per member: the sort's pairs
  size_t off_terms = 0;                                                    // per member: 4 doubles, term-major
  size_t off_enclosed = 0;                                                 // per member: E
  size_t off_ctotal = 0, off_cbase = 0;                                    // per group chunk
  size_t off_partials = 0;                                                 // per shell chunk: kRadialSums doubles
  size_t off_sort_tmp = 0, off_scan_tmp = 0, bytes = 0;
};

// sort_tmp_bytes / scan_tmp_bytes: the temporary storage the sort asks for at n_members pairs and key_bits bits, and the
// larger of what the exclusive scan asks for at n_groups + 1 and at n_rows + 1 entries
inline RadialPlan radial_plan(long long n_groups, long long n_members, int n_cuts, size_t sort_tmp_bytes,
                              size_t scan_tmp_bytes) {
  RadialPlan p;
  p.n_groups = n_groups;
  p.n_members = n_members;
  p.n_cuts = n_cuts;
  p.n_rows = n_groups * n_cuts;
  p.key_bits = radial_key_bits(n_groups);
  p.chunk_cap = radial_chunk_bound(n_members);
  auto blocks = [](long long lanes) { return (unsigned)((lanes + kGroupThreads - 1) / kGroupThreads); };
  p.group_blocks = blocks(n_groups + 1);
  p.member_blocks = blocks(n_members);
  p.row_blocks = blocks(p.n_rows + 1);
  p.chunk_blocks = (unsigned)(p.chunk_cap < kGroupMaxGrid ? p.chunk_cap : kGroupMaxGrid);
  const long long waves = kGroupThreads / 64;
  const long long cb = (p.chunk_cap + waves - 1) / waves;
  p.combine_blocks = (unsigned)(cb < kGroupMaxGrid ? cb : kGroupMaxGrid);
  p.group_scan_count = (size_t)n_groups + 1;
  p.row_scan_count = (size_t)p.n_rows + 1;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t off = at;
    at += group_align(bytes);
    return off;
  };
  const size_t g1 = p.group_scan_count, r1 = p.row_scan_count, m = (size_t)n_members, c = (size_t)p.chunk_cap;
  p.off_flag = take(sizeof(int));
  p.off_bad = take(g1 * sizeof(int));
  p.off_nchunks = take(g1 * sizeof(int));
  p.off_chunk_start = take(g1 * sizeof(int));
  p.off_first = take(g1 * sizeof(int));
  p.off_k = take(r1 * sizeof(int));
  p.off_snchunks = take(r1 * sizeof(int));
  p.off_schunk_start = take(r1 * sizeof(int));
  p.off_keys_in = take(m * sizeof(unsigned long long));
  p.off_keys_out = take(m * sizeof(unsigned long long));
  p.off_pos_in = take(m * sizeof(int));
  p.off_pos_out = take(m * sizeof(int));
  p.off_terms = take(m * kRadialSums * sizeof(double));
  p.off_enclosed = take(m * sizeof(double));
  p.off_ctotal = take(c * sizeof(double));
  p.off_cbase = take(c * sizeof(double));
  p.off_partials = take(c * kRadialSums * sizeof(double));
  p.off_sort_tmp = take(sort_tmp_bytes);
  p.off_scan_tmp = take(scan_tmp_bytes);
  p.bytes = at;
  return p;
}

}  // namespace nbh
