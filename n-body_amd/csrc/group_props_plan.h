// group_props_plan.h -- the host decisions of the group properties pass (group_props.hip; the model is in
// include/nbody_hip_group_props.h) as plain arithmetic: the two sizes S and C that say which form a
// group takes, the chunks of a group, the bound on the chunks of a call that the host can know without reading the
// catalogue back, the launch sizes, and the table of the workspace.  Plain C++17, no HIP include:
// group_props_plan_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make group_props_plan_check).
//
// group_props.hip derives a GroupPropsPlan ONCE per call and issues its launches from it; nothing here launches,
// allocates or reads device memory.  group_chunks carries NBH_GP_HD: the kernels cut a group exactly as the plan counts.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define NBH_GP_HD __host__ __device__
#else
#define NBH_GP_HD
#endif

namespace nbh {

// A group of at most kGroupSmall (S) members is summed by ONE LANE, serially in member order.
constexpr int kGroupSmall = 32;
// A larger group is cut into chunks of kGroupChunk (C) members counted from the group's own start (the last chunk may
// be shorter); one workgroup of kGroupThreads sums a chunk, every thread kGroupChunk / kGroupThreads members.
constexpr int kGroupChunk = 1024;
constexpr int kGroupThreads = 256;
constexpr int kGroupPerThread = kGroupChunk / kGroupThreads;
static_assert(kGroupChunk % kGroupThreads == 0 && kGroupThreads % 64 == 0 && kGroupSmall < kGroupChunk, "chunk shape");
// The chunk kernels walk the chunks of a call with a stride of their grid: at most this many workgroups are launched
// (8 per compute unit of a 256-unit device), however many chunks there are.  Which workgroup sums a chunk changes no
// bit: a chunk is summed by one workgroup, whichever.
constexpr long long kGroupMaxGrid = 2048;
// doubles of one chunk's partial record: pass 1 uses the first 7 {m, m x[3], m v[3]}, pass 2 all of them
// {L[3], 2K, I[6], 2W, r2 max, phi min, {r2 body, phi body} as two ints in one double's place}
constexpr int kGroupPartialDoubles = 14;

constexpr long long kGroupMaxMembers = 0x7fffffffLL;  // offsets are ints
constexpr long long kGroupMaxGroups = 0x7ffffffeLL;   // n_groups + 1 offsets, counted in an int

// chunks of a group of n members: 0 for the small form
NBH_GP_HD inline int group_chunks(long long n) {
  return n > kGroupSmall ? (int)((n + kGroupChunk - 1) / kGroupChunk) : 0;
}

// What the host knows of the chunks of a call.  A group in the chunked form has more than S members, so a catalogue of
// DISJOINT ranges has L <= n_members / (S + 1) of them, and a group of n members has (n - 1) / C + 1 chunks (integer
// division) <= (n - 1) / C + 1 (real): together at most n_members / C - L / C + L, whose floor is at most
// floor(n_members / C) + L.  Ranges that OVERLAP can exceed this bound: the kernels never sum a chunk number at or above
// it (chunk_cap below) and give the groups that reach beyond it status 1.
inline long long group_chunk_bound(long long n_members) {
  return n_members / kGroupChunk + n_members / (kGroupSmall + 1);
}

inline size_t group_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct GroupPropsPlan {
  long long n_groups = 0, n_members = 0;
  long long chunk_cap = 0;        // partial records allocated: no chunk number at or above it is ever summed
  unsigned count_blocks = 0;      // one lane per entry of the scan (n_groups + 1), kGroupThreads a workgroup
  unsigned small_blocks = 0;      // one lane per group: the small-form kernel
  unsigned chunk_blocks = 0;      // workgroups of the two chunk kernels (0: no group can be in the chunked form)
  unsigned combine_blocks = 0;    // one WAVE per chunk number, kGroupThreads / 64 waves a workgroup
  size_t scan_count = 0;          // n_groups + 1: the last entry of the scan is the number of chunks
  // the workspace, byte offsets from its (256-byte aligned) start
  size_t off_nchunks = 0, off_chunk_start = 0, off_bad = 0, off_partials = 0, off_scan_tmp = 0, bytes = 0;
};

// scan_tmp_bytes: the temporary storage rocprim's exclusive scan asks for at scan_count entries
inline GroupPropsPlan group_props_plan(long long n_groups, long long n_members, size_t scan_tmp_bytes) {
  GroupPropsPlan p;
  p.n_groups = n_groups;
  p.n_members = n_members;
  p.chunk_cap = group_chunk_bound(n_members);
  p.count_blocks = (unsigned)((n_groups + 1 + kGroupThreads - 1) / kGroupThreads);
  p.small_blocks = (unsigned)((n_groups + kGroupThreads - 1) / kGroupThreads);
  p.chunk_blocks = (unsigned)(p.chunk_cap < kGroupMaxGrid ? p.chunk_cap : kGroupMaxGrid);
  const long long waves = kGroupThreads / 64;
  const long long cb = (p.chunk_cap + waves - 1) / waves;
  p.combine_blocks = (unsigned)(cb < kGroupMaxGrid ? cb : kGroupMaxGrid);
  p.scan_count = (size_t)n_groups + 1;
  size_t at = 0;
  p.off_nchunks = at;
  at += group_align(p.scan_count * sizeof(int));
  p.off_chunk_start = at;
  at += group_align(p.scan_count * sizeof(int));
  p.off_bad = at;
  at += group_align((size_t)n_groups * sizeof(int));
  p.off_partials = at;
  at += group_align((size_t)p.chunk_cap * kGroupPartialDoubles * sizeof(double));
  p.off_scan_tmp = at;
  at += group_align(scan_tmp_bytes);
  p.bytes = at;
  return p;
}

}  // namespace nbh
