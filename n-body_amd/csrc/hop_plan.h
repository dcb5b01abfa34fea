// hop_plan.h -- the host decisions of the density-peak (HOP) groups (hop_groups.hip; the model is in
// include/nbody_hip_hop.h) as plain arithmetic: the validation of the arguments, the launch
// sizes, the passes of the pointer jumping, and the tables of the three workspaces.  Plain C++17, no HIP include:
// hop_check.cpp runs all of it on a CPU under AddressSanitizer and UBSan (make hop_check).
//
// hop_groups.hip derives a HopBodyPlan once per call from (count, the temporary storage rocPRIM asks for), and a
// HopRecordPlan once the record count has been read back; nothing here launches, allocates or reads device memory.
#pragma once

#include <cmath>
#include <cstddef>

#include "hop_common.h"

namespace nbh {

constexpr int kHopMaxK = 32;                          // NBODY_HIP_HOP_MAX_K
constexpr long long kHopMaxCount = 1LL << 30;         // bodies of a call
constexpr long long kHopMaxRecords = 0x7fffffffLL;    // directed boundary records of a call (the sort counts them in 31 bits)
constexpr int kHopThreads = 256;
constexpr int kHopJumpSteps = 64;                     // hops a lane follows in one pass of the pointer jumping
constexpr int kHopWords = 8;                          // 64-bit words the device hands the host (HopWord)
enum HopWord { kHopWordBad = 0, kHopWordRecords = 1, kHopWordPeaks = 2, kHopWordCandidates = 3, kHopWordAnchored = 4 };

// the parameters of a call, as nbody_hip_hop_params_t holds them
struct HopParams {
  int n_hop = 0, n_merge = 0, min_members = 0;
  double delta_outer = 0.0, delta_saddle = 0.0, delta_peak = 0.0;
};

// 0: legal; else why not
inline int hop_args_check(long long count, int k, const HopParams& p) {
  if (count < 1) return 1;
  if (count > kHopMaxCount) return 2;
  if (k < 1 || k > kHopMaxK) return 3;
  if (p.n_hop < 1 || p.n_hop > k) return 4;
  if (p.n_merge < 0 || p.n_merge > k) return 5;
  if (p.min_members < 1) return 6;
  if (!std::isfinite(p.delta_outer) || !std::isfinite(p.delta_saddle) || !std::isfinite(p.delta_peak)) return 7;
  if (!(0.0 <= p.delta_outer && p.delta_outer <= p.delta_saddle && p.delta_saddle <= p.delta_peak)) return 8;
  return 0;
}
inline const char* hop_args_message(int why) {
  switch (why) {
    case 1: return "Particle count must be greater than 0";
    case 2: return "body count exceeds 2^30";
    case 3: return "k must be 1 .. 32";
    case 4: return "n_hop must be 1 .. k";
    case 5: return "n_merge must be 0 .. k";
    case 6: return "min_members must be at least 1";
    case 7: return "the density thresholds must be finite";
    case 8: return "the density thresholds must satisfy 0 <= delta_outer <= delta_saddle <= delta_peak";
    default: return "";
  }
}

// slots of a row that the call reads at all: the bad-index check covers exactly these
inline int hop_read_slots(int n_hop, int n_merge) { return n_hop > n_merge ? n_hop : n_merge; }

// Passes of the pointer jumping.  A chain has at most count - 1 hops.  In one pass every lane follows up to
// kHopJumpSteps = 64 pointers and stores where it got to; whatever a pointer holds at any time is a body further along
// the chain, so after pass p a pointer is the peak or at least 64^p hops on: the least p with 64^p >= count - 1, and at
// least one pass.
inline int hop_jump_passes(long long count) {
  int p = 1;
  long long reach = kHopJumpSteps;
  while (reach < count - 1) {
    reach *= kHopJumpSteps;
    p++;
  }
  return p;
}

inline size_t hop_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline unsigned hop_blocks(long long lanes) { return (unsigned)((lanes + kHopThreads - 1) / kHopThreads); }

// The per-body workspace (ctx->hop): byte offsets from its 256-byte aligned start.
struct HopBodyPlan {
  long long count = 0;
  int qbits = 0;               // hop_bits_for(count): the edge key is (P << qbits) | Q
  int jump_passes = 0;
  unsigned body_blocks = 0;    // one lane per body
  unsigned scan_blocks = 0;    // one lane per entry of the record scan (count + 1)
  size_t scan_count = 0;       // count + 1
  size_t off_words = 0;        // kHopWords 64-bit words
  size_t off_select_count = 0; // one unsigned int: what the selection of the candidates counted
  size_t off_edge_count = 0;   // one unsigned int: the unique edges
  size_t off_catalogue_counts = 0;  // two 64-bit words: {n_groups, n_members}
  size_t off_next = 0;         // int per body: next, then peak
  size_t off_nrec = 0;         // int per body + 1: directed records the body writes
  size_t off_rstart = 0;       // 64-bit per body + 1: records before the body
  size_t off_root = 0;         // int per body: the union-find of the viable peaks, then root
  size_t off_anchor = 0;       // int per body: -1, or the round the peak was anchored in (0: viable)
  size_t off_estart = 0;       // int per body: -1, or where the peak's unique edges begin
  size_t off_cand_flags = 0;   // char per body: a live peak that is not viable
  size_t off_cand = 0;         // int per body: those peaks, ascending
  size_t off_labels = 0;       // int per body
  size_t off_sizes = 0;        // int per body: bodies per label, then the scan of the head flags
  size_t off_best_rho = 0;     // 64-bit per body: the greatest peak density bits of a root
  size_t off_best_peak = 0;    // int per body: the lowest peak of that density
  size_t off_keys_a = 0, off_keys_b = 0;  // unsigned int per body: the catalogue's sort keys (a: then the head flags)
  size_t off_body = 0;         // int per body: 0, 1, 2 ...
  size_t off_tmp = 0;          // the temporary storage of the scans, the selection and the catalogue's sort
  size_t bytes = 0;
};

// tmp_bytes: the largest temporary storage any rocPRIM call over the bodies asks for
inline HopBodyPlan hop_body_plan(long long count, size_t tmp_bytes) {
  HopBodyPlan p;
  p.count = count;
  p.qbits = hop_bits_for(count);
  p.jump_passes = hop_jump_passes(count);
  p.body_blocks = hop_blocks(count);
  p.scan_blocks = hop_blocks(count + 1);
  p.scan_count = (size_t)count + 1;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t off = at;
    at += hop_align(bytes);
    return off;
  };
  const size_t n = (size_t)count, n1 = n + 1;
  p.off_words = take(kHopWords * sizeof(long long));
  p.off_select_count = take(sizeof(unsigned int));
  p.off_edge_count = take(sizeof(unsigned int));
  p.off_catalogue_counts = take(2 * sizeof(long long));
  p.off_next = take(n * sizeof(int));
  p.off_nrec = take(n1 * sizeof(int));
  p.off_rstart = take(n1 * sizeof(long long));
  p.off_root = take(n * sizeof(int));
  p.off_anchor = take(n * sizeof(int));
  p.off_estart = take(n * sizeof(int));
  p.off_cand_flags = take(n * sizeof(char));
  p.off_cand = take(n * sizeof(int));
  p.off_labels = take(n * sizeof(int));
  p.off_sizes = take(n * sizeof(int));
  p.off_best_rho = take(n * sizeof(unsigned long long));
  p.off_best_peak = take(n * sizeof(int));
  p.off_keys_a = take(n * sizeof(unsigned int));
  p.off_keys_b = take(n * sizeof(unsigned int));
  p.off_body = take(n * sizeof(int));
  p.off_tmp = take(tmp_bytes);
  p.bytes = at;
  return p;
}

// The catalogue the context keeps between calls (ctx->hop_catalogue).
struct HopCataloguePlan {
  size_t off_offsets = 0;     // int per body + 1
  size_t off_members = 0;     // int per body
  size_t off_group_peak = 0;  // int per body
  size_t bytes = 0;
};
inline HopCataloguePlan hop_catalogue_plan(long long count) {
  HopCataloguePlan p;
  const size_t n = (size_t)count;
  p.off_offsets = 0;
  p.off_members = hop_align((n + 1) * sizeof(int));
  p.off_group_peak = p.off_members + hop_align(n * sizeof(int));
  p.bytes = p.off_group_peak + hop_align(n * sizeof(int));
  return p;
}

// The workspace of the boundary records (ctx->hop_records), sized once their number is known.  The unique edges and
// their maxima are written over the unsorted pairs, which are dead once the sort has run.
struct HopRecordPlan {
  long long records = 0;
  int key_bits = 0;            // the sort orders bits [0, 2 qbits)
  unsigned record_blocks = 0;  // one lane per record (and per unique edge: there are no more edges than records)
  size_t off_keys_in = 0, off_vals_in = 0;    // the records as written; then the unique edges' keys and maxima
  size_t off_keys_out = 0, off_vals_out = 0;  // the records sorted
  size_t off_tmp = 0;          // the temporary storage of the sort and of the segmented maximum
  size_t bytes = 0;
};
inline HopRecordPlan hop_record_plan(long long records, int qbits, size_t tmp_bytes) {
  HopRecordPlan p;
  p.records = records;
  p.key_bits = 2 * qbits;
  p.record_blocks = hop_blocks(records);
  const size_t r = (size_t)records * sizeof(unsigned long long);
  p.off_keys_in = 0;
  p.off_vals_in = hop_align(r);
  p.off_keys_out = p.off_vals_in + hop_align(r);
  p.off_vals_out = p.off_keys_out + hop_align(r);
  p.off_tmp = p.off_vals_out + hop_align(r);
  p.bytes = p.off_tmp + hop_align(tmp_bytes);
  return p;
}

}  // namespace nbh
