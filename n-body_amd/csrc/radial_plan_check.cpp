// radial_plan_check.cpp -- the host decisions of the radial profiles (radial_plan.h) on a CPU, under AddressSanitizer and
// UBSan (make radial_plan_check): the key bits against a count of the ordinals they have to tell apart, the chunk bound
// against the shells that random catalogues and random cuts make (the shell launches and partial records are sized from
// it), the launch sizes, the workspace table (regions in order, aligned, disjoint, large enough; a walk over them that
// touches every byte), and the validation of cuts and mode case by case.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "radial_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
#define EXPECT(cond, ...)              \
  do {                                 \
    checked++;                         \
    if (!(cond)) {                     \
      if (failures++ < 40) {           \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

int main() {
  // ---- the key bits: the ordinals 0 .. n_groups (n_groups + 1 values) must differ within the bits above the 32 of q
  EXPECT(radial_bits_for(1) == 0 && radial_bits_for(2) == 1 && radial_bits_for(3) == 2 && radial_bits_for(4) == 2 &&
             radial_bits_for(5) == 3, "bits_for at its first values");
  for (long long ng : {1LL, 2LL, 3LL, 4LL, 7LL, 8LL, 255LL, 256LL, 65535LL, 65536LL, 4194303LL, 4194304LL, kGroupMaxGroups}) {
    const int bits = radial_key_bits(ng);
    EXPECT(bits >= 33 && bits <= 64, "key bits %d for %lld groups", bits, ng);
    const int ob = bits - 32;
    EXPECT(ob == 63 || (ng >> ob) == 0, "the largest ordinal %lld fits %d bits", ng, ob);
    EXPECT(ob == 0 || (ng >> (ob - 1)) != 0, "%d bits are not one too many for %lld", ob, ng);
  }
  EXPECT(radial_key_bits(kGroupMaxGroups) == 63, "the largest catalogue: 31 ordinal bits");

  // ---- the chunk bound holds for the shells of any groups: cut random groups at random ranks
  std::mt19937_64 rng(2468);
  for (int trial = 0; trial < 20000; trial++) {
    long long members = 0, group_chunks_sum = 0, shell_chunks = 0;
    const int groups = 1 + (int)(rng() % 20);
    for (int g = 0; g < groups; g++) {
      const int kind = (int)(rng() % 4);
      const long long n = kind == 0   ? 1 + (long long)(rng() % kGroupSmall)
                          : kind == 1 ? kGroupSmall + 1 + (long long)(rng() % 70)
                          : kind == 2 ? (long long)kGroupChunk * (1 + (long long)(rng() % 4)) + (long long)(rng() % 3) - 1
                                      : 1 + (long long)(rng() % (3 * kGroupChunk));
      members += n;
      group_chunks_sum += group_chunks(n);
      const int cuts = 1 + (int)(rng() % kRadialMaxCuts);
      std::vector<long long> K(cuts);
      for (auto& k : K) k = kind == 1 && (rng() & 1) ? (long long)(rng() % 3) * (kGroupSmall + 1) % (n + 1) : (long long)(rng() % (n + 1));
      long long prev = 0;
      for (int c = 0; c < cuts; c++) {  // (K raised in cut order, as the row kernel raises it)
        const long long k = K[c] < prev ? prev : K[c];
        shell_chunks += group_chunks(k - prev);
        prev = k;
      }
    }
    // members positions of no group come on top: the bound only grows
    members += (long long)(rng() % 50);
    EXPECT(group_chunks_sum <= radial_chunk_bound(members), "%lld group chunks of %lld members", group_chunks_sum, members);
    EXPECT(shell_chunks <= radial_chunk_bound(members), "%lld shell chunks of %lld members", shell_chunks, members);
  }

  // ---- the plan: launch sizes and the workspace table
  const long long group_counts[] = {1, 2, 255, 256, 257, 1000, 1 << 20, 5000000, kGroupMaxGroups / 16};
  const long long member_counts[] = {0, 1, 33, 1024, 1025, 100000, 1 << 22, 123456789, kGroupMaxMembers};
  for (long long ng : group_counts)
    for (long long nm : member_counts)
      for (int nc : {1, 3, 16}) {
        const size_t sort_tmp = (size_t)(nm / 3 + 17), scan_tmp = 4099;
        const RadialPlan p = radial_plan(ng, nm, nc, sort_tmp, scan_tmp);
        EXPECT(p.n_groups == ng && p.n_members == nm && p.n_rows == ng * nc && p.n_cuts == nc, "plan(%lld, %lld, %d)", ng, nm, nc);
        EXPECT(p.n_rows <= kRadialMaxRows, "rows");
        EXPECT(p.key_bits == radial_key_bits(ng) && p.chunk_cap == radial_chunk_bound(nm), "bits and cap");
        auto covers = [](unsigned blocks, long long lanes) {
          return (long long)blocks * kGroupThreads >= lanes && ((long long)blocks - 1) * kGroupThreads < lanes;
        };
        EXPECT(covers(p.group_blocks, ng + 1), "group_blocks %u", p.group_blocks);
        EXPECT(nm == 0 ? p.member_blocks == 0 : covers(p.member_blocks, nm), "member_blocks %u", p.member_blocks);
        EXPECT(covers(p.row_blocks, p.n_rows + 1), "row_blocks %u", p.row_blocks);
        EXPECT(p.chunk_blocks <= kGroupMaxGrid && (long long)p.chunk_blocks <= p.chunk_cap &&
                   (p.chunk_cap == 0) == (p.chunk_blocks == 0), "chunk_blocks %u", p.chunk_blocks);
        EXPECT(p.combine_blocks <= kGroupMaxGrid && (p.chunk_cap == 0) == (p.combine_blocks == 0) &&
                   (p.combine_blocks == kGroupMaxGrid || (long long)p.combine_blocks * (kGroupThreads / 64) >= p.chunk_cap),
               "combine_blocks %u", p.combine_blocks);
        EXPECT(p.group_scan_count == (size_t)ng + 1 && p.row_scan_count == (size_t)p.n_rows + 1, "scan counts");
        const size_t g1 = (size_t)ng + 1, r1 = (size_t)p.n_rows + 1, m = (size_t)nm, c = (size_t)p.chunk_cap;
        const size_t offs[] = {p.off_flag, p.off_bad, p.off_nchunks, p.off_chunk_start, p.off_first, p.off_k, p.off_snchunks,
                               p.off_schunk_start, p.off_keys_in, p.off_keys_out, p.off_pos_in, p.off_pos_out, p.off_terms,
                               p.off_enclosed, p.off_ctotal, p.off_cbase, p.off_partials, p.off_sort_tmp, p.off_scan_tmp, p.bytes};
        const size_t need[] = {4, g1 * 4, g1 * 4, g1 * 4, g1 * 4, r1 * 4, r1 * 4, r1 * 4, m * 8, m * 8, m * 4, m * 4,
                               m * kRadialSums * 8, m * 8, c * 8, c * 8, c * kRadialSums * 8, sort_tmp, scan_tmp};
        constexpr int kRegions = (int)(sizeof(need) / sizeof(need[0]));
        static_assert(sizeof(offs) / sizeof(offs[0]) == kRegions + 1, "one offset per region and the end");
        EXPECT(offs[0] == 0, "the table starts at 0");
        for (int k = 0; k < kRegions; k++) {
          EXPECT(offs[k] % 256 == 0, "region %d aligned", k);
          EXPECT(offs[k + 1] >= offs[k] + need[k] && offs[k + 1] < offs[k] + need[k] + 256, "region %d holds %zu bytes", k, need[k]);
        }
      }
  {  // a small plan laid over real memory: every region written to its last byte, no byte twice
    const RadialPlan p = radial_plan(1000, 70000, 5, 12345, 777);
    std::vector<unsigned char> ws(p.bytes, 0);
    const size_t m = 70000, c = (size_t)p.chunk_cap;
    const size_t offs[] = {p.off_flag, p.off_bad, p.off_nchunks, p.off_chunk_start, p.off_first, p.off_k, p.off_snchunks,
                           p.off_schunk_start, p.off_keys_in, p.off_keys_out, p.off_pos_in, p.off_pos_out, p.off_terms,
                           p.off_enclosed, p.off_ctotal, p.off_cbase, p.off_partials, p.off_sort_tmp, p.off_scan_tmp};
    const size_t need[] = {4, 1001 * 4, 1001 * 4, 1001 * 4, 1001 * 4, 5001 * 4, 5001 * 4, 5001 * 4, m * 8, m * 8, m * 4, m * 4,
                           m * 32, m * 8, c * 8, c * 8, c * 32, 12345, 777};
    for (int k = 0; k < 19; k++)
      for (size_t b = 0; b < need[k]; b++) ws[offs[k] + b]++;
    size_t twice = 0;
    for (unsigned char v : ws) twice += v > 1;
    EXPECT(twice == 0, "%zu bytes belong to two regions", twice);
  }

  // ---- the cuts and the mode
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  {
    const double ok[] = {0.1, 0.5, 0.9, 1.0};
    EXPECT(radial_cuts_check(ok, 4, kRadialModeMass) == 0 && radial_cuts_check(ok, 4, kRadialModeNumber) == 0 &&
               radial_cuts_check(ok, 4, kRadialModeRadius) == 0, "legal cuts");
    EXPECT(radial_cuts_check(ok, 0, kRadialModeMass) == 1 && radial_cuts_check(ok, -1, kRadialModeMass) == 1, "n_cuts below 1");
    std::vector<double> many(kRadialMaxCuts + 1);
    for (int c = 0; c <= kRadialMaxCuts; c++) many[c] = (c + 1) / 32.0;
    EXPECT(radial_cuts_check(many.data(), kRadialMaxCuts, kRadialModeMass) == 0, "16 cuts");
    EXPECT(radial_cuts_check(many.data(), kRadialMaxCuts + 1, kRadialModeMass) == 1, "17 cuts");
    EXPECT(radial_cuts_check(ok, 4, 3) == 2 && radial_cuts_check(ok, 4, -1) == 2, "unknown mode");
    const double zero[] = {0.0, 0.5}, above[] = {0.5, 1.0000000000000002}, neg[] = {-0.0, 1.0}, hasnan[] = {0.5, nan};
    EXPECT(radial_cuts_check(zero, 2, kRadialModeMass) == 3 && radial_cuts_check(zero, 2, kRadialModeNumber) == 3, "fraction 0");
    EXPECT(radial_cuts_check(zero, 2, kRadialModeRadius) == 0 && radial_cuts_check(neg, 2, kRadialModeRadius) == 0, "radius 0");
    EXPECT(radial_cuts_check(above, 2, kRadialModeMass) == 3 && radial_cuts_check(above, 2, kRadialModeRadius) == 0, "above 1");
    EXPECT(radial_cuts_check(hasnan, 2, kRadialModeMass) == 3 && radial_cuts_check(hasnan, 2, kRadialModeRadius) == 3, "a NaN");
    const double negr[] = {-1.0, 1.0}, infs[] = {1.0, inf}, two_inf[] = {inf, inf}, equal[] = {0.5, 0.5}, down[] = {0.5, 0.25};
    EXPECT(radial_cuts_check(negr, 2, kRadialModeRadius) == 3, "a negative radius");
    EXPECT(radial_cuts_check(infs, 2, kRadialModeRadius) == 0 && radial_cuts_check(infs, 2, kRadialModeMass) == 3, "+inf");
    EXPECT(radial_cuts_check(two_inf, 2, kRadialModeRadius) == 4, "+inf twice");
    for (int mode = 0; mode < 3; mode++)
      EXPECT(radial_cuts_check(equal, 2, mode) == 4 && radial_cuts_check(down, 2, mode) == 4, "not strictly ascending, mode %d", mode);
    for (int why = 1; why <= 4; why++) EXPECT(radial_cuts_message(why)[0] != 0, "a message for %d", why);
  }
  if (failures) {
    std::printf("radial_plan_check: %d FAILURES in %lld checks\n", failures, checked);
    return 1;
  }
  std::printf("radial_plan_check: ok, %lld checks\n", checked);
  return 0;
}
