// group_props_plan_check.cpp -- the host decisions of the group properties (group_props_plan.h) on a CPU, under
// AddressSanitizer and UBSan (make group_props_plan_check): the chunk count of a group against a member-by-member cut,
// the chunk bound against every catalogue of disjoint ranges that random draws and the worst cases make (the launches
// and the partial records are sized from it, so a catalogue that exceeded it would lose groups), the launch sizes, and
// the workspace table (regions in order, aligned, disjoint, large enough; a walk over them that touches every byte).
// With `sizes` as its argument it prints S and C for the tests that mirror them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "group_props_plan.h"

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

// a group cut member by member: position p belongs to chunk p / C
static int chunks_by_members(long long n) {
  if (n <= kGroupSmall) return 0;
  int chunks = 0;
  long long last = -1;
  for (long long p = 0; p < n; p++) {
    const long long k = p / kGroupChunk;
    if (k != last) chunks++;
    last = k;
  }
  return chunks;
}

static void check_bound(const std::vector<long long>& sizes, const char* what) {
  long long members = 0, chunks = 0;
  for (long long n : sizes) {
    members += n;
    chunks += group_chunks(n);
  }
  EXPECT(chunks <= group_chunk_bound(members), "%s: %lld chunks of %lld members, bound %lld", what, chunks, members,
         group_chunk_bound(members));
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "sizes") == 0) {
    std::printf("S %d C %d threads %d\n", kGroupSmall, kGroupChunk, kGroupThreads);
    return 0;
  }
  // ---- the chunks of a group
  for (long long n = 0; n <= 5 * kGroupChunk + 3; n++)
    EXPECT(group_chunks(n) == chunks_by_members(n), "group_chunks(%lld) = %d", n, group_chunks(n));
  EXPECT(group_chunks(kGroupSmall) == 0 && group_chunks(kGroupSmall + 1) == 1, "the threshold");
  EXPECT(group_chunks(kGroupChunk) == 1 && group_chunks(kGroupChunk + 1) == 2, "the chunk edge");
  EXPECT(group_chunks(kGroupMaxMembers) == (int)((kGroupMaxMembers - 1) / kGroupChunk + 1), "the largest group");

  // ---- the bound: worst cases first (as many groups of S + 1 as fit; one group of everything; chunk edges), then draws
  for (long long members : {0LL, 1LL, 32LL, 33LL, 34LL, 65LL, 66LL, 1023LL, 1024LL, 1025LL, 1057LL, 1058LL, 2048LL, 2049LL,
                            33LL * 1024, 33LL * 1024 + 1, 1000003LL}) {
    std::vector<long long> s(members / (kGroupSmall + 1), kGroupSmall + 1);
    if (members % (kGroupSmall + 1)) s.push_back(members % (kGroupSmall + 1));
    check_bound(s, "groups of S + 1");
    check_bound({members}, "one group");
    if (members > kGroupChunk + 1) {
      std::vector<long long> t(members / (kGroupChunk + 1), kGroupChunk + 1);
      t.push_back(members % (kGroupChunk + 1));
      check_bound(t, "groups of C + 1");
    }
  }
  std::mt19937_64 rng(12345);
  for (int trial = 0; trial < 20000; trial++) {
    std::vector<long long> s;
    const int groups = 1 + (int)(rng() % 40);
    for (int g = 0; g < groups; g++) {
      const int kind = (int)(rng() % 5);
      long long n = kind == 0   ? 1 + (long long)(rng() % kGroupSmall)
                    : kind == 1 ? kGroupSmall + 1 + (long long)(rng() % 3)
                    : kind == 2 ? (long long)kGroupChunk * (1 + (long long)(rng() % 4)) + (long long)(rng() % 3) - 1
                    : kind == 3 ? 1 + (long long)(rng() % (3 * kGroupChunk))
                                : kGroupSmall + 1;
      s.push_back(n);
    }
    check_bound(s, "random catalogue");
  }

  // ---- the plan: launch sizes and the workspace table
  const long long group_counts[] = {1, 2, 255, 256, 257, 1000, 1 << 20, 5000000, kGroupMaxGroups};
  const long long member_counts[] = {0, 1, 33, 1024, 1025, 100000, 1 << 22, 123456789, kGroupMaxMembers};
  for (long long ng : group_counts)
    for (long long nm : member_counts)
      for (size_t tmp : {(size_t)0, (size_t)1, (size_t)4096, (size_t)1000001}) {
        const GroupPropsPlan p = group_props_plan(ng, nm, tmp);
        EXPECT(p.n_groups == ng && p.n_members == nm && p.chunk_cap == group_chunk_bound(nm), "plan(%lld, %lld)", ng, nm);
        EXPECT((long long)p.count_blocks * kGroupThreads >= ng + 1 && ((long long)p.count_blocks - 1) * kGroupThreads < ng + 1,
               "count_blocks %u for %lld groups", p.count_blocks, ng);
        EXPECT((long long)p.small_blocks * kGroupThreads >= ng && ((long long)p.small_blocks - 1) * kGroupThreads < ng,
               "small_blocks %u for %lld groups", p.small_blocks, ng);
        EXPECT(p.chunk_blocks <= kGroupMaxGrid && (long long)p.chunk_blocks <= p.chunk_cap &&
                   (p.chunk_cap == 0) == (p.chunk_blocks == 0),
               "chunk_blocks %u at cap %lld", p.chunk_blocks, p.chunk_cap);
        EXPECT(p.combine_blocks <= kGroupMaxGrid && (p.chunk_cap == 0) == (p.combine_blocks == 0) &&
                   (p.combine_blocks == kGroupMaxGrid ||
                    (long long)p.combine_blocks * (kGroupThreads / 64) >= p.chunk_cap),
               "combine_blocks %u at cap %lld", p.combine_blocks, p.chunk_cap);
        EXPECT(p.scan_count == (size_t)ng + 1, "scan_count");
        const size_t offs[] = {p.off_nchunks, p.off_chunk_start, p.off_bad, p.off_partials, p.off_scan_tmp, p.bytes};
        const size_t need[] = {((size_t)ng + 1) * 4, ((size_t)ng + 1) * 4, (size_t)ng * 4,
                               (size_t)p.chunk_cap * kGroupPartialDoubles * 8, tmp};
        EXPECT(offs[0] == 0, "the table starts at 0");
        for (int k = 0; k < 5; k++) {
          EXPECT(offs[k] % 256 == 0, "region %d aligned", k);
          EXPECT(offs[k + 1] >= offs[k] + need[k] && offs[k + 1] < offs[k] + need[k] + 256, "region %d holds %zu bytes", k, need[k]);
        }
      }
  // a small plan laid over real memory: every region written to its last byte, no byte twice (the sanitizer watches the ends)
  {
    const GroupPropsPlan p = group_props_plan(1000, 70000, 777);
    std::vector<unsigned char> ws(p.bytes, 0);
    const size_t offs[] = {p.off_nchunks, p.off_chunk_start, p.off_bad, p.off_partials, p.off_scan_tmp};
    const size_t need[] = {1001 * 4, 1001 * 4, 1000 * 4, (size_t)p.chunk_cap * kGroupPartialDoubles * 8, 777};
    for (int k = 0; k < 5; k++)
      for (size_t b = 0; b < need[k]; b++) ws[offs[k] + b]++;
    size_t twice = 0;
    for (unsigned char c : ws) twice += c > 1;
    EXPECT(twice == 0, "%zu bytes belong to two regions", twice);
  }
  if (failures) {
    std::printf("group_props_plan_check: %d FAILURES in %lld checks\n", failures, checked);
    return 1;
  }
  std::printf("group_props_plan_check: ok, %lld checks (S = %d, C = %d)\n", checked, kGroupSmall, kGroupChunk);
  return 0;
}
