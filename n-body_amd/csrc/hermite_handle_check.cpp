// hermite_handle_check.cpp -- the carve of hermite_carve.h on a CPU, under AddressSanitizer and UBSan (make handle_check):
// lists of (count, element size) against the chain the handles used to write out, o_next = o + up256(count * size).
// Every offset a multiple of 256, the regions in order and disjoint, the total the sum of the rounded sizes; and the
// typed form against a real allocation, every region written end to end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hermite_carve.h"

using nbh::Carve;

static int failures = 0;
#define EXPECT(cond, ...)             \
  do {                                \
    if (!(cond)) {                    \
      failures++;                     \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);       \
      std::printf("\n");              \
    }                                 \
  } while (0)

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Region {
  size_t count, elem;
};

static void check_list(const std::vector<Region>& list) {
  Carve c;
  size_t chain = 0, prev_end = 0;
  for (size_t k = 0; k < list.size(); k++) {
    const size_t at = c.reserve(list[k].count, list[k].elem);
    const size_t bytes = list[k].count * list[k].elem;
    EXPECT(at == chain, "region %zu at %zu, the chain says %zu", k, at, chain);
    EXPECT(at % 256 == 0, "region %zu at %zu is not 256-byte aligned", k, at);
    EXPECT(at >= prev_end, "region %zu at %zu overlaps its predecessor, which ends at %zu", k, at, prev_end);
    prev_end = at + bytes;
    chain += up256(bytes);
    EXPECT(c.total() == chain && c.total() >= prev_end, "total %zu after region %zu, the chain says %zu", c.total(), k, chain);
  }
}

struct E16 { char b[16]; };
struct E64 { char b[64]; };
struct E152 { char b[152]; };

// the typed form on a real allocation: one region of each element size, `count` elements each (0: an empty region)
static void check_typed(size_t count) {
  char* p1 = nullptr;
  float* p4 = nullptr;
  double* p8 = nullptr;
  E16* p16 = nullptr;
  E64* p64 = nullptr;
  E152* p152 = nullptr;
  Carve c;
  c.add(&p1, count);
  c.add(&p4, count);
  c.add(&p8, count);
  c.add(&p16, count);
  c.add(&p64, count);
  c.add(&p152, count);
  size_t want = 0;
  for (size_t e : {1, 4, 8, 16, 64, 152}) want += up256(count * e);
  EXPECT(c.total() == want, "typed total %zu for count %zu, the chain says %zu", c.total(), count, want);
  char* base = static_cast<char*>(std::aligned_alloc(256, c.total() ? c.total() : 256));
  c.place(base);
  char* const got[6] = {p1, reinterpret_cast<char*>(p4), reinterpret_cast<char*>(p8), reinterpret_cast<char*>(p16),
                        reinterpret_cast<char*>(p64), reinterpret_cast<char*>(p152)};
  const size_t elem[6] = {1, 4, 8, 16, 64, 152};
  size_t at = 0;
  for (int k = 0; k < 6; k++) {
    EXPECT(got[k] == base + at, "typed region %d of count %zu at %td, the chain says %zu", k, count, got[k] - base, at);
    std::memset(got[k], 0x5a, count * elem[k]);  // (the sanitizer sees a region that leaves the allocation)
    at += up256(count * elem[k]);
  }
  std::free(base);
}

int main() {
  const size_t elems[] = {1, 4, 8, 16, 64, 152};
  const size_t counts[] = {0, 1, 15, 16, 17, 63, 64, 65, 4096, ((size_t)1 << 30) - 1};
  // every (count, size) alone, every ordered pair of them, and one list of all sixty
  std::vector<Region> all;
  for (size_t c : counts)
    for (size_t e : elems) all.push_back(Region{c, e});
  for (const Region& a : all) {
    check_list({a});
    for (const Region& b : all) check_list({a, b, a});
  }
  check_list(all);
  // the lists of the handles at capacities around a rounding boundary: block (n), ensemble (n, B), events (n, B)
  for (size_t n : {(size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)63, (size_t)64, (size_t)65, (size_t)4096,
                   ((size_t)1 << 30) - 1})
    for (size_t B : {(size_t)1, n}) {
      check_list({{n, 16}, {n, 4}, {n, 4}, {n, 4}, {n, 4}, {2, 4}, {1, 4}, {22, 8}, {1, 48}});
      check_list({{n, 16}, {n, 4}, {n, 4}, {n, 4}, {n, 4}, {3 * n, 16}, {n, 12}, {B, 24}, {B, 4}, {B, 4}, {B, 32}, {B * 22, 8},
                  {B + 1, 8}});
      check_list({{n, 4}, {B, 8}, {B, 64}});
    }
  for (size_t count : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)63, (size_t)64, (size_t)65, (size_t)4096})
    check_typed(count);
  if (failures) {
    std::printf("hermite_handle_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("hermite_handle_check: ok\n");
  return 0;
}
