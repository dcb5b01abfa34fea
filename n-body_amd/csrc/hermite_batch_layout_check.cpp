// hermite_batch_layout_check.cpp -- the host arithmetic of an ensemble layout (hermite_batch_layout.h) on a CPU: the rules
// of nbody_hip_hermite_batch_set_layout and the offsets, items and workspace sizes derived from a layout, checked against
// a restatement.  Built with -fsanitize=address,undefined by `make layout_check` (no GPU, no HIP): every vector access
// below is then bounds-checked.  Exit code = number of failed checks.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hermite_batch_layout.h"

using namespace nbh;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    g_checks++;                                                                            \
    if (!(cond)) { g_fail++; std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static int check(const std::vector<size_t>& off, size_t max_systems, size_t max_particles, const char* wanted) {
  char msg[256] = "";
  const int rc = batch_layout_check(off.data(), off.size() - 1, max_systems, max_particles, msg, sizeof(msg));
  if (wanted && !std::strstr(msg, wanted)) {
    std::printf("  message \"%s\" lacks \"%s\"\n", msg, wanted);
    return -1;
  }
  return rc;
}

// a layout against its restatement: every body belongs to the system that holds it, the rows of the systems do not
// overlap and end inside the workspace, every (target block, tile) of every system is an item exactly once
static void verify(const std::vector<size_t>& off) {
  const size_t B = off.size() - 1;
  const BatchLayout lay = batch_layout_build(off.data(), B);
  CHECK(lay.sys.size() == B && lay.body_system.size() == off[B]);
  size_t adv = 0, prime = 0, items = 0;
  for (size_t s = 0; s < B; s++) {
    const size_t n = off[s + 1] - off[s];
    CHECK((size_t)lay.sys[s].first == off[s] && (size_t)lay.sys[s].n == n);
    CHECK(lay.sys[s].row_off == adv && lay.sys[s].prime_row_off == prime);
    // the largest row index the kernels form: [splits - 1][ceil4(n) - 1] and [tiles - 1][n_pad - 1]
    const size_t splits = (n + 1023) / 1024, n4 = (n + 3) / 4 * 4, tiles = (n + 255) / 256, n_pad = (n + 511) / 512 * 512;
    CHECK(batch_rows(n) == splits * n4 && batch_prime_rows(n) == tiles * n_pad);
    CHECK(batch_prime_items(n) == tiles * (n_pad / 512) && batch_prime_items(n) <= n);
    adv += splits * n4;
    prime += tiles * n_pad;
    for (size_t i = off[s]; i < off[s + 1]; i++) CHECK((size_t)lay.body_system[i] == s);
    std::vector<int> seen(tiles * (n_pad / 512), 0);
    for (size_t k = 0; k < tiles * (n_pad / 512); k++) {
      const BatchLayoutItem& it = lay.items[items + k];
      CHECK((size_t)it.system == s && it.tblock >= 0 && (size_t)it.tblock < n_pad / 512 && it.tile >= 0 && (size_t)it.tile < tiles);
      seen[(size_t)it.tblock * tiles + it.tile]++;
    }
    for (int c : seen) CHECK(c == 1);
    items += tiles * (n_pad / 512);
  }
  CHECK(lay.adv_rows == adv && lay.prime_rows == prime && lay.items.size() == items);
  CHECK(lay.prime_rows >= lay.adv_rows && lay.items.size() <= off[B]);
}

int main() {
  // the rules
  CHECK(check({0, 3, 260, 300}, 3, 300, nullptr) == 0);
  CHECK(check({0, 8, 8, 16}, 8, 64, "system 1 has 0 bodies") == 2);
  CHECK(check({0, 4097}, 8, 8192, "system 0 has 4097 bodies") == 2);
  CHECK(check({0, 4096}, 8, 8192, nullptr) == 0);
  CHECK(check({0, 12, 8, 16}, 8, 64, "strictly ascending: system 1") == 2);
  CHECK(check({1, 16}, 8, 64, "offsets[0] must be 0") == 2);
  CHECK(check({0, 4, 8, 16}, 2, 64, "number of systems must be in [1, 2], got 3") == 2);
  CHECK(check({0, 4, 17}, 2, 16, "system 1 ends at body 17") == 2);
  CHECK(check({0, 4, 16}, 2, 16, nullptr) == 0);
  {
    char msg[64];
    CHECK(batch_layout_check(nullptr, 1, 1, 1, msg, sizeof(msg)) == 1);
    const size_t zero[1] = {0};
    CHECK(batch_layout_check(zero, 0, 4, 16, msg, sizeof(msg)) == 2);
    char tiny[8];  // a message longer than its buffer is cut, not written past it
    const size_t bad[2] = {0, 5000};
    CHECK(batch_layout_check(bad, 1, 1, 10000, tiny, sizeof(tiny)) == 2 && std::strlen(tiny) == 7);
  }
  // the arithmetic at the edge sizes, alone and mixed, and on drawn layouts
  const size_t edge[] = {1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4095, 4096};
  std::vector<size_t> all{0};
  for (size_t n : edge) {
    verify({0, n});
    all.push_back(all.back() + n);
  }
  verify(all);
  verify({0, 3, 260, 265, 1290, 1354, 1355});
  std::mt19937 rng(7);
  for (int rep = 0; rep < 20; rep++) {
    std::vector<size_t> off{0};
    const int B = 1 + (int)(rng() % 300);
    for (int s = 0; s < B; s++) off.push_back(off.back() + 1 + rng() % (rep % 2 ? 4096 : 40));
    CHECK(check(off, (size_t)B, off.back(), nullptr) == 0);
    verify(off);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
