// hermite_batch_layout.h -- the host arithmetic of an ensemble layout (hermite_batch.hip): the rules of
// nbody_hip_hermite_batch_set_layout and, from the offsets, the per-system words, the system of every body, the work
// items of the priming sweep and the sizes of the row workspaces.  Plain C++ with no device and no HIP header, so that
// hermite_batch_layout_check.cpp can run it on a CPU under a sanitizer.
#pragma once

#include <cstddef>
#include <cstdio>
#include <vector>

namespace nbh {

// the shapes of the sweeps (hermite_batch.hip asserts them against the kernels' constants)
constexpr size_t kLayoutMaxSystem = 4096;     // NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX
constexpr size_t kLayoutSourceBlock = 1024;   // sources per source block of the narrow sweep
constexpr size_t kLayoutTargetGroup = 4;      // targets per group of the narrow sweep
constexpr size_t kLayoutTile = 256;           // sources per tile of the priming sweep
constexpr size_t kLayoutTargetBlock = 512;    // targets per block of the priming sweep

inline size_t layout_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
// rows [source block][ceil4(n_active)] of the advance, worst case n_active = n
inline size_t batch_rows(size_t n) {
  return layout_ceil_div(n, kLayoutSourceBlock) * (layout_ceil_div(n, kLayoutTargetGroup) * kLayoutTargetGroup);
}
// rows [tile][n_pad] of the priming, n_pad = ceil(n / 512) 512
inline size_t batch_prime_rows(size_t n) {
  return layout_ceil_div(n, kLayoutTile) * (layout_ceil_div(n, kLayoutTargetBlock) * kLayoutTargetBlock);
}
// (target block, tile) items of the priming sweep: never more than n
inline size_t batch_prime_items(size_t n) { return layout_ceil_div(n, kLayoutTile) * layout_ceil_div(n, kLayoutTargetBlock); }

// The rules of a layout.  0: fine; 1: a null array (a state error); 2: a rule broken (a validation error).  msg names
// the system.
inline int batch_layout_check(const size_t* offsets, size_t n_systems, size_t max_systems, size_t max_particles, char* msg,
                              size_t msg_len) {
  if (!offsets) {
    std::snprintf(msg, msg_len, "null offsets");
    return 1;
  }
  if (n_systems < 1 || n_systems > max_systems) {
    std::snprintf(msg, msg_len, "the number of systems must be in [1, %zu], got %zu", max_systems, n_systems);
    return 2;
  }
  if (offsets[0] != 0) {
    std::snprintf(msg, msg_len, "offsets[0] must be 0, got %zu (system 0)", offsets[0]);
    return 2;
  }
  for (size_t s = 0; s < n_systems; s++) {
    if (offsets[s + 1] < offsets[s]) {
      std::snprintf(msg, msg_len, "offsets must be strictly ascending: system %zu ends at %zu, before its start %zu", s,
                    offsets[s + 1], offsets[s]);
      return 2;
    }
    const size_t n = offsets[s + 1] - offsets[s];
    if (n < 1 || n > kLayoutMaxSystem) {
      std::snprintf(msg, msg_len, "system %zu has %zu bodies: every size must be in [1, %zu]", s, n, kLayoutMaxSystem);
      return 2;
    }
    if (offsets[s + 1] > max_particles) {
      std::snprintf(msg, msg_len, "system %zu ends at body %zu, beyond the ensemble's capacity %zu", s, offsets[s + 1],
                    max_particles);
      return 2;
    }
  }
  return 0;
}

struct BatchLayoutSystem {
  int first, n;                      // bodies [first, first + n)
  unsigned long long row_off;        // its rows of the advance, in float4
  unsigned long long prime_row_off;  // its rows of the priming
};
struct BatchLayoutItem { int system, tblock, tile, pad; };
struct BatchLayout {
  std::vector<BatchLayoutSystem> sys;
  std::vector<int> body_system;       // the system of body i
  std::vector<BatchLayoutItem> items;  // the priming sweep, system by system, target block by target block
  size_t adv_rows = 0, prime_rows = 0;
};

// from offsets that passed batch_layout_check
inline BatchLayout batch_layout_build(const size_t* offsets, size_t n_systems) {
  BatchLayout out;
  out.sys.resize(n_systems);
  out.body_system.resize(offsets[n_systems]);
  for (size_t s = 0; s < n_systems; s++) {
    const size_t first = offsets[s], n = offsets[s + 1] - first;
    out.sys[s] = BatchLayoutSystem{(int)first, (int)n, (unsigned long long)out.adv_rows, (unsigned long long)out.prime_rows};
    out.adv_rows += batch_rows(n);
    out.prime_rows += batch_prime_rows(n);
    for (size_t i = 0; i < n; i++) out.body_system[first + i] = (int)s;
    const int tblocks = (int)layout_ceil_div(n, kLayoutTargetBlock), tiles = (int)layout_ceil_div(n, kLayoutTile);
    for (int b = 0; b < tblocks; b++)
      for (int t = 0; t < tiles; t++) out.items.push_back(BatchLayoutItem{(int)s, b, t, 0});
  }
  return out;
}

}  // namespace nbh
