// hermite_batch_hierarchy_tests.cpp -- the hierarchies of nbody::BlockHermiteEnsemble (setHierarchy / hierarchy /
// hierarchySnapshot) on a real GPU.  Four hand-made systems (G = 1, eps = 0, dt_max = 1/64): a circular binary of two
// masses 2 at distance 1 with a single of mass 1 at x = 100 receding at 5 ("[0 1] 2", resolved from the first macro
// step), the same binary with the single bound at x = 20 ("[[0 1] 2]", one piece), a lone body, and two unbound bodies
// receding.  Separation radii 10, 10, 0, 1; kappa 5; stop when resolved.  The snapshot of the primed state has exact
// answers (every operation of the binary is exact); then four macro steps in one launch.  It prints, per system,
// "hierarchy <s> <resolved> <K> <macro> <nodes> <largest> <min_sep> <p> <q> stopped <word> done <macro steps>" and per
// composite "node <s> <id> <left> <right> <bodies> <mass> <a> <e> <r> <energy>" with the doubles as hexadecimal floats:
// tests/test_hermite_batch_hierarchy_gpu.py runs the ensemble through the Python host and wants the same lines.  Exit
// code = number of failed checks.
#include <cmath>
#include <cstdio>
#include <vector>

#include "nbody_facade.hpp"

using namespace nbody;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    g_checks++;                                                                            \
    if (!(cond)) { g_fail++; std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::exception& e) {
    std::printf("  refused: %s\n", e.what());
    return true;
  }
  return false;
}

static const size_t kOffsets[5] = {0, 3, 6, 7, 9};
static const size_t kSystems = 4, kN = 9;
static const float kSep[4] = {10.0f, 10.0f, 0.0f, 1.0f};
// {x, y, vx, vy, m}
static const float kBodies[9][5] = {{-0.5f, 0, 0, -1, 2}, {0.5f, 0, 0, 1, 2}, {100, 0, 5, 0, 1},
                                    {-0.5f, 0, 0, -1, 2}, {0.5f, 0, 0, 1, 2}, {20, 0, 0, 0.3f, 1},
                                    {0, 0, 0, 0, 1},
                                    {-1, 0, -3, 0, 1},    {1, 0, 3, 0, 1}};

int main() {
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(1.0f);
  direct.setSofteningParameter(0.0f);
  for (size_t i = 0; i < kN; i++) {
    h.pos_x[i] = kBodies[i][0]; h.pos_y[i] = kBodies[i][1]; h.pos_z[i] = 0.0f;
    h.vel_x[i] = kBodies[i][2]; h.vel_y[i] = kBodies[i][3]; h.vel_z[i] = 0.0f;
    h.mass[i] = kBodies[i][4];
  }
  ParticleDataManager::copyToDevice(d, h);
  {
    BlockHermiteEnsemble en;
    CHECK(throws([&] { en.setHierarchy(kSep); }));  // no layout yet
    en.setLayout(kOffsets, kSystems);
    const float negative[4] = {1.0f, -1.0f, 0.0f, 0.0f}, none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    CHECK(throws([&] { en.setHierarchy(negative); }));
    CHECK(throws([&] { en.setHierarchy(none, 0.0f, true); }));  // stop when resolved with no radius > 0
    CHECK(throws([&] { en.setHierarchy(nullptr, 0.0f, true); }));
    CHECK(throws([&] { en.setHierarchy(kSep, -1.0f); }));
    en.setHierarchy(kSep, 5.0f, true);
    std::vector<BatchHierarchy> rec(kSystems);
    std::vector<BatchNode> nodes(2 * kN);
    std::vector<BatchEvent> ev(kSystems);
    CHECK(throws([&] { en.hierarchy(rec.data()); }));  // not primed
    en.prime(&d, &direct, 1.0f / 64.0f);
    en.hierarchy(rec.data(), nodes.data());
    for (size_t s = 0; s < kSystems; s++)
      CHECK(rec[s].resolved == 0u && rec[s].macro == 0ull && std::isinf(rec[s].min_sep) && rec[s].min_p == 0xffffffffu);
    for (size_t k = 0; k < 2 * kN; k++) CHECK(nodes[k].left == 0u && nodes[k].bodies == 0u && nodes[k].mass == 0.0);
    // the snapshot of the primed state: exact answers
    en.hierarchySnapshot(&d, rec.data(), nodes.data());
    CHECK(rec[0].resolved == 1u && rec[0].top_count == 2u && rec[0].node_count == 4u && rec[0].largest == 2u &&
          rec[0].min_sep == 100.0 && rec[0].min_p == 2u && rec[0].min_q == 3u && rec[0].macro == 0ull);
    CHECK(nodes[3].left == 0u && nodes[3].right == 1u && nodes[3].parent == 0xffffffffu && nodes[3].bodies == 2u &&
          nodes[3].mass == 4.0 && nodes[3].a == 1.0 && nodes[3].e == 0.0 && nodes[3].r == 1.0 && nodes[3].energy == -2.0);
    CHECK(nodes[0].parent == 3u && nodes[1].parent == 3u && nodes[2].parent == 0xffffffffu && nodes[2].left == 0xffffffffu);
    CHECK(nodes[4].left == 0u && nodes[4].bodies == 0u && nodes[5].left == 0u);  // (the slots above node_count)
    CHECK(rec[1].resolved == 0u && rec[1].top_count == 1u && rec[1].node_count == 5u && rec[1].largest == 3u &&
          std::isinf(rec[1].min_sep));
    CHECK(nodes[6 + 4].left == 2u && nodes[6 + 4].right == 3u && nodes[6 + 3].parent == 4u);
    CHECK(rec[2].top_count == 0u && rec[2].node_count == 0u && std::isinf(rec[2].min_sep));  // n = 1: none
    CHECK(rec[3].resolved == 1u && rec[3].top_count == 2u && rec[3].node_count == 2u && rec[3].min_sep == 2.0);
    en.hierarchy(rec.data());
    for (size_t s = 0; s < kSystems; s++) CHECK(rec[s].macro == 0ull && rec[s].top_count == 0u);  // (the run's own: untouched)
    CHECK(en.running() == kSystems);
    en.advance(&d, 4);
    en.hierarchy(rec.data(), nodes.data());
    en.events(ev.data());
    for (size_t s = 0; s < kSystems; s++) {
      const BatchHierarchy& r = rec[s];
      std::printf("hierarchy %zu %u %u %llu %u %u %a %u %u stopped %u done %llu\n", s, r.resolved, r.top_count, r.macro,
                  r.node_count, r.largest, r.min_sep, r.min_p, r.min_q, ev[s].stopped, ev[s].macro_steps_done);
      const size_t n = kOffsets[s + 1] - kOffsets[s];
      for (size_t k = n; k < r.node_count; k++) {
        const BatchNode& c = nodes[2 * kOffsets[s] + k];
        std::printf("node %zu %zu %u %u %u %a %a %a %a %a\n", s, k, c.left, c.right, c.bodies, c.mass, c.a, c.e, c.r, c.energy);
      }
      CHECK(r.reserved[0] == 0.0 && r.reserved[1] == 0.0 && r.reserved[2] == 0.0);
    }
    CHECK(rec[0].resolved == 1u && rec[0].macro == 1ull && ev[0].stopped == 4u && ev[0].macro_steps_done == 1ull);
    CHECK(rec[1].resolved == 0u && rec[1].macro == 4ull && rec[1].top_count == 1u && ev[1].stopped == 0u);
    CHECK(rec[2].macro == 0ull && ev[2].stopped == 0u && ev[2].macro_steps_done == 4ull);
    CHECK(rec[3].resolved == 1u && rec[3].macro == 1ull && ev[3].stopped == 4u);
    CHECK(en.running() == 2);
    // a priming clears; hierarchies off: the records stay "none" whatever happens
    en.setHierarchy(nullptr);
    ParticleDataManager::copyToDevice(d, h);
    en.prime(&d, &direct, 1.0f / 64.0f);
    en.advance(&d, 1);
    en.hierarchy(rec.data(), nodes.data());
    for (size_t s = 0; s < kSystems; s++) CHECK(rec[s].resolved == 0u && rec[s].macro == 0ull && rec[s].top_count == 0u);
    for (size_t k = 0; k < 2 * kN; k++) CHECK(nodes[k].left == 0u && nodes[k].bodies == 0u);
    CHECK(en.running() == kSystems);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
