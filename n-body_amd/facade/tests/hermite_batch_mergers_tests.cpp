// hermite_batch_mergers_tests.cpp -- the mergers of nbody::BlockHermiteEnsemble (setMergers / applyMergers / mergers) on a
// real GPU.  The fixed 3-system ensemble of hermite_batch_tests.cpp (300 bodies of initUniform, seed 7, v = 0.1 (y, -x, 0),
// systems of 3, 257 and 40 bodies; G = 1.7, eps = 0.05, dt_max = 1/64) with two pairs brought to 0.01 of each other at rest,
// radius 0.02 each and nobody else any: bodies 0 and 2 of system 0 (hi is the last slot: nothing moves) and bodies 3 and
// 255 of system 1 (the body of slot 256 moves into 255); system 2 never touches.  Two rounds of advance(1), applyMergers.
// It prints, per system, "mstate <s> <n_live> <n_mergers> <flags> stopped <word> done <macro steps>", per log entry
// "merger <s> <slot_a> <slot_b> <id_a> <id_b> <moved_from> <contact_tick> <contact_macro> <contact_d2> <radius> <mass>
// <delta_ke> <delta_pe>" with the floats as hexadecimal floats, and "ids <s> <dead> <id of slots 0 1 2 3 255 256 in range>":
// tests/test_hermite_batch_mergers_gpu.py runs the ensemble through the Python host and wants the same lines.
// Exit code = number of failed checks.
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

static const size_t kOffsets[4] = {0, 3, 260, 300};
static const size_t kSystems = 3, kN = 300;
static const float kG = 1.7f, kEps = 0.05f, kDtMax = 1.0f / 64.0f;

static void fill(ParticleData& h, std::vector<float>& radii) {
  UniformDistParams up;
  up.min_bounds = Vec3(-1, -1, -1);
  up.max_bounds = Vec3(1, 1, 1);
  up.min_mass = 0.5f;
  up.max_mass = 1.5f;
  ParticleInitializer::initUniform(h, up, 7);
  for (size_t i = 0; i < kN; i++) {
    h.vel_x[i] = 0.1f * h.pos_y[i];
    h.vel_y[i] = -0.1f * h.pos_x[i];
  }
  radii.assign(kN, 0.0f);
  const size_t pairs[2][2] = {{0, 2}, {3 + 3, 3 + 255}};
  for (int k = 0; k < 2; k++)
    for (int e = 0; e < 2; e++) {
      const size_t i = pairs[k][e];
      h.pos_x[i] = 2.0f + (e ? 0.005f : -0.005f);
      h.pos_y[i] = h.pos_z[i] = 0.0f;
      h.vel_x[i] = h.vel_y[i] = h.vel_z[i] = 0.0f;
      radii[i] = 0.02f;
    }
}

int main() {
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  std::vector<float> radii;
  fill(h, radii);
  ParticleDataManager::copyToDevice(d, h);
  {
    BlockHermiteEnsemble en;
    CHECK(throws([&] { en.setMergers(); }));  // no layout yet
    en.setLayout(kOffsets, kSystems);
    en.setMergers();
    std::vector<BatchMergerState> st(kSystems);
    std::vector<BatchMerger> log(kN);
    std::vector<unsigned int> ids(kN);
    std::vector<BatchEvent> ev(kSystems);
    CHECK(throws([&] { en.mergers(st.data()); }));  // not primed
    en.prime(&d, &direct, kDtMax);
    CHECK(throws([&] { en.applyMergers(&d); }));    // no events with stop_on_contact
    en.setEvents(radii.data(), nullptr, false, true);
    en.prime(&d, &direct, kDtMax);
    en.mergers(st.data(), log.data(), ids.data());
    for (size_t s = 0; s < kSystems; s++) {
      CHECK(st[s].n_live == kOffsets[s + 1] - kOffsets[s] && st[s].n_mergers == 0u && st[s].flags == 0u);
      for (size_t i = kOffsets[s]; i < kOffsets[s + 1]; i++) CHECK(ids[i] == i - kOffsets[s] && log[i].mass == 0.0);
    }
    for (int round = 0; round < 2; round++) {
      en.advance(&d, 1);
      en.applyMergers(&d);
    }
    CHECK(en.running() == kSystems);
    en.mergers(st.data(), log.data(), ids.data());
    en.events(ev.data());
    for (size_t s = 0; s < kSystems; s++) {
      const size_t first = kOffsets[s], n = kOffsets[s + 1] - first;
      std::printf("mstate %zu %u %u %u stopped %u done %llu\n", s, st[s].n_live, st[s].n_mergers, st[s].flags, ev[s].stopped,
                  ev[s].macro_steps_done);
      for (unsigned int k = 0; k < st[s].n_mergers; k++) {
        const BatchMerger& m = log[first + k];
        std::printf("merger %zu %u %u %u %u %u %u %llu %a %a %a %a %a\n", s, m.slot_a, m.slot_b, m.id_a, m.id_b, m.moved_from,
                    m.contact_tick, m.contact_macro, (double)m.contact_d2, (double)m.radius, m.mass, m.delta_ke, m.delta_pe);
      }
      unsigned int dead = 0;
      for (size_t i = 0; i < n; i++) dead += ids[first + i] == 0xffffffffu;
      std::printf("ids %zu %u", s, dead);
      const size_t look[6] = {0, 1, 2, 3, 255, 256};
      for (size_t k : look)
        if (k < n) std::printf(" %u", ids[first + k]);
      std::printf("\n");
      CHECK(st[s].n_live + st[s].n_mergers == n && dead == st[s].n_mergers && st[s].flags == 0u && ev[s].stopped == 0u &&
            ev[s].macro_steps_done == 2ull);
    }
    CHECK(st[0].n_mergers == 1u && log[0].slot_a == 0u && log[0].slot_b == 2u && log[0].moved_from == 0xffffffffu);
    CHECK(st[1].n_mergers == 1u && log[3].slot_a == 3u && log[3].slot_b == 255u && log[3].moved_from == 256u &&
          ids[3 + 255] == 256u && ids[3 + 256] == 0xffffffffu);
    CHECK(st[2].n_mergers == 0u);
    // a priming restores the counts, the ids and an empty log; a new layout drops the configuration
    en.prime(&d, &direct, kDtMax);
    en.mergers(st.data(), log.data(), ids.data());
    for (size_t s = 0; s < kSystems; s++) CHECK(st[s].n_live == kOffsets[s + 1] - kOffsets[s] && st[s].n_mergers == 0u);
    CHECK(ids[3 + 256] == 256u && log[3].mass == 0.0);
    en.setLayout(kOffsets, kSystems);
    en.setEvents(radii.data(), nullptr, false, true);
    en.prime(&d, &direct, kDtMax);
    CHECK(throws([&] { en.applyMergers(&d); }));    // mergers are not configured
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
