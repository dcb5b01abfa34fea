// hermite_batch_events_tests.cpp -- the events of nbody::BlockHermiteEnsemble (setEvents / events / running) on a real GPU.
// The fixed ensemble of hermite_batch_tests.cpp: 300 bodies of initUniform (seed 7) with v = 0.1 (y, -x, 0), cut into
// systems of 3, 257 and 40 bodies; G = 1.7, eps = 0.05, dt_max = 1/64.  Every body has the radius 0.04, the budgets are
// (0, 0, 2) macro steps, the closest approach is tracked and a contact stops; advance(4).  Prints one line per system,
//   hermite_batch_events <s> stopped <..> done <..> closest <d2 bits> <i> <j> <macro> <tick> contact <d2 bits> <i> <j> <macro> <tick>
// and "hermite_batch_events running <n>", which tests/test_hermite_batch_events_gpu.py compares with the Python host's
// records of the same ensemble.  The self-checks are those that need no second host.  Exit code = number of failed checks.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
static const float kG = 1.7f, kEps = 0.05f, kDtMax = 1.0f / 64.0f, kRadius = 0.04f;
static const unsigned long long kLimits[3] = {0ull, 0ull, 2ull};

static unsigned int bits(float f) {
  unsigned int u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
}

int main() {
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
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
  ParticleDataManager::copyToDevice(d, h);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  const std::vector<float> radii(kN, kRadius);
  {
    BlockHermiteEnsemble en;
    CHECK(throws([&] { en.setEvents(radii.data()); }));  // no layout yet
    en.setLayout(kOffsets, kSystems);
    CHECK(throws([&] { en.setEvents(nullptr, nullptr, false, true); }));  // stop on contact without radii
    std::vector<float> bad(radii);
    bad[17] = -1.0f;
    CHECK(throws([&] { en.setEvents(bad.data()); }));
    en.setEvents(radii.data(), kLimits, true, true);
    std::vector<BatchEvent> ev(kSystems);
    CHECK(throws([&] { en.events(ev.data()); }));  // not primed
    en.prime(&d, &direct, kDtMax);
    CHECK(en.running() == kSystems);
    en.advance(&d, 4);
    en.events(ev.data());
    size_t running = 0;
    for (size_t s = 0; s < kSystems; s++) {
      const BatchEvent& e = ev[s];
      std::printf("hermite_batch_events %zu stopped %u done %llu closest %08x %u %u %llu %u contact %08x %u %u %llu %u\n", s,
                  e.stopped, e.macro_steps_done, bits(e.closest_d2), e.closest_i, e.closest_j, e.closest_macro,
                  e.closest_tick, bits(e.contact_d2), e.contact_i, e.contact_j, e.contact_macro, e.contact_tick);
      const size_t n = kOffsets[s + 1] - kOffsets[s];
      CHECK(e.stopped <= 2u && e.macro_steps_done >= 1 && e.macro_steps_done <= 4);
      CHECK(e.macro_steps_done == en.info((long long)s).macro_steps);
      CHECK(e.closest_i < n && e.closest_j < n && e.closest_i != e.closest_j && std::isfinite(e.closest_d2));
      CHECK(e.closest_macro < e.macro_steps_done && e.closest_tick >= 1u);
      if (e.stopped == 1u) {  // a contact: inside the last macro step that was completed, and no further than the radii
        CHECK(e.contact_i < n && e.contact_j < n && e.contact_d2 < (2 * kRadius) * (2 * kRadius));
        CHECK(e.contact_macro + 1 == e.macro_steps_done && e.closest_d2 <= e.contact_d2);
      } else {
        CHECK(e.contact_i == 0xffffffffu && e.contact_j == 0xffffffffu && std::isinf(e.contact_d2));
        CHECK(e.stopped == (kLimits[s] != 0 ? 2u : 0u));
        CHECK(e.macro_steps_done == (kLimits[s] != 0 ? kLimits[s] : 4ull));
      }
      running += e.stopped == 0u;
    }
    CHECK(en.running() == running);
    std::printf("hermite_batch_events running %zu\n", running);
    // back to the plain kernel: the running systems go on, the records stay as they were but for the counter
    en.setEvents();
    en.advance(&d, 1);
    std::vector<BatchEvent> after(kSystems);
    en.events(after.data());
    for (size_t s = 0; s < kSystems; s++) {
      CHECK(after[s].macro_steps_done == ev[s].macro_steps_done + 1);  // (the plain kernel knows no stop word)
      CHECK(bits(after[s].closest_d2) == bits(ev[s].closest_d2) && after[s].closest_tick == ev[s].closest_tick);
    }
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
