// hermite_batch_outcomes_tests.cpp -- the outcomes of nbody::BlockHermiteEnsemble (setOutcomes / outcomes) on a real GPU.
// The fixed 3-system ensemble of hermite_batch_tests.cpp (300 bodies of initUniform, seed 7, v = 0.1 (y, -x, 0), systems
// of 3, 257 and 40 bodies; G = 1.7, eps = 0.05, dt_max = 1/64) with one body of system 0 and the LAST body of system 1
// (system-local index 256: a thread's second body is never reached, its fifth wave is) put at (2, 0, 0) and sent outward
// at 8 and 64; escape radii 2.5, 2.5 and 0 (no test for system 2), stop on escape.  Twelve macro steps in one launch.
// It prints, per system, "outcome <s> <escaped> <escaper> <macro> <r> <vr> <energy> <rest_mass> stopped <word> done <macro
// steps>" with the doubles as hexadecimal floats: tests/test_hermite_batch_outcomes_gpu.py runs the ensemble through the
// Python host and wants the same lines.  Exit code = number of failed checks.
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
static const float kEscape[3] = {2.5f, 2.5f, 0.0f};

static void fill(ParticleData& h) {
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
  const size_t kicked[2] = {0, 259};
  const float speed[2] = {8.0f, 64.0f};
  for (int k = 0; k < 2; k++) {
    const size_t i = kicked[k];
    h.pos_x[i] = 2.0f;
    h.pos_y[i] = h.pos_z[i] = 0.0f;
    h.vel_x[i] = speed[k];
    h.vel_y[i] = h.vel_z[i] = 0.0f;
  }
}

int main() {
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  fill(h);
  ParticleDataManager::copyToDevice(d, h);
  {
    BlockHermiteEnsemble en;
    CHECK(throws([&] { en.setOutcomes(kEscape); }));  // no layout yet
    en.setLayout(kOffsets, kSystems);
    const float negative[3] = {1.0f, -1.0f, 0.0f}, none[3] = {0.0f, 0.0f, 0.0f};
    CHECK(throws([&] { en.setOutcomes(negative); }));
    CHECK(throws([&] { en.setOutcomes(none, true); }));     // stop on escape with no radius > 0
    CHECK(throws([&] { en.setOutcomes(nullptr, true); }));
    en.setOutcomes(kEscape, true);
    std::vector<BatchOutcome> out(kSystems);
    std::vector<BatchEvent> ev(kSystems);
    CHECK(throws([&] { en.outcomes(out.data()); }));  // not primed
    en.prime(&d, &direct, kDtMax);
    en.outcomes(out.data());
    for (size_t s = 0; s < kSystems; s++) CHECK(out[s].escaped == 0u && out[s].escaper == 0xffffffffu && out[s].macro == 0ull);
    CHECK(en.running() == kSystems);
    en.advance(&d, 12);
    en.outcomes(out.data());
    en.events(ev.data());
    size_t running = 0;
    for (size_t s = 0; s < kSystems; s++) {
      const BatchOutcome& o = out[s];
      std::printf("outcome %zu %u %u %llu %a %a %a %a stopped %u done %llu\n", s, o.escaped, o.escaper, o.macro, o.r, o.vr,
                  o.energy, o.rest_mass, ev[s].stopped, ev[s].macro_steps_done);
      CHECK(o.reserved == 0.0 && o.reserved2 == 0.0);
      if (o.escaped != 0u) {
        CHECK(ev[s].stopped == 3u && ev[s].macro_steps_done == o.macro && o.macro >= 1ull && o.macro <= 12ull);
        CHECK(o.escaper < kOffsets[s + 1] - kOffsets[s] && o.r > (double)kEscape[s] && o.vr > 0.0 && o.energy > 0.0 &&
              o.rest_mass > 0.0);
      } else {
        CHECK(ev[s].stopped == 0u && ev[s].macro_steps_done == 12ull && o.escaper == 0xffffffffu && o.r == 0.0);
        running++;
      }
    }
    CHECK(out[0].escaped >= 1u && out[0].escaper == 0u);    // the kicked bodies
    CHECK(out[1].escaped == 1u && out[1].escaper == 256u && out[1].macro == 1ull);
    CHECK(out[2].escaped == 0u);                            // (no test for system 2)
    CHECK(en.running() == running);
    // a priming clears; outcomes off: the records stay "none" whatever happens
    en.setOutcomes(nullptr);
    en.prime(&d, &direct, kDtMax);
    en.advance(&d, 1);
    en.outcomes(out.data());
    for (size_t s = 0; s < kSystems; s++) CHECK(out[s].escaped == 0u && out[s].escaper == 0xffffffffu);
    CHECK(en.running() == kSystems);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
