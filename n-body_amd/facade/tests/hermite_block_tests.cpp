// hermite_block_tests.cpp -- nbody::BlockHermiteIntegrator of the facade on a real GPU.
//   hermite_block_tests          self-test: two macro steps of 1,000 bodies; the schedule (ticks 0 at the macro boundary,
//                                body_steps = the sum of level_steps, levels in range), a level-0 run against
//                                HermiteIntegrator bit for bit, the refusals
//   hermite_block_tests hash     prints "hermite_block fnv <hash of pos and vel>" after two macro steps of the same case
//                                for tests/test_hermite_block_gpu.py, which runs it through the Python host and wants the
//                                same bits
// 1,000 bodies of initUniform (bit-exact in both host languages) with v = 0.1 (y, -x, 0), G = 1.7, eps = 0.05,
// dt_max = 1/64.  Exit code = number of failed checks.
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

struct SubclassedDirect : DirectForceCalculator {};

template <class F>
static bool refused(F&& f) {
  try {
    f();
  } catch (const ValidationException& e) {
    std::printf("  refused: %s\n", e.what());
    return true;
  }
  return false;
}

static const size_t kN = 1000;
static const float kG = 1.7f, kEps = 0.05f, kDtMax = 1.0f / 64.0f;

static void fill(ParticleData& d, ParticleData& h) {
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
}

static uint64_t hash_state(const ParticleData& h) {
  uint64_t fnv = 1469598103934665603ull;
  const float* arrays[6] = {h.pos_x, h.pos_y, h.pos_z, h.vel_x, h.vel_y, h.vel_z};
  for (const float* a : arrays) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(a);
    for (size_t k = 0; k < kN * sizeof(float); k++) { fnv ^= b[k]; fnv *= 1099511628211ull; }
  }
  return fnv;
}

int main(int argc, char** argv) {
  const bool hash_only = argc > 1 && std::strcmp(argv[1], "hash") == 0;
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  fill(d, h);
  uint64_t fnv = 0;
  {
    BlockHermiteIntegrator bi;
    bi.integrate(&d, &direct, kDtMax);
    bi.advance(&d, &direct, kDtMax, 1);
    ParticleDataManager::copyToHost(h, d);
    fnv = hash_state(h);
    std::printf("hermite_block fnv %016llx\n", (unsigned long long)fnv);
    if (!hash_only) {
      const BlockHermiteInfo in = bi.info();
      std::printf("  %llu block steps, %llu body steps, %llu narrow and %llu wide launches, %llu floor hits\n",
                  in.block_steps, in.body_steps, in.narrow_launches, in.wide_launches, in.floor_hits);
      unsigned long long by_level = 0;
      for (int k = 0; k < 21; k++) by_level += in.level_steps[k];
      CHECK(in.macro_steps == 2 && in.current_tick == 0);
      CHECK(by_level == in.body_steps && in.body_steps >= 2 * kN);
      CHECK(in.narrow_launches + in.wide_launches == in.block_steps);
      std::vector<int> lv(kN);
      std::vector<unsigned int> tk(kN);
      bi.getState(lv.data(), tk.data(), nullptr, nullptr);
      bool ok = true;
      for (size_t i = 0; i < kN; i++) ok = ok && lv[i] >= 0 && lv[i] <= in.max_level && tk[i] == 0u;
      CHECK(ok);
    }
  }
  if (!hash_only) {
    {  // two fresh runs agree bit for bit
      fill(d, h);
      BlockHermiteIntegrator bi;
      bi.advance(&d, &direct, kDtMax, 2);
      ParticleDataManager::copyToHost(h, d);
      CHECK(hash_state(h) == fnv);
    }
    {  // max_level = 0 is the shared-step integrator
      fill(d, h);
      BlockHermiteIntegrator bi;
      bi.setParameters(0.02f, 0.01f, 0);
      bi.advance(&d, &direct, kDtMax, 3);
      ParticleDataManager::copyToHost(h, d);
      const uint64_t a = hash_state(h);
      fill(d, h);
      HermiteIntegrator hi;
      hi.integrateSteps(&d, &direct, kDtMax, 3);
      ParticleDataManager::copyToHost(h, d);
      CHECK(hash_state(h) == a);
    }
    BlockHermiteIntegrator bi;
    SubclassedDirect sub;
    BarnesHutCalculator bh(0.5f);
    CHECK(refused([&] { bi.integrate(&d, &sub, kDtMax); }));
    CHECK(refused([&] { bi.integrate(&d, &bh, kDtMax); }));
    CHECK(refused([&] { bi.prime(&d, &sub, kDtMax); }));
    CHECK(refused([&] { bi.integrate(&d, &direct, 0.0f); }));
    CHECK(refused([&] { bi.integrate(&d, &direct, NAN); }));
    CHECK(refused([&] { bi.advance(&d, &direct, kDtMax, 0); }));
    CHECK(refused([&] { bi.setParameters(0.02f, 0.01f, 21); }));
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
  }
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
