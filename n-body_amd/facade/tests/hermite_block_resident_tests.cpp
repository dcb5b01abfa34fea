// hermite_block_resident_tests.cpp -- nbody::BlockHermiteIntegrator with BlockScheduling::Resident on a real GPU.
//   hermite_block_resident_tests        self-test: two resident macro steps of 1,000 bodies against two host-scheduled ones
//                                       (the counters; the bits agree when both take the narrow form throughout, which
//                                       the Python test checks -- here the host form chooses for itself), the schedule,
//                                       a switch at a macro boundary, the refusals
//   hermite_block_resident_tests hash   prints "hermite_block_resident fnv <hash of pos and vel>" after two resident macro
//                                       steps for tests/test_hermite_block_resident_gpu.py, which runs the case through
//                                       the Python host and wants the same bits
// The case of hermite_block_tests.cpp: 1,000 bodies of initUniform with v = 0.1 (y, -x, 0), G = 1.7, eps = 0.05,
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
  BlockHermiteInfo res;
  {
    BlockHermiteIntegrator bi;
    bi.setScheduling(BlockScheduling::Resident);
    bi.integrate(&d, &direct, kDtMax);
    bi.advance(&d, &direct, kDtMax, 1);
    ParticleDataManager::copyToHost(h, d);
    fnv = hash_state(h);
    std::printf("hermite_block_resident fnv %016llx\n", (unsigned long long)fnv);
    if (!hash_only) {
      res = bi.info();
      std::printf("  %llu block steps, %llu body steps, %llu narrow and %llu wide launches, %llu floor hits\n",
                  res.block_steps, res.body_steps, res.narrow_launches, res.wide_launches, res.floor_hits);
      unsigned long long by_level = 0;
      for (int k = 0; k < 21; k++) by_level += res.level_steps[k];
      CHECK(bi.getScheduling() == BlockScheduling::Resident);
      CHECK(res.macro_steps == 2 && res.current_tick == 0);
      CHECK(by_level == res.body_steps && res.body_steps >= 2 * kN);
      CHECK(res.narrow_launches == 0 && res.wide_launches == 0);  // (they count host-form launches)
      std::vector<int> lv(kN);
      std::vector<unsigned int> tk(kN);
      bi.getState(lv.data(), tk.data(), nullptr, nullptr);
      bool ok = true;
      for (size_t i = 0; i < kN; i++) ok = ok && lv[i] >= 0 && lv[i] <= res.max_level && tk[i] == 0u;
      CHECK(ok);
    }
  }
  if (!hash_only) {
    {  // two fresh resident runs agree bit for bit
      fill(d, h);
      BlockHermiteIntegrator bi;
      bi.setScheduling(BlockScheduling::Resident);
      bi.advance(&d, &direct, kDtMax, 2);
      ParticleDataManager::copyToHost(h, d);
      CHECK(hash_state(h) == fnv);
    }
    {  // a switch at a macro boundary keeps the priming and the counters; in the middle of a macro step it is refused
      fill(d, h);
      BlockHermiteIntegrator bi;
      bi.integrate(&d, &direct, kDtMax);
      bi.setScheduling(BlockScheduling::Resident);
      bi.integrate(&d, &direct, kDtMax);
      const BlockHermiteInfo in = bi.info();
      CHECK(in.macro_steps == 2 && in.current_tick == 0);
      CHECK(in.narrow_launches + in.wide_launches < in.block_steps);
      bi.blockStep(&d, &direct, kDtMax, 1);
      if (bi.info().current_tick != 0) {
        CHECK(throws([&] { bi.setScheduling(BlockScheduling::Host); }));
        CHECK(bi.getScheduling() == BlockScheduling::Resident);
      }
      bi.integrate(&d, &direct, kDtMax);
      CHECK(bi.info().current_tick == 0 && bi.info().macro_steps == 3);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
  }
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
