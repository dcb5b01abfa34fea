// hermite_batch_tests.cpp -- nbody::BlockHermiteEnsemble on a real GPU.
//   hermite_batch_tests        self-test: two macro steps of a fixed 3-system ensemble; every system against a
//                              BlockHermiteIntegrator in BlockScheduling::Resident on its bodies alone (pos / vel bit for
//                              bit, the counters), the sums of info(-1), a per-system dt_max, the refusals
//   hermite_batch_tests hash   prints "hermite_batch fnv <hash of pos and vel>" after the two macro steps for
//                              tests/test_hermite_batch_gpu.py, which runs the ensemble through the Python host and wants
//                              the same bits
// The ensemble: 300 bodies of initUniform (seed 7) with v = 0.1 (y, -x, 0), cut into systems of 3, 257 and 40 bodies;
// G = 1.7, eps = 0.05, dt_max = 1/64.  Exit code = number of failed checks.
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
static const float kG = 1.7f, kEps = 0.05f, kDtMax = 1.0f / 64.0f;

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

// system s of `all` alone, two resident macro steps of dt_max: its pos / vel into `out` (host, n bodies)
static BlockHermiteInfo alone(const ParticleData& all, size_t s, float dt_max, DirectForceCalculator& direct,
                              ParticleData& out) {
  const size_t first = kOffsets[s], n = kOffsets[s + 1] - first;
  ParticleData d;
  ParticleDataManager::allocateDevice(d, n);
  float* dst[7] = {out.pos_x, out.pos_y, out.pos_z, out.vel_x, out.vel_y, out.vel_z, out.mass};
  const float* src[7] = {all.pos_x, all.pos_y, all.pos_z, all.vel_x, all.vel_y, all.vel_z, all.mass};
  for (int c = 0; c < 7; c++) std::memcpy(dst[c], src[c] + first, n * sizeof(float));
  ParticleDataManager::copyToDevice(d, out);
  BlockHermiteIntegrator bi;
  bi.setScheduling(BlockScheduling::Resident);
  bi.advance(&d, &direct, dt_max, 2);
  ParticleDataManager::copyToHost(out, d);
  const BlockHermiteInfo in = bi.info();
  ParticleDataManager::freeDevice(d);
  return in;
}

static bool same_bits(const ParticleData& got, size_t first, const ParticleData& ref, size_t n) {
  const float* a[6] = {got.pos_x, got.pos_y, got.pos_z, got.vel_x, got.vel_y, got.vel_z};
  const float* b[6] = {ref.pos_x, ref.pos_y, ref.pos_z, ref.vel_x, ref.vel_y, ref.vel_z};
  for (int c = 0; c < 6; c++)
    if (std::memcmp(a[c] + first, b[c], n * sizeof(float)) != 0) return false;
  return true;
}

int main(int argc, char** argv) {
  const bool hash_only = argc > 1 && std::strcmp(argv[1], "hash") == 0;
  ParticleData d, h, h0;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h, kN);
  ParticleDataManager::allocateHost(h0, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  fill(h0);
  ParticleDataManager::copyToDevice(d, h0);
  {
    BlockHermiteEnsemble en;
    en.setLayout(kOffsets, kSystems);
    en.prime(&d, &direct, kDtMax);
    en.advance(&d, 2);
    ParticleDataManager::copyToHost(h, d);
    std::printf("hermite_batch fnv %016llx\n", (unsigned long long)hash_state(h));
    if (!hash_only) {
      const BlockHermiteInfo sum = en.info();
      unsigned long long block_steps = 0, body_steps = 0, macro_steps = 0;
      for (size_t s = 0; s < kSystems; s++) {
        const size_t n = kOffsets[s + 1] - kOffsets[s];
        ParticleData ref;
        ParticleDataManager::allocateHost(ref, n);
        const BlockHermiteInfo one = alone(h0, s, kDtMax, direct, ref);
        const BlockHermiteInfo got = en.info((long long)s);
        std::printf("  system %zu (%zu bodies): %llu block steps, %llu body steps\n", s, n, got.block_steps, got.body_steps);
        CHECK(same_bits(h, kOffsets[s], ref, n));
        CHECK(got.block_steps == one.block_steps && got.body_steps == one.body_steps && got.macro_steps == 2);
        CHECK(got.floor_hits == one.floor_hits && got.last_n_active == one.last_n_active && got.current_tick == 0);
        CHECK(std::memcmp(got.level_steps, one.level_steps, sizeof(got.level_steps)) == 0);
        CHECK(got.narrow_launches == 0 && got.wide_launches == 0 && got.narrow_below == 0);
        block_steps += got.block_steps;
        body_steps += got.body_steps;
        macro_steps += got.macro_steps;
        ParticleDataManager::freeHost(ref);
      }
      CHECK(sum.block_steps == block_steps && sum.body_steps == body_steps && sum.macro_steps == macro_steps);
      CHECK(sum.current_tick == 0 && sum.last_n_active == 0);
      std::vector<int> lv(kN);
      std::vector<unsigned int> tk(kN);
      en.getState(lv.data(), tk.data(), nullptr, nullptr);
      bool ok = true;
      for (size_t i = 0; i < kN; i++) ok = ok && lv[i] >= 0 && lv[i] <= sum.max_level && tk[i] == 0u;
      CHECK(ok);
    }
  }
  if (!hash_only) {
    {  // a dt_max of its own for system 1: that system equals its run alone at that dt_max, the others stay as they were
      const float dts[3] = {kDtMax, kDtMax / 2, kDtMax};
      ParticleDataManager::copyToDevice(d, h0);
      BlockHermiteEnsemble en;
      en.setLayout(kOffsets, kSystems);
      en.prime(&d, &direct, dts);
      en.advance(&d, 1);
      en.advance(&d, 1);
      ParticleData got;
      ParticleDataManager::allocateHost(got, kN);
      ParticleDataManager::copyToHost(got, d);
      const size_t n = kOffsets[2] - kOffsets[1];
      ParticleData ref;
      ParticleDataManager::allocateHost(ref, n);
      alone(h0, 1, dts[1], direct, ref);
      CHECK(same_bits(got, kOffsets[1], ref, n));
      CHECK(same_bits(got, 0, h, kOffsets[1]));  // (system 0 as in the first run)
      ParticleDataManager::freeHost(ref);
      ParticleDataManager::freeHost(got);
    }
    {  // refusals
      BlockHermiteEnsemble en;
      const size_t empty[3] = {0, 5, 5}, big[2] = {0, 4097}, down[3] = {0, 5, 3}, shifted[2] = {1, 5};
      CHECK(throws([&] { en.setLayout(empty, 2); }));
      CHECK(throws([&] { en.setLayout(big, 1); }));
      CHECK(throws([&] { en.setLayout(down, 2); }));
      CHECK(throws([&] { en.setLayout(shifted, 1); }));
      CHECK(throws([&] { en.advance(&d, 1); }));  // no handle yet
      en.setLayout(kOffsets, kSystems);
      CHECK(throws([&] { en.advance(&d, 1); }));  // not primed
      BarnesHutCalculator bh;
      CHECK(throws([&] { en.prime(&d, &bh, kDtMax); }));
      CHECK(throws([&] { en.prime(&d, &direct, 0.0f); }));
      CHECK(throws([&] { en.prime(&d, &direct, INFINITY); }));
      en.prime(&d, &direct, kDtMax);
      const size_t other[3] = {0, 100, 300};
      en.setLayout(other, 2);  // a new layout unprimes
      CHECK(throws([&] { en.advance(&d, 1); }));
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
  }
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  ParticleDataManager::freeHost(h0);
  return g_fail;
}
