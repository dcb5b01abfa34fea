// system_diag_tests.cpp -- the ensemble diagnostics (BlockHermiteEnsemble::diagnostics, BlockHermiteIntegrator::
// diagnostics) on a real GPU.
// The fixed ensemble of hermite_batch_tests.cpp: 300 bodies of initUniform (seed 7) with v = 0.1 (y, -x, 0), cut into
// systems of 3, 257 and 40 bodies; G = 1.7, eps = 0.05, dt_max = 1/64, two macro steps.  It prints one line per system,
//   system_diag <s> <the 16 doubles of the struct as 16 hex digits each> <min_i min_j bind_i bind_j n status>
// which tests/test_system_diag_gpu.py matches against the Python host's structs of the same ensemble, and checks every
// system against a BlockHermiteIntegrator in BlockScheduling::Resident on its bodies alone (the same bytes) and the
// refusals.  Exit code = number of failed checks.
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

static void print(size_t s, const SystemDiag& g) {
  uint64_t w[16];
  std::memcpy(w, &g, sizeof(w));  // the 16 doubles come first
  std::printf("system_diag %zu", s);
  for (uint64_t x : w) std::printf(" %016llx", (unsigned long long)x);
  std::printf(" %d %d %d %d %d %d\n", g.min_i, g.min_j, g.bind_i, g.bind_j, g.n, g.status);
}

int main() {
  ParticleData d, h0;
  ParticleDataManager::allocateDevice(d, kN);
  ParticleDataManager::allocateHost(h0, kN);
  DirectForceCalculator direct;
  direct.setGravitationalConstant(kG);
  direct.setSofteningParameter(kEps);
  fill(h0);
  ParticleDataManager::copyToDevice(d, h0);
  SystemDiag got[kSystems];
  std::memset(got, 0, sizeof(got));
  {
    BlockHermiteEnsemble en;
    en.setLayout(kOffsets, kSystems);
    CHECK(throws([&] { en.diagnostics(&d, got); }));  // not primed
    en.prime(&d, &direct, kDtMax);
    en.advance(&d, 2);
    en.diagnostics(&d, got);
    CHECK(throws([&] { en.diagnostics(nullptr, got); }));
    CHECK(throws([&] { en.diagnostics(&d, nullptr); }));
  }
  for (size_t s = 0; s < kSystems; s++) {
    print(s, got[s]);
    const size_t first = kOffsets[s], n = kOffsets[s + 1] - first;
    CHECK(got[s].status == 0 && got[s].n == (int)n);
    CHECK(got[s].kinetic > 0 && got[s].potential < 0 && got[s].min_sep > 0 && got[s].min_i >= 0 && got[s].min_i < got[s].min_j &&
          got[s].min_j < (int)n);
    // the system alone, through the single-system integrator: the same bytes
    ParticleData one, hone;
    ParticleDataManager::allocateDevice(one, n);
    ParticleDataManager::allocateHost(hone, n);
    float* dst[7] = {hone.pos_x, hone.pos_y, hone.pos_z, hone.vel_x, hone.vel_y, hone.vel_z, hone.mass};
    const float* src[7] = {h0.pos_x, h0.pos_y, h0.pos_z, h0.vel_x, h0.vel_y, h0.vel_z, h0.mass};
    for (int c = 0; c < 7; c++) std::memcpy(dst[c], src[c] + first, n * sizeof(float));
    ParticleDataManager::copyToDevice(one, hone);
    BlockHermiteIntegrator bi;
    bi.setScheduling(BlockScheduling::Resident);
    bi.advance(&one, &direct, kDtMax, 2);
    SystemDiag alone;
    std::memset(&alone, 0, sizeof(alone));
    bi.diagnostics(&one, &direct, &alone);
    CHECK(std::memcmp(&alone, &got[s], sizeof(SystemDiag)) == 0);
    if (s == 1) {  // in the middle of a macro step the bodies are not synchronised
      bi.setScheduling(BlockScheduling::Host);
      bi.blockStep(&one, &direct, kDtMax, 1);
      if (bi.info().current_tick != 0) CHECK(throws([&] { bi.diagnostics(&one, &direct, &alone); }));
      BarnesHutCalculator bh;
      CHECK(throws([&] { bi.diagnostics(&one, &bh, &alone); }));
    }
    ParticleDataManager::freeDevice(one);
    ParticleDataManager::freeHost(hone);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h0);
  return g_fail;
}
