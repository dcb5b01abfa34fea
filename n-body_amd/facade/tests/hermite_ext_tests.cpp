// hermite_ext_tests.cpp -- the extended state precision of nbody::HermiteIntegrator and nbody::BlockHermiteIntegrator on a
// real GPU.
//   hermite_ext_tests            self-test: two macro steps of 1,000 bodies in extended mode; the invariant hi = (float)X,
//                                lo = (float)(X - hi); a level-0 run against HermiteIntegrator in extended mode bit for
//                                bit; set / get round trip; invalidate zeroes the residuals; the default mode is fp32
//   hermite_ext_tests hash       prints "hermite_ext fnv <hash of hi and lo of pos and vel>" after the two macro steps
//                                for tests/test_hermite_ext_gpu.py, which runs the case through the Python host and
//                                wants the same bits
// 1,000 bodies of initUniform (bit-exact in both host languages), shrunk to 0.05 and moved to (64, -32, 16) in fp64 -- a
// state that is not fp32-representable -- with v = 0.1 (y, -x, 0), G = 1.7, eps = 0.01, dt_max = 1/64, max_level = 6.
// Exit code = number of failed checks.
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

static const size_t kN = 1000;
static const float kG = 1.7f, kEps = 0.01f, kDtMax = 1.0f / 64.0f;

// the fp64 state; the masses go to the device through the particle data
static void fill(ParticleData& d, ParticleData& h, std::vector<double>& X, std::vector<double>& V) {
  UniformDistParams up;
  up.min_bounds = Vec3(-1, -1, -1);
  up.max_bounds = Vec3(1, 1, 1);
  up.min_mass = 0.5f;
  up.max_mass = 1.5f;
  ParticleInitializer::initUniform(h, up, 7);
  const double c[3] = {64.0, -32.0, 16.0};
  X.resize(3 * kN);
  V.resize(3 * kN);
  for (size_t i = 0; i < kN; i++) {
    const float p[3] = {h.pos_x[i], h.pos_y[i], h.pos_z[i]};
    for (int k = 0; k < 3; k++) X[3 * i + k] = (double)p[k] * 0.05 + c[k];
    V[3 * i + 0] = (double)(0.1f * h.pos_y[i]);
    V[3 * i + 1] = (double)(-0.1f * h.pos_x[i]);
    V[3 * i + 2] = 0.0;
  }
  ParticleDataManager::copyToDevice(d, h);
}

// FNV-1a over the hi parts (pos_x .. vel_z of the particle data, as hermite_block_tests hashes them), then over the
// residuals (float)(X - hi) of pos and of vel as [N][3] arrays
static uint64_t hash_state(const ParticleData& h, const std::vector<double>& X, const std::vector<double>& V) {
  uint64_t fnv = 1469598103934665603ull;
  auto eat = [&fnv](const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < bytes; k++) { fnv ^= b[k]; fnv *= 1099511628211ull; }
  };
  const float* hi[6] = {h.pos_x, h.pos_y, h.pos_z, h.vel_x, h.vel_y, h.vel_z};
  for (const float* a : hi) eat(a, kN * sizeof(float));
  std::vector<float> lo(3 * kN);
  for (int part = 0; part < 2; part++) {
    const std::vector<double>& Z = part ? V : X;
    for (size_t i = 0; i < kN; i++)
      for (int c = 0; c < 3; c++) lo[3 * i + c] = (float)(Z[3 * i + c] - (double)hi[3 * part + c][i]);
    eat(lo.data(), lo.size() * sizeof(float));
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
  std::vector<double> X0, V0, X(3 * kN), V(3 * kN);
  fill(d, h, X0, V0);
  uint64_t fnv = 0;
  {
    BlockHermiteIntegrator bi;
    CHECK(bi.getStatePrecision() == StatePrecision::Fp32);
    bi.setParameters(0.02f, 0.01f, 6);
    bi.setStatePrecision(StatePrecision::Extended);
    bi.setExtendedState(&d, &direct, X0.data(), V0.data());
    bi.advance(&d, &direct, kDtMax, 2);
    bi.getExtendedState(&d, &direct, X.data(), V.data());
    ParticleDataManager::copyToHost(h, d);
    fnv = hash_state(h, X, V);
    std::printf("hermite_ext precision %s\n", bi.getStatePrecision() == StatePrecision::Extended ? "extended" : "fp32");
    std::printf("hermite_ext fnv %016llx\n", (unsigned long long)fnv);
    if (!hash_only) {
      bool hi_ok = true, lo_used = false;
      for (size_t i = 0; i < kN; i++) {
        // (a residual of exactly half an ulp makes hi + lo a tie: compare distances, do not round hi + lo)
        hi_ok = hi_ok && std::fabs(X[3 * i] - (double)h.pos_x[i]) <= 0.5 * (std::nextafter(std::fabs(h.pos_x[i]), INFINITY) - std::fabs(h.pos_x[i])) &&
                std::fabs(V[3 * i + 1] - (double)h.vel_y[i]) <= 0.5 * (std::nextafter(std::fabs(h.vel_y[i]), INFINITY) - std::fabs(h.vel_y[i]));
        lo_used = lo_used || X[3 * i] != (double)h.pos_x[i];
      }
      CHECK(hi_ok);    // the particle data holds the hi parts of the extended state
      CHECK(lo_used);  // and the residuals are in use
      bi.invalidate();  // the caller changed the state: the fp32 arrays are the truth
      bi.getExtendedState(&d, &direct, X.data(), V.data());
      bool widened = true;
      for (size_t i = 0; i < kN; i++) widened = widened && X[3 * i] == (double)h.pos_x[i] && V[3 * i] == (double)h.vel_x[i];
      CHECK(widened);
    }
  }
  if (!hash_only) {
    {  // two fresh runs agree bit for bit, hi and lo
      fill(d, h, X0, V0);
      BlockHermiteIntegrator bi;
      bi.setParameters(0.02f, 0.01f, 6);
      bi.setStatePrecision(StatePrecision::Extended);
      bi.setExtendedState(&d, &direct, X0.data(), V0.data());
      bi.integrate(&d, &direct, kDtMax);
      bi.integrate(&d, &direct, kDtMax);
      bi.getExtendedState(&d, &direct, X.data(), V.data());
      ParticleDataManager::copyToHost(h, d);
      CHECK(hash_state(h, X, V) == fnv);
    }
    {  // max_level = 0 is the shared-step integrator, in extended mode too
      fill(d, h, X0, V0);
      BlockHermiteIntegrator bi;
      bi.setParameters(0.02f, 0.01f, 0);
      bi.setStatePrecision(StatePrecision::Extended);
      bi.setExtendedState(&d, &direct, X0.data(), V0.data());
      bi.advance(&d, &direct, kDtMax, 3);
      bi.getExtendedState(&d, &direct, X.data(), V.data());
      ParticleDataManager::copyToHost(h, d);
      const uint64_t a = hash_state(h, X, V);
      fill(d, h, X0, V0);
      HermiteIntegrator hi;
      hi.setStatePrecision(StatePrecision::Extended);
      hi.setExtendedState(&d, &direct, X0.data(), V0.data());
      hi.integrateSteps(&d, &direct, kDtMax, 3);
      hi.getExtendedState(&d, &direct, X.data(), V.data());
      ParticleDataManager::copyToHost(h, d);
      CHECK(hash_state(h, X, V) == a);
      // set / get round trip: exact to the hi + lo representation
      hi.setExtendedState(&d, &direct, X0.data(), V0.data());
      hi.getExtendedState(&d, &direct, X.data(), V.data());
      bool close = true;
      for (size_t k = 0; k < 3 * kN; k++) close = close && std::fabs(X[k] - X0[k]) <= std::ldexp(std::fabs(X0[k]), -49);
      CHECK(close);
      hi.setStatePrecision(StatePrecision::Fp32);  // the fp32 mode returns the arrays widened
      hi.getExtendedState(&d, &direct, X.data(), V.data());
      bool widened = true;
      for (size_t k = 0; k < 3 * kN; k++) widened = widened && X[k] == (double)(float)X0[k];
      CHECK(widened);
    }
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
  }
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  return g_fail;
}
