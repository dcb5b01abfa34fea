// hermite_tests.cpp -- nbody::HermiteIntegrator and nbody::computeAccJerk of the facade on a real GPU.
//   two bodies: a and j against the closed form  a_0 = G m_1 d h^-3/2,  j_0 = G m_1 (w - 3 (d.w)/h d) h^-3/2
//     (d = r_1 - r_0, w = v_1 - v_0, h = |d|^2 + eps^2), and the opposite signs with m_0 for body 1
//   1,000 bodies of initUniform (bit-exact in both host languages) with v = 0.1 (y, -x, 0): ten steps of dt = 1e-3;
//     prints "hermite fnv <hash of pos and vel>", "hermite dt <suggestTimeStep(0.02)>" and "hermite ke <KE>" for
//     tests/test_hermite_gpu.py, which runs the same case through the Python host and wants the same bits
//   refusals: a subclass of DirectForceCalculator, the tree calculator, a bad dt, steps = 0
// Device float4 arrays are the pos_x arrays of ParticleData blocks of 4 n floats.  Exit code = number of failed checks.
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

struct Float4Array {
  ParticleData d, h;
  size_t n;
  explicit Float4Array(size_t count) : n(count) {
    ParticleDataManager::allocateDevice(d, 4 * n);
    ParticleDataManager::allocateHost(h, 4 * n);
    std::memset(h.pos_x, 0, 4 * n * sizeof(float));
  }
  ~Float4Array() {
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  float4* dev() { return reinterpret_cast<float4*>(d.pos_x); }
  float* row(size_t i) { return h.pos_x + 4 * i; }
  void download() { ParticleDataManager::copyToHost(h, d); }
};

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

int main() {
  const float G = 1.7f, eps = 0.05f;
  {  // two bodies
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, 2);
    ParticleDataManager::allocateHost(h, 2);
    ParticleInitializer::zeroAccelerations(h);
    const float x[2][3] = {{0.f, 0.f, 0.f}, {1.f, 0.5f, -0.25f}}, v[2][3] = {{0.f, 0.1f, 0.f}, {0.1f, -0.2f, 0.3f}};
    const float m[2] = {2.0f, 0.75f};
    for (int i = 0; i < 2; i++) {
      h.pos_x[i] = x[i][0]; h.pos_y[i] = x[i][1]; h.pos_z[i] = x[i][2];
      h.vel_x[i] = v[i][0]; h.vel_y[i] = v[i][1]; h.vel_z[i] = v[i][2];
      h.mass[i] = m[i];
    }
    ParticleDataManager::copyToDevice(d, h);
    Float4Array acc(2), jerk(2), jerk2(2);
    computeAccJerk(&d, G, eps, acc.dev(), jerk.dev());
    acc.download();
    jerk.download();
    double dd[3], ww[3], h2 = (double)(eps * eps), dw = 0.0;
    for (int a = 0; a < 3; a++) {
      dd[a] = (double)x[1][a] - x[0][a];
      ww[a] = (double)v[1][a] - v[0][a];
      h2 += dd[a] * dd[a];
      dw += dd[a] * ww[a];
    }
    const double h32 = std::pow(h2, -1.5);
    for (int i = 0; i < 2; i++) {
      const double s = i == 0 ? (double)G * m[1] : -(double)G * m[0];
      double na = 0.0, nj = 0.0, ea = 0.0, ej = 0.0;
      for (int a = 0; a < 3; a++) {
        const double aa = s * dd[a] * h32, jj = s * (ww[a] - 3.0 * dw / h2 * dd[a]) * h32;
        na += aa * aa; nj += jj * jj;
        ea += std::pow(acc.row(i)[a] - aa, 2); ej += std::pow(jerk.row(i)[a] - jj, 2);
      }
      CHECK(std::sqrt(ea) <= 1e-5 * std::sqrt(na));
      CHECK(std::sqrt(ej) <= 1e-5 * std::sqrt(nj));
    }
    // acc_* were left alone (zeros); priming writes them and keeps the same jerk
    ParticleDataManager::copyToHost(h, d);
    CHECK(h.acc_x[0] == 0.f && h.acc_y[1] == 0.f);
    DirectForceCalculator direct;
    direct.setGravitationalConstant(G);
    direct.setSofteningParameter(eps);
    HermiteIntegrator hi;
    bool state_error = false;  // not primed: the C ABI's ERR_STATE
    try { hi.suggestTimeStep(); } catch (const CudaException&) { state_error = true; }
    CHECK(state_error);
    hi.prime(&d, &direct);
    hi.getJerk(jerk2.dev());
    jerk2.download();
    CHECK(std::memcmp(jerk.row(0), jerk2.row(0), 8 * sizeof(float)) == 0);
    ParticleDataManager::copyToHost(h, d);
    CHECK(h.acc_x[0] == acc.row(0)[0] && h.acc_y[1] == acc.row(1)[1] && h.acc_z[1] == acc.row(1)[2]);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  {  // ten steps, for the Python host to reproduce bit for bit
    const size_t n = 1000;
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, n);
    ParticleDataManager::allocateHost(h, n);
    UniformDistParams up;
    up.min_bounds = Vec3(-1, -1, -1);
    up.max_bounds = Vec3(1, 1, 1);
    up.min_mass = 0.5f;
    up.max_mass = 1.5f;
    ParticleInitializer::initUniform(h, up, 7);
    for (size_t i = 0; i < n; i++) {
      h.vel_x[i] = 0.1f * h.pos_y[i];
      h.vel_y[i] = -0.1f * h.pos_x[i];
    }
    ParticleDataManager::copyToDevice(d, h);
    DirectForceCalculator direct;
    direct.setGravitationalConstant(G);
    direct.setSofteningParameter(eps);
    HermiteIntegrator hi;
    hi.integrateSteps(&d, &direct, 1e-3f, 4);
    for (int s = 0; s < 6; s++) hi.integrate(&d, &direct, 1e-3f);
    ParticleDataManager::copyToHost(h, d);
    uint64_t fnv = 1469598103934665603ull;
    const float* arrays[6] = {h.pos_x, h.pos_y, h.pos_z, h.vel_x, h.vel_y, h.vel_z};
    for (const float* a : arrays) {
      const unsigned char* b = reinterpret_cast<const unsigned char*>(a);
      for (size_t k = 0; k < n * sizeof(float); k++) { fnv ^= b[k]; fnv *= 1099511628211ull; }
    }
    std::printf("hermite fnv %016llx\n", (unsigned long long)fnv);
    std::printf("hermite dt %.9g\n", (double)hi.suggestTimeStep(0.02f));
    std::printf("hermite ke %.9g\n", (double)hi.computeKineticEnergy(&d));
    CHECK(hi.suggestTimeStep(0.02f) > 0.f && std::isfinite(hi.suggestTimeStep(0.02f)));

    // refusals
    SubclassedDirect sub;
    BarnesHutCalculator bh(0.5f);
    CHECK(refused([&] { hi.integrate(&d, &sub, 1e-3f); }));
    CHECK(refused([&] { hi.integrate(&d, &bh, 1e-3f); }));
    CHECK(refused([&] { hi.prime(&d, &sub); }));
    CHECK(refused([&] { hi.integrate(&d, &direct, 0.0f); }));
    CHECK(refused([&] { hi.integrate(&d, &direct, -1e-3f); }));
    CHECK(refused([&] { hi.integrate(&d, &direct, NAN); }));
    CHECK(refused([&] { hi.integrateSteps(&d, &direct, 1e-3f, 0); }));
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
