// potential_tests.cpp -- nbody::computePotential and the tree / grid computePotential methods of the facade on a
// real GPU.  4,096 bodies of ParticleInitializer::initSpherical (radius 10, seed 42), G = 1, eps = 0.1.  Prints one
// "pe <method> <value>" line per calculator (tests/test_potential_gpu.py compares them with the Python API on the same
// bodies) and checks: Direct and Barnes-Hut at theta = 0 against Integrator::computePotentialEnergy; 1/2 sum m phi
// against the returned PE; accelerations untouched by the potential calls.  Exit code = number of failed checks.
#include <cmath>
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

static double rel(double a, double b) { return std::fabs(a - b) / std::fabs(b); }

int main() {
  const size_t n = 4096;
  const float G = 1.0f, eps = 0.1f;
  ParticleData d, h, phi_d, phi_h;  // phi_d.pos_x: a device array of n floats for phi
  ParticleDataManager::allocateDevice(d, n);
  ParticleDataManager::allocateHost(h, n);
  ParticleDataManager::allocateDevice(phi_d, n);
  ParticleDataManager::allocateHost(phi_h, n);
  SphericalDistParams p;
  p.center = Vec3(0, 0, 0);
  p.radius = 10.0f;
  ParticleInitializer::initSpherical(h, p, 42);
  ParticleDataManager::copyToDevice(d, h);

  DirectForceCalculator direct(256);
  BarnesHutCalculator bh0(0.0f), bh(0.5f);
  SpatialHashCalculator hash(1.0f, 2.0f);
  ForceCalculator* calcs[] = {&direct, &bh0, &bh, &hash};
  const char* names[] = {"direct", "bh_theta0", "bh_theta0.5", "hash_cell1_cutoff2"};
  Integrator integ;
  const double ref = integ.computePotentialEnergy(&d, G, eps);
  std::printf("pe integrator %.17g\n", ref);

  for (int c = 0; c < 4; c++) {
    ForceCalculator* fc = calcs[c];
    fc->setGravitationalConstant(G);
    fc->setSofteningParameter(eps);
    fc->computeForces(&d);
    ParticleDataManager::copyToHost(h, d);
    const std::vector<float> ax(h.acc_x, h.acc_x + n), ay(h.acc_y, h.acc_y + n), az(h.acc_z, h.acc_z + n);
    const double pe = computePotential(*fc, &d, phi_d.pos_x);
    const double pe_only = computePotential(*fc, &d);
    std::printf("pe %s %.17g\n", names[c], pe);
    CHECK(pe == pe_only);
    CHECK(pe < 0.0);
    // 1/2 sum m phi of the downloaded fp32 phi: the returned PE to the rounding of phi
    ParticleDataManager::copyToHost(phi_h, phi_d);
    double half = 0.0;
    for (size_t i = 0; i < n; i++) half += 0.5 * (double)h.mass[i] * (double)phi_h.pos_x[i];
    CHECK(rel(half, pe) < 1e-7);
    // the potential calls write no accelerations
    ParticleDataManager::copyToHost(h, d);
    CHECK(std::memcmp(ax.data(), h.acc_x, n * sizeof(float)) == 0);
    CHECK(std::memcmp(ay.data(), h.acc_y, n * sizeof(float)) == 0);
    CHECK(std::memcmp(az.data(), h.acc_z, n * sizeof(float)) == 0);
    // Direct and the exact tree: the triangular fp64 sum of Integrator::computePotentialEnergy, whose float result
    // carries the fp32 rounding (6e-8); the two fp64 sums group their fp32 tile sums differently
    if (c < 2) CHECK(rel(pe, ref) < 1e-6);
  }
  // the tree / grid methods on the structure as built by the calls above
  const double t = bh.getTree()->computePotential(&d, 0.5f, G, eps);
  const double g = hash.getGrid()->computePotential(&d, 2.0f, G, eps);
  CHECK(t == computePotential(bh, &d));
  CHECK(g == computePotential(hash, &d));

  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  ParticleDataManager::freeDevice(phi_d);
  ParticleDataManager::freeHost(phi_h);
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
