// quadrupole_tests.cpp -- multipole order 2 through the facade on a real GPU.  4,096 bodies of
// ParticleInitializer::initSpherical (radius 10, seed 42), G = 1, eps = 0.1, theta = 0.5.  The order is set on a
// BarnesHutCalculator before its first computeForces; checks the order reaches the tree, the moment export, the
// errors, and that order 2 differs from order 1.  With an argument, writes the bodies, the order-2 accelerations and
// PE to that file (tests/test_bh_quadrupole_gpu.py compares them bit for bit with the Python API on the same bodies):
//   int64 n, float pos_x[n], pos_y[n], pos_z[n], mass[n], acc_x[n], acc_y[n], acc_z[n], double pe
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

template <class E, class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  const size_t n = 4096;
  const float G = 1.0f, eps = 0.1f, theta = 0.5f;
  ParticleData d, h;
  ParticleDataManager::allocateDevice(d, n);
  ParticleDataManager::allocateHost(h, n);
  SphericalDistParams p;
  p.center = Vec3(0, 0, 0);
  p.radius = 10.0f;
  ParticleInitializer::initSpherical(h, p, 42);
  ParticleDataManager::copyToDevice(d, h);

  BarnesHutCalculator quad(theta), mono(theta);
  for (BarnesHutCalculator* c : {&quad, &mono}) {
    c->setGravitationalConstant(G);
    c->setSofteningParameter(eps);
  }
  CHECK(quad.getMultipoleOrder() == 1);
  quad.setMultipoleOrder(2);  // before the first computeForces: the tree does not exist yet
  CHECK(quad.getMultipoleOrder() == 2 && quad.getTree() == nullptr);
  CHECK(throws<ValidationException>([&] { quad.setMultipoleOrder(3); }));
  CHECK(throws<ValidationException>([&] { quad.setMultipoleOrder(0); }));
  CHECK(quad.getMultipoleOrder() == 2);

  quad.computeForces(&d);
  CHECK(quad.getTree() != nullptr && quad.getTree()->getMultipoleOrder() == 2);
  ParticleDataManager::copyToHost(h, d);
  const std::vector<float> ax(h.acc_x, h.acc_x + n), ay(h.acc_y, h.acc_y + n), az(h.acc_z, h.acc_z + n);
  const double pe = computePotential(quad, &d);
  std::printf("pe quadrupole %.17g\n", pe);
  CHECK(pe < 0.0);
  // the moments: 6 per node, positive semi-definite diagonal, one-body leaves zero
  const std::vector<float> mom = quad.getTree()->copyMomentsToHost();
  CHECK(mom.size() == 6 * static_cast<size_t>(quad.getTree()->getNodeCount()));
  bool diag_ok = true;
  for (size_t k = 0; k < mom.size() / 6; k++) diag_ok = diag_ok && mom[6 * k] >= 0.f && mom[6 * k + 1] >= 0.f && mom[6 * k + 2] >= 0.f;
  CHECK(diag_ok);
  CHECK(mom[0] + mom[1] + mom[2] > 0.f);  // the root of a sphere of radius 10

  // order 1 on the same bodies: other forces, no moments
  mono.computeForces(&d);
  ParticleDataManager::copyToHost(h, d);
  CHECK(std::memcmp(ax.data(), h.acc_x, n * sizeof(float)) != 0);
  CHECK(throws<CudaException>([&] { (void)mono.getTree()->copyMomentsToHost(); }));
  // an order change without a rebuild is refused; the calculator rebuilds, so it goes on working
  mono.getTree()->setMultipoleOrder(2);
  CHECK(throws<CudaException>([&] { mono.getTree()->computeForces(&d, theta, G, eps); }));
  mono.setMultipoleOrder(2);
  mono.computeForces(&d);
  ParticleDataManager::copyToHost(h, d);
  CHECK(std::memcmp(ax.data(), h.acc_x, n * sizeof(float)) == 0);
  CHECK(std::memcmp(ay.data(), h.acc_y, n * sizeof(float)) == 0);
  CHECK(std::memcmp(az.data(), h.acc_z, n * sizeof(float)) == 0);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f != nullptr);
    if (f) {
      const int64_t nn = static_cast<int64_t>(n);
      std::fwrite(&nn, sizeof(nn), 1, f);
      for (const float* a : {h.pos_x, h.pos_y, h.pos_z, h.mass}) std::fwrite(a, sizeof(float), n, f);
      for (const std::vector<float>* a : {&ax, &ay, &az}) std::fwrite(a->data(), sizeof(float), n, f);
      std::fwrite(&pe, sizeof(pe), 1, f);
      std::fclose(f);
    }
  }
  ParticleDataManager::freeDevice(d);
  ParticleDataManager::freeHost(h);
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
