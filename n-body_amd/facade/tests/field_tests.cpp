// field_tests.cpp -- nbody::computeField and the tree / grid computeField methods of the facade on a real GPU: the
// known answers of the field at points that are not bodies.
//   one body of mass M at the origin:  a = -G M x (r^2 + eps^2)^-3/2,  phi = -G M (r^2 + eps^2)^-1/2  (the hash: phi
//     shifted by +G M (rc^2 + eps^2)^-1/2 inside the cutoff, exact zeros beyond it)
//   two equal bodies: a = 0 at the midpoint
//   4,096 bodies of initSpherical: Barnes-Hut at theta = 0 equals the Direct field; nobody's accelerations are written
// Device float4 arrays are the pos_x arrays of ParticleData blocks of 4 n floats.  Prints one "field <method> <phi at
// the first point>" line per calculator (tests/test_field_gpu.py compares them with the Python API).  Exit code = number
// of failed checks.
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

static bool close_to(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::fmax(std::fabs(b), 1e-30); }

// n float4 on the device inside a ParticleData block (pos_x of 4 n floats), with its host mirror
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
  void upload() { ParticleDataManager::copyToDevice(d, h); }
  void download() { ParticleDataManager::copyToHost(h, d); }
};

static void few_bodies(ParticleData& d, ParticleData& h, size_t n, const float (*xyz)[3], float mass) {
  ParticleDataManager::allocateDevice(d, n);
  ParticleDataManager::allocateHost(h, n);
  ParticleInitializer::zeroVelocities(h);
  ParticleInitializer::zeroAccelerations(h);
  for (size_t i = 0; i < n; i++) {
    h.pos_x[i] = xyz[i][0]; h.pos_y[i] = xyz[i][1]; h.pos_z[i] = xyz[i][2];
    h.mass[i] = mass;
  }
  ParticleDataManager::copyToDevice(d, h);
}

int main() {
  const float G = 1.5f, eps = 0.1f, M = 2.0f, rc = 2.0f;
  const double e2 = (double)(eps * eps);
  const char* names[] = {"direct", "bh_theta0", "bh_theta0.5", "hash_cell2_cutoff2"};
  // (a calculator sizes its tree / grid from the first body count it sees: one set per body set)
  struct Calcs {
    DirectForceCalculator direct{256};
    BarnesHutCalculator bh0{0.0f}, bh{0.5f};
    SpatialHashCalculator hash{2.0f, 2.0f};  // cutoff <= cell: the truncated sum over all bodies
    ForceCalculator* all[4] = {&direct, &bh0, &bh, &hash};
    Calcs(float G, float eps) {
      for (ForceCalculator* fc : all) {
        fc->setGravitationalConstant(G);
        fc->setSofteningParameter(eps);
      }
    }
  };

  {  // one body at the origin; five points, the last one beyond the cutoff
    Calcs cs(G, eps);
    ForceCalculator** calcs = cs.all;
    ParticleData d, h;
    const float at0[1][3] = {{0.f, 0.f, 0.f}};
    few_bodies(d, h, 1, at0, M);
    const size_t m = 5;
    const float pts[m][3] = {{0.5f, 0.f, 0.f}, {0.f, -1.25f, 0.f}, {0.3f, 0.4f, 1.2f}, {0.f, 0.f, 0.f}, {3.f, -4.f, 12.f}};
    Float4Array p(m), out(m);
    for (size_t k = 0; k < m; k++) std::memcpy(p.row(k), pts[k], 3 * sizeof(float));
    p.upload();
    for (int c = 0; c < 4; c++) {
      computeField(*calcs[c], &d, p.dev(), m, out.dev());
      out.download();
      std::printf("field %s %.9g\n", names[c], (double)out.row(0)[3]);
      for (size_t k = 0; k < m; k++) {
        const double r2 = (double)pts[k][0] * pts[k][0] + (double)pts[k][1] * pts[k][1] + (double)pts[k][2] * pts[k][2];
        const bool cut = c == 3 && !(r2 < (double)rc * rc);
        const double inv = 1.0 / std::sqrt(r2 + e2);
        const double f = cut ? 0.0 : -(double)G * M * inv * inv * inv;
        double phi = cut ? 0.0 : -(double)G * M * inv;
        if (c == 3 && !cut) phi += (double)G * M / std::sqrt((double)rc * rc + e2);
        for (int a = 0; a < 3; a++) CHECK(std::fabs(out.row(k)[a] - f * pts[k][a]) <= 1e-5 * std::fabs(f) * std::sqrt(r2) + 1e-30);
        CHECK(close_to(out.row(k)[3], phi, 1e-5) || (phi == 0.0 && out.row(k)[3] == 0.0f));
      }
    }
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }

  {  // two equal bodies: no force at the midpoint, phi = -2 G M / sqrt(r^2 + eps^2)
    Calcs cs(G, eps);
    ForceCalculator** calcs = cs.all;
    ParticleData d, h;
    const float two[2][3] = {{-0.5f, 0.25f, 1.0f}, {0.5f, -0.25f, -1.0f}};
    few_bodies(d, h, 2, two, M);
    Float4Array p(1), out(1);
    p.upload();  // the origin
    for (int c = 0; c < 4; c++) {
      computeField(*calcs[c], &d, p.dev(), 1, out.dev());
      out.download();
      const double r2 = 0.25 + 0.0625 + 1.0, inv = 1.0 / std::sqrt(r2 + e2);
      for (int a = 0; a < 3; a++) CHECK(std::fabs(out.row(0)[a]) <= 1e-6 * (double)G * M * inv * inv);
      double phi = -2.0 * (double)G * M * inv;
      if (c == 3) phi += 2.0 * (double)G * M / std::sqrt((double)rc * rc + e2);
      CHECK(close_to(out.row(0)[3], phi, 1e-5));
    }
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }

  {  // a sphere of bodies: the exact tree is the Direct field; nothing writes accelerations; methods = calculators
    const size_t n = 4096, m = 1000;
    Calcs cs(G, eps);
    DirectForceCalculator& direct = cs.direct;
    BarnesHutCalculator &bh0 = cs.bh0, &bh = cs.bh;
    SpatialHashCalculator& hash = cs.hash;
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, n);
    ParticleDataManager::allocateHost(h, n);
    SphericalDistParams sp;
    sp.center = Vec3(0, 0, 0);
    sp.radius = 10.0f;
    ParticleInitializer::initSpherical(h, sp, 42);
    ParticleDataManager::copyToDevice(d, h);
    direct.computeForces(&d);
    ParticleDataManager::copyToHost(h, d);
    const std::vector<float> ax(h.acc_x, h.acc_x + n), ay(h.acc_y, h.acc_y + n), az(h.acc_z, h.acc_z + n);
    Float4Array p(m), od(m), ot(m), om(m);
    for (size_t k = 0; k < m; k++) {  // a lattice through and around the sphere
      p.row(k)[0] = -13.5f + 3.0f * (float)(k % 10);
      p.row(k)[1] = -13.5f + 3.0f * (float)((k / 10) % 10);
      p.row(k)[2] = -13.5f + 3.0f * (float)(k / 100);
    }
    p.upload();
    computeField(direct, &d, p.dev(), m, od.dev());
    computeField(bh0, &d, p.dev(), m, ot.dev());
    od.download();
    ot.download();
    double worst_a = 0.0, worst_phi = 0.0;
    for (size_t k = 0; k < m; k++) {
      double da = 0.0, na = 0.0;
      for (int a = 0; a < 3; a++) {
        da += std::pow((double)ot.row(k)[a] - od.row(k)[a], 2);
        na += std::pow((double)od.row(k)[a], 2);
      }
      worst_a = std::fmax(worst_a, std::sqrt(da / na));
      worst_phi = std::fmax(worst_phi, std::fabs(((double)ot.row(k)[3] - od.row(k)[3]) / od.row(k)[3]));
      CHECK(od.row(k)[3] < 0.0f);
    }
    std::printf("field sphere: tree(theta 0) vs direct max rel a %.3e phi %.3e\n", worst_a, worst_phi);
    CHECK(worst_a < 1e-4);   // (a lattice point may sit where the forces nearly cancel: the per-point bound is the
    CHECK(worst_phi < 1e-5); //  Python suite's; phi has no cancellation)
    // the members on the structures the calculators built
    computeField(bh, &d, p.dev(), m, ot.dev());
    bh.getTree()->computeField(p.dev(), m, 0.5f, G, eps, om.dev());
    ot.download();
    om.download();
    CHECK(std::memcmp(ot.row(0), om.row(0), m * 4 * sizeof(float)) == 0);
    computeField(hash, &d, p.dev(), m, ot.dev());
    hash.getGrid()->computeField(p.dev(), m, rc, G, eps, om.dev());
    ot.download();
    om.download();
    CHECK(std::memcmp(ot.row(0), om.row(0), m * 4 * sizeof(float)) == 0);
    ParticleDataManager::copyToHost(h, d);
    CHECK(std::memcmp(ax.data(), h.acc_x, n * sizeof(float)) == 0);
    CHECK(std::memcmp(ay.data(), h.acc_y, n * sizeof(float)) == 0);
    CHECK(std::memcmp(az.data(), h.acc_z, n * sizeof(float)) == 0);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
