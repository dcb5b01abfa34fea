// neighbours_tests.cpp -- SpatialHashGrid::findNeighbours of the facade on a real GPU: known answers of the k nearest
// neighbours and the local density (nbody_hip_neighbours.h).
//   a 5 x 5 x 5 integer lattice, spacing 1, cell 1.5: the centre body's 26 neighbours are 6 at d2 = 1, 12 at 2 and 8 at 3,
//     each run ascending by index; k = 6 gives rho = 5 / (4 pi / 3); cell 1 flags the same answer as window-limited
//   two bodies at one place are each other's neighbour at d2 = 0 with status 3; a lone body has status 2, -1 and +inf
//   k = 0 and k = 33 are ValidationExceptions; an unbuilt grid is refused
//   2,000 bodies of initUniform (seed 42): a second call equals the first
// Prints "neighbours uniform <exact bodies> <index checksum> <dist2 checksum> <rho checksum>" (tests/
// test_neighbours_facade_gpu.py compares it with the Python API on the same bodies).  Exit code = number of failed checks.
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

static void bodies(ParticleData& d, ParticleData& h, const std::vector<Vec3>& xyz) {
  const size_t n = xyz.size();
  ParticleDataManager::allocateDevice(d, n);
  ParticleDataManager::allocateHost(h, n);
  ParticleInitializer::zeroVelocities(h);
  ParticleInitializer::zeroAccelerations(h);
  for (size_t i = 0; i < n; i++) {
    h.pos_x[i] = xyz[i].x; h.pos_y[i] = xyz[i].y; h.pos_z[i] = xyz[i].z;
    h.mass[i] = 1.0f;
  }
  ParticleDataManager::copyToDevice(d, h);
}

int main() {
  const double sphere = 4.1887902047863905;
  {  // the lattice
    std::vector<Vec3> xyz;
    for (int z = 0; z < 5; z++)
      for (int y = 0; y < 5; y++)
        for (int x = 0; x < 5; x++) xyz.push_back(Vec3((float)x, (float)y, (float)z));
    ParticleData d, h;
    bodies(d, h, xyz);
    const int c = 2 + 5 * 2 + 25 * 2;
    {
      SpatialHashGrid grid(125, 1.5f);
      grid.build(&d);
      NeighbourLists nl;
      grid.findNeighbours(26, nl);
      CHECK(nl.k == 26 && nl.index.size() == 125 * 26 && nl.dist2.size() == 125 * 26 && nl.rho.size() == 125 && nl.status.size() == 125);
      for (int s = 0; s < 26; s++) {
        CHECK(nl.dist2[(size_t)c * 26 + s] == (s < 6 ? 1.0f : s < 18 ? 2.0f : 3.0f));
        if (s != 0 && s != 6 && s != 18) CHECK(nl.index[(size_t)c * 26 + s] > nl.index[(size_t)c * 26 + s - 1]);
      }
      CHECK(nl.index[(size_t)c * 26] == c - 25 && nl.index[(size_t)c * 26 + 6] == c - 30 && nl.status[c] == 1);
      grid.findNeighbours(6, nl);
      const int faces[6] = {c - 25, c - 5, c - 1, c + 1, c + 5, c + 25};
      CHECK(std::memcmp(&nl.index[(size_t)c * 6], faces, sizeof(faces)) == 0);
      CHECK(nl.status[c] == 0 && nl.rho[c] == 5.0 / sphere);  // d2_k = 1 < 2.25
      for (int k : {0, 33, -4}) {
        bool refused = false;
        try {
          grid.findNeighbours(k, nl);
        } catch (const ValidationException& e) {
          refused = std::strstr(e.what(), "1 .. 32") != nullptr;
        }
        CHECK(refused);
      }
      CHECK(nl.k == 6 && nl.index.size() == 125 * 6);  // a refused call leaves `out` alone
    }
    {
      SpatialHashGrid grid(125, 1.0f);
      grid.build(&d);
      NeighbourLists nl;
      grid.findNeighbours(6, nl);
      CHECK(nl.status[c] == 1 && nl.rho[c] == 5.0 / sphere && nl.dist2[(size_t)c * 6 + 5] == 1.0f);  // 1 is not below fl(1 * 1)
      bool refused = false;
      SpatialHashGrid unbuilt(125, 1.0f);
      try {
        unbuilt.findNeighbours(6, nl);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  {  // coincident bodies, and a lone one
    const std::vector<Vec3> xyz = {Vec3(0, 0, 0), Vec3(3, 0, 0), Vec3(3, 0, 0), Vec3(0, 8, 0)};
    ParticleData d, h;
    bodies(d, h, xyz);
    SpatialHashGrid grid(4, 1.0f);
    grid.build(&d);
    NeighbourLists nl;
    grid.findNeighbours(1, nl);
    CHECK(nl.index[1] == 2 && nl.index[2] == 1 && nl.dist2[1] == 0.0f && nl.dist2[2] == 0.0f);
    CHECK(nl.status[1] == 3 && nl.status[2] == 3 && nl.rho[1] == 0.0 && nl.rho[2] == 0.0);
    CHECK(nl.status[3] == 2 && nl.index[3] == -1 && std::isinf(nl.dist2[3]) && nl.dist2[3] > 0 && nl.rho[3] == 0.0);
    CHECK(nl.status[0] == 2 && nl.index[0] == -1);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  {  // a uniform box
    const size_t n = 2000;
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, n);
    ParticleDataManager::allocateHost(h, n);
    UniformDistParams up;
    up.min_bounds = Vec3(-5, -5, -5);
    up.max_bounds = Vec3(5, 5, 5);
    ParticleInitializer::initUniform(h, up, 42);
    ParticleDataManager::copyToDevice(d, h);
    SpatialHashGrid grid(n, 0.75f);
    grid.build(&d);
    NeighbourLists a, b;
    grid.findNeighbours(8, a);
    grid.findNeighbours(8, b);
    CHECK(a.index == b.index && a.dist2 == b.dist2 && a.status == b.status);
    CHECK(std::memcmp(a.rho.data(), b.rho.data(), n * sizeof(double)) == 0);
    size_t exact = 0;
    unsigned long long si = 0, sd = 0, sr = 0;
    for (size_t i = 0; i < n; i++) exact += a.status[i] == 0 ? 1 : 0;
    for (size_t j = 0; j < n * 8; j++) {
      unsigned int bits;
      std::memcpy(&bits, &a.dist2[j], sizeof(bits));
      si = si * 1099511628211ULL + (unsigned long long)(unsigned int)a.index[j];
      sd = sd * 1099511628211ULL + bits;
    }
    for (size_t i = 0; i < n; i++) {
      unsigned long long bits;
      std::memcpy(&bits, &a.rho[i], sizeof(bits));
      sr = sr * 1099511628211ULL + bits;
    }
    CHECK(exact > 0 && exact < n);
    std::printf("neighbours uniform %zu %016llx %016llx %016llx\n", exact, si, sd, sr);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
