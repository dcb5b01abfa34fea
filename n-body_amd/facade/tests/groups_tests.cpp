// groups_tests.cpp -- SpatialHashGrid::findGroups of the facade on a real GPU: known answers of the friends-of-friends
// groups (nbody_hip_groups.h).
//   a 5 x 5 x 5 integer lattice, spacing 1, cell 1.5: b = 1 links nobody (d2 = 1 is not below 1), the next float above 1
//     links everything, b = 1.5 too
//   two bodies at one place are linked; min_members = 2 drops the singletons from the lists, not from the labels
//   b above the cell size is a ValidationException that names both values
//   2,000 bodies of initUniform (seed 42): the catalogue is consistent with its labels, and a second call equals the first
// Prints "groups uniform <n_groups> <n_members> <largest> <label checksum>" (tests/test_groups_gpu.py compares it with the
// Python API on the same bodies).  Exit code = number of failed checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
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

// the catalogue against its own labels: groups ascending by label, members ascending, every member labelled with the
// first member, every body of a kept group listed
static bool consistent(const GroupCatalogue& c, int min_members) {
  const size_t n = c.labels.size();
  if (c.offsets.size() != c.n_groups + 1 || c.offsets[0] != 0 || (size_t)c.offsets[c.n_groups] != c.members.size()) return false;
  std::vector<int> size(n, 0);
  for (size_t i = 0; i < n; i++) {
    if (c.labels[i] < 0 || (size_t)c.labels[i] > i || c.labels[(size_t)c.labels[i]] != c.labels[i]) return false;
    size[(size_t)c.labels[i]]++;
  }
  size_t kept = 0;
  for (size_t i = 0; i < n; i++) kept += size[(size_t)c.labels[i]] >= min_members ? 1 : 0;
  if (kept != c.members.size()) return false;
  int last = -1;
  for (size_t g = 0; g < c.n_groups; g++) {
    const int a = c.offsets[g], b = c.offsets[g + 1];
    if (b - a < min_members || c.members[(size_t)a] <= last) return false;
    last = c.members[(size_t)a];
    if (size[(size_t)last] != b - a) return false;
    for (int k = a; k < b; k++) {
      if (c.labels[(size_t)c.members[(size_t)k]] != last) return false;
      if (k > a && c.members[(size_t)k] <= c.members[(size_t)k - 1]) return false;
    }
  }
  return true;
}

int main() {
  {  // the lattice
    std::vector<Vec3> xyz;
    for (int z = 0; z < 5; z++)
      for (int y = 0; y < 5; y++)
        for (int x = 0; x < 5; x++) xyz.push_back(Vec3((float)x, (float)y, (float)z));
    ParticleData d, h;
    bodies(d, h, xyz);
    SpatialHashGrid grid(125, 1.5f);
    grid.build(&d);
    GroupCatalogue c;
    grid.findGroups(1.0f, 1, c);
    CHECK(c.n_groups == 125 && c.members.size() == 125 && consistent(c, 1));
    for (size_t i = 0; i < 125; i++) CHECK(c.labels[i] == (int)i && c.members[i] == (int)i && c.offsets[i] == (int)i);
    grid.findGroups(std::nextafter(1.0f, 2.0f), 1, c);
    CHECK(c.n_groups == 1 && c.members.size() == 125 && c.offsets[0] == 0 && c.offsets[1] == 125 && consistent(c, 1));
    for (size_t i = 0; i < 125; i++) CHECK(c.labels[i] == 0 && c.members[i] == (int)i);
    grid.findGroups(1.5f, 1, c);
    CHECK(c.n_groups == 1 && consistent(c, 1));
    grid.findGroups(1.0f, 2, c);  // nobody is kept
    CHECK(c.n_groups == 0 && c.members.empty() && c.offsets.size() == 1 && c.offsets[0] == 0 && c.labels[124] == 124);
    bool refused = false;
    try {
      grid.findGroups(1.75f, 1, c);
    } catch (const ValidationException& e) {
      refused = std::strstr(e.what(), "1.75") && std::strstr(e.what(), "1.5");
    }
    CHECK(refused);
    refused = false;
    try {
      grid.findGroups(1.0f, 0, c);
    } catch (const ValidationException&) {
      refused = true;
    }
    CHECK(refused);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  {  // coincident bodies, and min_members
    const std::vector<Vec3> xyz = {Vec3(0, 0, 0), Vec3(3, 0, 0), Vec3(3, 0, 0), Vec3(0, 3, 0), Vec3(3.25f, 0, 0)};
    ParticleData d, h;
    bodies(d, h, xyz);
    SpatialHashGrid grid(5, 1.0f);
    grid.build(&d);
    GroupCatalogue c;
    grid.findGroups(0.5f, 1, c);
    const int labels[5] = {0, 1, 1, 3, 1};
    CHECK(c.n_groups == 3 && consistent(c, 1) && std::memcmp(c.labels.data(), labels, sizeof(labels)) == 0);
    grid.findGroups(0.5f, 2, c);
    const int members[3] = {1, 2, 4};
    CHECK(c.n_groups == 1 && c.members.size() == 3 && std::memcmp(c.members.data(), members, sizeof(members)) == 0);
    CHECK(consistent(c, 2) && std::memcmp(c.labels.data(), labels, sizeof(labels)) == 0);
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
    GroupCatalogue a, b;
    grid.findGroups(0.6f, 2, a);
    grid.findGroups(0.6f, 2, b);
    CHECK(consistent(a, 2) && a.n_groups > 0 && a.n_groups < n);
    CHECK(a.labels == b.labels && a.offsets == b.offsets && a.members == b.members);
    int largest = 0;
    unsigned long long sum = 0;
    for (size_t g = 0; g < a.n_groups; g++) largest = std::max(largest, a.offsets[g + 1] - a.offsets[g]);
    for (size_t i = 0; i < n; i++) sum = sum * 1099511628211ULL + (unsigned long long)a.labels[i];
    std::printf("groups uniform %zu %zu %d %016llx\n", a.n_groups, a.members.size(), largest, sum);
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
