// hop_tests.cpp -- SpatialHashGrid::hopGroups of the facade on a real GPU (nbody_hip_hop.h has the model).
//   two clumps of 40 bodies each on a line, denser towards their middles, 10 apart, and one stray body between them:
//     two groups, each clump one, group_peak the clumps' middles, the stray body below delta_outer and in no group
//   the refusals: k out of range, n_hop above k, thresholds out of order (ValidationExceptions), an unbuilt grid
//   2,000 bodies of initUniform (seed 42), delta_outer the lower median of the densities: what every catalogue must
//     satisfy (peaks are fixed points, labels are peaks, offsets and members in order, group_peak in its group), a second
//     call equal to the first
// Prints "hop uniform <delta_outer bits> <n_groups> <n_members> <n_peaks> <rounds> <labels> <peak> <offsets> <members>
// <group_peak>" with a checksum of each array (tests/test_hop_facade_gpu.py compares it with the Python API and with the
// numpy restatement on the same bodies).  Exit code = number of failed checks.
#include <algorithm>
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

static unsigned long long checksum(const std::vector<int>& v) {
  unsigned long long s = 0;
  for (int w : v) s = s * 1099511628211ULL + (unsigned long long)(unsigned int)w;
  return s;
}

// what every catalogue satisfies, whatever the bodies
static void invariants(const HopCatalogue& c, size_t n) {
  const GroupCatalogue& g = c.groups;
  CHECK(g.labels.size() == n && c.peak.size() == n && g.offsets.size() == g.n_groups + 1 && c.group_peak.size() == g.n_groups);
  CHECK(g.offsets.front() == 0 && (size_t)g.offsets.back() == g.members.size() && c.status == 0 && c.rounds >= 1);
  bool ok = true;
  long long peaks = 0;
  for (size_t i = 0; i < n; i++) {
    const int p = c.peak[i];
    ok = ok && p >= 0 && (size_t)p < n && c.peak[(size_t)p] == p;
    peaks += p == (int)i ? 1 : 0;
    const int lab = g.labels[i];
    ok = ok && (lab == -1 || (lab >= 0 && (size_t)lab < n && c.peak[(size_t)lab] == lab && g.labels[(size_t)lab] == lab));
    ok = ok && (lab == -1 || lab == g.labels[(size_t)p]);  // (a labelled body is labelled through its peak)
  }
  CHECK(ok && peaks == c.n_peaks);
  ok = true;
  int last_label = -1;
  for (size_t q = 0; q < g.n_groups; q++) {
    const int o0 = g.offsets[q], o1 = g.offsets[q + 1];
    ok = ok && o0 < o1;
    const int lab = g.labels[(size_t)g.members[(size_t)o0]];
    ok = ok && lab > last_label;
    last_label = lab;
    for (int m = o0; m < o1; m++) {
      ok = ok && g.labels[(size_t)g.members[(size_t)m]] == lab && (m == o0 || g.members[(size_t)m] > g.members[(size_t)m - 1]);
    }
    const int gp = c.group_peak[q];
    ok = ok && gp >= 0 && (size_t)gp < n && c.peak[(size_t)gp] == gp && g.labels[(size_t)gp] == lab;
  }
  CHECK(ok);
}

int main() {
  {  // two clumps on a line and a stray body
    std::vector<Vec3> xyz;
    for (int clump = 0; clump < 2; clump++)
      for (int s = -20; s < 20; s++) {  // spacing grows away from the middle: x = sign(s) * (0.02 |s| + 0.002 s^2)
        const float a = std::fabs((float)s);
        xyz.push_back(Vec3(10.0f * clump + (s < 0 ? -1.0f : 1.0f) * (0.02f * a + 0.002f * a * a), 0.0f, 0.0f));
      }
    xyz.push_back(Vec3(5.0f, 0.0f, 0.0f));
    const size_t n = xyz.size();
    ParticleData d, h;
    bodies(d, h, xyz);
    SpatialHashGrid grid(n, 4.0f);
    grid.build(&d);
    NeighbourLists nl;
    HopParameters hp;
    hp.n_merge = 2;
    hp.delta_outer = 1.0;  // far above the stray body's density (about 0.01), below every clump body's (above 5)
    hp.delta_saddle = hp.delta_peak = hp.delta_outer;  // every peak is viable, every saddle inside a clump unites
    HopCatalogue c;
    grid.hopGroups(4, hp, c, &nl);
    CHECK(nl.k == 4 && nl.index.size() == n * 4 && nl.rho.size() == n);
    CHECK(nl.rho[80] < hp.delta_outer && nl.rho[0] > hp.delta_outer && nl.rho[79] > hp.delta_outer);
    invariants(c, n);
    CHECK(c.groups.n_groups == 2 && c.groups.members.size() == 80 && c.groups.labels[80] == -1);
    if (c.groups.n_groups == 2) {
      CHECK(c.groups.offsets[1] == 40 && c.groups.members[0] == 0 && c.groups.members[40] == 40 && c.groups.members[79] == 79);
      CHECK(c.group_peak[0] >= 17 && c.group_peak[0] <= 23 && c.group_peak[1] >= 57 && c.group_peak[1] <= 63);
      CHECK(c.groups.labels[0] == c.groups.labels[39] && c.groups.labels[40] == c.groups.labels[79] &&
            c.groups.labels[0] != c.groups.labels[40]);
    }
    // min_members above the clumps: no group, the labels stay
    HopCatalogue none;
    hp.min_members = 41;
    grid.hopGroups(4, hp, none);
    CHECK(none.groups.n_groups == 0 && none.groups.offsets.size() == 1 && none.groups.members.empty() &&
          none.groups.labels == c.groups.labels && none.peak == c.peak);
    hp.min_members = 1;
    // the refusals leave `out` alone
    for (int which = 0; which < 5; which++) {
      HopParameters bad = hp;
      int k = 4;
      if (which == 0) k = 0;
      if (which == 1) k = 33;
      if (which == 2) bad.n_hop = 5;
      if (which == 3) bad.delta_saddle = 0.5 * hp.delta_outer;
      if (which == 4) bad.n_merge = 5;
      bool refused = false;
      try {
        grid.hopGroups(k, bad, c);
      } catch (const ValidationException&) {
        refused = true;
      }
      CHECK(refused);
    }
    CHECK(c.groups.n_groups == 2 && c.peak.size() == n);
    bool refused = false;
    SpatialHashGrid unbuilt(n, 4.0f);
    try {
      unbuilt.hopGroups(4, hp, c);
    } catch (const std::exception&) {
      refused = true;
    }
    CHECK(refused);
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
    NeighbourLists nl;
    grid.findNeighbours(8, nl);
    std::vector<double> sorted;
    for (double r : nl.rho)
      if (r == r) sorted.push_back(r);
    std::sort(sorted.begin(), sorted.end());
    CHECK(!sorted.empty());
    HopParameters hp;
    hp.n_merge = 4;
    hp.delta_outer = sorted.empty() ? 0.0 : sorted[(sorted.size() - 1) / 2];  // the lower median
    HopCatalogue a, b;
    NeighbourLists used;
    grid.hopGroups(8, hp, a, &used);
    grid.hopGroups(8, hp, b);
    CHECK(used.index == nl.index && std::memcmp(used.rho.data(), nl.rho.data(), n * sizeof(double)) == 0);
    invariants(a, n);
    CHECK(a.groups.labels == b.groups.labels && a.peak == b.peak && a.groups.offsets == b.groups.offsets &&
          a.groups.members == b.groups.members && a.group_peak == b.group_peak && a.n_peaks == b.n_peaks && a.rounds == b.rounds);
    CHECK(a.groups.n_groups >= 2 && a.n_peaks > (long long)a.groups.n_groups);
    std::vector<GroupProperties> props;
    grid.groupProperties(&d, a.groups, props);
    CHECK(props.size() == a.groups.n_groups);
    for (size_t g = 0; g < props.size(); g++)
      CHECK(props[g].status == 0 && props[g].n == a.groups.offsets[g + 1] - a.groups.offsets[g]);
    unsigned long long bits;
    std::memcpy(&bits, &hp.delta_outer, sizeof(bits));
    std::printf("hop uniform %016llx %zu %zu %lld %lld %016llx %016llx %016llx %016llx %016llx\n", bits, a.groups.n_groups,
                a.groups.members.size(), a.n_peaks, a.rounds, checksum(a.groups.labels), checksum(a.peak),
                checksum(a.groups.offsets), checksum(a.groups.members), checksum(a.group_peak));
    ParticleDataManager::freeDevice(d);
    ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
