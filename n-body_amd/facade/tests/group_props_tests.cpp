// group_props_tests.cpp -- SpatialHashGrid::groupProperties of the facade on a real GPU (nbody_hip_group_props.h: the model).
//   an exact lattice (mirrored pairs about integer centres: every sum exact whatever its order) at the sizes at which the
//     pass changes its form (1, 2, 5, 32, 33, 1024, 1025, 2049), the bodies scattered over the index range: every field
//     of every struct against integer arithmetic
//   a group with a member = count and an empty group get status 1, n 0 and zeros; their neighbours are untouched
//   the error paths: null particle data, a catalogue whose offsets do not match its n_groups; no groups: no structs
//   2,000 bodies of initUniform (seed 42) with a shear velocity, groups at b = 0.6, phi of the grid's own potential
// Prints "group props uniform <n_groups> <checksum of the structs' bytes>" (tests/test_group_props_facade_gpu.py compares it
// with the Python API on the same bodies).  Exit code = number of failed checks.
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

static unsigned long long g_rng = 88172645463325252ULL;
static int draw(int lo, int hi) {  // xorshift64: the same lattice on every run
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return lo + (int)(g_rng % (unsigned long long)(hi - lo + 1));
}

struct Expected {
  long long M2 = 0, L2[3] = {0, 0, 0}, T2 = 0, I2[6] = {0, 0, 0, 0, 0, 0}, W16 = 0, r2 = -1, phi8 = 1;
  int c[3], V[3], r2_body = 0, phi_body = 0, n = 0, label = 0;
};

int main() {
  {  // the lattice
    const int sizes[] = {3, 1, 2, 5, 32, 33, 4, 1024, 1025, 1, 2049, 6};
    const int groups = (int)(sizeof(sizes) / sizeof(sizes[0]));
    int total = 0;
    for (int n : sizes) total += n;
    const int count = total + 501;  // 501 bodies of no group
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, (size_t)count);
    ParticleDataManager::allocateHost(h, (size_t)count);
    std::vector<float> phi((size_t)count);
    for (int i = 0; i < count; i++) {  // the background
      h.pos_x[i] = (float)draw(-600, 600); h.pos_y[i] = (float)draw(-600, 600); h.pos_z[i] = (float)draw(-600, 600);
      h.vel_x[i] = (float)draw(-20, 20); h.vel_y[i] = (float)draw(-20, 20); h.vel_z[i] = (float)draw(-20, 20);
      h.mass[i] = 3.0f;
      phi[(size_t)i] = (float)draw(-512, 0) / 8.0f;
    }
    GroupCatalogue cat;
    std::vector<Expected> want((size_t)groups);
    const float masses[4] = {0.5f, 1.0f, 2.0f, 4.0f};
    int at = 0;
    cat.offsets.push_back(0);
    for (int g = 0; g < groups; g++) {
      Expected& e = want[(size_t)g];
      e.n = sizes[g];
      for (int a = 0; a < 3; a++) { e.c[a] = draw(-512, 512); e.V[a] = draw(-16, 16); }
      int o[3] = {0, 0, 0}, w[3] = {0, 0, 0};
      float m = 1.0f;
      for (int k = 0; k < sizes[g]; k++, at++) {
        const int body = (int)(((long long)at * 7919 + 13) % count);  // 7919 is prime to count: a permutation
        const bool centre = (sizes[g] % 2) && k == sizes[g] - 1;
        int sign = (k % 2) ? -1 : 1;
        if (k % 2 == 0 || centre) {
          for (int a = 0; a < 3; a++) { o[a] = draw(-32, 32); w[a] = draw(-8, 8); }
          m = masses[draw(0, 3)];
        }
        if (centre) sign = 0;
        h.pos_x[body] = (float)(e.c[0] + sign * o[0]); h.pos_y[body] = (float)(e.c[1] + sign * o[1]); h.pos_z[body] = (float)(e.c[2] + sign * o[2]);
        h.vel_x[body] = (float)(e.V[0] + sign * w[0]); h.vel_y[body] = (float)(e.V[1] + sign * w[1]); h.vel_z[body] = (float)(e.V[2] + sign * w[2]);
        h.mass[body] = m;
        if (sizes[g] <= 6) phi[(size_t)body] = (float)(-40 + draw(0, 1)) / 8.0f;  // ties in the minimum
        cat.members.push_back(body);
        if (k == 0) e.label = body;
        const long long m2 = (long long)(2 * m), dd[3] = {sign * o[0], sign * o[1], sign * o[2]}, uu[3] = {sign * w[0], sign * w[1], sign * w[2]};
        e.M2 += m2;
        for (int a = 0; a < 3; a++) e.L2[a] += m2 * (dd[(a + 1) % 3] * uu[(a + 2) % 3] - dd[(a + 2) % 3] * uu[(a + 1) % 3]);
        e.T2 += m2 * (uu[0] * uu[0] + uu[1] * uu[1] + uu[2] * uu[2]);
        const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
        for (int q = 0; q < 6; q++) e.I2[q] += m2 * dd[pa[q]] * dd[pb[q]];
        const long long p8 = (long long)(8 * phi[(size_t)body]), r2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
        e.W16 += m2 * p8;
        if (r2 > e.r2 || (r2 == e.r2 && body < e.r2_body)) { e.r2 = r2; e.r2_body = body; }
        if (e.phi8 > 0 || p8 < e.phi8 || (p8 == e.phi8 && body < e.phi_body)) { e.phi8 = p8; e.phi_body = body; }
      }
      cat.offsets.push_back(at);
    }
    cat.n_groups = (size_t)groups;
    CHECK(count % 7919 != 0 && at == total);
    ParticleDataManager::copyToDevice(d, h);
    // phi on the device: in an array of a second block
    ParticleData dphi, hphi;
    ParticleDataManager::allocateDevice(dphi, (size_t)count);
    ParticleDataManager::allocateHost(hphi, (size_t)count);
    std::memcpy(hphi.pos_x, phi.data(), (size_t)count * sizeof(float));
    ParticleDataManager::copyToDevice(dphi, hphi);
    SpatialHashGrid grid((size_t)count, 64.0f);  // (the call is generic in the catalogue: the grid need not be built)
    std::vector<GroupProperties> out;
    grid.groupProperties(&d, cat, out, dphi.pos_x);
    CHECK(out.size() == (size_t)groups);
    for (int g = 0; g < groups && out.size() == (size_t)groups; g++) {
      const GroupProperties& o = out[(size_t)g];
      const Expected& e = want[(size_t)g];
      CHECK(o.status == 0 && o.n == e.n && o.label == e.label && o.mass == e.M2 / 2.0);
      for (int a = 0; a < 3; a++) CHECK(o.com[a] == e.c[a] && o.vel[a] == e.V[a] && o.ang_mom[a] == e.L2[a] / 2.0);
      CHECK(o.kinetic == e.T2 / 4.0 && o.potential == e.W16 / 32.0);
      for (int q = 0; q < 6; q++) CHECK(o.inertia[q] == e.I2[q] / 2.0);
      CHECK(o.r_max == std::sqrt((double)e.r2) && o.r_max_body == e.r2_body);
      CHECK(o.phi_min == e.phi8 / 8.0 && o.phi_min_body == e.phi_body);
      CHECK(o.reserved[0] == 0 && o.reserved[1] == 0 && o.reserved[2] == 0);
    }
    // without phi
    std::vector<GroupProperties> bare;
    grid.groupProperties(&d, cat, bare);
    for (int g = 0; g < groups && bare.size() == (size_t)groups; g++)
      CHECK(bare[(size_t)g].potential == 0.0 && bare[(size_t)g].phi_min == 0.0 && bare[(size_t)g].phi_min_body == -1 &&
            bare[(size_t)g].kinetic == out[(size_t)g].kinetic && bare[(size_t)g].r_max_body == out[(size_t)g].r_max_body);
    // a member = count in group 5 (33 members: the chunked form) and in group 0; an empty group after group 2
    GroupCatalogue bad = cat;
    bad.members[(size_t)bad.offsets[5] + 20] = count;
    bad.members[1] = count;
    const int empty_at = bad.offsets[3];
    bad.offsets.insert(bad.offsets.begin() + 3, empty_at);
    bad.n_groups++;
    std::vector<GroupProperties> spoiled;
    grid.groupProperties(&d, bad, spoiled, dphi.pos_x);
    CHECK(spoiled.size() == (size_t)groups + 1);
    GroupProperties zero;
    std::memset(&zero, 0, sizeof zero);
    zero.status = 1;
    for (size_t g = 0; g < spoiled.size() && spoiled.size() == (size_t)groups + 1; g++) {
      const size_t old = g < 3 ? g : g - 1;
      if (g == 0 || g == 3 || g == 6) CHECK(std::memcmp(&spoiled[g], &zero, sizeof zero) == 0);
      else CHECK(std::memcmp(&spoiled[g], &out[old], sizeof zero) == 0);
    }
    // the error paths
    bool refused = false;
    try { grid.groupProperties(nullptr, cat, out); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    refused = false;
    GroupCatalogue torn = cat;
    torn.n_groups++;
    try { grid.groupProperties(&d, torn, out); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    GroupCatalogue none;
    none.offsets.push_back(0);
    grid.groupProperties(&d, none, out);
    CHECK(out.empty());
    ParticleDataManager::freeDevice(d); ParticleDataManager::freeHost(h);
    ParticleDataManager::freeDevice(dphi); ParticleDataManager::freeHost(hphi);
  }
  {  // a uniform box: the Python API computes the same bytes
    const size_t n = 2000;
    ParticleData d, h, dphi;
    ParticleDataManager::allocateDevice(d, n);
    ParticleDataManager::allocateDevice(dphi, n);
    ParticleDataManager::allocateHost(h, n);
    UniformDistParams up;
    up.min_bounds = Vec3(-5, -5, -5);
    up.max_bounds = Vec3(5, 5, 5);
    ParticleInitializer::initUniform(h, up, 42);
    for (size_t i = 0; i < n; i++) {  // a shear flow: products of two floats, rounded once
      h.vel_x[i] = 0.5f * h.pos_y[i]; h.vel_y[i] = -0.25f * h.pos_z[i]; h.vel_z[i] = 0.125f * h.pos_x[i];
    }
    ParticleDataManager::copyToDevice(d, h);
    SpatialHashGrid grid(n, 0.75f);
    grid.build(&d);
    grid.computePotential(&d, 0.75f, 1.0f, 0.01f, dphi.pos_x);
    GroupCatalogue c;
    grid.findGroups(0.6f, 1, c);
    std::vector<GroupProperties> a, b;
    grid.groupProperties(&d, c, a, dphi.pos_x);
    grid.groupProperties(&d, c, b, dphi.pos_x);
    CHECK(a.size() == c.n_groups && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(GroupProperties)) == 0);
    size_t members = 0;
    for (const GroupProperties& o : a) {
      CHECK(o.status == 0 && o.n >= 1 && o.phi_min_body >= 0 && o.mass > 0.0);
      members += (size_t)o.n;
    }
    CHECK(members == n);
    unsigned long long sum = 0;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(a.data());
    for (size_t k = 0; k < a.size() * sizeof(GroupProperties) / 8; k++) sum = sum * 1099511628211ULL + words[k];
    std::printf("group props uniform %zu %016llx\n", a.size(), sum);
    ParticleDataManager::freeDevice(d); ParticleDataManager::freeDevice(dphi); ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
