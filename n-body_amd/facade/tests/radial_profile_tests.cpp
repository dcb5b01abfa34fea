// radial_profile_tests.cpp -- SpatialHashGrid::radialProfiles of the facade on a real GPU (nbody_hip_radial.h: the model).
//   an integer lattice (integer offsets about integer centres, masses powers of two, integer velocities along the offset's
//     one non-zero axis: every field exact) at the sizes at which the pass changes its form (1, 2, 5, 32, 33, 1024, 1025,
//     2049), the bodies scattered over the index range: the order, every cut and every sum against integer arithmetic on
//     a stable sort of the host, in the three modes
//   a group with a member = count and an empty group get status 1, n 0 and zero rows; their neighbours are untouched;
//     offsets out of order: every group
//   the error paths: null particle data, a torn catalogue, centres of the wrong size, cuts the library refuses; no groups
//   2,000 bodies of initUniform (seed 42) with a shear velocity, groups at b = 0.6, about their centres of mass
// Prints "radial profile uniform <n_groups> <checksum of the structs' bytes>" (tests/test_radial_profile_facade_gpu.py
// compares it with the Python API on the same bodies).  Exit code = number of failed checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nbody_facade.hpp"

using namespace nbody;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    g_checks++;                                                                            \
    if (!(cond)) { g_fail++; if (g_fail < 40) std::printf("  FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static unsigned long long g_rng = 88172645463325252ULL;
static int draw(int lo, int hi) {  // xorshift64: the same lattice on every run
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return lo + (int)(g_rng % (unsigned long long)(hi - lo + 1));
}

struct Member {
  int body, k, u, vtan2;  // |offset| along its axis, velocity along that axis (times the offset's sign), the rest squared
  double m;
};

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  {  // the lattice
    const int sizes[] = {3, 1, 2, 5, 32, 33, 4, 1024, 1025, 1, 2049, 6};
    const int groups = (int)(sizeof(sizes) / sizeof(sizes[0]));
    int total = 0;
    for (int n : sizes) total += n;
    const int count = total + 501;  // 501 bodies of no group
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, (size_t)count);
    ParticleDataManager::allocateHost(h, (size_t)count);
    for (int i = 0; i < count; i++) {  // the background
      h.pos_x[i] = (float)draw(-600, 600); h.pos_y[i] = (float)draw(-600, 600); h.pos_z[i] = (float)draw(-600, 600);
      h.vel_x[i] = (float)draw(-20, 20); h.vel_y[i] = (float)draw(-20, 20); h.vel_z[i] = (float)draw(-20, 20);
      h.mass[i] = 3.0f;
    }
    GroupCatalogue cat;
    std::vector<std::vector<Member>> want((size_t)groups);
    std::vector<double> centres, bulk;
    int at = 0;
    cat.offsets.push_back(0);
    for (int g = 0; g < groups; g++) {
      const int c[3] = {draw(-400, 400), draw(-400, 400), draw(-400, 400)}, V[3] = {draw(-16, 16), draw(-16, 16), draw(-16, 16)};
      for (int a = 0; a < 3; a++) { centres.push_back(c[a]); bulk.push_back(V[a]); }
      for (int p = 0; p < sizes[g]; p++, at++) {
        const int body = (int)(((long long)at * 7919) % count);  // scattered: 7919 is prime to count
        const int axis = draw(0, 2), k = p == 0 && g % 3 == 0 ? 0 : draw(-12, 12), w[3] = {draw(-6, 6), draw(-6, 6), draw(-6, 6)};
        float* pos[3] = {h.pos_x, h.pos_y, h.pos_z};
        float* vel[3] = {h.vel_x, h.vel_y, h.vel_z};
        for (int a = 0; a < 3; a++) { pos[a][body] = (float)(c[a] + (a == axis ? k : 0)); vel[a][body] = (float)(V[a] + w[a]); }
        const double m = std::ldexp(1.0, draw(-3, 3));
        h.mass[body] = (float)m;
        Member e;
        e.body = body; e.k = k < 0 ? -k : k; e.m = m;
        e.u = k == 0 ? 0 : (k < 0 ? -w[axis] : w[axis]);
        const int u2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        e.vtan2 = u2 - e.u * e.u;
        want[(size_t)g].push_back(e);
        cat.members.push_back(body);
      }
      cat.offsets.push_back(at);
    }
    cat.n_groups = (size_t)groups;
    CHECK(count % 7919 != 0 && at == total);
    ParticleDataManager::copyToDevice(d, h);
    for (auto& list : want)  // the radial order: ascending by (|offset|, position)
      std::stable_sort(list.begin(), list.end(), [](const Member& a, const Member& b) { return a.k < b.k; });
    SpatialHashGrid grid((size_t)count, 64.0f);  // (the call is generic in the catalogue: the grid need not be built)
    const std::vector<double> cuts[3] = {{0.125, 0.5, 1.0}, {0.1, 0.5, 1.0}, {0.0, 3.0, 7.5, inf}};
    std::vector<RadialGroup> G, clean_G;
    std::vector<RadialShell> S, clean_S;
    for (int mode = 0; mode < 3; mode++) {
      const size_t nc = cuts[mode].size();
      grid.radialProfiles(&d, cat, centres, cuts[mode], mode, G, S, &bulk);
      CHECK(G.size() == (size_t)groups && S.size() == (size_t)groups * nc);
      if (mode == 0) { clean_G = G; clean_S = S; }
      for (int g = 0; g < groups && G.size() == (size_t)groups; g++) {
        const std::vector<Member>& L = want[(size_t)g];
        const int n = sizes[g];
        double M = 0;
        for (const Member& e : L) M += e.m;  // exact: multiples of 1/8 below 2^24
        CHECK(G[(size_t)g].status == 0 && G[(size_t)g].n == n && G[(size_t)g].mass == M && G[(size_t)g].r_max == (double)L.back().k);
        CHECK(G[(size_t)g].reserved[0] == 0 && G[(size_t)g].reserved[1] == 0);
        int prev = 0;
        for (size_t c = 0; c < nc; c++) {
          const double cut = cuts[mode][c];
          int K = n;
          if (mode == RADIAL_NUMBER) {
            K = std::min(n, std::max(1, (int)std::ceil(cut * (double)n)));
          } else if (mode == RADIAL_MASS) {
            double E = 0;
            for (int s = 0; s < n; s++) { E += L[(size_t)s].m; if (E >= cut * M) { K = s + 1; break; } }
          } else {
            K = 0;
            while (K < n && (double)L[(size_t)K].k <= cut) K++;
          }
          double E = 0, sums[4] = {0, 0, 0, 0};
          for (int s = 0; s < K; s++) E += L[(size_t)s].m;
          for (int s = prev; s < K; s++) {
            const Member& e = L[(size_t)s];
            sums[0] += e.m; sums[1] += e.m * e.u; sums[2] += e.m * e.u * e.u; sums[3] += e.m * e.vtan2;
          }
          const RadialShell& o = S[(size_t)g * nc + c];
          CHECK(o.enclosed_count == K && o.count == K - prev && o.enclosed_mass == E);
          CHECK(o.radius == (mode == RADIAL_RADIUS ? cut : (double)L[(size_t)K - 1].k));
          CHECK(o.mass == sums[0] && o.m_vr == sums[1] && o.m_vr2 == sums[2] && o.m_vt2 == sums[3]);
          CHECK(o.reserved[0] == 0 && o.reserved[1] == 0);
          prev = K;
        }
      }
    }
    // without bulk velocities: the masses and the cuts are the same
    grid.radialProfiles(&d, cat, centres, cuts[0], RADIAL_MASS, G, S);
    for (size_t r = 0; r < S.size() && S.size() == clean_S.size(); r++)
      CHECK(S[r].enclosed_count == clean_S[r].enclosed_count && S[r].mass == clean_S[r].mass && S[r].radius == clean_S[r].radius);
    // a member = count in group 5 (33 members: the chunked form) and in group 0; an empty group after group 2
    GroupCatalogue bad = cat;
    bad.members[(size_t)bad.offsets[5] + 20] = count;
    bad.members[1] = count;
    const int empty_at = bad.offsets[3];
    bad.offsets.insert(bad.offsets.begin() + 3, empty_at);
    bad.n_groups++;
    std::vector<double> c2 = centres, b2 = bulk;
    c2.insert(c2.begin() + 9, 3, 0.0);
    b2.insert(b2.begin() + 9, 3, 0.0);
    grid.radialProfiles(&d, bad, c2, cuts[0], RADIAL_MASS, G, S, &b2);
    CHECK(G.size() == (size_t)groups + 1);
    RadialGroup zero;
    std::memset(&zero, 0, sizeof zero);
    zero.status = 1;
    const std::vector<RadialShell> zero_rows(3, RadialShell{});
    for (size_t g = 0; g < G.size() && G.size() == (size_t)groups + 1; g++) {
      const size_t old = g < 3 ? g : g - 1;
      if (g == 0 || g == 3 || g == 6) {
        CHECK(std::memcmp(&G[g], &zero, sizeof zero) == 0 && std::memcmp(&S[g * 3], zero_rows.data(), 3 * sizeof(RadialShell)) == 0);
      } else {
        CHECK(std::memcmp(&G[g], &clean_G[old], sizeof zero) == 0);
        CHECK(std::memcmp(&S[g * 3], &clean_S[old * 3], 3 * sizeof(RadialShell)) == 0);
      }
    }
    // offsets out of order: every group of the call
    GroupCatalogue back = cat;
    std::swap(back.offsets[4], back.offsets[5]);
    grid.radialProfiles(&d, back, centres, cuts[0], RADIAL_MASS, G, S, &bulk);
    for (size_t g = 0; g < G.size(); g++) CHECK(std::memcmp(&G[g], &zero, sizeof zero) == 0 && S[g * 3 + 2].enclosed_count == 0);
    // the error paths
    bool refused = false;
    try { grid.radialProfiles(nullptr, cat, centres, cuts[0], RADIAL_MASS, G, S); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    refused = false;
    GroupCatalogue torn = cat;
    torn.n_groups++;
    try { grid.radialProfiles(&d, torn, centres, cuts[0], RADIAL_MASS, G, S); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    refused = false;
    try { grid.radialProfiles(&d, cat, std::vector<double>(5, 0.0), cuts[0], RADIAL_MASS, G, S); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    for (const std::vector<double>& wrong : {std::vector<double>{0.5, 0.25}, std::vector<double>{0.0, 0.5}, std::vector<double>{0.5, 1.5},
                                             std::vector<double>{}, std::vector<double>(17, 0.5)}) {
      refused = false;
      try { grid.radialProfiles(&d, cat, centres, wrong, RADIAL_MASS, G, S); } catch (const ValidationException&) { refused = true; }
      CHECK(refused);
    }
    refused = false;
    try { grid.radialProfiles(&d, cat, centres, cuts[0], 3, G, S); } catch (const ValidationException&) { refused = true; }
    CHECK(refused);
    GroupCatalogue none;
    none.offsets.push_back(0);
    grid.radialProfiles(&d, none, std::vector<double>(), cuts[0], RADIAL_MASS, G, S);
    CHECK(G.empty() && S.empty());
    ParticleDataManager::freeDevice(d); ParticleDataManager::freeHost(h);
  }
  {  // a uniform box: the Python API computes the same bytes
    const size_t n = 2000;
    ParticleData d, h;
    ParticleDataManager::allocateDevice(d, n);
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
    GroupCatalogue c;
    grid.findGroups(0.6f, 1, c);
    std::vector<GroupProperties> props;
    grid.groupProperties(&d, c, props);
    std::vector<double> centres, bulk;
    for (const GroupProperties& o : props)
      for (int a = 0; a < 3; a++) { centres.push_back(o.com[a]); bulk.push_back(o.vel[a]); }
    const std::vector<double> cuts = {0.25, 0.5, 0.75, 1.0};
    std::vector<RadialGroup> G, G2;
    std::vector<RadialShell> S, S2;
    grid.radialProfiles(&d, c, centres, cuts, RADIAL_MASS, G, S, &bulk);
    grid.radialProfiles(&d, c, centres, cuts, RADIAL_MASS, G2, S2, &bulk);
    CHECK(G.size() == c.n_groups && !G.empty() && std::memcmp(G.data(), G2.data(), G.size() * sizeof(RadialGroup)) == 0 &&
          std::memcmp(S.data(), S2.data(), S.size() * sizeof(RadialShell)) == 0);
    size_t members = 0;
    for (size_t g = 0; g < G.size() && G.size() == props.size(); g++) {
      CHECK(G[g].status == 0 && G[g].n == props[g].n && S[g * 4 + 3].enclosed_count == G[g].n);
      CHECK(std::fabs(G[g].mass - props[g].mass) <= 1e-12 * props[g].mass && std::fabs(G[g].r_max - props[g].r_max) <= 1e-6 * props[g].r_max + 1e-30);
      members += (size_t)G[g].n;
    }
    CHECK(members == n);
    unsigned long long sum = 0;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(G.data());
    for (size_t k = 0; k < G.size() * sizeof(RadialGroup) / 8; k++) sum = sum * 1099511628211ULL + words[k];
    words = reinterpret_cast<const unsigned long long*>(S.data());
    for (size_t k = 0; k < S.size() * sizeof(RadialShell) / 8; k++) sum = sum * 1099511628211ULL + words[k];
    std::printf("radial profile uniform %zu %016llx\n", G.size(), sum);
    ParticleDataManager::freeDevice(d); ParticleDataManager::freeHost(h);
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail;
}
