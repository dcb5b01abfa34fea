// facade_device.cpp -- the symbols the reference's src/cuda/*.cu provide, implemented by
// forwarding to the C ABI (include/nbody_hip.h).  No arithmetic here except the host-side
// initialisers (which the reference also runs on the host, particle_init.cu:286-376).
#include <cmath>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <typeinfo>
#include <unordered_map>

#include "nbody_facade.hpp"
#include "nbody_hip.h"
#include "nbody_hip_diag.h"
#include "nbody_hip_events.h"
#include "nbody_hip_groups.h"
#include "nbody_hip_group_props.h"
#include "nbody_hip_radial.h"
#include "nbody_hip_hop.h"
#include "nbody_hip_neighbours.h"
#include "nbody_hip_mergers.h"
#include "nbody_hip_outcomes.h"
#include "nbody_hip_hierarchy.h"
#include "nbody_hip_comm.h"

namespace nbody {

namespace {

// Status -> exception, mirroring the reference's conventions (error_handling.hpp:29-136).
void check(int rc, const char* file, int line) {
  if (rc == NBODY_HIP_OK) return;
  const char* msg = nbody_hip_last_error();
  switch (rc) {
    case NBODY_HIP_ERR_VALIDATION: throw ValidationException(msg);
    case NBODY_HIP_ERR_RESOURCE:
      if (std::strstr(msg, "grid too large")) throw std::runtime_error(msg);  // force_spatial_hash.cu:252-254
      throw ResourceException(msg, 0, 0);
    default: throw CudaException(msg, file, line);
  }
}
#define NBODY_CHECK(call) check((call), __FILE__, __LINE__)

nbody_particle_data* raw(ParticleData* p) { return reinterpret_cast<nbody_particle_data*>(p); }
const nbody_particle_data* raw(const ParticleData* p) { return reinterpret_cast<const nbody_particle_data*>(p); }
static_assert(sizeof(ParticleData) == sizeof(nbody_particle_data), "ParticleData layout");
static_assert(sizeof(OctreeNode) == 76, "OctreeNode layout");
// the reference's sizes (measured with its own headers; oracle/layout_probe.cpp compares every
// member offset of both header sets)
static_assert(sizeof(BarnesHutTree) == 96, "BarnesHutTree must keep the reference's layout");
static_assert(sizeof(SpatialHashGrid) == 96, "SpatialHashGrid must keep the reference's layout");
static_assert(sizeof(Integrator) == 24, "Integrator must keep the reference's layout");

}  // namespace

nbody_hip_ctx* facadeContext() {
  static nbody_hip_ctx* ctx = nullptr;
  static std::once_flag once;
  std::call_once(once, [] { NBODY_CHECK(nbody_hip_ctx_create(&ctx, 0, nullptr)); });
  return ctx;
}

// ---- ParticleDataManager (particle_init.cu:143-283) ------------------------------------------
void ParticleDataManager::allocateDevice(ParticleData& data, size_t count) {
  NBODY_CHECK(nbody_hip_particles_alloc(raw(&data), count));
}
void ParticleDataManager::freeDevice(ParticleData& data) { NBODY_CHECK(nbody_hip_particles_free(raw(&data))); }

void ParticleDataManager::allocateHost(ParticleData& data, size_t count) {
  float** f = &data.pos_x;
  for (int k = 0; k < 13; k++) f[k] = new float[count]();
  data.count = count;
}
void ParticleDataManager::freeHost(ParticleData& data) {
  float** f = &data.pos_x;
  for (int k = 0; k < 13; k++) { delete[] f[k]; f[k] = nullptr; }
  data.count = 0;
}
void ParticleDataManager::copyToDevice(ParticleData& d_data, const ParticleData& h_data) {
  NBODY_CHECK(nbody_hip_ctx_synchronize(facadeContext()));
  NBODY_CHECK(nbody_hip_particles_upload(raw(&d_data), raw(&h_data)));
}
void ParticleDataManager::copyToHost(ParticleData& h_data, const ParticleData& d_data) {
  NBODY_CHECK(nbody_hip_ctx_synchronize(facadeContext()));
  NBODY_CHECK(nbody_hip_particles_download(raw(&h_data), raw(&d_data)));
}
void ParticleDataManager::copyPositionsToHost(float* x, float* y, float* z, const ParticleData& d) {
  ParticleData h, dd = d;
  h.count = d.count;
  // download() copies ten arrays; positions only need three -> temporary host arrays for the rest
  std::vector<float> scratch(d.count * 7);
  h.pos_x = x; h.pos_y = y; h.pos_z = z;
  float* s = scratch.data();
  h.vel_x = s; h.vel_y = s + d.count; h.vel_z = s + 2 * d.count; h.acc_x = s + 3 * d.count;
  h.acc_y = s + 4 * d.count; h.acc_z = s + 5 * d.count; h.mass = s + 6 * d.count;
  copyToHost(h, dd);
}
void ParticleDataManager::copyPositionsToDevice(ParticleData& d, const float* x, const float* y, const float* z) {
  ParticleData h;
  allocateHost(h, d.count);
  copyToHost(h, d);
  std::copy(x, x + d.count, h.pos_x);
  std::copy(y, y + d.count, h.pos_y);
  std::copy(z, z + d.count, h.pos_z);
  copyToDevice(d, h);
  freeHost(h);
}

// ---- ParticleInitializer: the three host recipes of particle_init.cu:286-376 ------------------
std::mt19937 ParticleInitializer::createRNG(unsigned int seed) { return std::mt19937(seed); }

void ParticleInitializer::zeroVelocities(ParticleData& h) {
  std::fill_n(h.vel_x, h.count, 0.0f); std::fill_n(h.vel_y, h.count, 0.0f); std::fill_n(h.vel_z, h.count, 0.0f);
}
void ParticleInitializer::zeroAccelerations(ParticleData& h) {
  float* six[] = {h.acc_x, h.acc_y, h.acc_z, h.acc_old_x, h.acc_old_y, h.acc_old_z};
  for (float* a : six) std::fill_n(a, h.count, 0.0f);
}

void ParticleInitializer::initUniform(ParticleData& h, const UniformDistParams& p, unsigned int seed) {
  std::mt19937 rng = createRNG(seed);
  std::uniform_real_distribution<float> ux(p.min_bounds.x, p.max_bounds.x), uy(p.min_bounds.y, p.max_bounds.y),
      uz(p.min_bounds.z, p.max_bounds.z), um(p.min_mass, p.max_mass);
  for (size_t i = 0; i < h.count; i++) {  // draw order per body: x, y, z, mass
    h.pos_x[i] = ux(rng); h.pos_y[i] = uy(rng); h.pos_z[i] = uz(rng);
    h.mass[i] = um(rng);
  }
  zeroVelocities(h);
  zeroAccelerations(h);
}

void ParticleInitializer::initSpherical(ParticleData& h, const SphericalDistParams& p, unsigned int seed) {
  std::mt19937 rng = createRNG(seed);
  std::uniform_real_distribution<float> u01(0.0f, 1.0f), um(p.min_mass, p.max_mass);
  for (size_t i = 0; i < h.count; i++) {  // draw order per body: radius, azimuth, polar, mass
    const float r = std::cbrt(u01(rng)) * p.radius;        // uniform in volume
    const float theta = u01(rng) * 2.0f * 3.14159265f;
    const float phi = std::acos(2.0f * u01(rng) - 1.0f);
    h.pos_x[i] = p.center.x + r * std::sin(phi) * std::cos(theta);
    h.pos_y[i] = p.center.y + r * std::sin(phi) * std::sin(theta);
    h.pos_z[i] = p.center.z + r * std::cos(phi);
    h.mass[i] = um(rng);
  }
  zeroVelocities(h);
  zeroAccelerations(h);
}

void ParticleInitializer::initDisk(ParticleData& h, const DiskDistParams& p, unsigned int seed) {
  std::mt19937 rng = createRNG(seed);
  std::uniform_real_distribution<float> u01(0.0f, 1.0f), um(p.min_mass, p.max_mass);
  for (size_t i = 0; i < h.count; i++) {  // draw order per body: radius, azimuth, height, mass
    const float r = std::sqrt(u01(rng)) * p.radius;
    const float theta = u01(rng) * 2.0f * 3.14159265f;
    const float z = (u01(rng) - 0.5f) * p.thickness;
    h.pos_x[i] = p.center.x + r * std::cos(theta);
    h.pos_y[i] = p.center.y + r * std::sin(theta);
    h.pos_z[i] = p.center.z + z;
    const float v = p.rotation_speed * std::sqrt(r);       // tangential
    h.vel_x[i] = -v * std::sin(theta);
    h.vel_y[i] = v * std::cos(theta);
    h.vel_z[i] = 0.0f;
    h.mass[i] = um(rng);
  }
  zeroAccelerations(h);
}

// ---- Direct ------------------------------------------------------------------------------------
void launchDirectForceKernel(ParticleData* d, float G, float eps2, int block_size) {
  NBODY_CHECK(nbody_hip_direct_forces(facadeContext(), raw(d), G, eps2, block_size));
}
DirectForceCalculator::DirectForceCalculator(int block_size) : block_size_(block_size) {}
void DirectForceCalculator::computeForces(ParticleData* d) {
  launchDirectForceKernel(d, G_, softening_eps2_, block_size_);
}

// ---- Direct, shared by the GPUs of one node (MI355X-native addition) -------------------------------
ShardedDirectCalculator::ShardedDirectCalculator(std::vector<int> devices, bool rccl)
    : devices_(std::move(devices)), rccl_(rccl) {
  if (devices_.empty()) {
    const int n = nbody_hip_device_count();
    for (int k = 0; k < n; k++) devices_.push_back(k);
  }
  NBODY_CHECK(nbody_hip_comm_init_all(static_cast<int>(devices_.size()), devices_.data(),
                                      rccl_ ? NBODY_HIP_TRANSPORT_RCCL : NBODY_HIP_TRANSPORT_P2P, &comm_));
}
ShardedDirectCalculator::~ShardedDirectCalculator() {
  nbody_hip_sharded_direct_destroy(sys_);
  nbody_hip_comm_destroy(comm_);
}
void ShardedDirectCalculator::computeForces(ParticleData* d) {
  const float eps = softening_eps_;  // the library squares it in fp32 exactly as setSofteningParameter does
  // sized from the count seen (like the tree / grid calculators, force_barnes_hut.cu:527-529); rebuilt when the
  // body count or a parameter changes (the setters are plain stores read at the next call)
  if (!sys_ || count_ != d->count || built_G_ != G_ || built_eps_ != eps) {
    nbody_hip_sharded_direct_destroy(sys_);
    sys_ = nullptr;
    NBODY_CHECK(nbody_hip_sharded_direct_create(comm_, d->count, G_, eps, &sys_));
    count_ = d->count;
    built_G_ = G_;
    built_eps_ = eps;
  }
  NBODY_CHECK(nbody_hip_sharded_direct_compute_forces(sys_, raw(d)));
}

Vec3 computeGravitationalForceCPU(const Vec3& p1, const Vec3& p2, float /*m1*/, float m2, float G, float eps) {
  // host helper of the reference (force_direct.cu:109-117): acceleration of body 1 due to body 2
  const Vec3 r = p2 - p1;
  const float inv = 1.0f / std::sqrt(r.length2() + eps * eps);
  return r * (G * m2 * (inv * inv * inv));
}

// ---- Barnes-Hut -----------------------------------------------------------------------------
BarnesHutTree::BarnesHutTree(size_t max_particles) : max_particles_(max_particles) {
  nbody_hip_tree* t = nullptr;
  NBODY_CHECK(nbody_hip_tree_create(facadeContext(), max_particles, &t));
  d_nodes_ = reinterpret_cast<OctreeNode*>(t);
}
BarnesHutTree::~BarnesHutTree() { nbody_hip_tree_destroy(handle()); }
void BarnesHutTree::driftBuild(ParticleData* d, float dt) {
  NBODY_CHECK(nbody_hip_tree_drift_build(handle(), raw(d), dt));
  int level_base[NBODY_HIP_TREE_LEVELS];
  NBODY_CHECK(nbody_hip_tree_stats(handle(), &node_count_, nullptr, nullptr, level_base));
  max_nodes_ = static_cast<size_t>(node_count_);
  max_depth_ = 0;  // the deepest level that holds nodes (the reference reports the depth its insertion reached)
  for (int l = 1; l < NBODY_HIP_TREE_LEVELS; l++) if (level_base[l] > level_base[l - 1]) max_depth_ = l - 1;
}
void BarnesHutTree::build(const ParticleData* d) {
  NBODY_CHECK(nbody_hip_tree_build(handle(), raw(d)));
  int level_base[NBODY_HIP_TREE_LEVELS];
  NBODY_CHECK(nbody_hip_tree_stats(handle(), &node_count_, nullptr, nullptr, level_base));
  max_nodes_ = static_cast<size_t>(node_count_);
  max_depth_ = 0;  // the deepest level that holds nodes (the reference reports the depth its insertion reached)
  for (int l = 1; l < NBODY_HIP_TREE_LEVELS; l++) if (level_base[l] > level_base[l - 1]) max_depth_ = l - 1;
}
void BarnesHutTree::computeForces(ParticleData* d, float theta, float G, float eps) {
  NBODY_CHECK(nbody_hip_tree_compute_forces(handle(), raw(d), theta, G, eps));
}
void BarnesHutTree::computeField(const float4* pts, size_t n, float theta, float G, float eps, float4* out) {
  NBODY_CHECK(nbody_hip_tree_field(handle(), reinterpret_cast<const nbody_float4*>(pts), n, theta, G, eps,
                                   reinterpret_cast<nbody_float4*>(out)));
}
double BarnesHutTree::computePotential(const ParticleData* d, float theta, float G, float eps, float* d_phi) {
  double pe = 0.0;
  NBODY_CHECK(nbody_hip_tree_potential(handle(), raw(d), theta, G, eps, d_phi, &pe));
  return pe;
}
void BarnesHutTree::copyNodesToHost() {
  h_nodes_.resize(static_cast<size_t>(node_count_));
  NBODY_CHECK(nbody_hip_tree_copy_nodes(handle(), h_nodes_.data(), node_count_, nullptr));
}
void BarnesHutTree::setMultipoleOrder(int order) { NBODY_CHECK(nbody_hip_tree_set_multipole_order(handle(), order)); }
int BarnesHutTree::getMultipoleOrder() const {
  int order = 1;
  NBODY_CHECK(nbody_hip_tree_get_multipole_order(handle(), &order));
  return order;
}
std::vector<float> BarnesHutTree::copyMomentsToHost() const {
  int nodes = 0;
  NBODY_CHECK(nbody_hip_tree_stats(handle(), &nodes, nullptr, nullptr, nullptr));
  std::vector<float> out(6 * static_cast<size_t>(nodes));
  NBODY_CHECK(nbody_hip_tree_copy_moments(handle(), out.data(), nodes));
  return out;
}
bool BarnesHutTree::verifyTreeStructure() const { return node_count_ > 0; }
bool BarnesHutTree::verifyMassConservation(const ParticleData* h) const {
  float total = 0.0f, root_mass = 0.0f;
  for (size_t i = 0; i < h->count; i++) total += h->mass[i];
  if (nbody_hip_tree_stats(handle(), nullptr, &root_mass, nullptr, nullptr) != NBODY_HIP_OK) return false;
  return std::abs(total - root_mass) < 0.001f * total;
}

// The multipole order of a calculator lives outside the object: BarnesHutCalculator keeps the reference's layout
// (oracle/layout_probe.cpp), and its tail padding may hold a subclass's members.  Calculators at order 1 have no entry.
namespace {
std::mutex g_order_mutex;
std::unordered_map<const BarnesHutCalculator*, int>& orderTable() {
  static std::unordered_map<const BarnesHutCalculator*, int> table;
  return table;
}
int calculatorOrder(const BarnesHutCalculator* c) {
  std::lock_guard<std::mutex> lock(g_order_mutex);
  const auto it = orderTable().find(c);
  return it == orderTable().end() ? 1 : it->second;
}
// the calculator's tree, created at the first use with the calculator's multipole order
BarnesHutTree& calculatorTree(std::unique_ptr<BarnesHutTree>& tree, const BarnesHutCalculator* c, size_t count) {
  if (!tree) {
    tree = std::make_unique<BarnesHutTree>(count);
    if (const int order = calculatorOrder(c); order != 1) tree->setMultipoleOrder(order);
  }
  return *tree;
}
}  // namespace

BarnesHutCalculator::BarnesHutCalculator(float theta) : theta_(theta) {}
BarnesHutCalculator::~BarnesHutCalculator() {
  std::lock_guard<std::mutex> lock(g_order_mutex);
  orderTable().erase(this);
}
void BarnesHutCalculator::setMultipoleOrder(int order) {
  if (order != 1 && order != 2) throw ValidationException("multipole order must be 1 or 2");
  if (tree_) tree_->setMultipoleOrder(order);
  std::lock_guard<std::mutex> lock(g_order_mutex);
  if (order == 1) orderTable().erase(this); else orderTable()[this] = order;
}
int BarnesHutCalculator::getMultipoleOrder() const { return calculatorOrder(this); }
void BarnesHutCalculator::computeForces(ParticleData* d) {
  calculatorTree(tree_, this, d->count);
  tree_->build(d);
  tree_->computeForces(d, theta_, G_, softening_eps_);
}

// ---- Spatial hash ----------------------------------------------------------------------------
SpatialHashGrid::SpatialHashGrid(size_t max_particles, float cell_size)
    : max_particles_(max_particles), cell_size_(cell_size) {
  nbody_hip_grid* g = nullptr;
  NBODY_CHECK(nbody_hip_grid_create(facadeContext(), max_particles, cell_size, &g));
  d_cell_start_ = reinterpret_cast<int*>(g);
}
SpatialHashGrid::~SpatialHashGrid() { nbody_hip_grid_destroy(handle()); }
void SpatialHashGrid::driftBuild(ParticleData* d, float dt) {
  NBODY_CHECK(nbody_hip_grid_drift_build(handle(), raw(d), dt));
  int dims[3];
  float lo[3], hi[3];
  NBODY_CHECK(nbody_hip_grid_info(handle(), dims, &total_cells_, lo, hi));
  grid_dims_ = make_int3(dims[0], dims[1], dims[2]);
  bbox_min_ = Vec3(lo[0], lo[1], lo[2]);
  bbox_max_ = Vec3(hi[0], hi[1], hi[2]);
}
void SpatialHashGrid::build(const ParticleData* d) {
  NBODY_CHECK(nbody_hip_grid_build(handle(), raw(d)));
  int dims[3];
  float lo[3], hi[3];
  NBODY_CHECK(nbody_hip_grid_info(handle(), dims, &total_cells_, lo, hi));
  grid_dims_ = make_int3(dims[0], dims[1], dims[2]);
  bbox_min_ = Vec3(lo[0], lo[1], lo[2]);
  bbox_max_ = Vec3(hi[0], hi[1], hi[2]);
}
void SpatialHashGrid::computeForces(ParticleData* d, float cutoff, float G, float eps) {
  NBODY_CHECK(nbody_hip_grid_compute_forces(handle(), raw(d), cutoff, G, eps));
}
void SpatialHashGrid::computeField(const float4* pts, size_t n, float cutoff, float G, float eps, float4* out) {
  NBODY_CHECK(nbody_hip_grid_field(handle(), reinterpret_cast<const nbody_float4*>(pts), n, cutoff, G, eps,
                                   reinterpret_cast<nbody_float4*>(out)));
}
void SpatialHashGrid::findGroups(float linking_length, int min_members, GroupCatalogue& out) {
  size_t built = 0;
  NBODY_CHECK(nbody_hip_grid_count(handle(), &built));
  // device ints inside a ParticleData block of built + 1 floats per array: labels, offsets, members
  ParticleData dev, host;
  ParticleDataManager::allocateDevice(dev, built + 1);
  ParticleDataManager::allocateHost(host, built + 1);
  try {
    long long counts[2] = {0, 0};
    NBODY_CHECK(nbody_hip_grid_groups(handle(), linking_length, min_members, reinterpret_cast<int*>(dev.pos_x), counts));
    NBODY_CHECK(nbody_hip_grid_groups_copy(handle(), reinterpret_cast<int*>(dev.pos_y), reinterpret_cast<int*>(dev.pos_z)));
    ParticleDataManager::copyToHost(host, dev);
    const size_t groups = static_cast<size_t>(counts[0]), members = static_cast<size_t>(counts[1]);
    out.n_groups = groups;
    out.labels.resize(built);
    out.offsets.resize(groups + 1);
    out.members.resize(members);
    std::memcpy(out.labels.data(), host.pos_x, built * sizeof(int));
    std::memcpy(out.offsets.data(), host.pos_y, (groups + 1) * sizeof(int));
    if (members) std::memcpy(out.members.data(), host.pos_z, members * sizeof(int));
  } catch (...) {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
    throw;
  }
  ParticleDataManager::freeDevice(dev);
  ParticleDataManager::freeHost(host);
}
void SpatialHashGrid::findNeighbours(int k, NeighbourLists& out) {
  size_t built = 0;
  NBODY_CHECK(nbody_hip_grid_count(handle(), &built));
  // device arrays inside a ParticleData block: index, dist2 (built * k words each), rho (built doubles), status
  // (a k out of range is the library's to refuse: the block only needs a size)
  const size_t kk = (size_t)(k < 2 ? 2 : k > NBODY_HIP_NEIGHBOURS_MAX_K ? NBODY_HIP_NEIGHBOURS_MAX_K : k);
  const size_t words = built * kk + 2;
  ParticleData dev, host;
  ParticleDataManager::allocateDevice(dev, words);
  ParticleDataManager::allocateHost(host, words);
  try {
    NBODY_CHECK(nbody_hip_grid_neighbours(handle(), k, 0, reinterpret_cast<int*>(dev.pos_x), dev.pos_y,
                                          reinterpret_cast<double*>(dev.pos_z), reinterpret_cast<int*>(dev.vel_x)));
    ParticleDataManager::copyToHost(host, dev);
    out.k = k;
    out.index.resize(built * (size_t)k);
    out.dist2.resize(built * (size_t)k);
    out.rho.resize(built);
    out.status.resize(built);
    if (built) {
      std::memcpy(out.index.data(), host.pos_x, built * (size_t)k * sizeof(int));
      std::memcpy(out.dist2.data(), host.pos_y, built * (size_t)k * sizeof(float));
      std::memcpy(out.rho.data(), host.pos_z, built * sizeof(double));
      std::memcpy(out.status.data(), host.vel_x, built * sizeof(int));
    }
  } catch (...) {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
    throw;
  }
  ParticleDataManager::freeDevice(dev);
  ParticleDataManager::freeHost(host);
}
void SpatialHashGrid::hopGroups(int k, const HopParameters& hp, HopCatalogue& out, NeighbourLists* neighbours) {
  size_t built = 0;
  NBODY_CHECK(nbody_hip_grid_count(handle(), &built));
  // device arrays inside a ParticleData block, as in findNeighbours: index, dist2, rho, status; then labels, peak,
  // offsets (built + 1 ints), members, group_peak
  const size_t kk = (size_t)(k < 2 ? 2 : k > NBODY_HIP_NEIGHBOURS_MAX_K ? NBODY_HIP_NEIGHBOURS_MAX_K : k);
  const size_t words = built * kk + 2;
  nbody_hip_hop_params_t p;
  p.n_hop = hp.n_hop == 0 ? k : hp.n_hop;
  p.n_merge = hp.n_merge;
  p.min_members = hp.min_members;
  p.reserved = 0;
  p.delta_outer = hp.delta_outer;
  p.delta_saddle = hp.delta_saddle < 0.0 ? 2.5 * hp.delta_outer : hp.delta_saddle;
  p.delta_peak = hp.delta_peak < 0.0 ? 3.0 * hp.delta_outer : hp.delta_peak;
  ParticleData dev, host;
  ParticleDataManager::allocateDevice(dev, words);
  ParticleDataManager::allocateHost(host, words);
  try {
    int* const index = reinterpret_cast<int*>(dev.pos_x);
    double* const rho = reinterpret_cast<double*>(dev.pos_z);
    NBODY_CHECK(nbody_hip_grid_neighbours(handle(), k, 0, index, dev.pos_y, rho, reinterpret_cast<int*>(dev.vel_x)));
    long long counts[5] = {0, 0, 0, 0, 0};
    NBODY_CHECK(nbody_hip_hop_groups(facadeContext(), (int)built, k, index, rho, &p, reinterpret_cast<int*>(dev.vel_y),
                                     reinterpret_cast<int*>(dev.vel_z), counts));
    NBODY_CHECK(nbody_hip_hop_groups_copy(facadeContext(), reinterpret_cast<int*>(dev.acc_x), reinterpret_cast<int*>(dev.acc_y),
                                          reinterpret_cast<int*>(dev.acc_z)));
    ParticleDataManager::copyToHost(host, dev);
    const size_t groups = static_cast<size_t>(counts[0]), members = static_cast<size_t>(counts[1]);
    out.groups.n_groups = groups;
    out.groups.labels.resize(built);
    out.peak.resize(built);
    out.groups.offsets.resize(groups + 1);
    out.groups.members.resize(members);
    out.group_peak.resize(groups);
    out.n_peaks = counts[2];
    out.rounds = counts[3];
    out.status = (int)counts[4];
    std::memcpy(out.groups.labels.data(), host.vel_y, built * sizeof(int));
    std::memcpy(out.peak.data(), host.vel_z, built * sizeof(int));
    std::memcpy(out.groups.offsets.data(), host.acc_x, (groups + 1) * sizeof(int));
    if (members) std::memcpy(out.groups.members.data(), host.acc_y, members * sizeof(int));
    if (groups) std::memcpy(out.group_peak.data(), host.acc_z, groups * sizeof(int));
    if (neighbours) {
      neighbours->k = k;
      neighbours->index.resize(built * (size_t)k);
      neighbours->dist2.resize(built * (size_t)k);
      neighbours->rho.resize(built);
      neighbours->status.resize(built);
      std::memcpy(neighbours->index.data(), host.pos_x, built * (size_t)k * sizeof(int));
      std::memcpy(neighbours->dist2.data(), host.pos_y, built * (size_t)k * sizeof(float));
      std::memcpy(neighbours->rho.data(), host.pos_z, built * sizeof(double));
      std::memcpy(neighbours->status.data(), host.vel_x, built * sizeof(int));
    }
  } catch (...) {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
    throw;
  }
  ParticleDataManager::freeDevice(dev);
  ParticleDataManager::freeHost(host);
}
void SpatialHashGrid::groupProperties(const ParticleData* d, const GroupCatalogue& c, std::vector<GroupProperties>& out,
                                      const float* d_phi) {
  static_assert(sizeof(GroupProperties) == 48 * sizeof(float) && sizeof(GroupProperties) == sizeof(nbody_hip_group_props) &&
                    offsetof(GroupProperties, inertia) == offsetof(nbody_hip_group_props, inertia) &&
                    offsetof(GroupProperties, phi_min) == offsetof(nbody_hip_group_props, phi_min) &&
                    offsetof(GroupProperties, n) == offsetof(nbody_hip_group_props, n) &&
                    offsetof(GroupProperties, status) == offsetof(nbody_hip_group_props, status),
                "GroupProperties restates nbody_hip_group_props (192 bytes)");
  if (!d) throw ValidationException("SpatialHashGrid::groupProperties: null particle data");
  if (c.offsets.size() != c.n_groups + 1) throw ValidationException("SpatialHashGrid::groupProperties: the catalogue needs n_groups + 1 offsets");
  out.assign(c.n_groups, GroupProperties{});
  if (c.n_groups == 0) return;
  // device memory inside a ParticleData block: the structs (48 floats a group) in pos_x, offsets in pos_y, members in pos_z
  const size_t floats = std::max(std::max(c.n_groups * 48, c.offsets.size()), std::max(c.members.size(), (size_t)1));
  ParticleData dev, host;
  ParticleDataManager::allocateDevice(dev, floats);
  ParticleDataManager::allocateHost(host, floats);
  try {
    std::memcpy(host.pos_y, c.offsets.data(), c.offsets.size() * sizeof(int));
    if (!c.members.empty()) std::memcpy(host.pos_z, c.members.data(), c.members.size() * sizeof(int));
    ParticleDataManager::copyToDevice(dev, host);
    NBODY_CHECK(nbody_hip_groups_properties(facadeContext(), raw(d), reinterpret_cast<const int*>(dev.pos_y),
                                            c.members.empty() ? nullptr : reinterpret_cast<const int*>(dev.pos_z),
                                            (long long)c.n_groups, (long long)c.members.size(), d_phi,
                                            reinterpret_cast<nbody_hip_group_props*>(dev.pos_x)));
    ParticleDataManager::copyToHost(host, dev);
    std::memcpy(out.data(), host.pos_x, c.n_groups * sizeof(GroupProperties));
  } catch (...) {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
    throw;
  }
  ParticleDataManager::freeDevice(dev);
  ParticleDataManager::freeHost(host);
}
void SpatialHashGrid::radialProfiles(const ParticleData* d, const GroupCatalogue& c, const std::vector<double>& centres,
                                     const std::vector<double>& cuts, int mode, std::vector<RadialGroup>& groups,
                                     std::vector<RadialShell>& shells, const std::vector<double>* bulk) {
  static_assert(sizeof(RadialGroup) == sizeof(nbody_hip_radial_group) && sizeof(RadialGroup) == 8 * sizeof(float) &&
                    offsetof(RadialGroup, n) == offsetof(nbody_hip_radial_group, n) &&
                    offsetof(RadialGroup, status) == offsetof(nbody_hip_radial_group, status),
                "RadialGroup restates nbody_hip_radial_group (32 bytes)");
  static_assert(sizeof(RadialShell) == sizeof(nbody_hip_radial_shell) && sizeof(RadialShell) == 16 * sizeof(float) &&
                    offsetof(RadialShell, m_vt2) == offsetof(nbody_hip_radial_shell, m_vt2) &&
                    offsetof(RadialShell, count) == offsetof(nbody_hip_radial_shell, count) &&
                    offsetof(RadialShell, enclosed_count) == offsetof(nbody_hip_radial_shell, enclosed_count),
                "RadialShell restates nbody_hip_radial_shell (64 bytes)");
  static_assert(RADIAL_MASS == NBODY_HIP_RADIAL_MASS && RADIAL_NUMBER == NBODY_HIP_RADIAL_NUMBER &&
                    RADIAL_RADIUS == NBODY_HIP_RADIAL_RADIUS, "RadialMode restates NBODY_HIP_RADIAL_*");
  if (!d) throw ValidationException("SpatialHashGrid::radialProfiles: null particle data");
  if (c.offsets.size() != c.n_groups + 1) throw ValidationException("SpatialHashGrid::radialProfiles: the catalogue needs n_groups + 1 offsets");
  if (centres.size() != 3 * c.n_groups) throw ValidationException("SpatialHashGrid::radialProfiles: centres needs 3 doubles a group");
  if (bulk && bulk->size() != 3 * c.n_groups) throw ValidationException("SpatialHashGrid::radialProfiles: bulk_velocities needs 3 doubles a group");
  if (cuts.empty() || cuts.size() > NBODY_HIP_RADIAL_MAX_CUTS) throw ValidationException("SpatialHashGrid::radialProfiles: 1 .. 16 cuts");
  const size_t rows = c.n_groups * cuts.size();
  groups.assign(c.n_groups, RadialGroup{});
  shells.assign(rows, RadialShell{});
  if (c.n_groups == 0) {  // (the cuts and the mode are still the library's to refuse)
    NBODY_CHECK(nbody_hip_groups_radial_profile(facadeContext(), raw(d), reinterpret_cast<const int*>(c.offsets.data()), nullptr, 0, 0,
                                                nullptr, nullptr, cuts.data(), (int)cuts.size(), mode, nullptr, nullptr, nullptr, nullptr));
    return;
  }
  // device memory inside a ParticleData block: the shell rows (16 floats a row) in pos_x, offsets in pos_y, members in
  // pos_z, the centres (6 floats a group) in vel_x, the bulk velocities in vel_y, the group structs (8 floats) in vel_z
  const size_t floats = std::max(std::max(rows * 16, c.offsets.size()), std::max(c.members.size(), c.n_groups * 8));
  ParticleData dev, host;
  ParticleDataManager::allocateDevice(dev, floats);
  ParticleDataManager::allocateHost(host, floats);
  try {
    std::memcpy(host.pos_y, c.offsets.data(), c.offsets.size() * sizeof(int));
    if (!c.members.empty()) std::memcpy(host.pos_z, c.members.data(), c.members.size() * sizeof(int));
    std::memcpy(host.vel_x, centres.data(), centres.size() * sizeof(double));
    if (bulk) std::memcpy(host.vel_y, bulk->data(), bulk->size() * sizeof(double));
    ParticleDataManager::copyToDevice(dev, host);
    NBODY_CHECK(nbody_hip_groups_radial_profile(
        facadeContext(), raw(d), reinterpret_cast<const int*>(dev.pos_y),
        c.members.empty() ? nullptr : reinterpret_cast<const int*>(dev.pos_z), (long long)c.n_groups,
        (long long)c.members.size(), reinterpret_cast<const double*>(dev.vel_x),
        bulk ? reinterpret_cast<const double*>(dev.vel_y) : nullptr, cuts.data(), (int)cuts.size(), mode,
        reinterpret_cast<nbody_hip_radial_group*>(dev.vel_z), reinterpret_cast<nbody_hip_radial_shell*>(dev.pos_x), nullptr,
        nullptr));
    ParticleDataManager::copyToHost(host, dev);
    std::memcpy(groups.data(), host.vel_z, c.n_groups * sizeof(RadialGroup));
    std::memcpy(shells.data(), host.pos_x, rows * sizeof(RadialShell));
  } catch (...) {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
    throw;
  }
  ParticleDataManager::freeDevice(dev);
  ParticleDataManager::freeHost(host);
}
double SpatialHashGrid::computePotential(const ParticleData* d, float cutoff, float G, float eps, float* d_phi) {
  double pe = 0.0;
  NBODY_CHECK(nbody_hip_grid_potential(handle(), raw(d), cutoff, G, eps, d_phi, &pe));
  return pe;
}
void SpatialHashGrid::copyCellDataToHost(std::vector<int>& cell_start, std::vector<int>& cell_end,
                                         std::vector<int>& particle_cells, std::vector<int>& sorted_indices) {
  size_t built = 0;
  NBODY_CHECK(nbody_hip_grid_count(handle(), &built));
  cell_start.resize(static_cast<size_t>(total_cells_));
  cell_end.resize(static_cast<size_t>(total_cells_));
  particle_cells.resize(built);
  sorted_indices.resize(built);
  NBODY_CHECK(nbody_hip_grid_copy_cell_data(handle(), cell_start.data(), cell_end.data(), particle_cells.data(),
                                            sorted_indices.data()));
}
int3 SpatialHashGrid::getCellIndex(float x, float y, float z, float cell_size) {
  return make_int3(static_cast<int>(std::floor(x / cell_size)), static_cast<int>(std::floor(y / cell_size)),
                   static_cast<int>(std::floor(z / cell_size)));
}
int SpatialHashGrid::hashCell(int3 c, int3 g) {
  const int cx = ((c.x % g.x) + g.x) % g.x, cy = ((c.y % g.y) + g.y) % g.y, cz = ((c.z % g.z) + g.z) % g.z;
  return cx + cy * g.x + cz * g.x * g.y;
}
bool SpatialHashGrid::verifyCellAssignment(const ParticleData* h) const {
  size_t built = 0;
  if (nbody_hip_grid_count(handle(), &built) != NBODY_HIP_OK) return false;
  std::vector<int> pc(built);
  if (nbody_hip_grid_copy_cell_data(handle(), nullptr, nullptr, pc.data(), nullptr) != NBODY_HIP_OK) return false;
  for (size_t i = 0; i < h->count && i < built; i++) {
    int3 c = getCellIndex(h->pos_x[i] - bbox_min_.x, h->pos_y[i] - bbox_min_.y, h->pos_z[i] - bbox_min_.z, cell_size_);
    c.x = std::max(0, std::min(c.x, grid_dims_.x - 1));
    c.y = std::max(0, std::min(c.y, grid_dims_.y - 1));
    c.z = std::max(0, std::min(c.z, grid_dims_.z - 1));
    if (pc[i] != c.x + c.y * grid_dims_.x + c.z * grid_dims_.x * grid_dims_.y) return false;
    const float lo[3] = {bbox_min_.x + c.x * cell_size_, bbox_min_.y + c.y * cell_size_, bbox_min_.z + c.z * cell_size_};
    const float p[3] = {h->pos_x[i], h->pos_y[i], h->pos_z[i]};
    for (int a = 0; a < 3; a++)
      if (p[a] < lo[a] || p[a] > lo[a] + cell_size_) return false;
  }
  return true;
}

SpatialHashCalculator::SpatialHashCalculator(float cell_size, float cutoff_radius)
    : cell_size_(cell_size), cutoff_radius_(cutoff_radius) {}
SpatialHashCalculator::~SpatialHashCalculator() = default;
void SpatialHashCalculator::computeForces(ParticleData* d) {
  if (!grid_) grid_ = std::make_unique<SpatialHashGrid>(d->count, cell_size_);
  grid_->build(d);
  grid_->computeForces(d, cutoff_radius_, G_, softening_eps_);
}

// ---- factory (force_spatial_hash.cu:380-401) -------------------------------------------------
std::unique_ptr<ForceCalculator> createForceCalculator(ForceMethod method, const SimulationConfig& cfg) {
  std::unique_ptr<ForceCalculator> calc;
  switch (method) {
    case ForceMethod::BARNES_HUT: calc = std::make_unique<BarnesHutCalculator>(cfg.barnes_hut_theta); break;
    case ForceMethod::SPATIAL_HASH:
      calc = std::make_unique<SpatialHashCalculator>(cfg.spatial_hash_cell_size, cfg.spatial_hash_cutoff);
      break;
    case ForceMethod::DIRECT_N2:
    default: calc = std::make_unique<DirectForceCalculator>(cfg.cuda_block_size); break;
  }
  calc->setGravitationalConstant(cfg.G);
  calc->setSofteningParameter(cfg.softening);
  return calc;
}

// ---- Integrator (integrator.cu:122-293) --------------------------------------------------------
void launchUpdatePositionsKernel(ParticleData* d, float dt, int) {
  NBODY_CHECK(nbody_hip_update_positions(facadeContext(), raw(d), dt));
}
void launchUpdateVelocitiesKernel(ParticleData* d, float dt, int) {
  NBODY_CHECK(nbody_hip_update_velocities(facadeContext(), raw(d), dt));
}
void launchStoreAccelerationsKernel(ParticleData* d, int) {
  NBODY_CHECK(nbody_hip_store_accelerations(facadeContext(), raw(d)));
}
float launchComputeKineticEnergyKernel(const ParticleData* d, int) {
  float e = 0.f;
  NBODY_CHECK(nbody_hip_kinetic_energy(facadeContext(), raw(d), &e));
  return e;
}
float launchComputePotentialEnergyKernel(const ParticleData* d, float G, float eps, int) {
  float e = 0.f;
  NBODY_CHECK(nbody_hip_potential_energy(facadeContext(), raw(d), G, eps, &e));
  return e;
}

double computePotential(ForceCalculator& fc, ParticleData* d, float* d_phi) {
  // the engine's own calculators exactly (the rule of Integrator::integrate); anything else: the Direct sum
  if (typeid(fc) == typeid(BarnesHutCalculator)) {
    auto& bc = static_cast<BarnesHutCalculator&>(fc);
    calculatorTree(bc.tree_, &bc, d->count);
    bc.tree_->build(d);
    return bc.tree_->computePotential(d, bc.getTheta(), bc.getGravitationalConstant(), bc.getSofteningParameter(), d_phi);
  }
  if (typeid(fc) == typeid(SpatialHashCalculator)) {
    auto& sc = static_cast<SpatialHashCalculator&>(fc);
    if (!sc.grid_) sc.grid_ = std::make_unique<SpatialHashGrid>(d->count, sc.getCellSize());
    sc.grid_->build(d);
    return sc.grid_->computePotential(d, sc.getCutoffRadius(), sc.getGravitationalConstant(), sc.getSofteningParameter(),
                                      d_phi);
  }
  double pe = 0.0;
  NBODY_CHECK(nbody_hip_direct_potential(facadeContext(), raw(d), fc.getGravitationalConstant(),
                                         fc.getSofteningParameter(), d_phi, &pe));
  return pe;
}

void computeField(ForceCalculator& fc, ParticleData* d, const float4* pts, size_t n, float4* out) {
  if (typeid(fc) == typeid(BarnesHutCalculator)) {  // (the rule of computePotential)
    auto& bc = static_cast<BarnesHutCalculator&>(fc);
    calculatorTree(bc.tree_, &bc, d->count);
    bc.tree_->build(d);
    return bc.tree_->computeField(pts, n, bc.getTheta(), bc.getGravitationalConstant(), bc.getSofteningParameter(), out);
  }
  if (typeid(fc) == typeid(SpatialHashCalculator)) {
    auto& sc = static_cast<SpatialHashCalculator&>(fc);
    if (!sc.grid_) sc.grid_ = std::make_unique<SpatialHashGrid>(d->count, sc.getCellSize());
    sc.grid_->build(d);
    return sc.grid_->computeField(pts, n, sc.getCutoffRadius(), sc.getGravitationalConstant(), sc.getSofteningParameter(), out);
  }
  NBODY_CHECK(nbody_hip_direct_field(facadeContext(), raw(d), reinterpret_cast<const nbody_float4*>(pts), n,
                                     fc.getGravitationalConstant(), fc.getSofteningParameter(),
                                     reinterpret_cast<nbody_float4*>(out)));
}

Integrator::Integrator(int block_size) : block_size_(block_size) {}
Integrator::~Integrator() = default;
void Integrator::ensureScratchBuffer(size_t) {}
void Integrator::integrate(ParticleData* d, ForceCalculator* fc, float dt) {
  // The plugin contract is the virtual call (force_calculator.hpp:36-58, integrator.cu:234): the
  // fused drift + force + kick launch sequence is taken only for EXACTLY the engine's own
  // DirectForceCalculator (a subclass overriding computeForces goes through the virtual), and only
  // with a block size computeForces itself would accept (otherwise the call below reports it).
  if (typeid(*fc) == typeid(DirectForceCalculator)) {
    const int bs = static_cast<DirectForceCalculator*>(fc)->getBlockSize();
    if (bs >= 1 && bs <= 1024) {
      const float eps = fc->getSofteningParameter();
      NBODY_CHECK(nbody_hip_integrate_direct(facadeContext(), raw(d), fc->getGravitationalConstant(), eps * eps, dt, 1));
      return;
    }
  }
  // the same rule for the engine's own tree / grid calculators: the drift rides on the packing pass of their
  // build (one pass over the bodies less; same arithmetic, same results); the first step creates the tree / grid
  // through computeForces as ever
  if (typeid(*fc) == typeid(BarnesHutCalculator)) {
    auto* bc = static_cast<BarnesHutCalculator*>(fc);
    if (BarnesHutTree* tree = bc->getTree()) {
      tree->driftBuild(d, dt);
      tree->computeForces(d, bc->getTheta(), bc->getGravitationalConstant(), bc->getSofteningParameter());
      updateVelocities(d, dt);
      return;
    }
  } else if (typeid(*fc) == typeid(SpatialHashCalculator)) {
    auto* sc = static_cast<SpatialHashCalculator*>(fc);
    if (SpatialHashGrid* grid = sc->getGrid()) {
      grid->driftBuild(d, dt);
      grid->computeForces(d, sc->getCutoffRadius(), sc->getGravitationalConstant(), sc->getSofteningParameter());
      updateVelocities(d, dt);
      return;
    }
  }
  NBODY_CHECK(nbody_hip_drift(facadeContext(), raw(d), dt));  // storeOldAccelerations + updatePositions, one pass
  fc->computeForces(d);
  updateVelocities(d, dt);
}
void Integrator::updatePositions(ParticleData* d, float dt) { launchUpdatePositionsKernel(d, dt, block_size_); }
void Integrator::updateVelocities(ParticleData* d, float dt) { launchUpdateVelocitiesKernel(d, dt, block_size_); }
void Integrator::storeOldAccelerations(ParticleData* d) { launchStoreAccelerationsKernel(d, block_size_); }
float Integrator::computeKineticEnergy(const ParticleData* d) { return launchComputeKineticEnergyKernel(d, block_size_); }
float Integrator::computePotentialEnergy(const ParticleData* d, float G, float eps) {
  return launchComputePotentialEnergyKernel(d, G, eps, block_size_);
}
float Integrator::computeTotalEnergy(const ParticleData* d, float G, float eps) {
  return computeKineticEnergy(d) + computePotentialEnergy(d, G, eps);
}

// ---- what the three Hermite classes check and convert alike ------------------------------------
namespace {
// the Hermite scheme is Direct-only, and the particle data is there
void requireDirect(const char* class_name, const char* method, const ForceCalculator* fc, const ParticleData* d) {
  const std::string where = std::string(class_name) + "::" + method;
  if (!fc || typeid(*fc) != typeid(DirectForceCalculator))
    throw ValidationException(where + ": the Hermite scheme is Direct-only -- it needs exactly a DirectForceCalculator (the "
                                      "tree and the grid have no jerk)");
  if (!d) throw ValidationException(where + ": null particle data");
}
void checkBlockParameters(float eta, float eta_start, int max_level) {
  if (!(eta > 0.f) || !std::isfinite(eta)) throw ValidationException("eta must be positive and finite");
  if (!(eta_start > 0.f) || !std::isfinite(eta_start)) throw ValidationException("eta_start must be positive and finite");
  if (max_level < 0 || max_level > 20) throw ValidationException("max_level must be in [0, 20]");
}
BlockHermiteInfo toInfo(const nbody_hip_hermite_block_info_t& in) {
  BlockHermiteInfo out;
  out.block_steps = in.block_steps;
  out.body_steps = in.body_steps;
  for (int k = 0; k < 21; k++) out.level_steps[k] = in.level_steps[k];
  out.floor_hits = in.floor_hits;
  out.narrow_launches = in.narrow_launches;
  out.wide_launches = in.wide_launches;
  out.macro_steps = in.macro_steps;
  out.current_tick = in.current_tick;
  out.last_n_active = in.last_n_active;
  out.max_level = in.max_level;
  out.narrow_below = in.narrow_below;
  return out;
}
}  // namespace

// ---- HermiteIntegrator (no reference counterpart) ---------------------------------------------
HermiteIntegrator::HermiteIntegrator(int block_size) : energies_(block_size) {}
HermiteIntegrator::~HermiteIntegrator() {
  if (handle_) nbody_hip_hermite_destroy(handle_);
}
nbody_hip_hermite* HermiteIntegrator::handleFor(const ParticleData* d, const ForceCalculator* fc, const char* method) {
  requireDirect("HermiteIntegrator", method, fc, d);
  if (handle_ && d->count > capacity_) {
    NBODY_CHECK(nbody_hip_hermite_destroy(handle_));
    handle_ = nullptr;
  }
  if (!handle_) {
    NBODY_CHECK(nbody_hip_hermite_create(facadeContext(), d->count, &handle_));
    capacity_ = d->count;
    NBODY_CHECK(nbody_hip_hermite_set_precision(handle_, static_cast<int>(precision_)));
  }
  return handle_;
}
void HermiteIntegrator::integrate(ParticleData* d, ForceCalculator* fc, float dt) { integrateSteps(d, fc, dt, 1); }
void HermiteIntegrator::integrateSteps(ParticleData* d, ForceCalculator* fc, float dt, int steps) {
  nbody_hip_hermite* h = handleFor(d, fc, "integrate");
  NBODY_CHECK(nbody_hip_hermite_step(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(), dt, steps));
}
void HermiteIntegrator::prime(ParticleData* d, ForceCalculator* fc) {
  nbody_hip_hermite* h = handleFor(d, fc, "prime");
  NBODY_CHECK(nbody_hip_hermite_prime(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter()));
}
void HermiteIntegrator::invalidate() {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_invalidate(handle_));
}
void HermiteIntegrator::getJerk(float4* d_out) const {
  NBODY_CHECK(nbody_hip_hermite_jerk(handle_, reinterpret_cast<nbody_float4*>(d_out)));
}
float HermiteIntegrator::suggestTimeStep(float eta) const {
  float out = 0.f;
  NBODY_CHECK(nbody_hip_hermite_suggest_dt(handle_, eta, &out));
  return out;
}
void HermiteIntegrator::setStatePrecision(StatePrecision p) {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_set_precision(handle_, static_cast<int>(p)));
  precision_ = p;
}
void HermiteIntegrator::setExtendedState(ParticleData* d, ForceCalculator* fc, const double* h_pos, const double* h_vel) {
  NBODY_CHECK(nbody_hip_hermite_set_state_f64(handleFor(d, fc, "setExtendedState"), raw(d), h_pos, h_vel));
}
void HermiteIntegrator::getExtendedState(ParticleData* d, ForceCalculator* fc, double* h_pos, double* h_vel) {
  NBODY_CHECK(nbody_hip_hermite_get_state_f64(handleFor(d, fc, "getExtendedState"), raw(d), h_pos, h_vel));
}

// ---- BlockHermiteIntegrator (no reference counterpart) ----------------------------------------
BlockHermiteIntegrator::BlockHermiteIntegrator(int block_size) : energies_(block_size) {}
BlockHermiteIntegrator::~BlockHermiteIntegrator() {
  if (handle_) nbody_hip_hermite_block_destroy(handle_);
}
nbody_hip_hermite_block* BlockHermiteIntegrator::handleFor(const ParticleData* d, const ForceCalculator* fc,
                                                           const char* method) {
  requireDirect("BlockHermiteIntegrator", method, fc, d);
  if (handle_ && d->count > capacity_) {
    NBODY_CHECK(nbody_hip_hermite_block_destroy(handle_));
    handle_ = nullptr;
  }
  if (!handle_) {
    NBODY_CHECK(nbody_hip_hermite_block_create(facadeContext(), d->count, &handle_));
    capacity_ = d->count;
    NBODY_CHECK(nbody_hip_hermite_block_set_params(handle_, eta_, eta_start_, max_level_));
    NBODY_CHECK(nbody_hip_hermite_block_set_precision(handle_, static_cast<int>(precision_)));
    NBODY_CHECK(nbody_hip_hermite_block_set_scheduling(handle_, static_cast<int>(scheduling_)));
  }
  return handle_;
}
void BlockHermiteIntegrator::setParameters(float eta, float eta_start, int max_level) {
  checkBlockParameters(eta, eta_start, max_level);
  eta_ = eta;
  eta_start_ = eta_start;
  max_level_ = max_level;
  if (handle_) NBODY_CHECK(nbody_hip_hermite_block_set_params(handle_, eta_, eta_start_, max_level_));
}
void BlockHermiteIntegrator::integrate(ParticleData* d, ForceCalculator* fc, float dt_max) {
  nbody_hip_hermite_block* h = handleFor(d, fc, "integrate");
  NBODY_CHECK(nbody_hip_hermite_block_advance(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(),
                                              dt_max, 1));
}
void BlockHermiteIntegrator::advance(ParticleData* d, ForceCalculator* fc, float dt_max, int macro_steps) {
  nbody_hip_hermite_block* h = handleFor(d, fc, "advance");
  NBODY_CHECK(nbody_hip_hermite_block_advance(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(),
                                              dt_max, macro_steps));
}
void BlockHermiteIntegrator::blockStep(ParticleData* d, ForceCalculator* fc, float dt_max, int block_steps) {
  nbody_hip_hermite_block* h = handleFor(d, fc, "blockStep");
  NBODY_CHECK(nbody_hip_hermite_block_step(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(),
                                           dt_max, block_steps));
}
void BlockHermiteIntegrator::prime(ParticleData* d, ForceCalculator* fc, float dt_max) {
  nbody_hip_hermite_block* h = handleFor(d, fc, "prime");
  NBODY_CHECK(nbody_hip_hermite_block_prime(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(),
                                            dt_max));
}
void BlockHermiteIntegrator::invalidate() {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_block_invalidate(handle_));
}
void BlockHermiteIntegrator::getLevels(int* h_out) const {
  NBODY_CHECK(nbody_hip_hermite_block_state(handle_, h_out, nullptr, nullptr, nullptr));
}
void BlockHermiteIntegrator::getState(int* h_levels, unsigned int* h_ticks, float* h_want, float4* h_jerk) const {
  NBODY_CHECK(nbody_hip_hermite_block_state(handle_, h_levels, h_ticks, h_want, reinterpret_cast<nbody_float4*>(h_jerk)));
}
BlockHermiteInfo BlockHermiteIntegrator::info() const {
  nbody_hip_hermite_block_info_t in;
  NBODY_CHECK(nbody_hip_hermite_block_info(handle_, &in));
  return toInfo(in);
}
// The structs of a diagnostics call come back through particle arrays, the device memory the C ABI hands out: pos_x of
// a scratch allocation of 38 floats (152 bytes) per system receives them.
namespace {
struct DiagScratch {
  ParticleData dev, host;
  explicit DiagScratch(size_t n_systems) {
    static_assert(sizeof(SystemDiag) == 38 * sizeof(float) && sizeof(SystemDiag) == sizeof(nbody_hip_system_diag) &&
                      offsetof(SystemDiag, min_i) == offsetof(nbody_hip_system_diag, min_i) &&
                      offsetof(SystemDiag, bind_e) == offsetof(nbody_hip_system_diag, bind_e),
                  "SystemDiag restates nbody_hip_system_diag (152 bytes)");
    ParticleDataManager::allocateDevice(dev, n_systems * 38);
    ParticleDataManager::allocateHost(host, n_systems * 38);
  }
  ~DiagScratch() {
    ParticleDataManager::freeDevice(dev);
    ParticleDataManager::freeHost(host);
  }
  nbody_hip_system_diag* out() { return reinterpret_cast<nbody_hip_system_diag*>(dev.pos_x); }
  void download(SystemDiag* h_out, size_t n_systems) {
    ParticleDataManager::copyToHost(host, dev);
    std::memcpy(h_out, host.pos_x, n_systems * sizeof(SystemDiag));
  }
};
}  // namespace
void BlockHermiteIntegrator::diagnostics(ParticleData* d, ForceCalculator* fc, SystemDiag* h_out) {
  nbody_hip_hermite_block* h = handleFor(d, fc, "diagnostics");
  if (!h_out) throw ValidationException("BlockHermiteIntegrator::diagnostics: null output pointer");
  DiagScratch s(1);
  NBODY_CHECK(nbody_hip_hermite_block_diagnostics(h, raw(d), fc->getGravitationalConstant(), fc->getSofteningParameter(),
                                                  s.out()));
  s.download(h_out, 1);
}
void BlockHermiteIntegrator::setStatePrecision(StatePrecision p) {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_block_set_precision(handle_, static_cast<int>(p)));
  precision_ = p;
}
void BlockHermiteIntegrator::setScheduling(BlockScheduling s) {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_block_set_scheduling(handle_, static_cast<int>(s)));
  scheduling_ = s;
}
void BlockHermiteIntegrator::setExtendedState(ParticleData* d, ForceCalculator* fc, const double* h_pos,
                                              const double* h_vel) {
  NBODY_CHECK(nbody_hip_hermite_block_set_state_f64(handleFor(d, fc, "setExtendedState"), raw(d), h_pos, h_vel));
}
void BlockHermiteIntegrator::getExtendedState(ParticleData* d, ForceCalculator* fc, double* h_pos, double* h_vel) {
  NBODY_CHECK(nbody_hip_hermite_block_get_state_f64(handleFor(d, fc, "getExtendedState"), raw(d), h_pos, h_vel));
}

// ---- BlockHermiteEnsemble (no reference counterpart) -------------------------------------------
BlockHermiteEnsemble::~BlockHermiteEnsemble() {
  if (handle_) nbody_hip_hermite_batch_destroy(handle_);
}
// the handle sized for the layout, with the layout on it (whose rules nbody_hip_hermite_batch_set_layout checks)
nbody_hip_hermite_batch* BlockHermiteEnsemble::handleFor(const char* method) {
  if (offsets_.size() < 2)
    throw ValidationException(std::string("BlockHermiteEnsemble::") + method + ": no layout, call setLayout first");
  size_t total = 1;
  for (size_t o : offsets_) total = o > total ? o : total;
  const size_t systems = offsets_.size() - 1;
  if (handle_ && (total > capacity_ || systems > max_systems_)) {
    NBODY_CHECK(nbody_hip_hermite_batch_destroy(handle_));
    handle_ = nullptr;
  }
  if (!handle_) {
    const size_t ms = systems < total ? systems : total;
    NBODY_CHECK(nbody_hip_hermite_batch_create(facadeContext(), total, ms, &handle_));
    capacity_ = total;
    max_systems_ = ms;
    layout_sent_ = false;
    NBODY_CHECK(nbody_hip_hermite_batch_set_params(handle_, eta_, eta_start_, max_level_));
    NBODY_CHECK(nbody_hip_hermite_batch_set_precision(handle_, static_cast<int>(precision_)));
  }
  if (!layout_sent_) {
    NBODY_CHECK(nbody_hip_hermite_batch_set_layout(handle_, offsets_.data(), systems));
    layout_sent_ = true;
  }
  return handle_;
}
void BlockHermiteEnsemble::setParameters(float eta, float eta_start, int max_level) {
  checkBlockParameters(eta, eta_start, max_level);
  eta_ = eta;
  eta_start_ = eta_start;
  max_level_ = max_level;
  if (handle_) NBODY_CHECK(nbody_hip_hermite_batch_set_params(handle_, eta_, eta_start_, max_level_));
}
void BlockHermiteEnsemble::setStatePrecision(StatePrecision p) {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_batch_set_precision(handle_, static_cast<int>(p)));
  precision_ = p;
}
void BlockHermiteEnsemble::setLayout(const size_t* offsets, size_t n_systems) {
  if (!offsets || n_systems < 1) throw ValidationException("BlockHermiteEnsemble::setLayout: n_systems + 1 >= 2 offsets needed");
  offsets_.assign(offsets, offsets + n_systems + 1);
  layout_sent_ = false;
  handleFor("setLayout");
}
void BlockHermiteEnsemble::prime(ParticleData* d, ForceCalculator* fc, const float* h_dt_max) {
  requireDirect("BlockHermiteEnsemble", "prime", fc, d);
  NBODY_CHECK(nbody_hip_hermite_batch_prime(handleFor("prime"), raw(d), fc->getGravitationalConstant(),
                                            fc->getSofteningParameter(), h_dt_max));
}
void BlockHermiteEnsemble::prime(ParticleData* d, ForceCalculator* fc, float dt_max) {
  const std::vector<float> dt(offsets_.size() > 1 ? offsets_.size() - 1 : 1, dt_max);
  prime(d, fc, dt.data());
}
void BlockHermiteEnsemble::invalidate() {
  if (handle_) NBODY_CHECK(nbody_hip_hermite_batch_invalidate(handle_));
}
void BlockHermiteEnsemble::advance(ParticleData* d, int macro_steps) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::advance: null particle data");
  NBODY_CHECK(nbody_hip_hermite_batch_advance(handle_, raw(d), macro_steps));
}
void BlockHermiteEnsemble::getState(int* h_levels, unsigned int* h_ticks, float* h_want, float4* h_jerk) const {
  NBODY_CHECK(nbody_hip_hermite_batch_state(handle_, h_levels, h_ticks, h_want, reinterpret_cast<nbody_float4*>(h_jerk)));
}
BlockHermiteInfo BlockHermiteEnsemble::info(long long system) const {
  nbody_hip_hermite_block_info_t in;
  NBODY_CHECK(nbody_hip_hermite_batch_info(handle_, system, &in));
  return toInfo(in);
}
void BlockHermiteEnsemble::diagnostics(ParticleData* d, SystemDiag* h_out) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::diagnostics: null particle data");
  if (!h_out) throw ValidationException("BlockHermiteEnsemble::diagnostics: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  DiagScratch s(systems);
  NBODY_CHECK(nbody_hip_hermite_batch_diagnostics(handle_, raw(d), s.out()));
  s.download(h_out, systems);
}
void BlockHermiteEnsemble::setEvents(const float* h_radii, const unsigned long long* h_max_macro_steps, bool track_closest,
                                     bool stop_on_contact) {
  const int flags = (track_closest ? NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST : 0) |
                    (stop_on_contact ? NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT : 0);
  NBODY_CHECK(nbody_hip_hermite_batch_set_events(handleFor("setEvents"), h_radii, h_max_macro_steps, flags));
}
void BlockHermiteEnsemble::events(BatchEvent* h_out) const {
  static_assert(sizeof(BatchEvent) == 64 && sizeof(BatchEvent) == sizeof(nbody_hip_batch_event_t) &&
                offsetof(BatchEvent, macro_steps_done) == offsetof(nbody_hip_batch_event_t, macro_steps_done) &&
                offsetof(BatchEvent, closest_d2) == offsetof(nbody_hip_batch_event_t, closest_d2) &&
                offsetof(BatchEvent, closest_macro) == offsetof(nbody_hip_batch_event_t, closest_macro) &&
                offsetof(BatchEvent, contact_d2) == offsetof(nbody_hip_batch_event_t, contact_d2) &&
                offsetof(BatchEvent, contact_tick) == offsetof(nbody_hip_batch_event_t, contact_tick) &&
                offsetof(BatchEvent, contact_macro) == offsetof(nbody_hip_batch_event_t, contact_macro),
                "BatchEvent is nbody_hip_batch_event_t field for field");
  if (!h_out) throw ValidationException("BlockHermiteEnsemble::events: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  NBODY_CHECK(nbody_hip_hermite_batch_events(handle_, reinterpret_cast<nbody_hip_batch_event_t*>(h_out), systems));
}
size_t BlockHermiteEnsemble::running() const {
  size_t n = 0;
  NBODY_CHECK(nbody_hip_hermite_batch_running(handle_, &n));
  return n;
}
void BlockHermiteEnsemble::setOutcomes(const float* h_escape_radii, bool stop_on_escape) {
  NBODY_CHECK(nbody_hip_batch_outcomes_set(handleFor("setOutcomes"), h_escape_radii,
                                           stop_on_escape ? NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE : 0));
}
void BlockHermiteEnsemble::outcomes(BatchOutcome* h_out) const {
  static_assert(sizeof(BatchOutcome) == 64 && sizeof(BatchOutcome) == sizeof(nbody_hip_batch_outcome_t) &&
                offsetof(BatchOutcome, escaped) == offsetof(nbody_hip_batch_outcome_t, escaped) &&
                offsetof(BatchOutcome, escaper) == offsetof(nbody_hip_batch_outcome_t, escaper) &&
                offsetof(BatchOutcome, macro) == offsetof(nbody_hip_batch_outcome_t, macro) &&
                offsetof(BatchOutcome, r) == offsetof(nbody_hip_batch_outcome_t, r) &&
                offsetof(BatchOutcome, vr) == offsetof(nbody_hip_batch_outcome_t, vr) &&
                offsetof(BatchOutcome, energy) == offsetof(nbody_hip_batch_outcome_t, energy) &&
                offsetof(BatchOutcome, rest_mass) == offsetof(nbody_hip_batch_outcome_t, rest_mass) &&
                offsetof(BatchOutcome, reserved) == offsetof(nbody_hip_batch_outcome_t, reserved) &&
                offsetof(BatchOutcome, reserved2) == offsetof(nbody_hip_batch_outcome_t, reserved2),
                "BatchOutcome is nbody_hip_batch_outcome_t field for field");
  if (!h_out) throw ValidationException("BlockHermiteEnsemble::outcomes: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  NBODY_CHECK(nbody_hip_batch_outcomes_get(handle_, reinterpret_cast<nbody_hip_batch_outcome_t*>(h_out), systems));
}
static_assert(sizeof(BatchHierarchy) == 64 && sizeof(BatchHierarchy) == sizeof(nbody_hip_batch_hierarchy_t) &&
              offsetof(BatchHierarchy, resolved) == offsetof(nbody_hip_batch_hierarchy_t, resolved) &&
              offsetof(BatchHierarchy, top_count) == offsetof(nbody_hip_batch_hierarchy_t, top_count) &&
              offsetof(BatchHierarchy, macro) == offsetof(nbody_hip_batch_hierarchy_t, macro) &&
              offsetof(BatchHierarchy, node_count) == offsetof(nbody_hip_batch_hierarchy_t, node_count) &&
              offsetof(BatchHierarchy, largest) == offsetof(nbody_hip_batch_hierarchy_t, largest) &&
              offsetof(BatchHierarchy, min_sep) == offsetof(nbody_hip_batch_hierarchy_t, min_sep) &&
              offsetof(BatchHierarchy, min_p) == offsetof(nbody_hip_batch_hierarchy_t, min_p) &&
              offsetof(BatchHierarchy, min_q) == offsetof(nbody_hip_batch_hierarchy_t, min_q) &&
              offsetof(BatchHierarchy, reserved) == offsetof(nbody_hip_batch_hierarchy_t, reserved),
              "BatchHierarchy is nbody_hip_batch_hierarchy_t field for field");
static_assert(sizeof(BatchNode) == 64 && sizeof(BatchNode) == sizeof(nbody_hip_batch_node_t) &&
              offsetof(BatchNode, left) == offsetof(nbody_hip_batch_node_t, left) &&
              offsetof(BatchNode, right) == offsetof(nbody_hip_batch_node_t, right) &&
              offsetof(BatchNode, parent) == offsetof(nbody_hip_batch_node_t, parent) &&
              offsetof(BatchNode, bodies) == offsetof(nbody_hip_batch_node_t, bodies) &&
              offsetof(BatchNode, mass) == offsetof(nbody_hip_batch_node_t, mass) &&
              offsetof(BatchNode, a) == offsetof(nbody_hip_batch_node_t, a) &&
              offsetof(BatchNode, e) == offsetof(nbody_hip_batch_node_t, e) &&
              offsetof(BatchNode, r) == offsetof(nbody_hip_batch_node_t, r) &&
              offsetof(BatchNode, energy) == offsetof(nbody_hip_batch_node_t, energy) &&
              offsetof(BatchNode, reserved) == offsetof(nbody_hip_batch_node_t, reserved),
              "BatchNode is nbody_hip_batch_node_t field for field");
void BlockHermiteEnsemble::setHierarchy(const float* h_separation_radii, float isolation, bool stop_on_resolved) {
  NBODY_CHECK(nbody_hip_batch_hierarchy_set(handleFor("setHierarchy"), h_separation_radii, isolation,
                                            stop_on_resolved ? NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED : 0));
}
void BlockHermiteEnsemble::hierarchy(BatchHierarchy* h_records, BatchNode* h_nodes) const {
  if (!h_records) throw ValidationException("BlockHermiteEnsemble::hierarchy: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  const size_t slots = h_nodes && !offsets_.empty() ? 2 * offsets_.back() : 0;
  NBODY_CHECK(nbody_hip_batch_hierarchy_get(handle_, reinterpret_cast<nbody_hip_batch_hierarchy_t*>(h_records), systems,
                                            reinterpret_cast<nbody_hip_batch_node_t*>(h_nodes), slots));
}
void BlockHermiteEnsemble::hierarchySnapshot(ParticleData* d, BatchHierarchy* h_records, BatchNode* h_nodes) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::hierarchySnapshot: null particle data");
  if (!h_records || !h_nodes) throw ValidationException("BlockHermiteEnsemble::hierarchySnapshot: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  const size_t slots = offsets_.empty() ? 0 : 2 * offsets_.back();
  NBODY_CHECK(nbody_hip_batch_hierarchy_snapshot(handle_, raw(d), reinterpret_cast<nbody_hip_batch_hierarchy_t*>(h_records),
                                                 systems, reinterpret_cast<nbody_hip_batch_node_t*>(h_nodes), slots));
}
void BlockHermiteEnsemble::setExtendedState(ParticleData* d, const double* h_pos, const double* h_vel) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::setExtendedState: null particle data");
  NBODY_CHECK(nbody_hip_hermite_batch_set_state_f64(handleFor("setExtendedState"), raw(d), h_pos, h_vel));
}
void BlockHermiteEnsemble::getExtendedState(ParticleData* d, double* h_pos, double* h_vel) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::getExtendedState: null particle data");
  NBODY_CHECK(nbody_hip_hermite_batch_get_state_f64(handleFor("getExtendedState"), raw(d), h_pos, h_vel));
}
static_assert(sizeof(BatchMergerState) == 32 && sizeof(BatchMergerState) == sizeof(nbody_hip_batch_merger_state_t) &&
              offsetof(BatchMergerState, n_live) == offsetof(nbody_hip_batch_merger_state_t, n_live) &&
              offsetof(BatchMergerState, n_mergers) == offsetof(nbody_hip_batch_merger_state_t, n_mergers) &&
              offsetof(BatchMergerState, flags) == offsetof(nbody_hip_batch_merger_state_t, flags) &&
              offsetof(BatchMergerState, reserved) == offsetof(nbody_hip_batch_merger_state_t, reserved),
              "BatchMergerState is nbody_hip_batch_merger_state_t field for field");
static_assert(sizeof(BatchMerger) == 64 && sizeof(BatchMerger) == sizeof(nbody_hip_batch_merger_t) &&
              offsetof(BatchMerger, slot_a) == offsetof(nbody_hip_batch_merger_t, slot_a) &&
              offsetof(BatchMerger, slot_b) == offsetof(nbody_hip_batch_merger_t, slot_b) &&
              offsetof(BatchMerger, id_a) == offsetof(nbody_hip_batch_merger_t, id_a) &&
              offsetof(BatchMerger, id_b) == offsetof(nbody_hip_batch_merger_t, id_b) &&
              offsetof(BatchMerger, moved_from) == offsetof(nbody_hip_batch_merger_t, moved_from) &&
              offsetof(BatchMerger, contact_tick) == offsetof(nbody_hip_batch_merger_t, contact_tick) &&
              offsetof(BatchMerger, contact_macro) == offsetof(nbody_hip_batch_merger_t, contact_macro) &&
              offsetof(BatchMerger, contact_d2) == offsetof(nbody_hip_batch_merger_t, contact_d2) &&
              offsetof(BatchMerger, radius) == offsetof(nbody_hip_batch_merger_t, radius) &&
              offsetof(BatchMerger, mass) == offsetof(nbody_hip_batch_merger_t, mass) &&
              offsetof(BatchMerger, delta_ke) == offsetof(nbody_hip_batch_merger_t, delta_ke) &&
              offsetof(BatchMerger, delta_pe) == offsetof(nbody_hip_batch_merger_t, delta_pe),
              "BatchMerger is nbody_hip_batch_merger_t field for field");
void BlockHermiteEnsemble::setMergers(bool enabled) {
  NBODY_CHECK(nbody_hip_batch_mergers_set(handleFor("setMergers"), enabled ? NBODY_HIP_BATCH_MERGERS_ON : 0));
}
void BlockHermiteEnsemble::applyMergers(ParticleData* d) {
  if (!d) throw ValidationException("BlockHermiteEnsemble::applyMergers: null particle data");
  NBODY_CHECK(nbody_hip_batch_mergers_apply(handleFor("applyMergers"), raw(d)));
}
void BlockHermiteEnsemble::mergers(BatchMergerState* h_state, BatchMerger* h_log, unsigned int* h_ids) const {
  if (!h_state) throw ValidationException("BlockHermiteEnsemble::mergers: null output pointer");
  const size_t systems = offsets_.size() > 1 ? offsets_.size() - 1 : 1;
  const size_t bodies = offsets_.empty() ? 0 : offsets_.back();
  NBODY_CHECK(nbody_hip_batch_mergers_get(handle_, reinterpret_cast<nbody_hip_batch_merger_state_t*>(h_state), systems,
                                          reinterpret_cast<nbody_hip_batch_merger_t*>(h_log), h_ids, bodies));
}

void computeAccJerk(ParticleData* d, float G, float eps, float4* d_acc_out, float4* d_jerk_out) {
  NBODY_CHECK(nbody_hip_direct_acc_jerk(facadeContext(), raw(d), G, eps, reinterpret_cast<nbody_float4*>(d_acc_out),
                                        reinterpret_cast<nbody_float4*>(d_jerk_out)));
}

}  // namespace nbody
