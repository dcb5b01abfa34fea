// nbody_facade.hpp -- C++ host facade over the C ABI of libnbody_hip.so.
//
// One header that re-declares, in namespace nbody, the part of the reference's public C++
// interface that its CUDA translation units (src/cuda/*.cu) implement:
//   types           include/nbody/types.hpp              (Vec3, enums, ParticleData, configs)
//   exceptions      include/nbody/error_handling.hpp:29-102
//   ForceCalculator + Direct / BarnesHut / SpatialHash calculators, createForceCalculator,
//   computeGravitationalForceCPU                          include/nbody/force_calculator.hpp
//   Integrator      include/nbody/integrator.hpp
//   ParticleDataManager, ParticleInitializer             include/nbody/particle_data.hpp
//   BarnesHutTree / OctreeNode, SpatialHashGrid          barnes_hut_tree.hpp, spatial_hash_grid.hpp
// Names, signatures, data-member order and defaults match the reference so that objects compiled
// against the reference's own headers (e.g. its unmodified src/core/particle_system.cpp) link and
// run against libnbody_facade.so -- see INTEGRATION.md and oracle/Makefile.ref.  Every method
// forwards to one C-ABI call; there is no arithmetic in this layer.
#pragma once

#include <cmath>
#include <cstddef>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#if !defined(__HIPCC__) && !defined(__CUDACC__)
#ifndef NBODY_FACADE_HAVE_INT3
#define NBODY_FACADE_HAVE_INT3
struct int3 { int x, y, z; };
inline constexpr int3 make_int3(int x, int y, int z) { return {x, y, z}; }
#endif
#ifndef NBODY_FACADE_HAVE_FLOAT4
#define NBODY_FACADE_HAVE_FLOAT4
struct alignas(16) float4 { float x, y, z, w; };  // points {x, y, z, -} and rows {ax, ay, az, phi} of computeField
#endif
#endif

struct nbody_hip_ctx;
struct nbody_hip_tree;
struct nbody_hip_grid;
struct nbody_hip_hermite;
struct nbody_hip_hermite_block;
struct nbody_hip_hermite_batch;
struct nbody_hip_comm;
struct nbody_hip_sharded_direct;

namespace nbody {

enum class ForceMethod { DIRECT_N2, BARNES_HUT, SPATIAL_HASH };
enum class InitDistribution { UNIFORM, SPHERICAL, DISK };

struct Vec3 {
  float x, y, z;
  Vec3() : x(0), y(0), z(0) {}
  Vec3(float a, float b, float c) : x(a), y(b), z(c) {}
  Vec3 operator+(const Vec3& v) const { return {x + v.x, y + v.y, z + v.z}; }
  Vec3 operator-(const Vec3& v) const { return {x - v.x, y - v.y, z - v.z}; }
  Vec3 operator*(float s) const { return {x * s, y * s, z * s}; }
  Vec3 operator/(float s) const { return {x / s, y / s, z / s}; }
  Vec3& operator+=(const Vec3& v) { x += v.x; y += v.y; z += v.z; return *this; }
  Vec3& operator-=(const Vec3& v) { x -= v.x; y -= v.y; z -= v.z; return *this; }
  float dot(const Vec3& v) const { return x * v.x + y * v.y + z * v.z; }
  float length2() const { return dot(*this); }
  float length() const { return std::sqrt(length2()); }
  Vec3 normalized() const { const float l = length(); return l > 0 ? *this / l : Vec3(); }
};
inline Vec3 operator*(float s, const Vec3& v) { return v * s; }

struct ParticleData {  // 13 device (or host) arrays + count, 112 bytes
  float *pos_x = nullptr, *pos_y = nullptr, *pos_z = nullptr;
  float *vel_x = nullptr, *vel_y = nullptr, *vel_z = nullptr;
  float *acc_x = nullptr, *acc_y = nullptr, *acc_z = nullptr;
  float *acc_old_x = nullptr, *acc_old_y = nullptr, *acc_old_z = nullptr;
  float* mass = nullptr;
  size_t count = 0;
};

struct SimulationConfig {
  size_t particle_count = 10000;
  InitDistribution init_distribution = InitDistribution::SPHERICAL;
  ForceMethod force_method = ForceMethod::DIRECT_N2;
  float dt = 0.001f;
  float G = 1.0f;
  float softening = 0.1f;
  float barnes_hut_theta = 0.5f;
  float spatial_hash_cell_size = 1.0f;
  float spatial_hash_cutoff = 2.0f;
  int cuda_block_size = 256;
};

struct UniformDistParams { Vec3 min_bounds, max_bounds; float min_mass = 1.0f, max_mass = 1.0f; };
struct SphericalDistParams { Vec3 center; float radius = 10.0f, min_mass = 1.0f, max_mass = 1.0f; };
struct DiskDistParams {
  Vec3 center; float radius = 10.0f, thickness = 1.0f, min_mass = 1.0f, max_mass = 1.0f,
      rotation_speed = 1.0f;
};

// ---- exceptions (same names, what() formats and accessors as the reference) ----------------
class CudaException : public std::runtime_error {
public:
  CudaException(const char* msg, const char* file, int line)
      : std::runtime_error(format(msg, file, line)), error_msg_(msg), file_(file), line_(line) {}
  const char* getErrorMsg() const { return error_msg_; }
  const char* getFile() const { return file_; }
  int getLine() const { return line_; }
private:
  static std::string format(const char* msg, const char* file, int line) {
    std::ostringstream o; o << "CUDA Error: " << msg << " at " << file << ":" << line; return o.str();
  }
  const char* error_msg_; const char* file_; int line_;
};
class ResourceException : public std::runtime_error {
public:
  ResourceException(const char* msg, size_t required, size_t available)
      : std::runtime_error(format(msg, required, available)), required_(required), available_(available) {}
  size_t getRequired() const { return required_; }
  size_t getAvailable() const { return available_; }
private:
  static std::string format(const char* msg, size_t r, size_t a) {
    std::ostringstream o; o << msg << " - Required: " << r << " bytes, Available: " << a << " bytes"; return o.str();
  }
  size_t required_, available_;
};
class ValidationException : public std::runtime_error {
public:
  explicit ValidationException(const std::string& msg) : std::runtime_error("Validation Error: " + msg) {}
};

// ---- device structures ---------------------------------------------------------------------
struct OctreeNode {  // 76 bytes
  Vec3 center; float half_size; Vec3 center_of_mass; float total_mass;
  int children[8]; int particle_index; bool is_leaf; int particle_count;
  OctreeNode() : half_size(0), total_mass(0), particle_index(-1), is_leaf(true), particle_count(0) {
    for (int& c : children) c = -1;
  }
};

class BarnesHutTree {
public:
  BarnesHutTree(size_t max_particles);
  ~BarnesHutTree();
  void build(const ParticleData* d_particles);
  // (facade only, no data member: the drift of a Velocity-Verlet step + build in one pass over the bodies,
  // nbody_hip_tree_drift_build; Integrator::integrate uses it for exactly the engine's own calculator)
  void driftBuild(ParticleData* d_particles, float dt);
  void computeForces(ParticleData* d_particles, float theta, float G, float eps);
  // (facade only, no data member) per-body potential over the force walk's interaction lists on the tree as built,
  // phi into d_phi (device, count floats) when not null; returns PE = 1/2 sum m phi (nbody_hip_tree_potential)
  double computePotential(const ParticleData* d_particles, float theta, float G, float eps, float* d_phi = nullptr);
  // (facade only, no data member) {ax, ay, az, phi} of the tree as built at n DEVICE points {x, y, z, -}
  // (nbody_hip_tree_field: the force walk's interaction list for each position, no self-skip)
  void computeField(const float4* d_points, size_t n, float theta, float G, float eps, float4* d_out);
  // (facade only, no data member) multipole order of the walk: 1 = monopoles (default), 2 = monopoles + quadrupoles
  // (nbody_hip_tree_set_multipole_order: takes effect at the next build; a walk before it throws CudaException, the
  // C ABI's ERR_STATE); copyMomentsToHost: 6 floats per node (Sxx, Syy, Szz, Sxy, Sxz, Syz) in the numbering of
  // copyNodesToHost, for a tree built at order 2 (CudaException otherwise)
  void setMultipoleOrder(int order);
  int getMultipoleOrder() const;
  std::vector<float> copyMomentsToHost() const;
  int getNodeCount() const { return node_count_; }
  int getMaxDepth() const { return max_depth_; }
  const OctreeNode* getNodes() const { return h_nodes_.data(); }
  void copyNodesToHost();
  bool verifyTreeStructure() const;
  bool verifyMassConservation(const ParticleData* h_particles) const;
private:
  // EXACTLY the reference's data members (barnes_hut_tree.hpp:57-74), same order and types:
  // sizeof == 96 under both header sets, so a caller compiled against the reference's header
  // (its tests build these objects on the stack) reserves what this constructor writes.
  // The engine's handle lives in the d_nodes_ slot (the device node array belongs to the
  // handle); the other two device pointers stay null.  Checked by oracle/layout_probe.cpp.
  OctreeNode* d_nodes_ = nullptr;
  int* d_sorted_indices_ = nullptr;
  unsigned int* d_morton_codes_ = nullptr;
  std::vector<OctreeNode> h_nodes_;
  size_t max_particles_;
  size_t max_nodes_ = 0;
  int node_count_ = 0;
  int max_depth_ = 0;
  Vec3 bbox_min_, bbox_max_;
  nbody_hip_tree* handle() const { return reinterpret_cast<nbody_hip_tree*>(d_nodes_); }
};

// (facade only) the friends-of-friends groups of a grid (SpatialHashGrid::findGroups; nbody_hip_groups.h), on the host:
// labels[i] = the lowest body index of the group of body i; the groups of at least min_members bodies ascending by label,
// group g = members[offsets[g] .. offsets[g + 1]), members ascending by index
struct GroupCatalogue {
  std::vector<int> labels, offsets, members;
  size_t n_groups = 0;
};

// (facade only) the fp64 properties of one group: nbody_hip_group_props of the C ABI, field for field
// (include/nbody_hip_group_props.h has the model); 192 bytes
struct GroupProperties {
  double mass, com[3], vel[3], ang_mom[3], kinetic, inertia[6], r_max, potential, phi_min;
  int n, label, r_max_body, phi_min_body;  // the bodies by ORIGINAL index, ties to the lowest; phi_min_body -1 without phi
  int status, reserved[3];                 // status 1: not a legal group (then n = 0 and zeros everywhere else)
};

// (facade only) the radial profile of one group and one of its shells: nbody_hip_radial_group and nbody_hip_radial_shell
// of the C ABI, field for field (include/nbody_hip_radial.h has the model); 32 and 64 bytes
struct RadialGroup {
  double mass, r_max;       // M; sqrt((double)q) of the last rank
  int n, status;            // status 1: catalogue / range / member index, 2: a NaN distance (then n = 0 and zeros)
  int reserved[2];
};
struct RadialShell {
  double radius, enclosed_mass;    // of the cut: sqrt((double)q) of rank K - 1 (radius mode: the cut itself); E(K - 1)
  double mass, m_vr, m_vr2, m_vt2;  // the shell's four sums
  int count, enclosed_count;       // K_c - K_(c-1); K_c
  int reserved[2];
};
enum RadialMode { RADIAL_MASS = 0, RADIAL_NUMBER = 1, RADIAL_RADIUS = 2 };  // NBODY_HIP_RADIAL_*

// (facade only) the k nearest neighbours of every body of a grid (SpatialHashGrid::findNeighbours;
// nbody_hip_neighbours.h has the model), on the host, rows in ORIGINAL body order: index[i * k + s] and dist2[i * k + s]
// ascending by (d2, index), -1 / +inf in unused slots; rho[i] the Casertano-Hut density; status[i] 0 exact, 1
// window-limited, 2 fewer than k candidates, 3 the k-th neighbour coincident
struct NeighbourLists {
  int k = 0;
  std::vector<int> index;
  std::vector<float> dist2;
  std::vector<double> rho;
  std::vector<int> status;
};

// (facade only) the density-peak (HOP) groups of a grid (SpatialHashGrid::hopGroups; nbody_hip_hop.h has the model), on
// the host: labels[i] = root[peak[i]] or -1, peak[i] the density maximum body i's chain ends at; the groups of at least
// min_members labelled bodies in the layout of GroupCatalogue, group_peak[g] the densest peak of group g
struct HopParameters {
  int n_hop = 0;            // 0: k
  int n_merge = 4, min_members = 1;
  double delta_outer = 0.0;
  double delta_saddle = -1.0, delta_peak = -1.0;  // negative: HOP's defaults, 2.5 and 3 times delta_outer
};
struct HopCatalogue {
  GroupCatalogue groups;  // labels, offsets, members, n_groups: what groupProperties and radialProfiles take
  std::vector<int> peak, group_peak;
  long long n_peaks = 0, rounds = 0;
  int status = 0;         // 1: a neighbour index at or past the body count (cannot happen with the grid's own lists)
};

class SpatialHashGrid {
public:
  SpatialHashGrid(size_t max_particles, float cell_size = 1.0f);
  ~SpatialHashGrid();
  void build(const ParticleData* d_particles);
  void driftBuild(ParticleData* d_particles, float dt);  // facade only, see BarnesHutTree::driftBuild
  void computeForces(ParticleData* d_particles, float cutoff, float G, float eps);
  // (facade only) the shifted truncated potential over the force's pair set on the grid as built (nbody_hip_grid_potential)
  double computePotential(const ParticleData* d_particles, float cutoff, float G, float eps, float* d_phi = nullptr);
  // (facade only, no data member) {ax, ay, az, phi} of the grid as built at n DEVICE points (nbody_hip_grid_field)
  void computeField(const float4* d_points, size_t n, float cutoff, float G, float eps, float4* d_out);
  // (facade only, no data member) the groups of the grid as built, linking_length <= the cell size (nbody_hip_grid_groups)
  void findGroups(float linking_length, int min_members, GroupCatalogue& out);
  // (facade only, no data member) the properties of the groups of ANY catalogue over d_particles, groups of any size
  // (nbody_hip_groups_properties): out[g] for group g.  d_phi: count floats on the DEVICE (computePotential's phi) or null.
  // The catalogue is uploaded and the structs are copied back: the call blocks.
  void groupProperties(const ParticleData* d_particles, const GroupCatalogue& catalogue, std::vector<GroupProperties>& out,
                       const float* d_phi = nullptr);
  // (facade only, no data member) the radial profiles of the groups of ANY ordered catalogue over d_particles about
  // centres[3 g ..] (nbody_hip_groups_radial_profile): groups[g], and shells[g * cuts.size() + c] for cut c -- mass or
  // number fractions in (0, 1] or radii >= 0, strictly ascending, at most 16.  bulk_velocities: 3 doubles a group or
  // null (zeros).  The catalogue is uploaded and the structs are copied back: the call blocks.
  void radialProfiles(const ParticleData* d_particles, const GroupCatalogue& catalogue, const std::vector<double>& centres,
                      const std::vector<double>& cuts, int mode, std::vector<RadialGroup>& groups,
                      std::vector<RadialShell>& shells, const std::vector<double>* bulk_velocities = nullptr);
  // (facade only, no data member) the k nearest candidates (1 <= k <= 32) of every body on the grid as built, with the
  // density and the status (nbody_hip_grid_neighbours).  The results are copied back: the call blocks.
  void findNeighbours(int k, NeighbourLists& out);
  // (facade only, no data member) the density-peak groups of the grid as built: the k nearest candidates and the density of
  // every body (nbody_hip_grid_neighbours), then nbody_hip_hop_groups on them.  The results are copied back: the call
  // blocks.  neighbours: when not null, it receives the lists the groups were found on.
  void hopGroups(int k, const HopParameters& params, HopCatalogue& out, NeighbourLists* neighbours = nullptr);
  int3 getGridDims() const { return grid_dims_; }
  float getCellSize() const { return cell_size_; }
  int getTotalCells() const { return total_cells_; }
  void copyCellDataToHost(std::vector<int>& cell_start, std::vector<int>& cell_end,
                          std::vector<int>& particle_cells, std::vector<int>& sorted_indices);
  bool verifyCellAssignment(const ParticleData* h_particles) const;
  static int3 getCellIndex(float x, float y, float z, float cell_size);
  static int hashCell(int3 cell, int3 grid_dims);
private:
  int *d_cell_start_ = nullptr, *d_cell_end_ = nullptr, *d_particle_cell_ = nullptr,
      *d_sorted_indices_ = nullptr, *d_cell_counts_ = nullptr;
  size_t max_particles_;
  float cell_size_;
  int3 grid_dims_{0, 0, 0};
  int total_cells_ = 0;
  Vec3 bbox_min_, bbox_max_;
  // the reference's data members only (spatial_hash_grid.hpp:36-52; sizeof == 96 under both
  // header sets).  The engine's handle lives in the d_cell_start_ slot; the body count of the
  // last build is asked from the handle.
  nbody_hip_grid* handle() const { return reinterpret_cast<nbody_hip_grid*>(d_cell_start_); }
};

// ---- the strategy interface (the plugin boundary) ---------------------------------------------
class ForceCalculator {
public:
  virtual ~ForceCalculator() = default;
  virtual void computeForces(ParticleData* d_particles) = 0;
  virtual ForceMethod getMethod() const = 0;
  void setSofteningParameter(float eps) { softening_eps_ = eps; softening_eps2_ = eps * eps; }
  void setGravitationalConstant(float G) { G_ = G; }
  float getSofteningParameter() const noexcept { return softening_eps_; }
  float getGravitationalConstant() const noexcept { return G_; }
protected:
  float softening_eps_ = 0.01f;
  float softening_eps2_ = 0.0001f;
  float G_ = 1.0f;
};

class DirectForceCalculator : public ForceCalculator {
public:
  explicit DirectForceCalculator(int block_size = 256);
  void computeForces(ParticleData* d_particles) override;
  ForceMethod getMethod() const noexcept override { return ForceMethod::DIRECT_N2; }
  void setBlockSize(int size) { block_size_ = size; }
  int getBlockSize() const noexcept { return block_size_; }
private:
  int block_size_;
};

// MI355X-native addition (no reference counterpart; the reference is single-GPU): Direct N^2 shared by `ndev`
// GPUs of one node behind the SAME plugin interface -- computeForces(ParticleData*) on a whole-system
// ParticleData that lives on device 0; positions go out and accelerations come back as peer copies over
// xGMI (include/nbody_hip_comm.h: nbody_hip_comm_init_all + nbody_hip_sharded_direct_compute_forces).
// Drops into Integrator::integrate / ParticleSystem like any user-defined ForceCalculator.
class ShardedDirectCalculator : public ForceCalculator {
public:
  // devices: the GPUs to share the work (empty = all visible devices); rccl: RCCL collectives instead of peer copies
  explicit ShardedDirectCalculator(std::vector<int> devices = {}, bool rccl = false);
  ~ShardedDirectCalculator() override;
  void computeForces(ParticleData* d_particles) override;
  ForceMethod getMethod() const noexcept override { return ForceMethod::DIRECT_N2; }
  int getDeviceCount() const noexcept { return static_cast<int>(devices_.size()); }
private:
  std::vector<int> devices_;
  bool rccl_;
  ::nbody_hip_comm* comm_ = nullptr;
  ::nbody_hip_sharded_direct* sys_ = nullptr;
  size_t count_ = 0;
  float built_G_ = 0.f, built_eps_ = -1.f;
};

class BarnesHutCalculator : public ForceCalculator {
public:
  explicit BarnesHutCalculator(float theta = 0.5f);
  ~BarnesHutCalculator();
  void computeForces(ParticleData* d_particles) override;
  ForceMethod getMethod() const noexcept override { return ForceMethod::BARNES_HUT; }
  void setTheta(float theta) { theta_ = theta; }
  float getTheta() const noexcept { return theta_; }
  BarnesHutTree* getTree() noexcept { return tree_.get(); }
  // (facade only, no data member: kept in a table outside the object) multipole order of the tree, 1 (default) or 2;
  // set before or after the first computeForces, it applies from the next one
  void setMultipoleOrder(int order);
  int getMultipoleOrder() const;
private:
  friend double computePotential(ForceCalculator& force_calc, ParticleData* d_particles, float* d_phi);
  friend void computeField(ForceCalculator& force_calc, ParticleData* d_particles, const float4* d_points, size_t n,
                           float4* d_out);
  std::unique_ptr<BarnesHutTree> tree_;
  float theta_;
};

class SpatialHashCalculator : public ForceCalculator {
public:
  SpatialHashCalculator(float cell_size = 1.0f, float cutoff_radius = 2.0f);
  ~SpatialHashCalculator();
  void computeForces(ParticleData* d_particles) override;
  ForceMethod getMethod() const noexcept override { return ForceMethod::SPATIAL_HASH; }
  void setCellSize(float size) { cell_size_ = size; }
  void setCutoffRadius(float radius) { cutoff_radius_ = radius; }
  float getCellSize() const noexcept { return cell_size_; }
  float getCutoffRadius() const noexcept { return cutoff_radius_; }
  SpatialHashGrid* getGrid() noexcept { return grid_.get(); }
private:
  friend double computePotential(ForceCalculator& force_calc, ParticleData* d_particles, float* d_phi);
  friend void computeField(ForceCalculator& force_calc, ParticleData* d_particles, const float4* d_points, size_t n,
                           float4* d_out);
  std::unique_ptr<SpatialHashGrid> grid_;
  float cell_size_;
  float cutoff_radius_;
};

std::unique_ptr<ForceCalculator> createForceCalculator(ForceMethod method, const SimulationConfig& config);
// (facade only) PE = 1/2 sum m_i phi_i in the calculator's own model, phi into d_phi (device, count floats) when not
// null: the engine's Barnes-Hut and spatial-hash calculators build their structure (as computeForces does, without
// writing acc_*) and use its potential; every other calculator, ShardedDirectCalculator included, gets the
// single-GPU Direct sum (nbody_hip_direct_potential).
double computePotential(ForceCalculator& force_calc, ParticleData* d_particles, float* d_phi = nullptr);
// {ax, ay, az, phi} of the calculator's own model at n DEVICE points (facade only): the engine's Barnes-Hut and
// spatial-hash calculators build their structure as computePotential does, everything else is the Direct sum
// (nbody_hip_{tree,grid,direct}_field).  acc_* are not written.
void computeField(ForceCalculator& force_calc, ParticleData* d_particles, const float4* d_points, size_t n, float4* d_out);
Vec3 computeGravitationalForceCPU(const Vec3& p1, const Vec3& p2, float m1, float m2, float G, float eps);

class Integrator {
public:
  explicit Integrator(int block_size = 256);
  ~Integrator();
  void integrate(ParticleData* d_particles, ForceCalculator* force_calc, float dt);
  void updatePositions(ParticleData* d_particles, float dt);
  void updateVelocities(ParticleData* d_particles, float dt);
  void storeOldAccelerations(ParticleData* d_particles);
  float computeKineticEnergy(const ParticleData* d_particles);
  float computePotentialEnergy(const ParticleData* d_particles, float G, float eps);
  float computeTotalEnergy(const ParticleData* d_particles, float G, float eps);
  void ensureScratchBuffer(size_t particle_count);
  void setBlockSize(int size) { block_size_ = size; }
  int getBlockSize() const noexcept { return block_size_; }
private:
  int block_size_;
  float* d_scratch_ = nullptr;  // unused here: reductions use the context's workspace
  int scratch_blocks_ = 0;
};

// MI355X-native addition (no reference counterpart): the fourth-order Hermite integrator (PEC form of Makino & Aarseth
// 1992) on the Direct force-and-jerk kernel, nbody_hip_hermite_* of the C ABI.  Direct-only: it accepts EXACTLY the
// engine's own DirectForceCalculator (typeid, the rule of Integrator::integrate's fused path; G and eps are that
// calculator's) and throws ValidationException for anything else, a subclass included -- the tree and the grid have no
// jerk.  After a step acc_* = a1 and acc_old_* = a as after a Velocity-Verlet step; the jerk stays on the handle.  (a1,
// j1) belong to the predicted state: a run continued from a checkpoint agrees with the uninterrupted one to truncation
// order, not bit for bit.  A class of its own: no existing class changes size or layout.
// State precision of the two Hermite integrators (nbody_hip_hermite[_block]_set_precision).  Extended: the state of a
// body is pos + pos_lo, vel + vel_lo with fp32 residuals on the handle; pos_* / vel_* stay the fp32 roundings, the pair
// sweep forms d = (hi_j - hi_i) + (lo_j - lo_i).  A switch re-primes; switching to Extended starts with residuals 0;
// invalidate() in extended mode zeroes them.
enum class StatePrecision { Fp32 = 0, Extended = 1 };

class HermiteIntegrator {
public:
  explicit HermiteIntegrator(int block_size = 256);
  ~HermiteIntegrator();
  HermiteIntegrator(const HermiteIntegrator&) = delete;
  HermiteIntegrator& operator=(const HermiteIntegrator&) = delete;
  void integrate(ParticleData* d_particles, ForceCalculator* force_calc, float dt);
  void integrateSteps(ParticleData* d_particles, ForceCalculator* force_calc, float dt, int steps);
  void prime(ParticleData* d_particles, ForceCalculator* force_calc);  // (a, j) at the current state; writes acc_*
  void invalidate();  // the caller changed x, v, m, G or eps behind the integrator: the next step primes again
  void getJerk(float4* d_out) const;  // {jx, jy, jz, 0} per body into a DEVICE array (CudaException if not primed)
  float suggestTimeStep(float eta = 0.02f) const;  // eta min |a| / |j| of the last evaluation (a hint; blocking)
  void setStatePrecision(StatePrecision p);
  StatePrecision getStatePrecision() const noexcept { return precision_; }
  // X, V: HOST arrays [count][3] in fp64.  set: hi into the particle data, lo onto the handle, unprimes; get: hi + lo
  void setExtendedState(ParticleData* d_particles, ForceCalculator* force_calc, const double* h_pos, const double* h_vel);
  void getExtendedState(ParticleData* d_particles, ForceCalculator* force_calc, double* h_pos, double* h_vel);
  float computeKineticEnergy(const ParticleData* d_particles) { return energies_.computeKineticEnergy(d_particles); }
  float computePotentialEnergy(const ParticleData* d_particles, float G, float eps) {
    return energies_.computePotentialEnergy(d_particles, G, eps);
  }
  float computeTotalEnergy(const ParticleData* d_particles, float G, float eps) {
    return energies_.computeTotalEnergy(d_particles, G, eps);
  }
  void setBlockSize(int size) { energies_.setBlockSize(size); }
  int getBlockSize() const noexcept { return energies_.getBlockSize(); }
private:
  ::nbody_hip_hermite* handleFor(const ParticleData* d_particles, const ForceCalculator* force_calc, const char* method);
  Integrator energies_;
  ::nbody_hip_hermite* handle_ = nullptr;
  size_t capacity_ = 0;
  StatePrecision precision_ = StatePrecision::Fp32;
};

// MI355X-native addition (no reference counterpart): the Hermite integrator with INDIVIDUAL BLOCK TIME STEPS,
// nbody_hip_hermite_block_* of the C ABI.  Body i steps with dt_max 2^-k_i, its level chosen by the Aarseth criterion;
// integrate() advances the system by one MACRO step dt_max, after which every body is at the same time.  Direct-only by
// the typeid rule of HermiteIntegrator.  With BlockScheduling::Host (the default) every stepping call blocks; with
// Resident (systems of up to 4,096 bodies) one workgroup runs the block steps of a macro step inside one launch and the
// stepping calls return at once; Auto takes the resident form below the measured crossover.  A resident run equals the
// host-scheduled narrow-form run bit for bit.  A class of its own: no existing class changes size or layout.
enum class BlockScheduling { Host = 0, Resident = 1, Auto = 2 };
// per-system fp64 energies, momenta, closest and most bound pair: nbody_hip_system_diag of the C ABI, field for field
// (include/nbody_hip.h has the model); 152 bytes
struct SystemDiag {
  double mass, com[3], momentum[3], ang_mom[3], kinetic, potential, min_sep, bind_energy, bind_a, bind_e;
  int min_i, min_j, bind_i, bind_j;  // system-local, i < j; -1, -1: none
  int n, status;                     // status 1: not a legal range of bodies (then n = 0 and nothing else is written)
};
struct BlockHermiteInfo {
  unsigned long long block_steps, body_steps, level_steps[21], floor_hits, narrow_launches, wide_launches, macro_steps;
  unsigned int current_tick, last_n_active;
  int max_level, narrow_below;
};
class BlockHermiteIntegrator {
public:
  explicit BlockHermiteIntegrator(int block_size = 256);
  ~BlockHermiteIntegrator();
  BlockHermiteIntegrator(const BlockHermiteIntegrator&) = delete;
  BlockHermiteIntegrator& operator=(const BlockHermiteIntegrator&) = delete;
  void setParameters(float eta = 0.02f, float eta_start = 0.01f, int max_level = 16);  // at the next priming
  void integrate(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max);  // one macro step
  void advance(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max, int macro_steps);
  void blockStep(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max, int block_steps = 1);
  void prime(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max);
  void invalidate();
  void getLevels(int* h_out) const;  // HOST array of count levels (CudaException if not primed)
  void getState(int* h_levels, unsigned int* h_ticks, float* h_want, float4* h_jerk) const;  // HOST arrays, any may be null
  BlockHermiteInfo info() const;
  // the fp64 diagnostics of the system (nbody_hip_hermite_block_diagnostics: at most 4,096 bodies, at a macro boundary;
  // G and eps from force_calc) into ONE HOST struct; blocks for the copy
  void diagnostics(ParticleData* d_particles, ForceCalculator* force_calc, SystemDiag* h_out);
  void setStatePrecision(StatePrecision p);
  StatePrecision getStatePrecision() const noexcept { return precision_; }
  // only at a macro boundary (CudaException in the middle of a macro step); the priming and the counters stay
  void setScheduling(BlockScheduling s);
  BlockScheduling getScheduling() const noexcept { return scheduling_; }
  // X, V: HOST arrays [count][3] in fp64.  set: hi into the particle data, lo onto the handle, unprimes (CudaException in the middle of a macro step); get: hi + lo
  void setExtendedState(ParticleData* d_particles, ForceCalculator* force_calc, const double* h_pos, const double* h_vel);
  void getExtendedState(ParticleData* d_particles, ForceCalculator* force_calc, double* h_pos, double* h_vel);
  float computeKineticEnergy(const ParticleData* d_particles) { return energies_.computeKineticEnergy(d_particles); }
  float computePotentialEnergy(const ParticleData* d_particles, float G, float eps) {
    return energies_.computePotentialEnergy(d_particles, G, eps);
  }
  float computeTotalEnergy(const ParticleData* d_particles, float G, float eps) {
    return energies_.computeTotalEnergy(d_particles, G, eps);
  }
  void setBlockSize(int size) { energies_.setBlockSize(size); }
  int getBlockSize() const noexcept { return energies_.getBlockSize(); }
private:
  ::nbody_hip_hermite_block* handleFor(const ParticleData* d_particles, const ForceCalculator* force_calc,
                                       const char* method);
  Integrator energies_;
  ::nbody_hip_hermite_block* handle_ = nullptr;
  size_t capacity_ = 0;
  float eta_ = 0.02f, eta_start_ = 0.01f;
  int max_level_ = 16;
  StatePrecision precision_ = StatePrecision::Fp32;
  BlockScheduling scheduling_ = BlockScheduling::Host;
};

// MI355X-native addition (no reference counterpart): the block-step Hermite integrator for ENSEMBLES,
// nbody_hip_hermite_batch_* of the C ABI.  B independent small systems, stored back to back in one ParticleData (system s
// the bodies [offsets[s], offsets[s+1]), 1 to 4,096 of them), advanced by one launch with one workgroup per system; no
// pair is formed across systems; dt_max is per system, everything else is shared.  System s of a run equals a
// BlockHermiteIntegrator in BlockScheduling::Resident on those bodies alone bit for bit.  Direct-only by the typeid rule
// of HermiteIntegrator; prime() and advance() return at once.  A class of its own: no existing class changes size or
// layout.
// one system's record of the ensemble EVENTS: nbody_hip_batch_event_t of the C ABI, field for field (64 bytes).  "None":
// d2 = +inf, i = j = 0xFFFFFFFF.
struct BatchEvent {
  unsigned int stopped;                 // 0 running, 1 contact, 2 budget, 3 escape (setOutcomes), 4 resolved (setHierarchy)
  unsigned int reserved;
  unsigned long long macro_steps_done;
  float closest_d2;
  unsigned int closest_i, closest_j, closest_tick;
  unsigned long long closest_macro;
  float contact_d2;
  unsigned int contact_i, contact_j, contact_tick;
  unsigned long long contact_macro;
};
// one system's record of the ensemble OUTCOMES: nbody_hip_batch_outcome_t of the C ABI, field for field (64 bytes).
// "None": escaped = 0, escaper = 0xFFFFFFFF, the rest 0.
struct BatchOutcome {
  unsigned int escaped;      // bodies that escape at the boundary of the first escape
  unsigned int escaper;      // the lowest escaping index (system-local)
  unsigned long long macro;  // completed macro steps at that boundary (>= 1)
  double r, vr, energy;      // the escaper against the centre of mass of all the rest
  double rest_mass;
  double reserved, reserved2;
};
// one system's record of the ensemble HIERARCHIES and one slot of its node table: nbody_hip_batch_hierarchy_t and
// nbody_hip_batch_node_t of the C ABI, field for field (64 bytes each).  "None": all 0 but min_sep = +inf and
// min_p = min_q = 0xFFFFFFFF; the slots at and above node_count are zero.
struct BatchHierarchy {
  unsigned int resolved;      // 0 or 1
  unsigned int top_count;     // the pieces of the forest
  unsigned long long macro;   // completed macro steps at the examined boundary; 0: never examined
  unsigned int node_count;    // n + composites made
  unsigned int largest;       // bodies in the largest top node
  double min_sep;             // the smallest separation of two top nodes, and the pair
  unsigned int min_p, min_q;
  double reserved[3];
};
struct BatchNode {
  unsigned int left, right;   // 0xFFFFFFFF for a leaf
  unsigned int parent;        // 0xFFFFFFFF for a top node
  unsigned int bodies;
  double mass, a, e, r, energy;
  double reserved;
};
// one system's merger state and one entry of its log (ensemble MERGERS): nbody_hip_batch_merger_state_t (32 bytes) and
// nbody_hip_batch_merger_t (64 bytes) of the C ABI, field for field.  moved_from = 0xFFFFFFFF: no body moved.
struct BatchMergerState {
  unsigned int n_live;       // live bodies: the slots [0, n_live) of the system
  unsigned int n_mergers;    // entries of the log since the priming
  unsigned int flags;        // 1: a contact record was refused
  unsigned int reserved[5];
};
struct BatchMerger {
  unsigned int slot_a, slot_b;  // lo, hi
  unsigned int id_a, id_b;      // the merged body keeps id_a
  unsigned int moved_from;
  unsigned int contact_tick;
  unsigned long long contact_macro;
  float contact_d2;
  float radius;
  double mass;                  // M in fp64
  double delta_ke, delta_pe;
};

class BlockHermiteEnsemble {
public:
  BlockHermiteEnsemble() = default;
  ~BlockHermiteEnsemble();
  BlockHermiteEnsemble(const BlockHermiteEnsemble&) = delete;
  BlockHermiteEnsemble& operator=(const BlockHermiteEnsemble&) = delete;
  void setParameters(float eta = 0.02f, float eta_start = 0.01f, int max_level = 16);  // at the next priming
  void setStatePrecision(StatePrecision p);
  StatePrecision getStatePrecision() const noexcept { return precision_; }
  // n_systems + 1 offsets: offsets[0] = 0, strictly ascending, every size in [1, 4096]; a new layout unprimes
  void setLayout(const size_t* offsets, size_t n_systems);
  void prime(ParticleData* d_particles, ForceCalculator* force_calc, const float* h_dt_max);  // HOST array of n_systems
  void prime(ParticleData* d_particles, ForceCalculator* force_calc, float dt_max);           // the same for every system
  void invalidate();
  void advance(ParticleData* d_particles, int macro_steps = 1);
  void getState(int* h_levels, unsigned int* h_ticks, float* h_want, float4* h_jerk) const;  // HOST arrays over all bodies, any may be null
  void getJerk(float4* h_jerk) const { getState(nullptr, nullptr, nullptr, h_jerk); }
  BlockHermiteInfo info(long long system = -1) const;  // -1: the sums over the systems
  // the fp64 diagnostics of every system (nbody_hip_hermite_batch_diagnostics; a primed ensemble) into a HOST array of
  // n_systems structs; blocks for the copy
  void diagnostics(ParticleData* d_particles, SystemDiag* h_out);
  // per-system stopping conditions and encounter records (nbody_hip_hermite_batch_set_events; after setLayout, which
  // drops them).  h_radii: one value per body of the ensemble or null; h_max_macro_steps: one budget per system (0: none)
  // or null; all of nothing: back to the plain kernel.  A recorded advance keeps the kernel form it recorded.
  void setEvents(const float* h_radii = nullptr, const unsigned long long* h_max_macro_steps = nullptr,
                 bool track_closest = false, bool stop_on_contact = false);
  void events(BatchEvent* h_out) const;  // HOST array of n_systems records; blocks; a primed ensemble
  size_t running() const;                // systems neither stopped nor in a schedule error; blocks
  // per-system escape detection (nbody_hip_batch_outcomes_set; after setLayout, which drops it).  h_escape_radii: one
  // value per system, 0: no test, or null: outcomes off; stop_on_escape: a system with a first escape stops (stop word 3)
  void setOutcomes(const float* h_escape_radii, bool stop_on_escape = false);
  void outcomes(BatchOutcome* h_out) const;  // HOST array of n_systems records; blocks; a primed ensemble
  // per-system hierarchy decomposition (nbody_hip_batch_hierarchy_set; after setLayout, which drops it).
  // h_separation_radii: one value per system, 0: no examination, or null: hierarchies off; isolation: kappa;
  // stop_on_resolved: a resolved system stops (stop word 4)
  void setHierarchy(const float* h_separation_radii, float isolation = 0.0f, bool stop_on_resolved = false);
  // HOST arrays of n_systems records and (or null) 2 n_total node slots; blocks; a primed ensemble
  void hierarchy(BatchHierarchy* h_records, BatchNode* h_nodes = nullptr) const;
  // the same of the state as it is now, by a kernel of its own into scratch: the run's records are not touched
  void hierarchySnapshot(ParticleData* d_particles, BatchHierarchy* h_records, BatchNode* h_nodes);
  void setExtendedState(ParticleData* d_particles, const double* h_pos, const double* h_vel);
  void getExtendedState(ParticleData* d_particles, double* h_pos, double* h_vel);
  // sticky-sphere mergers between launches (nbody_hip_batch_mergers_set; after setLayout, which drops it; needs
  // setEvents with radii and stop_on_contact).  applyMergers: every system that stopped on contact merges its recorded
  // pair, shrinks by one body, is primed again alone and runs on; asynchronous, recordable after one eager call
  void setMergers(bool enabled = true);
  void applyMergers(ParticleData* d_particles);
  // HOST arrays: n_systems states, and (each may be null) n_total log entries -- system s from offsets[s], n_mergers of
  // them -- and n_total ids; blocks; a primed ensemble
  void mergers(BatchMergerState* h_state, BatchMerger* h_log = nullptr, unsigned int* h_ids = nullptr) const;
private:
  ::nbody_hip_hermite_batch* handleFor(const char* method);
  ::nbody_hip_hermite_batch* handle_ = nullptr;
  size_t capacity_ = 0, max_systems_ = 0;
  std::vector<size_t> offsets_;
  bool layout_sent_ = false;
  float eta_ = 0.02f, eta_start_ = 0.01f;
  int max_level_ = 16;
  StatePrecision precision_ = StatePrecision::Fp32;
};

// (facade only) Direct acceleration and jerk at the bodies into DEVICE arrays of d_particles->count rows {x, y, z, 0}
// (nbody_hip_direct_acc_jerk); d_acc_out == nullptr: the accelerations go to acc_* instead, which are otherwise left alone
void computeAccJerk(ParticleData* d_particles, float G, float eps, float4* d_acc_out, float4* d_jerk_out);

class ParticleDataManager {
public:
  static void allocateDevice(ParticleData& data, size_t count);
  static void freeDevice(ParticleData& data);
  static void allocateHost(ParticleData& data, size_t count);
  static void freeHost(ParticleData& data);
  static void copyToDevice(ParticleData& d_data, const ParticleData& h_data);
  static void copyToHost(ParticleData& h_data, const ParticleData& d_data);
  static void copyPositionsToHost(float* h_pos_x, float* h_pos_y, float* h_pos_z, const ParticleData& d_data);
  static void copyPositionsToDevice(ParticleData& d_data, const float* h_pos_x, const float* h_pos_y,
                                    const float* h_pos_z);
};

class ParticleInitializer {
public:
  static void initUniform(ParticleData& h_data, const UniformDistParams& params, unsigned int seed = 42);
  static void initSpherical(ParticleData& h_data, const SphericalDistParams& params, unsigned int seed = 42);
  static void initDisk(ParticleData& h_data, const DiskDistParams& params, unsigned int seed = 42);
  static void zeroVelocities(ParticleData& h_data);
  static void zeroAccelerations(ParticleData& h_data);
private:
  static std::mt19937 createRNG(unsigned int seed);
};

// launch wrappers the reference declares as free functions (integrator.hpp:153-158)
void launchUpdatePositionsKernel(ParticleData* d_particles, float dt, int block_size);
void launchUpdateVelocitiesKernel(ParticleData* d_particles, float dt, int block_size);
void launchStoreAccelerationsKernel(ParticleData* d_particles, int block_size);
float launchComputeKineticEnergyKernel(const ParticleData* d_particles, int block_size);
float launchComputePotentialEnergyKernel(const ParticleData* d_particles, float G, float eps, int block_size);
void launchDirectForceKernel(ParticleData* d_particles, float G, float eps2, int block_size);

// the process-wide HIP context the facade launches on (device 0, null stream, like the reference)
nbody_hip_ctx* facadeContext();

}  // namespace nbody
