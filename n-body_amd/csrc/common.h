// common.h -- internal declarations shared by the HIP translation units of libnbody_hip.so.
// gfx950 (MI355X) only; wave64; no CUDA compatibility layer.
#pragma once

#ifndef NBH_SORT_MERGE_LIMIT
#define NBH_SORT_MERGE_LIMIT (300 * 1000)
#endif

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "direct_plan.h"
#include "nbody_hip.h"

namespace nbh {

constexpr int kWave = 64;
constexpr int kBlock = 256;   // 4 waves: one per SIMD of a CU
constexpr int kNumCU = 256;   // MI355X
static_assert(kDirectBlock == kBlock && kDirectCU == kNumCU, "direct_plan.h sizes its grids for this block and this device");
// rocPRIM's radix sort switches from its merge-sort path (2 launches per doubling: 22 at 2^20 keys)
// to Onesweep above `merge_sort_limit` (default 2^20, i.e. exactly NOT at the BASELINE size); measured:
// merge sort wins at 262,144 keys (0.24 vs 0.26 ms tree build), Onesweep from 524,288 (0.14 vs 0.18 ms)
constexpr size_t kSortMergeLimit = NBH_SORT_MERGE_LIMIT;
// (... and from kOwnSortFromTree / kOwnSortFromGrid bodies a radix sort of our own takes over: body_sort.h)
// workgroups of the key kernels that also histogram the digits (each flushes its non-empty bins with global atomics)
#ifndef NBH_HIST_BLOCKS
#define NBH_HIST_BLOCKS 256
#endif
#ifndef NBH_HIST_THREADS
#define NBH_HIST_THREADS 1024
#endif

#ifdef __HIPCC__
// x + v dt + a (dt^2 / 2) as p + fma(a, h, v * dt): the contraction nvcc's default -fmad makes of
// integrator.cu:16-19 -- one definition, so that the SoA, fused and float4 drift kernels round identically
// (a sharded run then reproduces the single-GPU one bit for bit).
__device__ __forceinline__ float drift1(float p, float v, float a, float dt, float h) {
  return p + __builtin_fmaf(a, h, v * dt);
}
// Per-body potential (nbody_hip_*_potential): s = the fp64 sum of m_j / sqrt(r^2 + eps^2) (the hash: minus the
// shift) over body i's interaction list.  phi_i = -G s rounded once to fp32; terms[i] = m_i s feeds the PE
// reduction (potential_finish), so PE = 1/2 sum m_i phi_i is summed from the unrounded sums.
__device__ __forceinline__ void store_potential(int i, float m, double s, float G, float* phi, double* terms) {
  if (phi) phi[i] = (float)(-(double)G * s);
  if (terms) terms[i] = (double)m * s;
}
// One row of a field call (nbody_hip_*_field) at point p from the fp64 sums of m d / r^3 over its interaction list and
// the finished fp64 potential phi (each method forms -G sum m / r its own way: the sign of an exactly zero sum is
// part of its output): {G sx, G sy, G sz, phi}, each rounded once to fp32 -- or four NaN for a non-finite point,
// whatever the sums hold.
__device__ __forceinline__ float4 field_row(const float4 p, float G, double sx, double sy, double sz, double phi) {
  const bool finite = (p.x - p.x) + (p.y - p.y) + (p.z - p.z) == 0.f;
  const float nan = __builtin_nanf("");
  return finite ? make_float4((float)((double)G * sx), (float)((double)G * sy), (float)((double)G * sz),
                              (float)phi)
                : make_float4(nan, nan, nan, nan);
}
#endif

// energy.hip: the workspace of a potential call in ctx->reduce -- `extra` doubles for the caller (the Direct
// sweep's per-split sums), then the per-body terms when a PE is wanted (*terms = nullptr otherwise)
int potential_begin(nbody_hip_ctx* ctx, size_t n, size_t extra, bool want_pe, double** extra_out, double** terms);
// PE = -G/2 sum terms over n bodies in a fixed order (bitwise reproducible); blocks.  pe == nullptr: nothing.
int potential_finish(nbody_hip_ctx* ctx, size_t n, float G, double* pe);
// the argument checks the three potential calls share (not capturable: a diagnostic that may block)
int potential_check(nbody_hip_ctx* ctx, const nbody_particle_data* d, const float* phi, const double* pe);

// barnes_hut.hip: false with NBH_FIELD_SORT=0 in the environment -- the tree / grid field calls then take their points
// in caller order (measurement hook; read at every call)
bool field_sort_enabled();

void set_error(const char* fmt, ...);
int fail(nbody_hip_status code, const char* file, int line, const char* fmt, ...);

#define NBH_FAIL(code, ...) ::nbh::fail((code), __FILE__, __LINE__, __VA_ARGS__)

// calls that hand data back to the host cannot be recorded into a step graph
#define NBH_NOT_CAPTURABLE(ctx, what)                                                          \
  do {                                                                                        \
    if ((ctx)->capturing) {                                                                   \
      (ctx)->capture_failed = true;                                                           \
      return NBH_FAIL(NBODY_HIP_ERR_STATE, "%s cannot be recorded into a step graph", what);   \
    }                                                                                         \
  } while (0)

// HIP call that turns an error into NBODY_HIP_ERR_DEVICE (or _RESOURCE for OOM),
// message "<call>: <hip error string> at file:line" (ref: CUDA_CHECK, error_handling.hpp:104-114)
#define NBH_HIP(call)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      return ::nbh::fail(e_ == hipErrorOutOfMemory ? NBODY_HIP_ERR_RESOURCE                   \
                                                   : NBODY_HIP_ERR_DEVICE,                    \
                         __FILE__, __LINE__, "%s: %s", #call, hipGetErrorString(e_));         \
    }                                                                                         \
  } while (0)

// After a kernel launch (ref: CUDA_CHECK_KERNEL, error_handling.hpp:116-136; no sync in release)
#define NBH_LAUNCH_CHECK() NBH_HIP(hipGetLastError())

struct Workspace {
  void* ptr = nullptr;
  size_t bytes = 0;
  unsigned long long generation = 0;  // bumped whenever `ptr` is replaced (step graphs bake it in)
  int reserve(size_t want);  // grows (never shrinks); returns status
  void release();
};

}  // namespace nbh

struct nbody_hip_group_props;  // include/nbody_hip_group_props.h
struct nbody_hip_radial_group;  // include/nbody_hip_radial.h
struct nbody_hip_radial_shell;

struct nbody_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;      // caller-owned stream launches go to (nullptr = null stream)
  nbh::Workspace posm;               // packed {x,y,z,m} of the bodies        (direct, energy)
  nbh::Workspace partial;            // per-source-split partial accelerations (direct)
  nbh::Workspace reduce;             // block partials for energy reductions
  nbh::Workspace groups;             // chunk tables and partials of the group properties (group_props_plan.h)
  nbh::Workspace centre;             // chunk sums of the density centre (density_centre.hip)
  nbh::Workspace radial;             // sort pairs, terms and chunk tables of the radial profiles (radial_plan.h)
  // density-peak groups (hop_plan.h).  Their call cannot be recorded into a step graph, so no recording holds a pointer
  // into these three and their generations are not part of generation()
  nbh::Workspace hop;                // per-body arrays
  nbh::Workspace hop_records;        // boundary records, their sort and the unique edges
  nbh::Workspace hop_catalogue;      // offsets, members and group peaks of the last accepted call
  long long hop_count = -1, hop_groups = 0, hop_members = 0;  // of that catalogue (hop_count < 0: there is none)
  hipEvent_t hop_events[7] = {};     // the stage boundaries of a search, made at the first one
  float hop_stage_ms[6] = {};        // device time of the six stages of the last search with status 0
  bool hop_stages_valid = false;
  double* host_scalar = nullptr;     // pinned, 4 doubles
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t capture_stream = nullptr;  // library-owned, only used while recording a step graph
  hipStream_t user_stream = nullptr;     // ctx->stream saved by capture_begin
  bool capturing = false;
  mutable bool capture_failed = false;           // a non-capturable call was made while recording
  nbh::DirectTuning tune;  // nbody_hip_direct_tuning, _deterministic, _slot_budget (direct_plan.h)
  int last_direct_kernel = -1;  // what the last Direct launch ran: 0 one-sided, 1 symmetric + atomics, 2 symmetric + slots
  // bumped when a tree / grid of this context re-sizes or frees device arrays a recorded step graph
  // may point into; together with the workspaces' generations it dates a recording
  unsigned long long alloc_generation = 0;
  // replays of recorded step graphs so far: a replay runs launches this library did not see, so state the host
  // side assumes about device buffers between calls (a tree's re-armed bounding box) is dated with it
  unsigned long long graph_replays = 0;
  unsigned long long generation() const {
    return posm.generation + partial.generation + reduce.generation + groups.generation + centre.generation + radial.generation +
           alloc_generation;
  }
};

namespace nbh {

// v + (a_old + a) dt/2 as one explicit chain (add, then fma): integrator.cu:33-35 under nvcc's default
// contraction; shared by every kick (SoA, float4, fused into the force finalize) so they round alike
__device__ __forceinline__ float kick1(float v, float a_old, float a_new, float dt_half) {
  return __builtin_fmaf(a_old + a_new, dt_half, v);
}

// host dispatch on a template flag: f(std::true_type{}) or f(std::false_type{})
template <class F>
inline void with_flag(bool flag, F&& f) {
  if (flag) f(std::true_type{}); else f(std::false_type{});
}
// ... and on a template number, bodies per lane above all: f(std::integral_constant<int, v>{}) for the one of Vs that v
// is; false (and no call) when it is none of them
template <int... Vs, class F>
inline bool with_int(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// direct_sym.hip: direct_plan (direct_plan.h) of an all-pairs call on this context, from its tuning and its workspace;
// query_device: the budget rule may ask the (current) device for its free memory
DirectPlan device_direct_plan(const nbody_hip_ctx* ctx, size_t n, float eps2, bool query_device);

// group_props.hip: the properties of the groups of a catalogue in device memory (nbody_hip_groups_properties, which
// checks the context alone before it comes here; nbody_hip_grid_groups_properties with the catalogue of a grid)
int group_props_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev, const int* members_dev,
                       long long n_groups, long long n_members, const float* phi_dev_or_null,
                       ::nbody_hip_group_props* out_dev);

// radial_profile.hip: the radial profiles of the groups of an ordered catalogue in device memory
// (nbody_hip_groups_radial_profile, which checks the context alone before it comes here;
// nbody_hip_grid_groups_radial_profile with the catalogue of a grid)
int radial_profile_launch(nbody_hip_ctx* ctx, const nbody_particle_data* d, const int* offsets_dev, const int* members_dev,
                          long long n_groups, long long n_members, const double* centres_dev, const double* vels_dev_or_null,
                          const double* cuts_host, int n_cuts, int mode, ::nbody_hip_radial_group* groups_out_dev,
                          ::nbody_hip_radial_shell* shells_out_dev, int* sorted_members_dev_or_null,
                          float* sorted_q_dev_or_null);

// direct.hip
int direct_packed(nbody_hip_ctx* ctx, const float4* targets, size_t n_targets,
                  const float4* sources, size_t n_sources, float G, float eps2,
                  // output selection (exactly one of acc4 / soa is used)
                  float4* acc4, int accumulate, float* ax, float* ay, float* az,
                  // optional fused velocity update (soa output only): v += (a_old + a) * half_dt
                  float* vx, float* vy, float* vz, const float* aox, const float* aoy,
                  const float* aoz, float half_dt);
// direct_sym.hip: all-pairs with action = -reaction (targets == sources), as planned (plan.symmetric)
int direct_symmetric(nbody_hip_ctx* ctx, DirectPlan plan, const float4* posm, size_t n, float G, float eps2,
                     float4* acc4, int accumulate, float* ax, float* ay, float* az, float* vx,
                     float* vy, float* vz, const float* aox, const float* aoy, const float* aoz,
                     float half_dt);
int direct_symmetric_pair(nbody_hip_ctx* ctx, const float4* pi, size_t ni, const float4* pj, size_t nj,
                          float G, float eps2, float4* acc_i, int accumulate_i, float4* acc_j,
                          int accumulate_j);
int pack_posm(nbody_hip_ctx* ctx, const float* x, const float* y, const float* z, const float* m,
              size_t n, float4* out);

// spatial_hash.hip: order-preserving-integer bounding box of packed bodies into enc[6]
// (min x,y,z then max x,y,z); decode with ordered_to_float on the device.
int launch_bbox_init(nbody_hip_ctx* ctx, unsigned int* enc);
// drift of a Velocity-Verlet step fused with the packing and the bounding box of the following build:
// a_old <- a ; x += v dt + a dt^2/2 ; posm <- {x, y, z, m} ; enc <- box   (nbody_hip_{tree,grid}_drift_build)
int launch_drift_pack_bbox(nbody_hip_ctx* ctx, nbody_particle_data* d, float dt, float4* posm, unsigned int* enc,
                           bool init = true);
int launch_bbox(nbody_hip_ctx* ctx, const float4* posm, int n, unsigned int* enc, bool init = true);
int launch_pack_bbox(nbody_hip_ctx* ctx, const float* x, const float* y, const float* z, const float* m, int n,
                     float4* posm, unsigned int* enc, bool init = true);

__device__ __forceinline__ unsigned int float_to_ordered(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_float(unsigned int o) {
  const unsigned int u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// The *_destroy entry points may be reached while the process is exiting (a host language's garbage collector running
// after the HIP runtime's own static destructors): a runtime that is gone answers hipErrorDeinitialized -- or throws
// from inside (std::bad_variant_access out of hipStreamSynchronize was seen once: rc 134).  Then nothing is freed --
// the address space is about to disappear anyway -- and nothing may propagate across the C ABI.
inline bool runtime_alive() noexcept {
  try {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return n > 0;
  } catch (...) {
    return false;
  }
}
#define NBH_DESTROY_BEGIN          \
  if (!nbh::runtime_alive()) return NBODY_HIP_OK; \
  try {
#define NBH_DESTROY_END            \
  } catch (...) {                  \
  }                                \
  return NBODY_HIP_OK;

// Entry points that work on SEVERAL devices (the sharded systems, the communicator) hipSetDevice their way through the
// local ranks; the caller's current device is put back on every exit path -- the facade and the reference model are
// "current device, null stream" (ref: include/nbody/force_calculator.hpp:8-19), so a caller's next allocation or
// null-stream launch must land where it was before the call.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() noexcept {
    try {
      if (hipGetDevice(&prev) != hipSuccess) {
        prev = -1;
        (void)hipGetLastError();
      }
    } catch (...) {  // (a runtime that is already gone: see runtime_alive)
      prev = -1;
    }
  }
  ~DeviceGuard() {
    try {
      if (prev >= 0) (void)hipSetDevice(prev);
    } catch (...) {
    }
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace nbh
