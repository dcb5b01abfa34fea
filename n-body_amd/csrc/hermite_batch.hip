// hermite_batch.hip -- the block-step Hermite integrator for ENSEMBLES: B independent small systems, stored back to back
// in one nbody_particle_data, advanced by one launch with ONE WORKGROUP PER SYSTEM (no reference counterpart).  The
// model is that of hermite_block.hip (include/nbody_hip.h, DESIGN.md sections 4.10 and 4.13) applied to each system
// separately: system s is the bodies [offsets[s], offsets[s+1]), between 1 and 4,096 of them, no pair is formed across
// systems, dt_max is per system, everything else is shared.  The oracle is bit equality: system s of an ensemble run
// equals a single-system run in resident scheduling (block_resident_kernel) on those bodies alone, whatever its place
// in the batch and whatever the other systems are.
//
// Priming, three launches for the whole ensemble (the sums of hermite_evaluate at n <= 4,096, where one_sided_shape gives two
// targets per lane and one split per 256-source tile):
//   batch_pack_kernel            SoA -> {x, m}, {v, 0} (and {x_lo, 0}) of every body
//   batch_prime_sweep_kernel     one workgroup per (system, 512-target block, 256-source tile): the fp32 chain of
//                                jerk_tile<2, GUARD, EXT> over the tile's sources in index order (padded sources:
//                                m = 0 at rest at the origin), one fp32 row per tile
//   batch_prime_finalize_kernel  rows added in fp64 in tile order, G in fp64, rounded to fp32 -> acc_*, jerk; then the
//                                rule of block_prime_kernel with the system's own dt_max; ticks, counters, status <- 0
// Advance, ONE launch per call: batch_resident_kernel, grid = B workgroups of 512 threads.  Workgroup s runs the block
// step of block_resident_kernel (resident_block_step, hermite_block_common.h) on its own slice -- t, the prediction, the
// active set in LDS, the narrow sweep, block_finalize_body, the level histogram -- to the macro boundary, macro_steps
// times over: a fast system never waits for a slow one.  Workgroups do not communicate: no grid barrier, no
// wait on memory, no device-side launch; every loop is bounded; a system whose schedule cannot be writes its own status
// word and stops, and launches queued behind skip that system only.  The per-system words (first body, n, row offset,
// dt_max, counters) live in device arrays indexed by the workgroup and are moved to scalar registers.

#include <cmath>
#include <cstring>
#include <vector>

#include <cstddef>

#include "hermite_batch_hierarchy_common.h"
#include "hermite_batch_layout.h"
#include "hermite_batch_mergers_common.h"
#include "hermite_batch_outcomes_common.h"
#include "hermite_batch_plan.h"
#include "hermite_block_common.h"
#include "hermite_handle.h"
#include "nbody_hip_events.h"
#include "nbody_hip_hierarchy.h"
#include "nbody_hip_mergers.h"
#include "nbody_hip_outcomes.h"
#include "system_diag.h"

namespace nbh {

constexpr int kBatchMaxN = NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX;
constexpr int kPrimeR = 2;                       // targets per lane of the priming sweep: one_sided_shape's R below 32,768
constexpr int kPrimeTargets = kBlock * kPrimeR;  // 512-target blocks

// what the device knows about the layout of system s, and a work item of the priming sweep (hermite_batch_layout.h)
typedef BatchLayoutSystem BatchSystem;
typedef BatchLayoutItem BatchPrimeItem;
static_assert(kLayoutMaxSystem == (size_t)kBatchMaxN && kLayoutSourceBlock == (size_t)kBlock * kNarrowS &&
              kLayoutTargetGroup == (size_t)kNarrowT && kLayoutTile == (size_t)TS &&
              kLayoutTargetBlock == (size_t)kPrimeTargets, "hermite_batch_layout.h restates the shapes of the sweeps");

// the counters of system s (the status word has an array of its own: status[s] != 0, the schedule went out of range)
struct BatchState {
  unsigned long long block_steps, body_steps, macro_steps;
  unsigned int last_n_active, pad;
};

// an ensemble launch: the arrays of the whole ensemble, passed once and offset by the system's first body and first row
// inside the kernel, and the per-system words
struct BatchArgs {
  ResidentArrays p;
  const BatchSystem* sys;
  const float* dt_max;         // [B]
  unsigned int* status;        // [B]
  BatchState* state;           // [B]
  unsigned long long* counters;  // [B][kCounters]
  int L;
  float G, eps2, eta;
};

// ---------------------------------------------------------------------------------
// Priming 1: the plain pack of every body of the ensemble (hermite_predict_pack_kernel<EXT> at dt = 0)
// ---------------------------------------------------------------------------------
template <bool EXT>
__global__ __launch_bounds__(kBlock) void batch_pack_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, const float* __restrict__ vx,
                                                            const float* __restrict__ vy, const float* __restrict__ vz,
                                                            const float* __restrict__ m, HermiteLo lo, int n,
                                                            float4* __restrict__ posm, float4* __restrict__ vel,
                                                            float4* __restrict__ plo) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  posm[i] = make_float4(x[i], y[i], z[i], m[i]);
  vel[i] = make_float4(vx[i], vy[i], vz[i], 0.f);
  if constexpr (EXT) plo[i] = make_float4(lo.x[i], lo.y[i], lo.z[i], 0.f);
}

// ---------------------------------------------------------------------------------
// Priming 2: one (system, 512-target block, 256-source tile) per workgroup of 256 threads.  The tile body of
// direct_jerk_kernel<2, GUARD, EXT, false> (jerk_tile, hermite_common.h) for one tile, with targets, sources and padding
// confined to the system: lane tid holds the targets tblock 512 + tid and + 256 of the system, the tile's sources go
// through LDS and are taken in index order.  pa / pj[tile][k], k the target's index inside the system,
// n_pad = ceil(n / 512) 512.
// ---------------------------------------------------------------------------------
template <bool GUARD, bool EXT>
__global__ __launch_bounds__(kBlock) void batch_prime_sweep_kernel(const BatchPrimeItem* __restrict__ items,
                                                                   const BatchSystem* __restrict__ sys,
                                                                   const float4* __restrict__ posm_all,
                                                                   const float4* __restrict__ vel_all,
                                                                   const float4* __restrict__ plo_all,
                                                                   float4* __restrict__ pa_all,
                                                                   float4* __restrict__ pj_all, float eps2) {
  const BatchPrimeItem it = items[blockIdx.x];
  const int s = uniform_i(it.system), tblock = uniform_i(it.tblock), tile = uniform_i(it.tile);
  const BatchSystem w = sys[s];
#include "hermite_batch_prime_sweep.inc"
}

// ---------------------------------------------------------------------------------
// Priming 3: one thread per body of the ensemble.  The sums of hermite_finalize_kernel (rows in tile order in fp64, G in
// fp64, rounded to fp32) -> acc_*, jerk; then block_prime_kernel's rule with the system's dt_max.  The first body of a
// system zeroes that system's counters and status word.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void batch_prime_finalize_kernel(
    const int* __restrict__ body_system, const BatchSystem* __restrict__ sys, const float* __restrict__ dt_max,
    const float4* __restrict__ pa_all, const float4* __restrict__ pj_all, int n_total, float G, float eta_s, int L,
    float* __restrict__ ax, float* __restrict__ ay, float* __restrict__ az, float4* __restrict__ jerk,
    int* __restrict__ level, unsigned int* __restrict__ tick, float* __restrict__ want, unsigned int* __restrict__ status,
    BatchState* __restrict__ state, unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_total) return;
  const int s = body_system[i];
  const BatchSystem w = sys[s];
  const int k = i - w.first;  // 0 <= k < n
  const int tiles = (w.n + TS - 1) / TS;
  const int n_pad = (w.n + kPrimeTargets - 1) / kPrimeTargets * kPrimeTargets;
  const float4* pa = pa_all + w.prime_row_off;
  const float4* pj = pj_all + w.prime_row_off;
  const float& dt = dt_max[s];  // (a reference: a copy hoists the load and changes the instruction stream)
#include "hermite_batch_prime_finalize.inc"
  if (k == 0) {
    status[s] = 0u;
    state[s] = BatchState{0ull, 0ull, 0ull, 0u, 0u};
    for (int c = 0; c < kCounters; c++) counters[(size_t)s * kCounters + c] = 0ull;
  }
}

// what the EVENT form of the advance takes besides; all null in the plain form, which reads none
struct BatchEventArgs {
  const float* radii;                    // [bodies of the ensemble]
  const unsigned long long* limits;      // [B], 0: none
  nbody_hip_batch_event_t* events;       // [B]
  unsigned int flags;
};

static_assert(sizeof(nbody_hip_batch_event_t) == 64 && offsetof(nbody_hip_batch_event_t, stopped) == 0 &&
              offsetof(nbody_hip_batch_event_t, macro_steps_done) == 8 && offsetof(nbody_hip_batch_event_t, closest_d2) == 16 &&
              offsetof(nbody_hip_batch_event_t, closest_i) == 20 && offsetof(nbody_hip_batch_event_t, closest_j) == 24 &&
              offsetof(nbody_hip_batch_event_t, closest_tick) == 28 && offsetof(nbody_hip_batch_event_t, closest_macro) == 32 &&
              offsetof(nbody_hip_batch_event_t, contact_d2) == 40 && offsetof(nbody_hip_batch_event_t, contact_i) == 44 &&
              offsetof(nbody_hip_batch_event_t, contact_j) == 48 && offsetof(nbody_hip_batch_event_t, contact_tick) == 52 &&
              offsetof(nbody_hip_batch_event_t, contact_macro) == 56, "nbody_hip_batch_event_t is a fixed 64-byte record");
static_assert(kBatchMaxN <= (1 << 12), "a key holds two system-local indices of 12 bits");

// the key of a record's pair (kKeyNone when it holds none) and back
__device__ __forceinline__ unsigned long long event_key(const float d2, const unsigned int i, const unsigned int j) {
  return i == 0xffffffffu ? kKeyNone : pair_key(d2, (int)i, (int)j);
}
__device__ __forceinline__ void event_unkey(const unsigned long long key, float* d2, unsigned int* i, unsigned int* j) {
  *d2 = key == kKeyNone ? __builtin_inff() : __uint_as_float((unsigned int)(key >> 32));
  *i = key == kKeyNone ? 0xffffffffu : (unsigned int)(key >> 12) & 0xfffffu;
  *j = key == kKeyNone ? 0xffffffffu : (unsigned int)key & 0xfffu;
}

// the record of a system that holds no pair: running, 0 macro steps (the device and the host read-out write the same one)
__host__ __device__ inline void event_record_none(nbody_hip_batch_event_t* e) {
  e->stopped = 0u;
  e->reserved = 0u;
  e->macro_steps_done = 0ull;
  e->closest_d2 = e->contact_d2 = __builtin_inff();
  e->closest_i = e->closest_j = e->contact_i = e->contact_j = 0xffffffffu;
  e->closest_tick = e->contact_tick = 0u;
  e->closest_macro = e->contact_macro = 0ull;
}

// every record of the ensemble to "none", running, 0 macro steps (the priming; the first configuration of a handle)
__global__ __launch_bounds__(kBlock) void batch_events_clear_kernel(nbody_hip_batch_event_t* __restrict__ events, int B) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= B) return;
  nbody_hip_batch_event_t e;
  event_record_none(&e);
  events[s] = e;
}

// ---------------------------------------------------------------------------------
// OUTCOMES (include/nbody_hip.h "ensemble OUTCOMES"): what the advance takes besides, and the
// escape test of one system at a macro boundary.
// ---------------------------------------------------------------------------------
struct BatchOutcomeArgs {
  const float* r_esc;                    // [B], 0: no test
  nbody_hip_batch_outcome_t* out;        // [B]
  unsigned int flags;
};

static_assert(sizeof(nbody_hip_batch_outcome_t) == 64 && offsetof(nbody_hip_batch_outcome_t, escaped) == 0 &&
              offsetof(nbody_hip_batch_outcome_t, escaper) == 4 && offsetof(nbody_hip_batch_outcome_t, macro) == 8 &&
              offsetof(nbody_hip_batch_outcome_t, r) == 16 && offsetof(nbody_hip_batch_outcome_t, vr) == 24 &&
              offsetof(nbody_hip_batch_outcome_t, energy) == 32 && offsetof(nbody_hip_batch_outcome_t, rest_mass) == 40 &&
              offsetof(nbody_hip_batch_outcome_t, reserved) == 48 && offsetof(nbody_hip_batch_outcome_t, reserved2) == 56,
              "nbody_hip_batch_outcome_t is a fixed 64-byte record");
static_assert(kBatchMaxN <= 8 * kResidentBlock, "the escape test takes at most 8 bodies per thread");

// the record of a system from which nothing has escaped (the device and the host read-out write the same one)
__host__ __device__ inline void outcome_record_none(nbody_hip_batch_outcome_t* o) {
  o->escaped = 0u;
  o->escaper = 0xffffffffu;
  o->macro = 0ull;
  o->r = o->vr = o->energy = o->rest_mass = o->reserved = o->reserved2 = 0.0;
}

// every outcome record of the ensemble to "none" (the priming; the first configuration of a handle)
__global__ __launch_bounds__(kBlock) void batch_outcomes_clear_kernel(nbody_hip_batch_outcome_t* __restrict__ out, int B) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= B) return;
  nbody_hip_batch_outcome_t o;
  outcome_record_none(&o);
  out[s] = o;
}

// body i of the system (i < n) from the state in memory
template <bool EXT>
__device__ __forceinline__ DiagBody outcome_load(const ResidentArrays& P, const int i) {
  float lx = 0.f, ly = 0.f, lz = 0.f, lvx = 0.f, lvy = 0.f, lvz = 0.f;
  if constexpr (EXT) {
    lx = P.lo.x[i]; ly = P.lo.y[i]; lz = P.lo.z[i];
    lvx = P.lo.vx[i]; lvy = P.lo.vy[i]; lvz = P.lo.vz[i];
  }
  return diag_body(P.d.x[i], P.d.y[i], P.d.z[i], lx, ly, lz, P.d.vx[i], P.d.vy[i], P.d.vz[i], lvx, lvy, lvz, P.mass[i]);
}

// The escape test of the workgroup's system at a macro boundary; called by all 512 threads under a uniform condition.
// Two passes over the bodies, at most 8 per thread and every index below n: the sums in the model's fixed order, then the
// per-body test with an integer count and a minimum index.  True (uniform): a body escapes, and thread 0 has stored the
// record.  Only reads the state.  No atomics, no loop that n does not bound.
template <bool EXT>
__device__ __forceinline__ bool batch_outcome_test(const ResidentSystem& S, const double r_esc,
                                                   const unsigned long long macro, nbody_hip_batch_outcome_t* rec) {
  constexpr int kWaves = kResidentBlock / kWave;
  __shared__ double wsum[kWaves][kOutcomeSums];
  __shared__ unsigned int wcnt[kWaves], wmin[kWaves];
  const int tid = threadIdx.x, n = S.n;
  const ResidentArrays& P = S.p;
  __syncthreads();  // the corrector's stores of this workgroup are visible; the last test's LDS has been read
  OutcomeSums s;
  outcome_sums_zero(s);
  for (int i = tid; i < n; i += kResidentBlock) outcome_body_add(s, outcome_load<EXT>(P, i));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    OutcomeSums o;
#pragma unroll
    for (int c = 0; c < kOutcomeSums; c++) o.v[c] = __shfl_down(s.v[c], off, 64);
    outcome_sums_add(s, o);  // (lane 0 ends with the wave's sum; the lanes above the reach of off are not used)
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < kOutcomeSums; c++) wsum[tid >> 6][c] = s.v[c];
  }
  __syncthreads();
  OutcomeSums T;
#pragma unroll
  for (int c = 0; c < kOutcomeSums; c++) T.v[c] = wsum[0][c];
#pragma unroll
  for (int k = 1; k < kWaves; k++) {
    OutcomeSums o;
#pragma unroll
    for (int c = 0; c < kOutcomeSums; c++) o.v[c] = wsum[k][c];
    outcome_sums_add(T, o);
  }
  const double G = (double)S.G;
  unsigned int cnt = 0u, mn = 0xffffffffu;
  for (int i = tid; i < n; i += kResidentBlock) {
    if (outcome_body(T, outcome_load<EXT>(P, i), G, r_esc).escapes) {
      cnt++;
      mn = min(mn, (unsigned int)i);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += (unsigned int)__shfl_xor((int)cnt, off, 64);
    mn = min(mn, (unsigned int)__shfl_xor((int)mn, off, 64));
  }
  if ((tid & 63) == 0) {
    wcnt[tid >> 6] = cnt;
    wmin[tid >> 6] = mn;
  }
  __syncthreads();
  cnt = wcnt[0];
  mn = wmin[0];
#pragma unroll
  for (int k = 1; k < kWaves; k++) {
    cnt += wcnt[k];
    mn = min(mn, wmin[k]);
  }
  cnt = (unsigned int)uniform_i((int)cnt);
  mn = (unsigned int)uniform_i((int)mn);
  if (cnt == 0u || mn >= (unsigned int)n) return false;  // (uniform; cnt != 0 implies mn < n)
  if (tid == 0) {
    const OutcomeBody o = outcome_body(T, outcome_load<EXT>(P, (int)mn), G, r_esc);
    nbody_hip_batch_outcome_t e;
    e.escaped = cnt;
    e.escaper = mn;
    e.macro = macro;
    e.r = o.r;
    e.vr = o.vr;
    e.energy = o.e;
    e.rest_mass = o.rest_mass;
    e.reserved = e.reserved2 = 0.0;
    *rec = e;
  }
  return true;
}

// ---------------------------------------------------------------------------------
// HIERARCHIES (include/nbody_hip.h "ensemble HIERARCHIES"): what the advance takes besides, and
// the decomposition of one system at a macro boundary.
// ---------------------------------------------------------------------------------
struct BatchHierarchyArgs {
  const float* r_sep;                    // [B], 0: no examination
  nbody_hip_batch_hierarchy_t* rec;      // [B]
  nbody_hip_batch_node_t* nodes;         // [2 bodies of the ensemble]: system s from slot 2 first
  float kappa;
  unsigned int flags;
};

static_assert(sizeof(nbody_hip_batch_hierarchy_t) == 64 && offsetof(nbody_hip_batch_hierarchy_t, resolved) == 0 &&
              offsetof(nbody_hip_batch_hierarchy_t, top_count) == 4 && offsetof(nbody_hip_batch_hierarchy_t, macro) == 8 &&
              offsetof(nbody_hip_batch_hierarchy_t, node_count) == 16 && offsetof(nbody_hip_batch_hierarchy_t, largest) == 20 &&
              offsetof(nbody_hip_batch_hierarchy_t, min_sep) == 24 && offsetof(nbody_hip_batch_hierarchy_t, min_p) == 32 &&
              offsetof(nbody_hip_batch_hierarchy_t, min_q) == 36 && offsetof(nbody_hip_batch_hierarchy_t, reserved) == 40,
              "nbody_hip_batch_hierarchy_t is a fixed 64-byte record");
static_assert(sizeof(nbody_hip_batch_node_t) == 64 && offsetof(nbody_hip_batch_node_t, left) == 0 &&
              offsetof(nbody_hip_batch_node_t, right) == 4 && offsetof(nbody_hip_batch_node_t, parent) == 8 &&
              offsetof(nbody_hip_batch_node_t, bodies) == 12 && offsetof(nbody_hip_batch_node_t, mass) == 16 &&
              offsetof(nbody_hip_batch_node_t, a) == 24 && offsetof(nbody_hip_batch_node_t, e) == 32 &&
              offsetof(nbody_hip_batch_node_t, r) == 40 && offsetof(nbody_hip_batch_node_t, energy) == 48 &&
              offsetof(nbody_hip_batch_node_t, reserved) == 56, "nbody_hip_batch_node_t is a fixed 64-byte slot");
static_assert(kHierNodes * 4 <= kResidentBlock && kHierNodes <= 256,
              "a thread copies at most one 16-byte piece of the table; a node id fits 8 bits of a key and of the top list");

// every hierarchy record of the ensemble to "none" (the priming; the first configuration of a handle)
__global__ __launch_bounds__(kBlock) void batch_hierarchy_clear_kernel(nbody_hip_batch_hierarchy_t* __restrict__ rec, int B) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= B) return;
  nbody_hip_batch_hierarchy_t r;
  hier_record_none(&r);
  rec[s] = r;
}

// The workgroup's minimum of the keys (and the sum of cnt): xor shuffles inside the wave, one LDS stage of the eight
// waves' values behind ONE barrier, every thread folds the eight alike.  Uniform on return.  wb, wp, wc: 8 entries each,
// not read by anyone since the last barrier.
__device__ __forceinline__ HierKey hier_reduce(HierKey k, unsigned int& cnt, unsigned long long* wb, unsigned int* wp,
                                               unsigned int* wc) {
  constexpr int kWaves = kResidentBlock / kWave;
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    HierKey o;
    o.bits = __shfl_xor(k.bits, off, 64);
    o.pq = (unsigned int)__shfl_xor((int)k.pq, off, 64);
    cnt += (unsigned int)__shfl_xor((int)cnt, off, 64);
    if (hier_key_less(o, k)) k = o;
  }
  if ((tid & 63) == 0) {
    wb[tid >> 6] = k.bits;
    wp[tid >> 6] = k.pq;
    wc[tid >> 6] = cnt;
  }
  __syncthreads();
  k = HierKey{wb[0], wp[0]};
  cnt = wc[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++) {
    const HierKey o{wb[w], wp[w]};
    if (hier_key_less(o, k)) k = o;
    cnt += wc[w];
  }
  k.bits = uniform_u64(k.bits);
  k.pq = (unsigned int)uniform_i((int)k.pq);
  cnt = (unsigned int)uniform_i((int)cnt);
  return k;
}

// The examination of the workgroup's system (2 <= n <= 64) at a macro boundary; called by all 512 threads under a
// uniform condition.  The leaves go to LDS; each round deals the K (K - 1) / 2 <= 2,016 pairs of the top set over the
// threads in triangular order (thread t: the pairs t, t + 512, ..., at most four), reduces the key of the candidate
// with the smallest a, and thread 0 appends the composite while the first K threads close the gap in the top list (kept
// in rising id order, so position order is id order).  Two barriers a round, at most n - 1 rounds.  Then the four
// criteria and the smallest separation over the top pairs; thread 0 writes the record, the workgroup the 2 n slots.
// True (uniform): resolved.  Only reads the state.  No atomics, no loop that n does not bound.
template <bool EXT>
__device__ __forceinline__ bool batch_hierarchy_test(const ResidentSystem& S, const double r_sep, const double kappa,
                                                     const unsigned long long macro, nbody_hip_batch_hierarchy_t* rec,
                                                     nbody_hip_batch_node_t* table) {
  constexpr int kWaves = kResidentBlock / kWave;
  __shared__ HierNode node[kHierNodes];
  __shared__ __align__(16) nbody_hip_batch_node_t slot[kHierNodes];
  __shared__ unsigned char top[2][kHierMax];
  __shared__ unsigned long long wbits[2][kWaves];
  __shared__ unsigned int wpq[2][kWaves], wcnt[2][kWaves];
  const int tid = threadIdx.x, n = S.n;
  if (n < 2 || n > kHierMax) return false;  // (uniform; the callers do not come here)
  __syncthreads();  // the corrector's stores of this workgroup are visible; the last examination's LDS has been read
  if (tid < 2 * n) {
    nbody_hip_batch_node_t z;
    z.left = z.right = z.parent = z.bodies = 0u;
    z.mass = z.a = z.e = z.r = z.energy = z.reserved = 0.0;
    if (tid < n) {
      const HierNode b = outcome_load<EXT>(S.p, tid);
      node[tid] = b;
      hier_node_leaf(&z, b.m);
      top[0][tid] = (unsigned char)tid;
    }
    slot[tid] = z;
  }
  __syncthreads();
  const double G = (double)S.G;
  int K = n, count = n, cur = 0;
  unsigned int unused = 0u;
  for (int k = 0; k < n - 1; k++) {  // (K = n - k >= 2)
    const int pairs = K * (K - 1) / 2;
    HierKey best = hier_key_none();
    for (int t = tid; t < pairs; t += kResidentBlock) {
      int i, j;
      hier_pair_index(t, &i, &j);
      const unsigned int p = top[cur][i], q = top[cur][j];  // i < j < K, so p < q < count
      const HierPair o = hier_pair(node[p], node[q], G);
      if (o.candidate) {
        const HierKey key = hier_key(o.a, p, q);
        if (hier_key_less(key, best)) best = key;
      }
    }
    best = hier_reduce(best, unused, wbits[0], wpq[0], wcnt[0]);
    if (hier_key_is_none(best)) break;  // (uniform)
    const unsigned int p = best.pq >> 8, q = best.pq & 0xffu, c = (unsigned int)count;  // c <= 2 n - 2
    if (tid == 0) {
      const HierNode a = node[p], b = node[q];
      const HierPair o = hier_pair(a, b, G);  // (a pure function of the two nodes: the bits the key was made of)
      node[c] = hier_composite(a, b, o.M);
      nbody_hip_batch_node_t s;
      s.left = p;
      s.right = q;
      s.parent = kHierNone;
      s.bodies = slot[p].bodies + slot[q].bodies;
      s.mass = o.M;
      s.a = o.a;
      s.e = hier_ecc(a, b, G, o.M, o.eps);
      s.r = o.r;
      s.energy = o.eps;
      s.reserved = 0.0;
      slot[c] = s;
      slot[p].parent = slot[q].parent = c;
      top[cur ^ 1][K - 2] = (unsigned char)c;  // (the largest id: the list stays in rising order)
    }
    if (tid < K) {
      const unsigned int id = top[cur][tid];
      if (id != p && id != q) top[cur ^ 1][tid - (id > p ? 1 : 0) - (id > q ? 1 : 0)] = (unsigned char)id;
    }
    __syncthreads();
    cur ^= 1;
    K--;
    count++;
  }
  // the top pairs: the four criteria (an integer count of the pairs that miss one) and the smallest separation
  const int pairs = K * (K - 1) / 2;
  HierKey sep = hier_key_none();
  unsigned int failed = 0u;
  for (int t = tid; t < pairs; t += kResidentBlock) {
    int i, j;
    hier_pair_index(t, &i, &j);
    const unsigned int p = top[cur][i], q = top[cur][j];
    const HierPair o = hier_pair(node[p], node[q], G);
    if (!hier_pair_resolved(o, hier_apo(slot[p].a, slot[p].e), hier_apo(slot[q].a, slot[q].e), r_sep, kappa)) failed++;
    if (o.r == o.r) {  // (a NaN separation is never the smallest)
      const HierKey key = hier_key(o.r, p, q);
      if (hier_key_less(key, sep)) sep = key;
    }
  }
  sep = hier_reduce(sep, failed, wbits[1], wpq[1], wcnt[1]);
  const bool resolved = K >= 2 && failed == 0u;
  if (tid == 0) {
    unsigned int largest = 0u;
    for (int i = 0; i < K; i++) largest = max(largest, slot[top[cur][i]].bodies);
    nbody_hip_batch_hierarchy_t r;
    hier_record_none(&r);
    r.resolved = resolved ? 1u : 0u;
    r.top_count = (unsigned int)K;
    r.macro = macro;
    r.node_count = (unsigned int)count;
    r.largest = largest;
    if (!hier_key_is_none(sep)) {
      r.min_sep = hier_key_value(sep);
      r.min_p = sep.pq >> 8;
      r.min_q = sep.pq & 0xffu;
    }
    *rec = r;
  }
  // the table: 2 n slots of 64 bytes as 16-byte pieces, at most one a thread (the slots from count on are zero)
  if (tid < 8 * n) reinterpret_cast<uint4*>(table)[tid] = reinterpret_cast<const uint4*>(slot)[tid];
  return resolved;
}

// The snapshot (nbody_hip_batch_hierarchy_snapshot): one workgroup per system, the same examination of the state in
// memory into scratch records and tables.  The tables have been zeroed; a system outside 2 .. 64 bodies gets "none".
template <bool EXT>
__global__ __launch_bounds__(kResidentBlock) void batch_hierarchy_snapshot_kernel(
    const ResidentArrays P, const BatchSystem* __restrict__ sys, const BatchState* __restrict__ state,
    const float* __restrict__ r_sep_or_null, const float kappa, const float G, nbody_hip_batch_hierarchy_t* __restrict__ rec,
    nbody_hip_batch_node_t* __restrict__ nodes) {
  const int sidx = blockIdx.x;
  const BatchSystem w = sys[sidx];
  const int first = uniform_i(w.first), n = uniform_i(w.n);
  if (n < 2 || n > kHierMax) {  // (uniform)
    if (threadIdx.x == 0) {
      nbody_hip_batch_hierarchy_t r;
      hier_record_none(&r);
      rec[sidx] = r;
    }
    return;
  }
  ResidentSystem S{};
  S.p.d = HermiteArrays{P.d.x + first,  P.d.y + first,  P.d.z + first,  P.d.vx + first,  P.d.vy + first,  P.d.vz + first,
                        P.d.ax + first, P.d.ay + first, P.d.az + first, P.d.aox + first, P.d.aoy + first, P.d.aoz + first};
  if constexpr (EXT)
    S.p.lo = HermiteLo{P.lo.x + first, P.lo.y + first, P.lo.z + first, P.lo.vx + first, P.lo.vy + first, P.lo.vz + first};
  S.p.mass = P.mass + first;
  S.n = n;
  S.G = G;
  float r_sep = 0.f;
  if (r_sep_or_null) r_sep = __int_as_float(uniform_i(__float_as_int(r_sep_or_null[sidx])));
  const unsigned long long macro = uniform_u64(state[sidx].macro_steps);
  batch_hierarchy_test<EXT>(S, (double)r_sep, (double)kappa, macro, rec + sidx, nodes + 2 * (size_t)first);
}

// ---------------------------------------------------------------------------------
// The advance: grid = B workgroups of 512 threads, workgroup s on system s.  The block step is resident_block_step
// (hermite_block_common.h), the one block_resident_kernel (hermite_block.hip) calls: the same expressions in the same
// order between the same barriers, so system s has the bits of a single-system resident run.  Bounded: at most
// macro_steps (2^L + 1) block steps.  No communication between workgroups, no atomics on global memory.
// EVENTS: the step tracks the pair keys (TRACK) and hands back the block step's two
// workgroup-uniform minima; the system's record is held in registers, alike in every thread, so its stop conditions are
// uniform, and thread 0 writes it at the end of the launch with the counters.  The macro loop only ever ends EARLIER
// than the plain form's.
// ---------------------------------------------------------------------------------
template <bool EXT, bool GUARD, bool EVENTS>
__global__ __launch_bounds__(kResidentBlock) void batch_resident_kernel(const BatchArgs A, const BatchEventArgs E,
                                                                         int macro_steps) {
  constexpr bool TRACK = EVENTS, OUTCOMES = false, HIERARCHY = false;
  const BatchOutcomeArgs O{};    // (never read: OUTCOMES is false)
  const BatchHierarchyArgs H{};  // (never read: HIERARCHY is false)
  // the included text reads exactly these names, which must be in scope here: the compile-time flags EXT, GUARD, EVENTS,
  // TRACK, OUTCOMES, HIERARCHY; the arguments A (BatchArgs), E (BatchEventArgs), O (BatchOutcomeArgs), H
  // (BatchHierarchyArgs) and macro_steps (int)
#include "hermite_batch_resident_body.inc"
}

// the form with OUTCOMES: the record logic with the escape test at every macro boundary; TRACK:
// events are configured too (else the untracked sweep runs under the record logic: no radii, no budget, no keys)
template <bool EXT, bool GUARD, bool TRACK>
__global__ __launch_bounds__(kResidentBlock) void batch_outcomes_kernel(const BatchArgs A, const BatchEventArgs E,
                                                                         const BatchOutcomeArgs O, int macro_steps) {
  constexpr bool EVENTS = true, OUTCOMES = true, HIERARCHY = false;
  const BatchHierarchyArgs H{};  // (never read: HIERARCHY is false)
  // the included text reads exactly these names, which must be in scope here: the compile-time flags EXT, GUARD, EVENTS,
  // TRACK, OUTCOMES, HIERARCHY; the arguments A (BatchArgs), E (BatchEventArgs), O (BatchOutcomeArgs), H
  // (BatchHierarchyArgs) and macro_steps (int)
#include "hermite_batch_resident_body.inc"
}

// the form with HIERARCHIES: the record logic with the examination at every macro boundary.  The
// escape test stays gated at run time: O.r_esc is null when no outcomes are configured, else r_esc > 0 decides as before.
template <bool EXT, bool GUARD, bool TRACK>
__global__ __launch_bounds__(kResidentBlock) void batch_hierarchy_kernel(const BatchArgs A, const BatchEventArgs E,
                                                                          const BatchOutcomeArgs O,
                                                                          const BatchHierarchyArgs H, int macro_steps) {
  constexpr bool EVENTS = true, OUTCOMES = true, HIERARCHY = true;
  // the included text reads exactly these names, which must be in scope here: the compile-time flags EXT, GUARD, EVENTS,
  // TRACK, OUTCOMES, HIERARCHY; the arguments A (BatchArgs), E (BatchEventArgs), O (BatchOutcomeArgs), H
  // (BatchHierarchyArgs) and macro_steps (int)
#include "hermite_batch_resident_body.inc"
}

// ---------------------------------------------------------------------------------
// MERGERS (include/nbody_hip.h "ensemble MERGERS"): the pass between two advance launches.  Three
// launches: batch_merge_kernel (one workgroup per system: the merge, the compaction, the log, the records, the pack of
// the priming for that system, and the mark), then the priming's sweep and finalize restricted to the marked systems.
// The mark is the pass's own word per system: set by the merge, read by the two kernels behind it, cleared by the last.
// ---------------------------------------------------------------------------------
static_assert(sizeof(nbody_hip_batch_merger_state_t) == 32 && offsetof(nbody_hip_batch_merger_state_t, n_live) == 0 &&
              offsetof(nbody_hip_batch_merger_state_t, n_mergers) == 4 && offsetof(nbody_hip_batch_merger_state_t, flags) == 8 &&
              offsetof(nbody_hip_batch_merger_state_t, reserved) == 12,
              "nbody_hip_batch_merger_state_t is a fixed 32-byte record");
static_assert(sizeof(nbody_hip_batch_merger_t) == 64 && offsetof(nbody_hip_batch_merger_t, slot_a) == 0 &&
              offsetof(nbody_hip_batch_merger_t, slot_b) == 4 && offsetof(nbody_hip_batch_merger_t, id_a) == 8 &&
              offsetof(nbody_hip_batch_merger_t, id_b) == 12 && offsetof(nbody_hip_batch_merger_t, moved_from) == 16 &&
              offsetof(nbody_hip_batch_merger_t, contact_tick) == 20 && offsetof(nbody_hip_batch_merger_t, contact_macro) == 24 &&
              offsetof(nbody_hip_batch_merger_t, contact_d2) == 32 && offsetof(nbody_hip_batch_merger_t, radius) == 36 &&
              offsetof(nbody_hip_batch_merger_t, mass) == 40 && offsetof(nbody_hip_batch_merger_t, delta_ke) == 48 &&
              offsetof(nbody_hip_batch_merger_t, delta_pe) == 56, "nbody_hip_batch_merger_t is a fixed 64-byte entry");
constexpr int kMergerStateWords = (int)(sizeof(nbody_hip_batch_merger_state_t) / sizeof(unsigned int));

struct BatchMergeArgs {
  ResidentArrays p;                        // the state of the whole ensemble; posm / vel / plo: the pack of the priming
  float* mass;                             // (p.mass is read-only)
  BatchSystem* sys;                        // n is the live count: written here
  const unsigned int* status;              // [B]
  nbody_hip_batch_event_t* events;         // [B]
  float* radii;                            // [bodies]
  unsigned int* ids;                       // [bodies]
  nbody_hip_batch_merger_state_t* mstate;  // [B]
  nbody_hip_batch_merger_t* log;           // [bodies]: system s from its first body
  unsigned int* mark;                      // [B]
  float G, eps2;
};

// ids 0 .. n-1, an empty log, the live counts back to the layout's n, no marks (the priming, before its sweep reads the
// counts; the first configuration of a handle): one thread per body of the layout
__global__ __launch_bounds__(kBlock) void batch_mergers_clear_kernel(
    const int* __restrict__ body_system, const unsigned long long* __restrict__ offsets, BatchSystem* __restrict__ sys,
    int n_total, unsigned int* __restrict__ ids, nbody_hip_batch_merger_t* __restrict__ log,
    nbody_hip_batch_merger_state_t* __restrict__ mstate, unsigned int* __restrict__ mark) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_total) return;
  const int s = body_system[i];
  const unsigned long long first = offsets[s];
  const unsigned int n0 = (unsigned int)(offsets[s + 1] - first), k = (unsigned int)((unsigned long long)i - first);
  ids[i] = k;
  nbody_hip_batch_merger_t e;
  e.slot_a = e.slot_b = e.id_a = e.id_b = e.moved_from = e.contact_tick = 0u;
  e.contact_macro = 0ull;
  e.contact_d2 = e.radius = 0.f;
  e.mass = e.delta_ke = e.delta_pe = 0.0;
  log[i] = e;
  if (k == 0u) {
    sys[s].n = (int)n0;
    nbody_hip_batch_merger_state_t m;
    m.n_live = n0;
    m.n_mergers = m.flags = 0u;
    for (int c = 0; c < 5; c++) m.reserved[c] = 0u;
    mstate[s] = m;
    mark[s] = 0u;
  }
}

// The merge: grid = B workgroups of 256 threads, workgroup s on system s.  A system that is not concerned leaves at once
// (uniform) having written nothing.  Else: the two bodies and the merged one in registers, alike in every thread; the sum
// of the potential delta over the other live bodies in the model's fixed order (stride 256, shuffles at 32 .. 1, the four
// waves in rising order); behind ONE barrier -- every read of the old state is done -- thread 0 stores the merged body,
// moves the last live body into the gap, kills the last slot, writes the log entry, the state, the event record, the live
// count and the mark; behind a second barrier the workgroup packs the n - 1 live bodies as batch_pack_kernel does.  Every
// index is below the live count n the kernel read; no atomics; both barriers under uniform conditions.
template <bool EXT>
__global__ __launch_bounds__(kBlock) void batch_merge_kernel(const BatchMergeArgs A) {
  constexpr int kWaves = kBlock / kWave;
  __shared__ double wsum[kWaves];
  const int tid = threadIdx.x, sidx = blockIdx.x;
  const nbody_hip_batch_event_t ev = A.events[sidx];
  const unsigned int stopped = (unsigned int)uniform_i((int)ev.stopped);
  const unsigned int status = (unsigned int)uniform_i((int)A.status[sidx]);
  if (!merger_concerned(stopped, status)) return;  // (uniform) nothing of the system is touched
  const BatchSystem w = A.sys[sidx];
  const int first = uniform_i(w.first), n = uniform_i(w.n);
  const MergerSlots sl = merger_slots((unsigned int)uniform_i((int)ev.contact_i), (unsigned int)uniform_i((int)ev.contact_j),
                                      (unsigned int)n);
  if (!sl.valid) {  // (uniform) the system stays stopped
    if (tid == 0) A.mstate[sidx].flags |= NBODY_HIP_BATCH_MERGER_BAD_RECORD;
    return;
  }
  const int lo = (int)sl.lo, hi = (int)sl.hi, last = n - 1;  // 0 <= lo < hi <= last
  ResidentArrays P{};
  P.d = HermiteArrays{A.p.d.x + first,  A.p.d.y + first,  A.p.d.z + first,  A.p.d.vx + first,  A.p.d.vy + first,
                      A.p.d.vz + first, A.p.d.ax + first, A.p.d.ay + first, A.p.d.az + first, nullptr, nullptr, nullptr};
  if constexpr (EXT)
    P.lo = HermiteLo{A.p.lo.x + first,  A.p.lo.y + first,  A.p.lo.z + first,
                     A.p.lo.vx + first, A.p.lo.vy + first, A.p.lo.vz + first};
  P.mass = A.p.mass + first;
  float* const mass = A.mass + first;
  float* const radii = A.radii + first;
  unsigned int* const ids = A.ids + first;

  const DiagBody a = outcome_load<EXT>(P, lo), b = outcome_load<EXT>(P, hi);
  const MergerBody mb = merger_merge(a, b, EXT);
  const DiagBody mg = merger_stored(mb);
  const double eps2 = (double)A.eps2;
  double others = 0.0;
  for (int k = tid; k < n; k += kBlock)
    if (k != lo && k != hi) others += merger_pair_delta(mg, a, b, outcome_load<EXT>(P, k), eps2);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) others += __shfl_down(others, off, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = others;
  __syncthreads();  // every read of the old state is done; the waves' sums are in LDS
  if (tid == 0) {
    others = wsum[0];
#pragma unroll
    for (int k = 1; k < kWaves; k++) others += wsum[k];
    nbody_hip_batch_merger_t e;
    e.slot_a = sl.lo;
    e.slot_b = sl.hi;
    e.id_a = ids[lo];
    e.id_b = ids[hi];
    e.moved_from = sl.moved_from;
    e.contact_tick = ev.contact_tick;
    e.contact_macro = ev.contact_macro;
    e.contact_d2 = ev.contact_d2;
    e.radius = merger_radius(radii[lo], radii[hi]);
    e.mass = mb.M;
    e.delta_ke = merger_delta_ke(mg, a, b);
    e.delta_pe = merger_delta_pe(others, a, b, (double)A.G, eps2);
    // the merged body into lo (the id of lo stays)
    P.d.x[lo] = mb.x.hi;   P.d.y[lo] = mb.y.hi;   P.d.z[lo] = mb.z.hi;
    P.d.vx[lo] = mb.vx.hi; P.d.vy[lo] = mb.vy.hi; P.d.vz[lo] = mb.vz.hi;
    if constexpr (EXT) {
      P.lo.x[lo] = mb.x.lo;   P.lo.y[lo] = mb.y.lo;   P.lo.z[lo] = mb.z.lo;
      P.lo.vx[lo] = mb.vx.lo; P.lo.vy[lo] = mb.vy.lo; P.lo.vz[lo] = mb.vz.lo;
    }
    mass[lo] = mb.mass;
    radii[lo] = e.radius;
    if (hi != last) {  // the last live body closes the gap
      P.d.x[hi] = P.d.x[last];   P.d.y[hi] = P.d.y[last];   P.d.z[hi] = P.d.z[last];
      P.d.vx[hi] = P.d.vx[last]; P.d.vy[hi] = P.d.vy[last]; P.d.vz[hi] = P.d.vz[last];
      if constexpr (EXT) {
        P.lo.x[hi] = P.lo.x[last];   P.lo.y[hi] = P.lo.y[last];   P.lo.z[hi] = P.lo.z[last];
        P.lo.vx[hi] = P.lo.vx[last]; P.lo.vy[hi] = P.lo.vy[last]; P.lo.vz[hi] = P.lo.vz[last];
      }
      mass[hi] = mass[last];
      radii[hi] = radii[last];
      ids[hi] = ids[last];
    }
    // the last slot dies; its position stays
    P.d.vx[last] = P.d.vy[last] = P.d.vz[last] = 0.f;
    P.d.ax[last] = P.d.ay[last] = P.d.az[last] = 0.f;
    if constexpr (EXT) {
      P.lo.x[last] = P.lo.y[last] = P.lo.z[last] = 0.f;
      P.lo.vx[last] = P.lo.vy[last] = P.lo.vz[last] = 0.f;
    }
    mass[last] = 0.f;
    radii[last] = 0.f;
    ids[last] = kMergerNone;
    // the log, the state, the live count, the event record, the mark
    nbody_hip_batch_merger_state_t* const ms = A.mstate + sidx;
    const unsigned int nm = ms->n_mergers;  // n_mergers + n_live is the layout's n: the entry lies inside the system's range
    A.log[(size_t)first + nm] = e;
    ms->n_mergers = nm + 1u;
    ms->n_live = (unsigned int)last;
    A.sys[sidx].n = last;
    // (field by field: a copy of ev kept twelve bytes of it in a per-thread array, which the compiler moved to 3 KB of LDS)
    nbody_hip_batch_event_t r;
    r.stopped = 0u;
    r.reserved = 0u;
    r.macro_steps_done = ev.macro_steps_done;  // (kept)
    r.closest_d2 = r.contact_d2 = __builtin_inff();
    r.closest_i = r.closest_j = r.contact_i = r.contact_j = 0xffffffffu;
    r.closest_tick = r.contact_tick = 0u;
    r.closest_macro = r.contact_macro = 0ull;
    A.events[sidx] = r;
    A.mark[sidx] = 1u;
  }
  __syncthreads();  // thread 0's stores of this workgroup are visible
  // the pack of the priming for the n - 1 live bodies (batch_pack_kernel)
  float4* const posm = A.p.posm + first;
  float4* const vel = A.p.vel + first;
  float4* const plo = A.p.plo + first;  // (extended only)
  for (int k = tid; k < last; k += kBlock) {
    posm[k] = make_float4(P.d.x[k], P.d.y[k], P.d.z[k], P.mass[k]);
    vel[k] = make_float4(P.d.vx[k], P.d.vy[k], P.d.vz[k], 0.f);
    if constexpr (EXT) plo[k] = make_float4(P.lo.x[k], P.lo.y[k], P.lo.z[k], 0.f);
  }
}

// The priming's sweep for the marked systems: batch_prime_sweep_kernel, statement for statement, behind two uniform exits
// -- the system is not marked; the item lies outside the tiles and target blocks of the LIVE count (the items are the
// layout's, made for the n of the priming, and a smaller n_pad moves the rows) -- so a merged system gets the rows a fresh
// system of n - 1 bodies gets.
template <bool GUARD, bool EXT>
__global__ __launch_bounds__(kBlock) void batch_reprime_sweep_kernel(const BatchPrimeItem* __restrict__ items,
                                                                     const BatchSystem* __restrict__ sys,
                                                                     const unsigned int* __restrict__ mark,
                                                                     const float4* __restrict__ posm_all,
                                                                     const float4* __restrict__ vel_all,
                                                                     const float4* __restrict__ plo_all,
                                                                     float4* __restrict__ pa_all,
                                                                     float4* __restrict__ pj_all, float eps2) {
  const BatchPrimeItem it = items[blockIdx.x];
  const int s = uniform_i(it.system), tblock = uniform_i(it.tblock), tile = uniform_i(it.tile);
  if (uniform_i((int)mark[s]) == 0) return;  // (uniform)
  const BatchSystem w = sys[s];
  // (uniform) no such item in a system of n bodies
  if (tblock * kPrimeTargets >= uniform_i(w.n) || tile * TS >= uniform_i(w.n)) return;
#include "hermite_batch_prime_sweep.inc"
}

// The priming's finalize for the marked systems: one workgroup per system, the expressions of
// batch_prime_finalize_kernel for each live body; the counters, the status word and the step counts are NOT reset.  The
// workgroup is the only reader of its system's mark in this launch and clears it behind a barrier (uniform condition).
__global__ __launch_bounds__(kBlock) void batch_reprime_finalize_kernel(
    const BatchSystem* __restrict__ sys, unsigned int* __restrict__ mark, const float* __restrict__ dt_max,
    const float4* __restrict__ pa_all, const float4* __restrict__ pj_all, float G, float eta_s, int L, float* __restrict__ ax,
    float* __restrict__ ay, float* __restrict__ az, float4* __restrict__ jerk, int* __restrict__ level,
    unsigned int* __restrict__ tick, float* __restrict__ want) {
  const int s = blockIdx.x;
  if (uniform_i((int)mark[s]) == 0) return;  // (uniform)
  const BatchSystem w = sys[s];
  const int first = uniform_i(w.first), n = uniform_i(w.n);
  const int tiles = (n + TS - 1) / TS;
  const int n_pad = (n + kPrimeTargets - 1) / kPrimeTargets * kPrimeTargets;
  const float4* pa = pa_all + uniform_u64(w.prime_row_off);
  const float4* pj = pj_all + uniform_u64(w.prime_row_off);
  const float dt = __int_as_float(uniform_i(__float_as_int(dt_max[s])));
  for (int k = threadIdx.x; k < n; k += kBlock) {
    const int i = first + k;
#include "hermite_batch_prime_finalize.inc"
  }
  __syncthreads();  // every thread has read the mark
  if (threadIdx.x == 0) mark[s] = 0u;
}

}  // namespace nbh

using namespace nbh;

constexpr int kStoreSnapshot = kBatchFeatures, kBatchStores = kBatchFeatures + 1;  // the features, then the snapshot's scratch

// (the fields every Hermite handle has, the per-body state jerk / level / tick / want, the parameters par and what the
// entry points do with them: hermite_handle.h)
struct nbody_hip_hermite_batch : BlockHandleCore {
  static constexpr const char *kNoun = "block-step Hermite ensemble", *kOwner = "ensemble's";
  nbody_hip_hermite_batch(nbody_hip_ctx* c, size_t n, size_t systems) : BlockHandleCore(c, n, kNoun, kOwner), max_systems(systems) {}
  size_t max_systems;
  // device state by capacity behind the per-body arrays, in the same allocation, made at the first layout
  int* body_system = nullptr;            // the system of body i
  float4* posm = nullptr;                // {xp, m}, {vp, 0}, {xp_lo, 0}: 3 max_particles float4
  BatchPrimeItem* items = nullptr;       // at most one item per body (ceil(n/256) ceil(n/512) <= n)
  BatchSystem* sys = nullptr;
  float* dt_dev = nullptr;
  unsigned int* status = nullptr;
  BatchState* state = nullptr;
  unsigned long long* counters = nullptr;
  unsigned long long* offsets_dev = nullptr;  // the layout's offsets, for the diagnostics: max_systems + 1 entries
  // rows, by layout: grown at set_layout, never during an advance
  float4* rows = nullptr;
  size_t rows_held = 0;                  // float4
  // pinned staging of dt_max and the event of its last upload
  float* dt_pinned = nullptr;
  hipEvent_t dt_uploaded = nullptr;
  // the layout
  std::vector<size_t> offsets;           // B + 1 entries; empty: no layout yet
  size_t n_items = 0, adv_rows = 0, prime_rows = 0;
  // what is configured, and whether an advance or a merger pass may be recorded since the priming (hermite_batch_plan.h)
  BatchFeatures feat;
  // the features' device memory by capacity, one allocation each, made by the first configuration (the snapshot's scratch:
  // by its first call) and kept to the end: the table kBatchStore below
  void* feat_mem[kBatchStores] = {};
  // the events: radii [max_particles], limits and records [max_systems]
  float* radii = nullptr;
  unsigned long long* limits = nullptr;
  nbody_hip_batch_event_t* events = nullptr;
  // the outcomes (section 4.19): escape radii and records [max_systems]
  float* r_esc = nullptr;
  nbody_hip_batch_outcome_t* outcomes = nullptr;
  // the hierarchies (section 4.20): separation radii and records [max_systems], node tables [2 max_particles]; the
  // snapshot's scratch records and tables
  float* r_sep = nullptr;
  nbody_hip_batch_hierarchy_t* hier = nullptr;
  nbody_hip_batch_node_t* hier_nodes = nullptr;
  nbody_hip_batch_hierarchy_t* snap_rec = nullptr;
  nbody_hip_batch_node_t* snap_nodes = nullptr;
  // the mergers (section 4.21): ids and log [max_particles], state and marks [max_systems]
  unsigned int* ids = nullptr;
  nbody_hip_batch_merger_t* mrg_log = nullptr;
  nbody_hip_batch_merger_state_t* mrg_state = nullptr;
  unsigned int* mrg_mark = nullptr;
};

// ---- the features' device memory -------------------------------------------------------------
// One entry per allocation: what it holds, and how its records are put to "none".  clear takes B records and n bodies:
// the layout's at a priming, which clears every feature that has ever been allocated whether it is on or not; by capacity
// (the mergers: the layout's bodies) at the first configuration, because a priming that came before the buffers could not
// clear them.
typedef nbody_hip_hermite_batch Batch;
struct BatchFeatureStore {
  void (*carve)(Carve&, Batch*, size_t n, size_t B);                 // n: max_particles, B: max_systems
  int (*clear)(Batch*, size_t B, size_t n, hipStream_t st);           // (null: nothing to clear)
};
static dim3 batch_blocks(size_t n) { return dim3((unsigned int)((n + kBlock - 1) / kBlock)); }
template <class T>
static int batch_records_clear(void (*kernel)(T*, int), T* rec, size_t B, hipStream_t st) {
  hipLaunchKernelGGL(kernel, batch_blocks(B), dim3(kBlock), 0, st, rec, (int)B);
  NBH_LAUNCH_CHECK();
  return NBODY_HIP_OK;
}
static const BatchFeatureStore kBatchStore[kBatchStores] = {
    // events
    {[](Carve& c, Batch* h, size_t n, size_t B) { c.add(&h->radii, n); c.add(&h->limits, B); c.add(&h->events, B); },
     [](Batch* h, size_t B, size_t, hipStream_t st) { return batch_records_clear(batch_events_clear_kernel, h->events, B, st); }},
    // outcomes
    {[](Carve& c, Batch* h, size_t, size_t B) { c.add(&h->r_esc, B); c.add(&h->outcomes, B); },
     [](Batch* h, size_t B, size_t, hipStream_t st) { return batch_records_clear(batch_outcomes_clear_kernel, h->outcomes, B, st); }},
    // hierarchies: the records, then the 2 n node slots
    {[](Carve& c, Batch* h, size_t n, size_t B) { c.add(&h->r_sep, B); c.add(&h->hier, B); c.add(&h->hier_nodes, 2 * n); },
     [](Batch* h, size_t B, size_t n, hipStream_t st) {
       if (int rc = batch_records_clear(batch_hierarchy_clear_kernel, h->hier, B, st)) return rc;
       NBH_HIP(hipMemsetAsync(h->hier_nodes, 0, 2 * n * sizeof(nbody_hip_batch_node_t), st));
       return (int)NBODY_HIP_OK;
     }},
    // mergers: ids, log, state, marks and the LIVE COUNTS of the layout's n bodies (n is the layout's, never the capacity)
    {[](Carve& c, Batch* h, size_t n, size_t B) {
       c.add(&h->ids, n); c.add(&h->mrg_log, n); c.add(&h->mrg_state, B); c.add(&h->mrg_mark, B);
     },
     [](Batch* h, size_t, size_t n, hipStream_t st) {
       hipLaunchKernelGGL(batch_mergers_clear_kernel, batch_blocks(n), dim3(kBlock), 0, st, h->body_system, h->offsets_dev,
                          h->sys, (int)n, h->ids, h->mrg_log, h->mrg_state, h->mrg_mark);
       NBH_LAUNCH_CHECK();
       return (int)NBODY_HIP_OK;
     }},
    // the snapshot's scratch: written whole by every call
    {[](Carve& c, Batch* h, size_t n, size_t B) { c.add(&h->snap_rec, B); c.add(&h->snap_nodes, 2 * n); }, nullptr},
};

// the allocation of entry `which`, made once (the device is set); *fresh gains its bit when this call made it
static int batch_feature_reserve(nbody_hip_hermite_batch* h, int which, unsigned int* fresh) {
  if (h->feat_mem[which]) return NBODY_HIP_OK;
  Carve c;
  kBatchStore[which].carve(c, h, h->max_particles, h->max_systems);
  NBH_HIP(hipMalloc(&h->feat_mem[which], c.total()));
  c.place(h->feat_mem[which]);
  *fresh |= 1u << which;
  return NBODY_HIP_OK;
}
// the entries of the bit set `which` to "none", in the table's order
static int batch_features_clear(nbody_hip_hermite_batch* h, unsigned int which, size_t B, size_t n, hipStream_t st) {
  for (int f = 0; f < kBatchStores; f++)
    if ((which >> f & 1u) != 0u && kBatchStore[f].clear)
      if (int rc = kBatchStore[f].clear(h, B, n, st)) return rc;
  return NBODY_HIP_OK;
}
// the entries that have ever been allocated
static unsigned int batch_features_held(const nbody_hip_hermite_batch* h) {
  unsigned int held = 0u;
  for (int f = 0; f < kBatchStores; f++) held |= h->feat_mem[f] ? 1u << f : 0u;
  return held;
}

// one allocation, made at the first layout: the per-body arrays, then (256-byte aligned, in this order) what the
// layout and the per-system words need
static int batch_reserve(nbody_hip_hermite_batch* h) {
  if (h->mem) return NBODY_HIP_OK;
  const size_t n = h->max_particles, B = h->max_systems;
  Carve c;
  block_carve_bodies(c, h);
  c.add(&h->body_system, n);
  c.add(&h->posm, 3 * n);
  c.add(&h->items, n);
  c.add(&h->sys, B);
  c.add(&h->dt_dev, B);
  c.add(&h->status, B);
  c.add(&h->state, B);
  c.add(&h->counters, B * kCounters);
  c.add(&h->offsets_dev, B + 1);
  NBH_HIP(hipMalloc(&h->mem, c.total()));
  c.place(h->mem);
  NBH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->dt_pinned), B * sizeof(float), hipHostMallocDefault));
  NBH_HIP(hipEventCreateWithFlags(&h->dt_uploaded, hipEventDisableTiming));
  return NBODY_HIP_OK;
}

// The rules of a layout (include/nbody_hip.h; hermite_batch_layout.h): plain host arithmetic, no device.
static int batch_check_layout(const nbody_hip_hermite_batch* h, const size_t* offsets, size_t n_systems) {
  char msg[256];
  const int rc = batch_layout_check(offsets, n_systems, h->max_systems, h->max_particles, msg, sizeof(msg));
  if (rc == 0) return NBODY_HIP_OK;
  return NBH_FAIL(rc == 1 ? NBODY_HIP_ERR_STATE : NBODY_HIP_ERR_VALIDATION, "%s", msg);
}

extern "C" int nbody_hip_hermite_batch_create(nbody_hip_ctx* ctx, size_t max_particles_total, size_t max_systems,
                                              nbody_hip_hermite_batch** out) {
  if (int rc = handle_create_check(ctx, max_particles_total, out)) return rc;
  if (max_systems == 0 || max_systems > max_particles_total)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "max_systems must be in [1, %zu], got %zu", max_particles_total, max_systems);
  *out = new nbody_hip_hermite_batch(ctx, max_particles_total, max_systems);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_destroy(nbody_hip_hermite_batch* h) {
  if (!h) return NBODY_HIP_OK;
  NBH_DESTROY_BEGIN
  if (h->mem || h->lo_mem || h->rows) {
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    if (h->mem) (void)hipFree(h->mem);
    if (h->lo_mem) (void)hipFree(h->lo_mem);
    if (h->rows) (void)hipFree(h->rows);
    for (void* m : h->feat_mem)
      if (m) (void)hipFree(m);
    if (h->dt_pinned) (void)hipHostFree(h->dt_pinned);
    if (h->dt_uploaded) (void)hipEventDestroy(h->dt_uploaded);
  }
  delete h;
  NBH_DESTROY_END
}

extern "C" int nbody_hip_hermite_batch_set_params(nbody_hip_hermite_batch* h, float eta, float eta_start, int max_level) {
  if (int rc = handle_null(h)) return rc;
  return h->par.set(eta, eta_start, max_level);
}

extern "C" int nbody_hip_hermite_batch_set_precision(nbody_hip_hermite_batch* h, int mode) {
  if (int rc = handle_precision_check(h, mode)) return rc;
  if (mode == h->precision) return NBODY_HIP_OK;
  return handle_precision_switch(h, mode);
}

extern "C" int nbody_hip_hermite_batch_get_precision(nbody_hip_hermite_batch* h, int* mode) {
  return handle_get_precision(h, mode);
}

extern "C" int nbody_hip_hermite_batch_set_layout(nbody_hip_hermite_batch* h, const size_t* offsets_host,
                                                  size_t n_systems) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "an ensemble layout");
  if (int rc = batch_check_layout(h, offsets_host, n_systems)) return rc;
  h->primed = false;  // (a new layout unprimes, whatever follows)
  h->feat.reset();    // (... and drops every configuration -- the radii are per body of the old layout -- but no allocation)
  h->offsets.clear();
  // the per-system words, the system of every body and the work items of the priming sweep
  const BatchLayout lay = batch_layout_build(offsets_host, n_systems);
  const size_t adv = lay.adv_rows, prime = lay.prime_rows;
  NBH_HIP(hipSetDevice(h->ctx->device));
  if (int rc = batch_reserve(h)) return rc;
  const size_t rows_wanted = 2 * (prime > adv ? prime : adv);  // pa and pj; the priming's are the larger
  hipStream_t st = h->ctx->stream;
  if (rows_wanted > h->rows_held) {
    NBH_HIP(hipStreamSynchronize(st));  // (launches still queued use the old rows)
    if (h->rows) NBH_HIP(hipFree(h->rows));
    h->rows = nullptr;
    h->rows_held = 0;
    NBH_HIP(hipMalloc(reinterpret_cast<void**>(&h->rows), rows_wanted * sizeof(float4)));
    h->rows_held = rows_wanted;
  }
  NBH_HIP(hipMemcpyAsync(h->sys, lay.sys.data(), lay.sys.size() * sizeof(BatchSystem), hipMemcpyHostToDevice, st));
  NBH_HIP(hipMemcpyAsync(h->body_system, lay.body_system.data(), lay.body_system.size() * sizeof(int), hipMemcpyHostToDevice, st));
  NBH_HIP(hipMemcpyAsync(h->items, lay.items.data(), lay.items.size() * sizeof(BatchPrimeItem), hipMemcpyHostToDevice, st));
  const std::vector<unsigned long long> off64(offsets_host, offsets_host + n_systems + 1);
  NBH_HIP(hipMemcpyAsync(h->offsets_dev, off64.data(), off64.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  NBH_HIP(hipStreamSynchronize(st));  // (the vectors go away)
  h->offsets.assign(offsets_host, offsets_host + n_systems + 1);
  h->n_items = lay.items.size();
  h->adv_rows = adv;
  h->prime_rows = prime;
  return NBODY_HIP_OK;
}

static int batch_check_data(nbody_hip_hermite_batch* h, const nbody_particle_data* d) {
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (h->offsets.empty()) return NBH_FAIL(NBODY_HIP_ERR_STATE, "the ensemble has no layout: call set_layout first");
  if (d->count != h->offsets.back())
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle count %zu differs from the layout's %zu bodies in %zu systems",
                    d->count, h->offsets.back(), h->offsets.size() - 1);
  return NBODY_HIP_OK;
}

// an advance, a pass or a diagnostic of other arrays than the primed ones
static int batch_check_primed_arrays(const nbody_hip_hermite_batch* h, const nbody_particle_data* d) {
  if (d->count != h->count || d->pos_x != h->pos_x)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "the particle count or the arrays differ from the primed ones (%zu bodies): prime "
                    "again", h->count);
  return NBODY_HIP_OK;
}
// a read-out with one record per system
static int batch_check_systems(const nbody_hip_hermite_batch* h, size_t n_systems) {
  if (n_systems != h->offsets.size() - 1)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the layout has %zu systems, got room for %zu records", h->offsets.size() - 1,
                    n_systems);
  return NBODY_HIP_OK;
}
// the opening of a read-out: a handle, no recording, somewhere to write, primed
static int batch_readout_begin(const nbody_hip_hermite_batch* h, const char* what, const void* out) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, what);
  if (!out) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  if (!h->primed) return handle_not_primed(h);
  return NBODY_HIP_OK;
}
// the opening of a configuration call: a handle, no recording, a layout, known flags
static int batch_set_begin(const nbody_hip_hermite_batch* h, const char* what, int flags, int known, const char* noun,
                           const char* names) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, what);
  if (h->offsets.empty()) return NBH_FAIL(NBODY_HIP_ERR_STATE, "the ensemble has no layout: call set_layout first");
  char msg[kBatchMsg];
  if (batch_unknown_flags(flags, known, noun, names, msg, sizeof(msg))) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", msg);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_prime(nbody_hip_hermite_batch* h, nbody_particle_data* d, float G, float eps,
                                             const float* dt_max_host) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a block-step Hermite ensemble priming");
  if (int rc = batch_check_data(h, d)) return rc;
  if (!dt_max_host) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null dt_max array");
  const size_t B = h->offsets.size() - 1;
  for (size_t s = 0; s < B; s++)
    if (int rc = check_dt(dt_max_host[s], s)) return rc;
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  h->primed = false;
  hipStream_t st = h->ctx->stream;
  NBH_HIP(hipEventSynchronize(h->dt_uploaded));  // (the staging buffer of an earlier priming)
  memcpy(h->dt_pinned, dt_max_host, B * sizeof(float));
  NBH_HIP(hipMemcpyAsync(h->dt_dev, h->dt_pinned, B * sizeof(float), hipMemcpyHostToDevice, st));
  NBH_HIP(hipEventRecord(h->dt_uploaded, st));
  h->par.take();
  const int n = (int)d->count;
  const int blocks = (n + kBlock - 1) / kBlock;
  const bool ext = h->precision == 1;
  const float eps2 = eps * eps;
  const bool guard = direct_guard(eps2);  // (as the single-system forms)
  float4 *posm = h->posm, *vel = posm + h->max_particles, *plo = vel + h->max_particles;
  float4 *pa = h->rows, *pj = h->rows + h->prime_rows;
  // whatever has ever been configured starts over, on or not.  The mergers first: the sweep reads the live counts
  const unsigned int held = batch_features_held(h), mergers = 1u << kFeatMergers;
  if (int rc = batch_features_clear(h, held & mergers, B, d->count, st)) return rc;
  with_flag(ext, [&](auto EX) {
    hipLaunchKernelGGL((batch_pack_kernel<decltype(EX)::value>), dim3(blocks), dim3(kBlock), 0, st, d->pos_x, d->pos_y,
                       d->pos_z, d->vel_x, d->vel_y, d->vel_z, d->mass, h->lo, n, posm, vel, plo);
  });
  NBH_LAUNCH_CHECK();
  with_flags(guard, ext, [&](auto GD, auto EX) {
    hipLaunchKernelGGL((batch_prime_sweep_kernel<decltype(GD)::value, decltype(EX)::value>), dim3((unsigned int)h->n_items),
                       dim3(kBlock), 0, st, h->items, h->sys, posm, vel, plo, pa, pj, eps2);
  });
  NBH_LAUNCH_CHECK();
  hipLaunchKernelGGL(batch_prime_finalize_kernel, dim3(blocks), dim3(kBlock), 0, st, h->body_system, h->sys, h->dt_dev, pa,
                     pj, n, G, h->par.eta_start, h->par.L, d->acc_x, d->acc_y, d->acc_z, h->jerk, h->level, h->tick,
                     h->want, h->status, h->state, h->counters);
  NBH_LAUNCH_CHECK();
  // ... then, behind the finalize, the event, outcome and hierarchy records and the node tables
  if (int rc = batch_features_clear(h, held & ~mergers, B, d->count, st)) return rc;
  handle_primed_for(h, d, G, eps);
  h->feat.ran_eagerly = false;
  h->feat.mrg_ran_eagerly = false;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_invalidate(nbody_hip_hermite_batch* h) {
  if (int rc = handle_null(h)) return rc;
  return handle_invalidate(h);
}

extern "C" int nbody_hip_hermite_batch_advance(nbody_hip_hermite_batch* h, nbody_particle_data* d, int macro_steps) {
  if (int rc = handle_null(h)) return rc;
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (macro_steps < 1) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "macro_steps must be at least 1");
  if (!h->primed) return handle_not_primed(h);
  if (int rc = batch_check_primed_arrays(h, d)) return rc;
  nbody_hip_ctx* ctx = h->ctx;
  if (ctx->capturing && !h->feat.ran_eagerly) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "a block-step Hermite ensemble advance cannot be recorded into a step graph before "
                    "it has run once eagerly with these parameters");
  }
  NBH_HIP(hipSetDevice(ctx->device));
  const BatchArgs A{resident_arrays(h, d, h->posm, h->max_particles, h->rows, h->rows + h->adv_rows), h->sys, h->dt_dev,
                    h->status, h->state, h->counters, h->par.L, h->G, h->eps * h->eps, h->par.eta};
  // the kernel form and what its argument blocks hold (hermite_batch_plan.h): E with the tracked sweep's radii and budgets
  // (section 4.15) or with the records alone, O for the escape test (4.19), H for the examination (4.20)
  const BatchFeatures& f = h->feat;
  const BatchAdvancePlan plan = batch_advance_plan(f);
  BatchEventArgs E{};
  if (plan.E == BatchEventBlock::Full) E = BatchEventArgs{h->radii, h->limits, h->events, f.flags[kFeatEvents]};
  if (plan.E == BatchEventBlock::Records) E = BatchEventArgs{nullptr, nullptr, h->events, 0u};
  const BatchOutcomeArgs O = plan.O_full ? BatchOutcomeArgs{h->r_esc, h->outcomes, f.flags[kFeatOutcomes]} : BatchOutcomeArgs{};
  const BatchHierarchyArgs H = plan.H_full ? BatchHierarchyArgs{h->r_sep, h->hier, h->hier_nodes, f.kappa, f.flags[kFeatHierarchy]}
                                           : BatchHierarchyArgs{};
  const bool ext = h->precision == 1, guard = direct_guard(A.eps2);
  const dim3 grid((unsigned int)(h->offsets.size() - 1)), block(kResidentBlock);
  with_flags(ext, guard, [&](auto EX, auto GD) {
    with_flag(plan.track, [&](auto TR) {
      constexpr bool X = decltype(EX)::value, D = decltype(GD)::value, T = decltype(TR)::value;
      switch (plan.form) {
        case BatchForm::Resident:
          hipLaunchKernelGGL((batch_resident_kernel<X, D, T>), grid, block, 0, ctx->stream, A, E, macro_steps);
          break;
        case BatchForm::Outcomes:
          hipLaunchKernelGGL((batch_outcomes_kernel<X, D, T>), grid, block, 0, ctx->stream, A, E, O, macro_steps);
          break;
        case BatchForm::Hierarchy:
          hipLaunchKernelGGL((batch_hierarchy_kernel<X, D, T>), grid, block, 0, ctx->stream, A, E, O, H, macro_steps);
          break;
      }
    });
  });
  NBH_LAUNCH_CHECK();
  if (!ctx->capturing) h->feat.ran_eagerly = true;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_state(nbody_hip_hermite_batch* h, int* levels, unsigned int* ticks, float* want,
                                             nbody_float4* jerk) {
  return handle_block_state(h, levels, ticks, want, jerk);
}

extern "C" int nbody_hip_hermite_batch_info(nbody_hip_hermite_batch* h, long long system,
                                            nbody_hip_hermite_block_info_t* out) {
  if (int rc = handle_info_begin(h, out)) return rc;
  const long long B = (long long)h->offsets.size() - 1;
  if (system < -1 || (B >= 1 && system >= B) || (B < 1 && system >= 0))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "system must be -1 (the sums) or in [0, %lld), got %lld", B < 0 ? 0 : B, system);
  if (!h->primed) return NBODY_HIP_OK;
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  std::vector<unsigned int> status((size_t)B);
  const size_t s0 = system < 0 ? 0 : (size_t)system, ns = system < 0 ? (size_t)B : 1;
  std::vector<BatchState> state(ns);
  std::vector<unsigned long long> c(ns * kCounters);
  NBH_HIP(hipMemcpyAsync(status.data(), h->status, status.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipMemcpyAsync(state.data(), h->state + s0, ns * sizeof(BatchState), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipMemcpyAsync(c.data(), h->counters + s0 * kCounters, c.size() * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  for (size_t s = 0; s < (size_t)B; s++)
    if (status[s] != 0u) {
      h->primed = false;
      return NBH_FAIL(NBODY_HIP_ERR_STATE, "block-step schedule out of range (system %zu)", s);
    }
  for (size_t s = 0; s < ns; s++) {
    out->block_steps += state[s].block_steps;
    out->body_steps += state[s].body_steps;
    out->macro_steps += state[s].macro_steps;
    info_add_counters(out, &c[s * kCounters]);
  }
  if (system >= 0) out->last_n_active = state[0].last_n_active;  // (the sums: 0; current_tick is 0 at a boundary)
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_set_state_f64(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                     const double* pos_host, const double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "setting the extended state")) return rc;
  return handle_set_state(h, d, pos_host, vel_host);
}

extern "C" int nbody_hip_hermite_batch_get_state_f64(nbody_hip_hermite_batch* h, nbody_particle_data* d, double* pos_host,
                                                     double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "reading the extended state")) return rc;
  return handle_get_state(h, d, pos_host, vel_host);
}

// The diagnostics of every system of the layout (system_diag.hip): the handle's residuals in extended mode, the primed G
// and eps.  Asynchronous, allocates nothing, reads nothing back: capturable.
extern "C" int nbody_hip_hermite_batch_diagnostics(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                   nbody_hip_system_diag* out_device) {
  if (int rc = handle_null(h)) return rc;
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (!out_device) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  if (h->offsets.empty()) return NBH_FAIL(NBODY_HIP_ERR_STATE, "the ensemble has no layout: call set_layout first");
  if (!h->primed) return handle_not_primed(h);
  if (int rc = batch_check_primed_arrays(h, d)) return rc;
  const DiagLo lo{h->lo.x, h->lo.y, h->lo.z, h->lo.vx, h->lo.vy, h->lo.vz};
  // (a handle that has had mergers configured: the form with live counts, section 4.21)
  return system_diag_launch(h->ctx, d, h->precision == 1 ? &lo : nullptr, nullptr, nullptr, h->offsets_dev,
                            h->offsets.size() - 1, h->G, h->eps, out_device,
                            h->mrg_state ? &h->mrg_state->n_live : nullptr, kMergerStateWords);
}

// What the configuration calls of the events, the outcomes and the hierarchies do behind their checks.  Off: no device is
// set and no device memory touched.  On: the feature's memory and that of the events -- the stop words live in the event
// records -- each cleared if this call made it; the caller's arrays are uploaded (null: zeros) and have been read on return.
struct BatchUpload {
  void** to;  // the handle's pointer, set by the reserve
  const void* from_or_null;
  size_t bytes;
};
static int batch_feature_off(nbody_hip_hermite_batch* h, BatchFeature which) {
  h->feat.turn(which, false);
  return NBODY_HIP_OK;
}
static int batch_feature_set(nbody_hip_hermite_batch* h, BatchFeature which, const BatchUpload* up, int n_up, int flags,
                             float kappa) {
  NBH_HIP(hipSetDevice(h->ctx->device));
  unsigned int fresh = 0u;
  if (int rc = batch_feature_reserve(h, kFeatEvents, &fresh)) return rc;
  if (int rc = batch_feature_reserve(h, which, &fresh)) return rc;
  hipStream_t st = h->ctx->stream;
  for (int k = 0; k < n_up; k++)
    if (up[k].from_or_null)
      NBH_HIP(hipMemcpyAsync(*up[k].to, up[k].from_or_null, up[k].bytes, hipMemcpyHostToDevice, st));
    else
      NBH_HIP(hipMemsetAsync(*up[k].to, 0, up[k].bytes, st));
  if (int rc = batch_features_clear(h, fresh, h->max_systems, h->max_particles, st)) return rc;
  NBH_HIP(hipStreamSynchronize(st));  // (the caller's arrays have been read)
  h->feat.turn(which, true);          // (another kernel form: one eager advance before a recording)
  h->feat.flags[which] = (unsigned int)flags;
  if (which == kFeatHierarchy) h->feat.kappa = kappa;
  return NBODY_HIP_OK;
}

// ---- the events: configuration and read-out (include/nbody_hip_events.h) ---------------------------------------------
extern "C" int nbody_hip_hermite_batch_set_events(nbody_hip_hermite_batch* h, const float* radii_host_or_null,
                                                  const unsigned long long* limits_host_or_null, int flags) {
  if (int rc = batch_set_begin(h, "a configuration of the ensemble's events", flags,
                               NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST | NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT, "event",
                               "TRACK_CLOSEST 1, STOP_ON_CONTACT 2"))
    return rc;
  if ((flags & NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT) && !radii_host_or_null)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "STOP_ON_CONTACT needs radii: without them no pair is ever in contact");
  const size_t B = h->offsets.size() - 1, n = h->offsets.back();
  char msg[kBatchMsg];
  if (batch_bad_body_radii(radii_host_or_null, h->offsets.data(), B, msg, sizeof(msg)))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", msg);
  if (!radii_host_or_null && !limits_host_or_null && flags == 0) return batch_feature_off(h, kFeatEvents);  // the plain kernel
  const BatchUpload up[2] = {{reinterpret_cast<void**>(&h->radii), radii_host_or_null, n * sizeof(float)},
                             {reinterpret_cast<void**>(&h->limits), limits_host_or_null, B * sizeof(unsigned long long)}};
  return batch_feature_set(h, kFeatEvents, up, 2, flags, 0.f);
}

// status words, counters and records of all systems, after the stream's work; a handle that never had event memory:
// "none" records.  macro_steps_done comes from the state, whatever kernel form ran.
static int batch_events_read(nbody_hip_hermite_batch* h, std::vector<unsigned int>& status, std::vector<BatchState>& state,
                             std::vector<nbody_hip_batch_event_t>& ev) {
  const size_t B = h->offsets.size() - 1;
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  status.resize(B);
  state.resize(B);
  ev.resize(B);
  NBH_HIP(hipMemcpyAsync(status.data(), h->status, B * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipMemcpyAsync(state.data(), h->state, B * sizeof(BatchState), hipMemcpyDeviceToHost, st));
  if (h->events)
    NBH_HIP(hipMemcpyAsync(ev.data(), h->events, B * sizeof(nbody_hip_batch_event_t), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  for (size_t s = 0; s < B; s++) {
    if (!h->events) event_record_none(&ev[s]);
    ev[s].macro_steps_done = state[s].macro_steps;
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_events(nbody_hip_hermite_batch* h, nbody_hip_batch_event_t* out_host,
                                              size_t n_systems) {
  if (int rc = batch_readout_begin(h, "an event read-out", out_host)) return rc;
  if (int rc = batch_check_systems(h, n_systems)) return rc;
  std::vector<unsigned int> status;
  std::vector<BatchState> state;
  std::vector<nbody_hip_batch_event_t> ev;
  if (int rc = batch_events_read(h, status, state, ev)) return rc;
  memcpy(out_host, ev.data(), n_systems * sizeof(nbody_hip_batch_event_t));
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_batch_running(nbody_hip_hermite_batch* h, size_t* n_running) {
  if (int rc = batch_readout_begin(h, "an event read-out", n_running)) return rc;
  std::vector<unsigned int> status;
  std::vector<BatchState> state;
  std::vector<nbody_hip_batch_event_t> ev;
  if (int rc = batch_events_read(h, status, state, ev)) return rc;
  size_t running = 0;
  for (size_t s = 0; s < status.size(); s++) running += status[s] == 0u && ev[s].stopped == 0u;
  *n_running = running;
  return NBODY_HIP_OK;
}

// ---- the outcomes: configuration and read-out (include/nbody_hip_outcomes.h) -----------------------------------------
extern "C" int nbody_hip_batch_outcomes_set(nbody_hip_hermite_batch* h, const float* escape_radii_host_or_null, int flags) {
  if (int rc = batch_set_begin(h, "a configuration of the ensemble's outcomes", flags, NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE,
                               "outcome", "STOP_ON_ESCAPE 1"))
    return rc;
  char msg[kBatchMsg];
  bool positive = false;
  if (batch_bad_system_radii(escape_radii_host_or_null, h->offsets.data(), h->offsets.size() - 1, "escape", 0, &positive, msg,
                             sizeof(msg)))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", msg);
  if ((flags & NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE) && !positive)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "STOP_ON_ESCAPE needs an escape radius > 0: without one no body ever escapes");
  if (!escape_radii_host_or_null) return batch_feature_off(h, kFeatOutcomes);  // (flags == 0)
  const BatchUpload up{reinterpret_cast<void**>(&h->r_esc), escape_radii_host_or_null, (h->offsets.size() - 1) * sizeof(float)};
  return batch_feature_set(h, kFeatOutcomes, &up, 1, flags, 0.f);
}

extern "C" int nbody_hip_batch_outcomes_get(nbody_hip_hermite_batch* h, nbody_hip_batch_outcome_t* out_host,
                                            size_t n_systems) {
  if (int rc = batch_readout_begin(h, "an outcome read-out", out_host)) return rc;
  if (int rc = batch_check_systems(h, n_systems)) return rc;
  if (!h->outcomes) {
    for (size_t s = 0; s < n_systems; s++) outcome_record_none(&out_host[s]);
    return NBODY_HIP_OK;
  }
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  NBH_HIP(hipMemcpyAsync(out_host, h->outcomes, n_systems * sizeof(nbody_hip_batch_outcome_t), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  return NBODY_HIP_OK;
}

// ---- the hierarchies: configuration, read-out and snapshot (include/nbody_hip_hierarchy.h) ---------------------------
extern "C" int nbody_hip_batch_hierarchy_set(nbody_hip_hermite_batch* h, const float* sep_radii_host_or_null, float kappa,
                                             int flags) {
  if (int rc = batch_set_begin(h, "a configuration of the ensemble's hierarchies", flags,
                               NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED, "hierarchy", "STOP_ON_RESOLVED 1"))
    return rc;
  if (!(kappa >= 0.0f) || !finite_f(kappa))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the isolation factor kappa must be non-negative and finite, got %g",
                    (double)kappa);
  char msg[kBatchMsg];
  bool positive = false;
  if (batch_bad_system_radii(sep_radii_host_or_null, h->offsets.data(), h->offsets.size() - 1, "separation",
                             (size_t)NBODY_HIP_BATCH_HIERARCHY_MAX, &positive, msg, sizeof(msg)))
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", msg);
  if ((flags & NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED) && !positive)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "STOP_ON_RESOLVED needs a separation radius > 0: without one no system is "
                    "ever examined");
  if (!sep_radii_host_or_null) return batch_feature_off(h, kFeatHierarchy);  // (flags == 0)
  const BatchUpload up{reinterpret_cast<void**>(&h->r_sep), sep_radii_host_or_null, (h->offsets.size() - 1) * sizeof(float)};
  return batch_feature_set(h, kFeatHierarchy, &up, 1, flags, kappa);
}

// the count checks of the two read-outs
static int batch_hierarchy_counts(const nbody_hip_hermite_batch* h, size_t n_systems, size_t n_slots, bool nodes) {
  if (int rc = batch_check_systems(h, n_systems)) return rc;
  if (nodes && n_slots != 2 * h->offsets.back())
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the layout has %zu bodies and so %zu node slots, got room for %zu",
                    h->offsets.back(), 2 * h->offsets.back(), n_slots);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_batch_hierarchy_get(nbody_hip_hermite_batch* h, nbody_hip_batch_hierarchy_t* records_host,
                                             size_t n_systems, nbody_hip_batch_node_t* nodes_host_or_null, size_t n_slots) {
  if (int rc = batch_readout_begin(h, "a hierarchy read-out", records_host)) return rc;
  if (int rc = batch_hierarchy_counts(h, n_systems, n_slots, nodes_host_or_null != nullptr)) return rc;
  if (!h->hier) {
    for (size_t s = 0; s < n_systems; s++) hier_record_none(&records_host[s]);
    if (nodes_host_or_null) memset(nodes_host_or_null, 0, n_slots * sizeof(nbody_hip_batch_node_t));
    return NBODY_HIP_OK;
  }
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  NBH_HIP(hipMemcpyAsync(records_host, h->hier, n_systems * sizeof(nbody_hip_batch_hierarchy_t), hipMemcpyDeviceToHost, st));
  if (nodes_host_or_null)
    NBH_HIP(hipMemcpyAsync(nodes_host_or_null, h->hier_nodes, n_slots * sizeof(nbody_hip_batch_node_t),
                           hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_batch_hierarchy_snapshot(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                  nbody_hip_batch_hierarchy_t* records_host, size_t n_systems,
                                                  nbody_hip_batch_node_t* nodes_host, size_t n_slots) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a hierarchy snapshot");
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (!records_host || !nodes_host) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  if (!h->primed) return handle_not_primed(h);
  if (int rc = batch_check_primed_arrays(h, d)) return rc;
  if (int rc = batch_hierarchy_counts(h, n_systems, n_slots, true)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  unsigned int fresh = 0u;
  if (int rc = batch_feature_reserve(h, kStoreSnapshot, &fresh)) return rc;
  hipStream_t st = h->ctx->stream;
  NBH_HIP(hipMemsetAsync(h->snap_nodes, 0, n_slots * sizeof(nbody_hip_batch_node_t), st));
  const ResidentArrays P = resident_arrays(h, d, h->posm, h->max_particles, h->rows, h->rows + h->adv_rows);
  const bool on = h->feat.on[kFeatHierarchy];
  const float* r_sep = on ? h->r_sep : nullptr;
  const float kappa = on ? h->feat.kappa : 0.f;
  with_flag(h->precision == 1, [&](auto EX) {
    hipLaunchKernelGGL((batch_hierarchy_snapshot_kernel<decltype(EX)::value>), dim3((unsigned int)n_systems),
                       dim3(kResidentBlock), 0, st, P, h->sys, h->state, r_sep, kappa, h->G, h->snap_rec, h->snap_nodes);
  });
  NBH_LAUNCH_CHECK();
  NBH_HIP(hipMemcpyAsync(records_host, h->snap_rec, n_systems * sizeof(nbody_hip_batch_hierarchy_t), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipMemcpyAsync(nodes_host, h->snap_nodes, n_slots * sizeof(nbody_hip_batch_node_t), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  return NBODY_HIP_OK;
}

// ---- the mergers: configuration, the pass and the read-out (include/nbody_hip_mergers.h) ------------------------------
extern "C" int nbody_hip_batch_mergers_set(nbody_hip_hermite_batch* h, int flags) {
  if (int rc = batch_set_begin(h, "a configuration of the ensemble's mergers", flags, NBODY_HIP_BATCH_MERGERS_ON, "merger",
                               "MERGERS_ON 1"))
    return rc;
  if (flags != 0 && !h->feat_mem[kFeatMergers]) {
    // (no system of this layout has merged yet: the clear gives every system the layout's count; it is not waited for)
    NBH_HIP(hipSetDevice(h->ctx->device));
    unsigned int fresh = 0u;
    if (int rc = batch_feature_reserve(h, kFeatMergers, &fresh)) return rc;
    if (int rc = batch_features_clear(h, fresh, h->max_systems, h->offsets.back(), h->ctx->stream)) return rc;
  }
  h->feat.turn(kFeatMergers, flags != 0);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_batch_mergers_apply(nbody_hip_hermite_batch* h, nbody_particle_data* d) {
  if (int rc = handle_null(h)) return rc;
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (!h->primed) return handle_not_primed(h);
  if (!h->feat.on[kFeatMergers])
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "the ensemble's mergers are not configured: call mergers_set first");
  if (!h->feat.on[kFeatEvents] || (h->feat.flags[kFeatEvents] & NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT) == 0u)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "mergers need the events configured with radii and STOP_ON_CONTACT: without them no "
                    "system ever stops on a contact");
  if (int rc = batch_check_primed_arrays(h, d)) return rc;
  nbody_hip_ctx* ctx = h->ctx;
  if (ctx->capturing && !h->feat.mrg_ran_eagerly) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "a merger pass cannot be recorded into a step graph before it has run once eagerly "
                    "since the priming");
  }
  NBH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  float4 *pa = h->rows, *pj = h->rows + h->prime_rows;  // (the rows of the priming: nothing is kept in them between calls)
  const BatchMergeArgs A{resident_arrays(h, d, h->posm, h->max_particles, pa, pj), d->mass, h->sys, h->status, h->events,
                         h->radii, h->ids, h->mrg_state, h->mrg_log, h->mrg_mark, h->G, h->eps * h->eps};
  const bool ext = h->precision == 1, guard = direct_guard(A.eps2);  // (as the priming)
  const dim3 grid((unsigned int)(h->offsets.size() - 1));
  with_flag(ext, [&](auto EX) {
    hipLaunchKernelGGL((batch_merge_kernel<decltype(EX)::value>), grid, dim3(kBlock), 0, st, A);
  });
  NBH_LAUNCH_CHECK();
  with_flags(guard, ext, [&](auto GD, auto EX) {
    hipLaunchKernelGGL((batch_reprime_sweep_kernel<decltype(GD)::value, decltype(EX)::value>), dim3((unsigned int)h->n_items),
                       dim3(kBlock), 0, st, h->items, h->sys, h->mrg_mark, A.p.posm, A.p.vel, A.p.plo, pa, pj, A.eps2);
  });
  NBH_LAUNCH_CHECK();
  hipLaunchKernelGGL(batch_reprime_finalize_kernel, grid, dim3(kBlock), 0, st, h->sys, h->mrg_mark, h->dt_dev, pa, pj, h->G,
                     h->par.eta_start, h->par.L, d->acc_x, d->acc_y, d->acc_z, h->jerk, h->level, h->tick, h->want);
  NBH_LAUNCH_CHECK();
  if (!ctx->capturing) h->feat.mrg_ran_eagerly = true;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_batch_mergers_get(nbody_hip_hermite_batch* h, nbody_hip_batch_merger_state_t* state_host,
                                           size_t n_systems, nbody_hip_batch_merger_t* log_host_or_null,
                                           unsigned int* ids_host_or_null, size_t n_bodies) {
  if (int rc = batch_readout_begin(h, "a merger read-out", state_host)) return rc;
  if (int rc = batch_check_systems(h, n_systems)) return rc;
  if (n_bodies != h->offsets.back())
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the layout has %zu bodies, got room for %zu", h->offsets.back(), n_bodies);
  if (!h->feat_mem[kFeatMergers]) {  // never configured: nothing has merged
    memset(state_host, 0, n_systems * sizeof(*state_host));
    for (size_t s = 0; s < n_systems; s++) {
      state_host[s].n_live = (unsigned int)(h->offsets[s + 1] - h->offsets[s]);
      if (ids_host_or_null)
        for (size_t i = h->offsets[s]; i < h->offsets[s + 1]; i++) ids_host_or_null[i] = (unsigned int)(i - h->offsets[s]);
    }
    if (log_host_or_null) memset(log_host_or_null, 0, n_bodies * sizeof(*log_host_or_null));
    return NBODY_HIP_OK;
  }
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  NBH_HIP(hipMemcpyAsync(state_host, h->mrg_state, n_systems * sizeof(*state_host), hipMemcpyDeviceToHost, st));
  if (log_host_or_null)
    NBH_HIP(hipMemcpyAsync(log_host_or_null, h->mrg_log, n_bodies * sizeof(*log_host_or_null), hipMemcpyDeviceToHost, st));
  if (ids_host_or_null)
    NBH_HIP(hipMemcpyAsync(ids_host_or_null, h->ids, n_bodies * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  return NBODY_HIP_OK;
}
