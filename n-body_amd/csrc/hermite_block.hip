// hermite_block.hip -- the fourth-order Hermite integrator with INDIVIDUAL BLOCK TIME STEPS for gfx950 (MI355X), on a
// rectangular force-and-jerk sweep: n_active gathered targets against all N predicted sources (no reference
// counterpart).  The model (include/nbody_hip.h):
//
//   one call advances the system by macro steps dt_max; body i steps with dt_i = dt_max 2^-k_i, level k_i in 0..L;
//   time inside a macro step is an integer tick in [0, 2^L], tick_i the time of body i's last correction (a multiple
//   of 2^(L - k_i)); pos / vel / acc of body i and its jerk on the handle are its state AT tick_i.
//
// One block step:
//   block_min_kernel               t = min_i (tick_i + 2^(L - k_i))                      (integer atomicMin)
//   block_compact_predict_kernel   every body predicted to t over h_i = (t - tick_i) dt_max / 2^L into ctx->posm
//                                  ({xp, m}, {vp, 0}); the bodies with tick_i + 2^(L - k_i) = t appended to the index
//                                  list (wave ballot + one integer atomicAdd per wave: the ORDER of the list differs from
//                                  run to run, nothing that is computed depends on it)
//   -- the host reads {t, n_active} (8 bytes, the context's pinned scalar) and sizes the next two launches --
//   direct_jerk_kernel<.., GATHER> WIDE: the shared step's own sweep (hermite.hip, hermite_launch_jerk) with the targets
//                                  gathered through the list; at n_active = N the launch shape is one_sided_shape(N, N), so a
//                                  run whose bodies all sit on level 0 is the shared-step integrator bit for bit
//   direct_jerk_active_narrow_kernel  NARROW (small active sets): lanes hold sources, the few targets are uniform
//                                  across the wave; per-target lane sums in fp32 over the lane's sources, then fp64 over
//                                  the wave (xor butterfly) and the four waves (LDS, wave order): a fixed order
//   block_finalize_active_kernel   splits in fixed order, G in fp64, the corrector over dt_i, the new level (Aarseth
//                                  criterion), want_i, tick_i <- t
// A body outside the active set has none of its arrays written.  No floating-point atomics anywhere: results are bitwise
// reproducible from run to run.
//
// EXTENDED STATE PRECISION (nbody_hip_hermite_block_set_precision): every kernel of the block
// step is a template on the precision (EXT), one text each.  block_compact_predict_kernel<true> predicts every body from
// hi + lo to {xp_hi, m}, {vp_hi, 0}, {xp_lo, 0}, the sweeps form d = (hi_j - hi_i) + (lo_j - lo_i),
// block_finalize_active_kernel<true> corrects to hi + lo; the fp32 instantiations are handed HermiteLo{} and a null plo
// and read neither.  A body outside the active set has none of its arrays written, its residuals included.
//
// RESIDENT SCHEDULING (nbody_hip_hermite_block_set_scheduling): for small systems one workgroup
// (block_resident_kernel) runs the block steps of a whole macro step inside one launch, with the bodies of the narrow
// form and of the finalize pass; the host reads nothing back and the call can be recorded into a step graph.

#include <cmath>
#include <cstring>

#include "hermite_common.h"
#include "hermite_block_common.h"
#include "hermite_handle.h"
#include "system_diag.h"

namespace nbh {

// (kNarrowBelow, the narrow form's sizes and the three predicates of a block step: direct_plan.h)
static_assert(kNarrowSources == kBlock * kNarrowS && kNarrowTargets == kNarrowT, "direct_plan.h sizes the narrow form");
// (kTickNone, kMaxLevel, kCounters, the level rules, the narrow bodies, block_finalize_body and the resident block step:
// hermite_block_common.h)

// Priming: want = eta_s |a| / |j| (+inf when |j| = 0), the smallest level with dt_max 2^-k <= want, tick 0
__global__ __launch_bounds__(kBlock) void block_prime_kernel(const float* __restrict__ ax, const float* __restrict__ ay,
                                                             const float* __restrict__ az,
                                                             const float4* __restrict__ jerk, int n, float eta_s,
                                                             float dt_max, int L, int* __restrict__ level,
                                                             unsigned int* __restrict__ tick, float* __restrict__ want,
                                                             unsigned int* __restrict__ sched,
                                                             unsigned long long* __restrict__ counters) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) {
    sched[0] = kTickNone;
    sched[1] = 0u;
    for (int c = 0; c < kCounters; c++) counters[c] = 0ull;
  }
  if (i >= n) return;
  float w;
  level[i] = block_prime_level(ax[i], ay[i], az[i], jerk[i], eta_s, dt_max, L, &w);
  tick[i] = 0u;
  want[i] = w;
}

// t = min over the bodies of the tick of their next correction
__global__ __launch_bounds__(kBlock) void block_min_kernel(const int* __restrict__ level,
                                                           const unsigned int* __restrict__ tick, int n, int L,
                                                           unsigned int* __restrict__ sched) {
  __shared__ unsigned int red[kBlock / kWave];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  unsigned int nt = kTickNone;
  if (i < n) nt = tick[i] + (1u << (L - level[i]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nt = min(nt, (unsigned int)__shfl_down((int)nt, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int v = red[0];
#pragma unroll
    for (int k = 1; k < kBlock / kWave; k++) v = min(v, red[k]);
    if (v != kTickNone) atomicMin(&sched[0], v);
  }
}

// every body predicted to t = sched[0] (EXT: from hi + lo, {xp_lo, 0} written too); the active ones appended to the list
template <bool EXT>
__global__ __launch_bounds__(kBlock) void block_compact_predict_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
    const float* __restrict__ vx, const float* __restrict__ vy, const float* __restrict__ vz,
    const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az,
    const float* __restrict__ m, HermiteLo lo, const float4* __restrict__ jerk, const int* __restrict__ level,
    const unsigned int* __restrict__ tick, int n, int L, float dt_max, unsigned int* __restrict__ sched,
    int* __restrict__ list, float4* __restrict__ posm, float4* __restrict__ vel, float4* __restrict__ plo) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned int t = sched[0];
  bool active = false;
  if (i < n) {
    const unsigned int ti = tick[i];
    const double h = (double)(t - ti) * (double)dt_max / (double)(1u << L);
    hermite_predict<EXT>(h, x, y, z, vx, vy, vz, ax, ay, az, m, lo, jerk, i, posm, vel, plo);
    active = ti + (1u << (L - level[i])) == t;
  }
  const unsigned long long mask = __ballot(active);
  if (mask == 0ull) return;  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  unsigned int base = 0u;
  if (lane == 0) base = atomicAdd(&sched[1], (unsigned int)__popcll(mask));
  base = (unsigned int)__shfl((int)base, 0, 64);
  if (active) list[base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull))] = i;
}

// ---------------------------------------------------------------------------------
// Narrow form.  grid = (ceil(n / 1024), ceil(n_active / 4)); block = 256.  Lane `tid` of source block bx holds the
// sources bx 1024 + s 256 + tid, s < 4 (padded: m = 0 at rest at the origin), so all 64 lanes of every wave have pair
// work down to n_active = 1; the block's (up to) four targets are uniform.  Per target: the lane's fp32 sums over its
// sources, converted to fp64, summed over the wave by an xor butterfly and over the four waves in wave order -- a fixed
// order that depends on nothing but the target and the sources.  One row per (source block, target), rounded to fp32
// like the rows of the wide form, for the same finalize pass.
// Its three bodies (narrow_load_sources, narrow_target, narrow_row: hermite_block_common.h) are those of the resident
// block step (resident_block_step, the step of block_resident_kernel and of batch_resident_kernel of hermite_batch.hip),
// whose 256-lane sub-blocks run them in the same order: that is the whole of their bit equality.
// ---------------------------------------------------------------------------------
// EXT: extended state precision, d = (hi_j - hi_i) + (lo_j - lo_i) with the residuals {xp_lo, 0} in plo (fp32: plo is
// not read).
template <bool GUARD, bool EXT>
__global__ __launch_bounds__(kBlock) void direct_jerk_active_narrow_kernel(const float4* __restrict__ posm,
                                                                           const float4* __restrict__ vel,
                                                                           const float4* __restrict__ plo,
                                                                           const int* __restrict__ list, int n_active,
                                                                           int n, float4* __restrict__ pa,
                                                                           float4* __restrict__ pj, int n_pad,
                                                                           float eps2) {
  __shared__ double red[kNarrowT][6][kBlock / kWave];
  const int tid = threadIdx.x;
  float4 sp[kNarrowS], sv[kNarrowS], sl[kNarrowS];
  narrow_load_sources<EXT>(posm, vel, plo, blockIdx.x * (kBlock * kNarrowS), tid, n, sp, sv, sl);
  const int k0 = blockIdx.y * kNarrowT;
#pragma unroll
  for (int q = 0; q < kNarrowT; q++) {
    const int k = k0 + q;
    if (k < n_active) {  // (uniform over the block)
      const int i = list[k];
      const float4 tp = posm[i], tv = vel[i];
      float4 tl = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (EXT) tl = plo[i];
      const NarrowSums r = narrow_target<GUARD, EXT>(sp, sv, sl, tp, tv, tl, eps2);
      if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) red[q][c][tid >> 6] = r.v[c];
      }
    }
  }
  __syncthreads();
  if (tid < kNarrowT && k0 + tid < n_active) {
    double s[6];
#pragma unroll
    for (int c = 0; c < 6; c++) s[c] = narrow_row(red[tid][c]);
    const size_t o = (size_t)blockIdx.x * n_pad + (k0 + tid);
    pa[o] = make_float4((float)s[0], (float)s[1], (float)s[2], 0.f);
    pj[o] = make_float4((float)s[3], (float)s[4], (float)s[5], 0.f);
  }
}

// Finalize of the active bodies (block_finalize_body<EXT>: the corrector on the fp32 or on the extended state; the level
// rule is the same).  Re-arms the schedule words for the next block step.
template <bool EXT>
__global__ __launch_bounds__(kBlock) void block_finalize_active_kernel(
    const float4* __restrict__ pa, const float4* __restrict__ pj, int splits, int n_pad,
    const int* __restrict__ list, int n_active, float G, float dt_max, int L, unsigned int t, float eta,
    HermiteArrays d, HermiteLo lo, float4* __restrict__ jerk, int* __restrict__ level, unsigned int* __restrict__ tick,
    float* __restrict__ want, unsigned int* __restrict__ sched, unsigned long long* __restrict__ counters) {
  __shared__ unsigned int hist[kCounters];
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (threadIdx.x < kCounters) hist[threadIdx.x] = 0u;
  __syncthreads();
  if (k == 0) {
    sched[0] = kTickNone;
    sched[1] = 0u;
  }
  if (k < n_active)
    block_finalize_body<EXT>(pa, pj, splits, n_pad, k, list[k], G, dt_max, L, t, eta, d, lo, jerk, level, tick, want, hist);
  __syncthreads();
  if (threadIdx.x < kCounters && hist[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// ---------------------------------------------------------------------------------
// Resident form (nbody_hip_hermite_block_set_scheduling).  ONE workgroup of 512 threads runs
// whole block steps back to back -- resident_block_step (hermite_block_common.h): t, the prediction of all bodies, the
// active list, the narrow sweep, the corrector and the levels, with __syncthreads() between the phases -- until the
// macro boundary or until its budget of block steps is used up: no launch and no host read per block step.  Per target
// the step sums in the order of the host-scheduled narrow form, with its bodies, so the two agree bit for bit.  No
// cooperative launch, no grid barrier, no wait on memory; every loop is bounded (at most 2^L + 1 block steps per
// launch), and a schedule that cannot be (empty active set, t not ahead of the current tick or beyond 2^L, boundary not
// reached) leaves a status word behind, which the launches queued after it see first.
// ---------------------------------------------------------------------------------
// automatic scheduling (mode 2) takes the resident form below this many bodies: the largest measured N at which it beats
// the host form by more than the spread of the host form's repeats (profiles/r12_hermite_block_resident.txt)
constexpr size_t kResidentBelow = NBODY_HIP_HERMITE_BLOCK_RESIDENT_BELOW;

// the schedule of the handle while the device owns it
struct BlockResidentState {
  unsigned int status;         // 0 fine; else the block-step schedule went out of range (see bad_*)
  unsigned int cur_tick;       // 0 at a macro boundary
  unsigned int last_n_active;
  unsigned int bad_t, bad_tick, bad_n_active;
  unsigned long long block_steps, body_steps, macro_steps;
};

__global__ void block_resident_seed_kernel(BlockResidentState* rs, unsigned int cur_tick, unsigned int last_n_active,
                                           unsigned long long block_steps, unsigned long long body_steps,
                                           unsigned long long macro_steps) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rs->status = 0u;
    rs->cur_tick = cur_tick;
    rs->last_n_active = last_n_active;
    rs->bad_t = rs->bad_tick = rs->bad_n_active = 0u;
    rs->block_steps = block_steps;
    rs->body_steps = body_steps;
    rs->macro_steps = macro_steps;
  }
}

// budget: block steps this launch may take; to_boundary: the launch is one macro step of an advance (it must reach the
// boundary) rather than a step call (which may stop before it)
template <bool EXT, bool GUARD>
__global__ __launch_bounds__(kResidentBlock) void block_resident_kernel(const ResidentSystem S, BlockResidentState* const rs,
                                                                        unsigned int budget, int to_boundary) {
  const unsigned int end = 1u << S.L;
  const unsigned int status_in = (unsigned int)uniform_i((int)rs->status);
  unsigned int cur = (unsigned int)uniform_i((int)rs->cur_tick);
  __syncthreads();  // (thread 0 writes these words at the end)
  if (status_in != 0u) return;  // an earlier launch gave up: nothing is touched

  const unsigned int max_steps = to_boundary ? end + 1u : min(budget, end + 1u);
  unsigned int status = 0u, bad_t = 0u, bad_n = 0u, last_n = 0u;
  unsigned long long steps = 0ull, bodies = 0ull;
  bool boundary = false;
  for (unsigned int it = 0; it < max_steps; it++) {
    ResidentStep st;
    if (!resident_block_step<EXT, GUARD, false>(S, cur, st)) {  // (uniform)
      status = 1u;
      bad_t = st.t;
      bad_n = st.n_active;
      break;
    }
    steps++;
    bodies += st.n_active;
    last_n = st.n_active;
    if (st.t == end) {
      cur = 0u;
      boundary = true;
      break;
    }
    cur = st.t;
  }
  if (threadIdx.x == 0) {
    rs->cur_tick = cur;
    rs->block_steps += steps;
    rs->body_steps += bodies;
    if (steps != 0ull) rs->last_n_active = last_n;
    if (boundary) rs->macro_steps += 1ull;
    if (status == 0u && to_boundary && !boundary) {  // 2^L + 1 block steps and no boundary
      status = 2u;
      bad_t = cur;
    }
    if (status != 0u) {
      rs->bad_t = bad_t;
      rs->bad_tick = cur;
      rs->bad_n_active = bad_n;
      rs->status = status;
    }
  }
}

}  // namespace nbh

using namespace nbh;

// (the fields every Hermite handle has, the per-body state jerk / level / tick / want, the parameters par and what the
// entry points do with them: hermite_handle.h)
struct nbody_hip_hermite_block : BlockHandleCore {
  static constexpr const char *kNoun = "block-step Hermite integrator", *kOwner = "integrator's";
  nbody_hip_hermite_block(nbody_hip_ctx* c, size_t n) : BlockHandleCore(c, n, kNoun, kOwner) {}
  // device state behind the per-body arrays, in the same allocation
  int* list = nullptr;                  // the active set of the current block step
  unsigned int* sched = nullptr;        // {t, n_active} of the current block step
  unsigned int* hint = nullptr;         // the hint word of the priming evaluation (not used further)
  unsigned long long* counters = nullptr;  // level_steps[21], floor_hits
  BlockResidentState* rs = nullptr;     // the schedule while the resident form owns it (on_device)
  int narrow_below = 0;  // 0 automatic
  float dt_max = 0.f;    // primed for this macro step, besides what the core records
  // schedule as the host knows it
  unsigned int cur_tick = 0, last_n_active = 0;
  unsigned long long block_steps = 0, body_steps = 0, narrow_launches = 0, wide_launches = 0, macro_steps = 0;
  // scheduling: 0 host, 1 resident, 2 automatic; the form of the last step / advance call (-1: none since priming).
  // on_device: resident launches are queued and *rs is the truth -- cur_tick, last_n_active, block_steps, body_steps
  // and macro_steps above are stale until block_sync_schedule reads them back
  int scheduling = 0, last_form = -1;
  bool on_device = false;
};

// one allocation, made at first use: the per-body arrays, then (256-byte aligned, in this order) the active list, the
// two schedule words, the hint word, the counters and the resident schedule
static int block_reserve(nbody_hip_hermite_block* h) {
  if (h->mem) return NBODY_HIP_OK;
  Carve c;
  block_carve_bodies(c, h);
  c.add(&h->list, h->max_particles);
  c.add(&h->sched, 2);
  c.add(&h->hint, 1);
  c.add(&h->counters, kCounters);
  c.add(&h->rs, 1);
  NBH_HIP(hipMalloc(&h->mem, c.total()));
  c.place(h->mem);
  return NBODY_HIP_OK;
}

static int block_prime(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps, float dt_max) {
  if (int rc = block_reserve(h)) return rc;
  h->primed = false;
  if (int rc = hermite_evaluate(h->ctx, d, h->lo_or_null(), nullptr, G, eps, 0.0f, 0, nullptr, nullptr, h->jerk, h->hint))
    return rc;
  h->par.take();
  const int n = (int)d->count;
  hipLaunchKernelGGL(block_prime_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, h->ctx->stream, d->acc_x,
                     d->acc_y, d->acc_z, h->jerk, n, h->par.eta_start, dt_max, h->par.L, h->level, h->tick, h->want,
                     h->sched, h->counters);
  NBH_LAUNCH_CHECK();
  handle_primed_for(h, d, G, eps);
  h->dt_max = dt_max;
  h->cur_tick = 0;
  h->last_n_active = 0;
  h->block_steps = h->body_steps = h->narrow_launches = h->wide_launches = h->macro_steps = 0;
  h->last_form = -1;
  h->on_device = false;  // (launches still queued run before the priming: same stream)
  return NBODY_HIP_OK;
}

// the refusal of a schedule that cannot be: found by the host form's range check or left behind by a resident launch
static int block_schedule_fail(const ScheduleFault& f) {
  return NBH_FAIL(NBODY_HIP_ERR_STATE, "block-step schedule out of range: tick %u (was %u of %u), %u of %zu bodies active",
                  f.t, f.was, f.end, f.n_active, f.n);
}

// The schedule back from the device when the resident form owns it: waits for the stream.  A launch that gave up
// (status word) is reported like the host form's own range check, and unprimes the handle.
static int block_sync_schedule(nbody_hip_hermite_block* h) {
  if (!h->on_device) return NBODY_HIP_OK;
  NBH_HIP(hipSetDevice(h->ctx->device));
  BlockResidentState rs;
  NBH_HIP(hipMemcpyAsync(&rs, h->rs, sizeof(rs), hipMemcpyDeviceToHost, h->ctx->stream));
  NBH_HIP(hipStreamSynchronize(h->ctx->stream));
  h->cur_tick = rs.cur_tick;
  h->last_n_active = rs.last_n_active;
  h->block_steps = rs.block_steps;
  h->body_steps = rs.body_steps;
  h->macro_steps = rs.macro_steps;
  if (rs.status != 0u) {
    h->primed = false;
    h->cur_tick = 0;
    h->on_device = false;
    return block_schedule_fail(ScheduleFault{rs.bad_t, rs.bad_tick, 1u << h->par.L, rs.bad_n_active, h->count, true});
  }
  return NBODY_HIP_OK;
}

static bool block_same(const nbody_hip_hermite_block* h, const nbody_particle_data* d, float G, float eps,
                       float dt_max) {
  return handle_primed_same(h, d, G, eps) && h->dt_max == dt_max;
}

// at tick 0 a call with other parameters than the primed ones primes again; inside a macro step it is refused
static int block_begin(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps, float dt_max) {
  if (block_same(h, d, G, eps, dt_max)) return NBODY_HIP_OK;
  if (h->primed && h->cur_tick != 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE,
                    "dt_max, G, eps, the particle count or the arrays changed in the middle of a macro step (tick %u of "
                    "%u): finish it with the parameters it was started with, or invalidate",
                    h->cur_tick, 1u << h->par.L);
  return block_prime(h, d, G, eps, dt_max);
}

static int block_one_step(nbody_hip_hermite_block* h, nbody_particle_data* d) {
  nbody_hip_ctx* ctx = h->ctx;
  const size_t n = d->count;
  const int blocks = (int)((n + kBlock - 1) / kBlock);
  const bool ext = h->precision == 1;
  if (int rc = ctx->posm.reserve((ext ? 3 : 2) * n * sizeof(float4))) return rc;
  float4* posm = static_cast<float4*>(ctx->posm.ptr);
  float4* vel = posm + n;
  float4* plo = ext ? vel + n : nullptr;
  const HermiteLo lo = ext ? h->lo : HermiteLo{};
  const int L = h->par.L;
  hipLaunchKernelGGL(block_min_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, h->level, h->tick, (int)n, L, h->sched);
  NBH_LAUNCH_CHECK();
  with_flag(ext, [&](auto EX) {
    hipLaunchKernelGGL(block_compact_predict_kernel<decltype(EX)::value>, dim3(blocks), dim3(kBlock), 0, ctx->stream,
                       d->pos_x, d->pos_y, d->pos_z, d->vel_x, d->vel_y, d->vel_z, d->acc_x, d->acc_y, d->acc_z, d->mass, lo,
                       h->jerk, h->level, h->tick, (int)n, L, h->dt_max, h->sched, h->list, posm, vel, plo);
  });
  NBH_LAUNCH_CHECK();
  unsigned int* host = reinterpret_cast<unsigned int*>(ctx->host_scalar);
  NBH_HIP(hipMemcpyAsync(host, h->sched, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
  NBH_HIP(hipStreamSynchronize(ctx->stream));
  const ScheduleFault sched = block_schedule_check(host[0], h->cur_tick, L, host[1], n);
  if (sched.bad) return block_schedule_fail(sched);
  const unsigned int t = sched.t, n_active = sched.n_active, end = sched.end;

  // plan: the narrow kernel with its sizes, or the shared step's sweep gathered through the list (per target the sums
  // of the shared step) with its shape; either way two partial arrays [splits][n_pad]
  const float eps2 = h->eps * h->eps;
  const bool guard = direct_guard(eps2), narrow = block_takes_narrow(h->narrow_below, n_active, n);
  const NarrowSizes z = narrow_sizes(n, n_active);
  const OneSidedShape s = one_sided_shape(no_tuning(), n_active, n);
  const int splits = narrow ? z.splits : s.splits, n_pad = narrow ? z.n_pad : s.n_pad;
  // reserve
  if (int rc = ctx->partial.reserve((size_t)2 * splits * n_pad * sizeof(float4))) return rc;
  float4* const pa = static_cast<float4*>(ctx->partial.ptr);
  float4* const pj = pa + (size_t)splits * n_pad;
  // sweep, finalize
  if (narrow) {
    with_flags(guard, ext, [&](auto GD, auto EX) {
      hipLaunchKernelGGL((direct_jerk_active_narrow_kernel<decltype(GD)::value, decltype(EX)::value>), dim3(z.splits, z.groups),
                         dim3(kBlock), 0, ctx->stream, posm, vel, plo, h->list, (int)n_active, (int)n, pa, pj, n_pad, eps2);
    });
    h->narrow_launches++;
  } else {
    hermite_launch_jerk(ctx, s, guard, posm, vel, plo, h->list, (int)n_active, (int)n, pa, pj, eps2);
    h->wide_launches++;
  }
  NBH_LAUNCH_CHECK();
  with_flag(ext, [&](auto EX) {
    hipLaunchKernelGGL(block_finalize_active_kernel<decltype(EX)::value>, dim3((n_active + kBlock - 1) / kBlock),
                       dim3(kBlock), 0, ctx->stream, pa, pj, splits, n_pad, h->list, (int)n_active, h->G, h->dt_max, L, t,
                       h->par.eta, hermite_arrays(d), lo, h->jerk, h->level, h->tick, h->want, h->sched, h->counters);
  });
  NBH_LAUNCH_CHECK();
  h->block_steps++;
  h->body_steps += n_active;
  h->last_n_active = n_active;
  if (t == end) {
    h->cur_tick = 0;
    h->macro_steps++;
  } else {
    h->cur_tick = t;
  }
  return NBODY_HIP_OK;
}

// The resident form: `launches` launches of one workgroup each (an advance: one per macro step; a step: one with its
// budget of block steps).  Nothing is read back.  While a step graph is recorded nothing may be allocated and the
// schedule must already be on the device (the step-graph rule: run it once eagerly first).
static int block_resident_run(nbody_hip_hermite_block* h, nbody_particle_data* d, int launches, unsigned int budget,
                              bool to_boundary) {
  nbody_hip_ctx* ctx = h->ctx;
  const size_t n = d->count;
  const bool ext = h->precision == 1;
  // plan: the narrow sizes with every body active
  const NarrowSizes z = narrow_sizes(n, n);
  const size_t want_posm = (ext ? 3 : 2) * n * sizeof(float4), want_partial = z.bytes();
  if (ctx->capturing && (!h->on_device || ctx->posm.bytes < want_posm || ctx->partial.bytes < want_partial)) {
    ctx->capture_failed = true;
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "a resident block-step Hermite step cannot be recorded into a step graph before "
                    "it has run once eagerly with these parameters");
  }
  if (int rc = ctx->posm.reserve(want_posm)) return rc;
  if (int rc = ctx->partial.reserve(want_partial)) return rc;
  if (!h->on_device) {  // the host form, or a priming, owned the schedule
    hipLaunchKernelGGL(block_resident_seed_kernel, dim3(1), dim3(kWave), 0, ctx->stream, h->rs, h->cur_tick,
                       h->last_n_active, h->block_steps, h->body_steps, h->macro_steps);
    NBH_LAUNCH_CHECK();
    h->on_device = true;
  }
  ResidentSystem S;
  float4* const pa = static_cast<float4*>(ctx->partial.ptr);
  S.p = resident_arrays(h, d, static_cast<float4*>(ctx->posm.ptr), n, pa, pa + z.rows());
  S.counters = h->counters;
  S.radii = nullptr;
  S.n = (int)n;
  S.L = h->par.L;
  S.G = h->G;
  S.eps2 = h->eps * h->eps;
  S.dt_max = h->dt_max;
  S.eta = h->par.eta;
  const bool guard = direct_guard(S.eps2);  // (as the host form)
  for (int s = 0; s < launches; s++) {
    with_flags(ext, guard, [&](auto EX, auto GD) {
      hipLaunchKernelGGL((block_resident_kernel<decltype(EX)::value, decltype(GD)::value>), dim3(1), dim3(kResidentBlock), 0,
                         ctx->stream, S, h->rs, budget, to_boundary ? 1 : 0);
    });
    NBH_LAUNCH_CHECK();
  }
  h->last_form = 1;
  return NBODY_HIP_OK;
}

// Common front of step and advance: the checks, the form this call takes (0 host, 1 resident), the schedule read back
// when the call needs it, and the (re-)priming rules of block_begin.
static int block_enter(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps, float dt_max, int steps,
                       const char* what, const char* steps_msg, int* form) {
  if (int rc = handle_null(h)) return rc;  // (before h->scheduling is read)
  // (capturable: a resident step / advance on a handle primed for exactly these parameters may be recorded)
  if (int rc = handle_check(h, d, what, h->scheduling != 0)) return rc;
  if (int rc = check_dt(dt_max)) return rc;
  if (steps < 1) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", steps_msg);
  if (int rc = check_eps(eps)) return rc;
  if (h->scheduling == 1 && d->count > (size_t)NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle count %zu exceeds the limit of resident scheduling, %d bodies",
                    d->count, NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX);
  *form = block_takes_resident(h->scheduling, d->count, kResidentBelow, NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX) ? 1 : 0;
  const bool same = block_same(h, d, G, eps, dt_max);
  if (*form == 0 || !same) NBH_NOT_CAPTURABLE(h->ctx, what);  // (the host form reads back; a priming allocates)
  NBH_HIP(hipSetDevice(h->ctx->device));
  if (*form == 0 || !same) {
    if (int rc = block_sync_schedule(h)) return rc;
    if (*form == 0) h->on_device = false;  // the host owns the schedule from here
  }
  return block_begin(h, d, G, eps, dt_max);
}

extern "C" int nbody_hip_hermite_block_create(nbody_hip_ctx* ctx, size_t max_particles, nbody_hip_hermite_block** out) {
  if (int rc = handle_create_check(ctx, max_particles, out)) return rc;
  *out = new nbody_hip_hermite_block(ctx, max_particles);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_destroy(nbody_hip_hermite_block* h) {
  if (!h) return NBODY_HIP_OK;
  NBH_DESTROY_BEGIN
  handle_free(h, h->mem);
  handle_free(h, h->lo_mem);
  delete h;
  NBH_DESTROY_END
}

extern "C" int nbody_hip_hermite_block_set_params(nbody_hip_hermite_block* h, float eta, float eta_start,
                                                  int max_level) {
  if (int rc = handle_null(h)) return rc;
  return h->par.set(eta, eta_start, max_level);
}

extern "C" int nbody_hip_hermite_block_prime(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                             float dt_max) {
  if (int rc = handle_check(h, d, "a block-step Hermite priming")) return rc;
  if (int rc = check_dt(dt_max)) return rc;
  if (int rc = check_eps(eps)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  return block_prime(h, d, G, eps, dt_max);
}

extern "C" int nbody_hip_hermite_block_invalidate(nbody_hip_hermite_block* h) {
  if (int rc = handle_null(h)) return rc;
  h->cur_tick = 0;
  h->on_device = false;
  return handle_invalidate(h);
}

static int block_mid_step(const nbody_hip_hermite_block* h, const char* what) {
  if (h->primed && h->cur_tick != 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "%s in the middle of a macro step (tick %u of %u): finish it, or invalidate", what,
                    h->cur_tick, 1u << h->par.L);
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_set_precision(nbody_hip_hermite_block* h, int mode) {
  if (int rc = handle_precision_check(h, mode)) return rc;
  if (mode == h->precision) return NBODY_HIP_OK;
  if (int rc = block_sync_schedule(h)) return rc;
  if (int rc = block_mid_step(h, "the state precision cannot be switched")) return rc;
  return handle_precision_switch(h, mode);
}

extern "C" int nbody_hip_hermite_block_get_precision(nbody_hip_hermite_block* h, int* mode) {
  return handle_get_precision(h, mode);
}

extern "C" int nbody_hip_hermite_block_set_state_f64(nbody_hip_hermite_block* h, nbody_particle_data* d,
                                                     const double* pos_host, const double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "setting the extended state")) return rc;
  if (int rc = block_sync_schedule(h)) return rc;
  if (int rc = block_mid_step(h, "the state cannot be set")) return rc;
  return handle_set_state(h, d, pos_host, vel_host);
}

extern "C" int nbody_hip_hermite_block_get_state_f64(nbody_hip_hermite_block* h, nbody_particle_data* d, double* pos_host,
                                                     double* vel_host) {
  if (int rc = handle_state_check(h, d, pos_host, vel_host, "reading the extended state")) return rc;
  return handle_get_state(h, d, pos_host, vel_host);
}

extern "C" int nbody_hip_hermite_block_step(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                            float dt_max, int block_steps) {
  int form = 0;
  if (int rc = block_enter(h, d, G, eps, dt_max, block_steps, "a block-step Hermite step", "block_steps must be at least 1",
                           &form))
    return rc;
  if (form == 1) return block_resident_run(h, d, 1, (unsigned int)block_steps, false);
  h->last_form = 0;
  for (int s = 0; s < block_steps; s++) {
    if (int rc = block_one_step(h, d)) {
      h->primed = false;
      h->cur_tick = 0;
      return rc;
    }
    if (h->cur_tick == 0) break;  // a macro boundary: every body at the same time
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_advance(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                               float dt_max, int macro_steps) {
  int form = 0;
  if (int rc = block_enter(h, d, G, eps, dt_max, macro_steps, "a block-step Hermite macro step",
                           "macro_steps must be at least 1", &form))
    return rc;
  if (form == 1) return block_resident_run(h, d, macro_steps, 0u, true);
  h->last_form = 0;
  for (int s = 0; s < macro_steps; s++) {
    do {
      if (int rc = block_one_step(h, d)) {
        h->primed = false;
        h->cur_tick = 0;
        return rc;
      }
    } while (h->cur_tick != 0);
  }
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_state(nbody_hip_hermite_block* h, int* levels, unsigned int* ticks, float* want,
                                             nbody_float4* jerk) {
  return handle_block_state(h, levels, ticks, want, jerk);
}

extern "C" int nbody_hip_hermite_block_set_levels(nbody_hip_hermite_block* h, const int* levels_host) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "setting block-step levels");
  if (!levels_host) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null levels");
  if (!h->primed) return handle_not_primed(h);
  if (int rc = block_sync_schedule(h)) return rc;
  const int L = h->par.L;
  if (h->cur_tick != 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "levels can only be set at tick 0, the macro step is at tick %u of %u",
                    h->cur_tick, 1u << L);
  for (size_t i = 0; i < h->count; i++)
    if (levels_host[i] < 0 || levels_host[i] > L)
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "level %d of body %zu is outside [0, %d]", levels_host[i], i, L);
  NBH_HIP(hipSetDevice(h->ctx->device));
  NBH_HIP(hipMemcpyAsync(h->level, levels_host, h->count * sizeof(int), hipMemcpyHostToDevice, h->ctx->stream));
  NBH_HIP(hipStreamSynchronize(h->ctx->stream));  // (the caller's array may go away)
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_tuning(nbody_hip_hermite_block* h, int narrow_below) {
  if (int rc = handle_null(h)) return rc;
  if (narrow_below < 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "narrow_below must not be negative");
  h->narrow_below = narrow_below;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_set_scheduling(nbody_hip_hermite_block* h, int mode) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a scheduling switch");
  if (mode < 0 || mode > 2)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "scheduling must be 0 (host), 1 (resident) or 2 (automatic), got %d", mode);
  if (mode == h->scheduling) return NBODY_HIP_OK;
  if (int rc = block_sync_schedule(h)) return rc;
  if (int rc = block_mid_step(h, "the scheduling cannot be switched")) return rc;
  h->scheduling = mode;  // the priming and the counters stay: the forms share level / tick / jerk / want
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_get_scheduling(nbody_hip_hermite_block* h, int* mode, int* last_form) {
  if (int rc = handle_null(h)) return rc;
  if (!mode || !last_form) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  *mode = h->scheduling;
  *last_form = h->primed ? h->last_form : -1;
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hermite_block_info(nbody_hip_hermite_block* h, nbody_hip_hermite_block_info_t* out) {
  if (int rc = handle_info_begin(h, out)) return rc;
  out->narrow_below = h->narrow_below > 0 ? h->narrow_below : kNarrowBelow;
  if (!h->primed) return NBODY_HIP_OK;
  if (int rc = block_sync_schedule(h)) return rc;
  NBH_HIP(hipSetDevice(h->ctx->device));
  unsigned long long c[kCounters];
  NBH_HIP(hipMemcpyAsync(c, h->counters, sizeof(c), hipMemcpyDeviceToHost, h->ctx->stream));
  NBH_HIP(hipStreamSynchronize(h->ctx->stream));
  out->block_steps = h->block_steps;
  out->body_steps = h->body_steps;
  info_add_counters(out, c);
  out->narrow_launches = h->narrow_launches;
  out->wide_launches = h->wide_launches;
  out->macro_steps = h->macro_steps;
  out->current_tick = h->cur_tick;
  out->last_n_active = h->last_n_active;
  return NBODY_HIP_OK;
}

// The diagnostics of the one system the handle integrates (system_diag.hip), with its residuals in extended mode.  The
// bodies must stand at a macro boundary; in resident scheduling the schedule is read from the device first.
extern "C" int nbody_hip_hermite_block_diagnostics(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                                   nbody_hip_system_diag* out_device) {
  if (int rc = handle_null(h)) return rc;  // (before h->on_device is read)
  if (int rc = handle_check(h, d, "reading the device schedule for the diagnostics", !h->on_device)) return rc;
  if (!out_device) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  if (int rc = check_eps(eps)) return rc;
  if (d->count > (size_t)NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the diagnostics take one system of at most %d bodies, got %zu",
                    NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX, d->count);
  if (int rc = block_sync_schedule(h)) return rc;
  if (int rc = block_mid_step(h, "the bodies are not synchronised")) return rc;
  const DiagLo lo{h->lo.x, h->lo.y, h->lo.z, h->lo.vx, h->lo.vy, h->lo.vz};
  return system_diag_launch(h->ctx, d, h->precision == 1 ? &lo : nullptr, nullptr, nullptr, nullptr, 1, G, eps, out_device);
}
