// hermite_handle.h -- the host side the three Hermite handles share (hermite.hip, hermite_block.hip, hermite_batch.hip;
// DESIGN.md section 4.18): the fields every handle has and what its entry points do with them, one text each.  The
// entry points themselves stay written out in their files; a handle's own steps (block_sync_schedule, block_mid_step,
// the layout of an ensemble) stand between the shared halves.  Host code only: nothing here is seen by a kernel.
#pragma once

#include <cstring>

#include "hermite_block_common.h"
#include "hermite_carve.h"

namespace nbh {

// What every handle holds.  noun: "Hermite integrator", "block-step Hermite integrator" or "block-step Hermite
// ensemble", as its messages call it; owner: the word of the capacity message, "integrator's" or "ensemble's".  A
// handle type H derives from it and names the two as H::kNoun and H::kOwner (a null handle has no fields to read).
struct HermiteHandleCore {
  nbody_hip_ctx* ctx;
  size_t max_particles;
  const char *noun, *owner;
  bool primed = false;
  // what the handle was primed for: a step with another count, G, eps or position array primes again
  size_t count = 0;
  float G = 0.f, eps = 0.f;
  const float* pos_x = nullptr;
  // state precision: 0 fp32, 1 extended (the residuals lo, 24 bytes per body, allocated at the first switch to 1)
  int precision = 0;
  float* lo_mem = nullptr;
  HermiteLo lo{};

  HermiteHandleCore(nbody_hip_ctx* c, size_t n, const char* noun_, const char* owner_)
      : ctx(c), max_particles(n), noun(noun_), owner(owner_) {}
  const HermiteLo* lo_or_null() const { return precision == 1 ? &lo : nullptr; }
};

// ---- argument checks with the reference wording ------------------------------------------------------------------------
// (check order and wording of validateTimeStep, ref: src/utils/error_handling.cpp:91-103: positive, finite, then the
// softening; where a call checks its step count, that stands between check_dt and check_eps)
inline int check_dt(float dt) {
  if (dt <= 0.0f) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Time step must be positive");
  if (!finite_f(dt)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Time step must be a finite number");
  return NBODY_HIP_OK;
}
inline int check_dt(float dt, size_t system) {  // (an ensemble: the message names the system)
  if (dt <= 0.0f) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Time step must be positive (system %zu)", system);
  if (!finite_f(dt)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Time step must be a finite number (system %zu)", system);
  return NBODY_HIP_OK;
}
inline int check_eps(float eps) {
  if (!(eps >= 0.0f)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Softening parameter must be non-negative");
  return NBODY_HIP_OK;
}

// ---- create, destroy, the checks at the head of an entry point ---------------------------------------------------------
template <class H>
int handle_create_check(const nbody_hip_ctx* ctx, size_t max_particles, H** out) {
  if (!out) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null output pointer");
  *out = nullptr;
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  if (max_particles == 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "Particle count must be greater than 0");
  if (max_particles > 0x3fffffffu) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "body count exceeds 2^30");
  return NBODY_HIP_OK;
}

// device memory of a handle that is going away: the stream's work first
inline void handle_free(const HermiteHandleCore* h, void* mem) {
  if (!mem) return;
  (void)hipSetDevice(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  (void)hipFree(mem);
}

template <class H>
int handle_null(const H* h) {
  if (!h || !h->ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null %s", H::kNoun);
  return NBODY_HIP_OK;
}

inline int handle_not_primed(const HermiteHandleCore* h) {
  return NBH_FAIL(NBODY_HIP_ERR_STATE, "the %s is not primed", h->noun);
}

// the arrays of the particle data, and its count against the capacity
inline int handle_check_data(const HermiteHandleCore* h, const nbody_particle_data* d) {
  if (int rc = hermite_check_arrays(h->ctx, d, true)) return rc;
  if (d->count > h->max_particles)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "particle count %zu exceeds the %s capacity %zu", d->count, h->owner,
                    h->max_particles);
  return NBODY_HIP_OK;
}

// (capturable: the call may be recorded into a step graph -- it reads nothing back and allocates nothing)
template <class H>
int handle_check(const H* h, const nbody_particle_data* d, const char* what, bool capturable = false) {
  if (int rc = handle_null(h)) return rc;
  if (!capturable) NBH_NOT_CAPTURABLE(h->ctx, what);
  return handle_check_data(h, d);
}

// ---- the state precision ------------------------------------------------------------------------------------------------
// set_precision is handle_precision_check, `if (mode == h->precision) return NBODY_HIP_OK;`, the handle's own refusals,
// handle_precision_switch
template <class H>
int handle_precision_check(const H* h, int mode) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a state-precision switch");
  if (mode != 0 && mode != 1)
    return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "state precision must be 0 (fp32) or 1 (extended), got %d", mode);
  return NBODY_HIP_OK;
}
inline int handle_precision_switch(HermiteHandleCore* h, int mode) {
  if (mode == 1)
    if (int rc = hermite_lo_zero(h->ctx, h->max_particles, &h->lo_mem, &h->lo)) return rc;
  h->precision = mode;
  h->primed = false;
  return NBODY_HIP_OK;
}
template <class H>
int handle_get_precision(const H* h, int* mode) {
  if (int rc = handle_null(h)) return rc;
  if (!mode) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  *mode = h->precision;
  return NBODY_HIP_OK;
}

// invalidate, after the null check and what the handle forgets besides
inline int handle_invalidate(HermiteHandleCore* h) {
  h->primed = false;
  // extended mode: the caller changed the state, the fp32 arrays are the truth
  if (h->precision == 1) return hermite_lo_zero(h->ctx, h->max_particles, &h->lo_mem, &h->lo);
  return NBODY_HIP_OK;
}

// ---- set / get_state_f64: handle_state_check, the handle's own refusals, handle_set_state or handle_get_state ----------
template <class H>
int handle_state_check(const H* h, const nbody_particle_data* d, const void* pos, const void* vel, const char* what) {
  if (int rc = handle_check(h, d, what)) return rc;
  if (!pos || !vel) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null state array");
  return NBODY_HIP_OK;
}
inline int handle_set_state(HermiteHandleCore* h, nbody_particle_data* d, const double* pos, const double* vel) {
  NBH_HIP(hipSetDevice(h->ctx->device));
  h->primed = false;
  return hermite_state_set_f64(h->ctx, d, h->lo_or_null(), pos, vel);
}
inline int handle_get_state(const HermiteHandleCore* h, const nbody_particle_data* d, double* pos, double* vel) {
  NBH_HIP(hipSetDevice(h->ctx->device));
  return hermite_state_get_f64(h->ctx, d, h->lo_or_null(), pos, vel);
}

// ---- what the handle was primed for ------------------------------------------------------------------------------------
inline void handle_primed_for(HermiteHandleCore* h, const nbody_particle_data* d, float G, float eps) {
  h->primed = true;
  h->count = d->count;
  h->G = G;
  h->eps = eps;
  h->pos_x = d->pos_x;
}
inline bool handle_primed_same(const HermiteHandleCore* h, const nbody_particle_data* d, float G, float eps) {
  return h->primed && h->count == d->count && h->G == G && h->eps == eps && h->pos_x == d->pos_x;
}

inline HermiteArrays hermite_arrays(const nbody_particle_data* d) {
  return HermiteArrays{d->pos_x, d->pos_y, d->pos_z, d->vel_x, d->vel_y, d->vel_z, d->acc_x, d->acc_y, d->acc_z,
                       d->acc_old_x, d->acc_old_y, d->acc_old_z};
}

// host dispatch on two template flags: f(std::bool_constant<a>{}, std::bool_constant<b>{})
template <class F>
inline void with_flags(bool a, bool b, F&& f) {
  with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); });
}

// ---- the block-step handles (hermite_block.hip, hermite_batch.hip) -----------------------------------------------------
// set_params writes the pending parameters, a priming takes them over
struct BlockParams {
  float eta_set = 0.02f, eta_start_set = 0.01f;
  int max_level_set = 16;
  float eta = 0.02f, eta_start = 0.01f;
  int L = 16;

  int set(float eta_, float eta_start_, int max_level_) {
    if (!(eta_ > 0.0f) || !finite_f(eta_)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "eta must be positive and finite");
    if (!(eta_start_ > 0.0f) || !finite_f(eta_start_))
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "eta_start must be positive and finite");
    if (max_level_ < 0 || max_level_ > kMaxLevel)
      return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "max_level must be in [0, %d], got %d", kMaxLevel, max_level_);
    eta_set = eta_;
    eta_start_set = eta_start_;
    max_level_set = max_level_;
    return NBODY_HIP_OK;
  }
  void take() { eta = eta_set; eta_start = eta_start_set; L = max_level_set; }
};

struct BlockHandleCore : HermiteHandleCore {
  using HermiteHandleCore::HermiteHandleCore;
  // device state by capacity, one allocation made at first use: per body
  void* mem = nullptr;
  float4* jerk = nullptr;  // {jx, jy, jz, 0} of body i at tick_i
  int* level = nullptr;
  unsigned int* tick = nullptr;
  float* want = nullptr;   // what the criterion asked for at the body's last correction (diagnostics)
  BlockParams par;
};

// the per-body regions every block-step handle carves first, in this order
inline void block_carve_bodies(Carve& c, BlockHandleCore* h) {
  c.add(&h->jerk, h->max_particles);
  c.add(&h->level, h->max_particles);
  c.add(&h->tick, h->max_particles);
  c.add(&h->want, h->max_particles);
}

// what both resident launches pass of the arrays: the particle data, the handle's per-body state, the predicted sources
// (three arrays `stride` float4 apart; the third in extended mode only) and the rows pa, pj
inline ResidentArrays resident_arrays(const BlockHandleCore* h, const nbody_particle_data* d, float4* posm, size_t stride,
                                      float4* pa, float4* pj) {
  return ResidentArrays{hermite_arrays(d), h->lo, d->mass, h->jerk, h->level, h->tick, h->want,
                        posm, posm + stride, posm + 2 * stride, pa, pj};
}

// nbody_hip_hermite_block_state / _batch_state: whichever of the four arrays is asked for, to the host
template <class H>
int handle_block_state(const H* h, int* levels, unsigned int* ticks, float* want, nbody_float4* jerk) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a block-step state read-out");
  if (!h->primed) return handle_not_primed(h);
  NBH_HIP(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  const size_t n = h->count;
  if (levels) NBH_HIP(hipMemcpyAsync(levels, h->level, n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (ticks) NBH_HIP(hipMemcpyAsync(ticks, h->tick, n * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  if (want) NBH_HIP(hipMemcpyAsync(want, h->want, n * sizeof(float), hipMemcpyDeviceToHost, st));
  if (jerk) NBH_HIP(hipMemcpyAsync(jerk, h->jerk, n * sizeof(float4), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  return NBODY_HIP_OK;
}

// the head of an info read-out: the checks, *out zeroed, the deepest level in force
template <class H>
int handle_info_begin(const H* h, nbody_hip_hermite_block_info_t* out) {
  if (int rc = handle_null(h)) return rc;
  NBH_NOT_CAPTURABLE(h->ctx, "a block-step info read-out");
  if (!out) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "null output pointer");
  memset(out, 0, sizeof(*out));
  out->max_level = h->primed ? h->par.L : h->par.max_level_set;
  return NBODY_HIP_OK;
}
// the device counters c[kCounters] of one system added in: level_steps[0 .. kMaxLevel], floor_hits
inline void info_add_counters(nbody_hip_hermite_block_info_t* out, const unsigned long long* c) {
  for (int k = 0; k <= kMaxLevel; k++) out->level_steps[k] += c[k];
  out->floor_hits += c[kMaxLevel + 1];
}

}  // namespace nbh
