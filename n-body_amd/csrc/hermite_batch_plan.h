// hermite_batch_plan.h -- the host decisions of the ensemble integrator (hermite_batch.hip) as plain
// code: which of the four features (events 4.15, outcomes 4.19, hierarchies 4.20, mergers 4.21) are configured and when
// that forbids a recording, which kernel form an advance launches with what in its argument blocks, and the argument
// checks the four configuration calls share.  Plain C++17, no HIP include: hermite_batch_plan_check.cpp runs all of it on
// a CPU under AddressSanitizer and UBSan (make batch_plan_check) against the code it replaces.  Nothing here launches,
// allocates or reads device memory.
#pragma once

#include <cstddef>
#include <cstdio>

namespace nbh {

// ---------------------------------------------------------------------------------------
// THE FEATURES: what the configuration calls leave in the handle
// ---------------------------------------------------------------------------------------
enum BatchFeature { kFeatEvents = 0, kFeatOutcomes, kFeatHierarchy, kFeatMergers, kBatchFeatures };

struct BatchFeatures {
  bool on[kBatchFeatures] = {false, false, false, false};
  unsigned int flags[kFeatMergers] = {0u, 0u, 0u};  // of the events, the outcomes and the hierarchies, as configured
  float kappa = 0.f;                                // the hierarchies' isolation factor
  bool ran_eagerly = false;      // since the priming: an advance may be recorded into a step graph
  bool mrg_ran_eagerly = false;  // since the priming: a merger pass may be recorded into a step graph

  // a new layout: every configuration goes (the allocations stay); the two recording words are the priming's to clear
  void reset() {
    for (int f = 0; f < kBatchFeatures; f++) on[f] = false;
    flags[kFeatEvents] = flags[kFeatOutcomes] = flags[kFeatHierarchy] = 0u;
    kappa = 0.f;
  }
  // A configuration call that passed its checks.  The recording rule: one eager advance before a recording whenever the
  // on-bit of the events, the outcomes or the hierarchies changes value -- the kernel form or what it reads differs --
  // and not when only flags, radii or kappa of a feature that stays on change (the caller writes flags and kappa after
  // this).  The mergers' word follows the same rule for the pass, and turning them off clears it.  Off: the feature's
  // flags (and kappa) go back to 0.
  void turn(BatchFeature f, bool to) {
    if (f == kFeatMergers) {
      if (!to || !on[f]) mrg_ran_eagerly = false;
    } else {
      if (on[f] != to) ran_eagerly = false;
      if (!to) {
        flags[f] = 0u;
        if (f == kFeatHierarchy) kappa = 0.f;
      }
    }
    on[f] = to;
  }
};

// ---------------------------------------------------------------------------------------
// THE ADVANCE: the kernel form, its TRACK / EVENTS template flag and what each argument block holds
// ---------------------------------------------------------------------------------------
enum class BatchForm { Resident, Outcomes, Hierarchy };  // batch_resident_kernel, batch_outcomes_kernel, batch_hierarchy_kernel
// E: the radii, the budgets, the records and the flags; the records alone ({nullptr, nullptr, events, 0}: the record
// logic runs without events, over the untracked sweep); nothing (the plain form reads none of it)
enum class BatchEventBlock { Empty, Records, Full };

struct BatchAdvancePlan {
  BatchForm form;
  bool track;         // EVENTS of the resident form, TRACK of the other two: events are configured
  BatchEventBlock E;
  bool O_full;        // else empty: the hierarchy form reads O.r_esc != nullptr to know whether the escape test runs
  bool H_full;        // else unused: the kernel has no such argument
};

inline BatchAdvancePlan batch_advance_plan(const BatchFeatures& f) {
  const bool ev = f.on[kFeatEvents], records = f.on[kFeatOutcomes] || f.on[kFeatHierarchy];
  BatchAdvancePlan p;
  p.form = f.on[kFeatHierarchy] ? BatchForm::Hierarchy : f.on[kFeatOutcomes] ? BatchForm::Outcomes : BatchForm::Resident;
  p.track = ev;
  p.E = ev ? BatchEventBlock::Full : records ? BatchEventBlock::Records : BatchEventBlock::Empty;
  p.O_full = f.on[kFeatOutcomes];
  p.H_full = f.on[kFeatHierarchy];
  return p;
}

// ---------------------------------------------------------------------------------------
// THE CHECKS of the configuration calls.  Each returns true when the argument is refused, with the message in msg; all of
// them are validation errors.
// ---------------------------------------------------------------------------------------
constexpr size_t kBatchMsg = 320;

inline bool batch_finite(float v) { return v - v == 0.0f; }  // (finite_f of hermite_common.h)

// noun: "event", "outcome", "hierarchy", "merger"; names: the known flags as the message lists them
inline bool batch_unknown_flags(int flags, int known, const char* noun, const char* names, char* msg, size_t msg_len) {
  if ((flags & ~known) == 0) return false;
  std::snprintf(msg, msg_len, "unknown %s flag bits 0x%x (known: %s)", noun, (unsigned int)(flags & ~known), names);
  return true;
}

// one radius per system (null: none), non-negative and finite; noun: "escape", "separation".  max_bodies != 0: a system
// of more bodies must have the radius 0 (the hierarchies).  *positive: some radius is > 0.
inline bool batch_bad_system_radii(const float* radii_or_null, const size_t* offsets, size_t n_systems, const char* noun,
                                   size_t max_bodies, bool* positive, char* msg, size_t msg_len) {
  *positive = false;
  if (!radii_or_null) return false;
  for (size_t s = 0; s < n_systems; s++) {
    const float r = radii_or_null[s];
    const size_t n = offsets[s + 1] - offsets[s];
    if (!(r >= 0.0f) || !batch_finite(r)) {
      std::snprintf(msg, msg_len, "the %s radius of system %zu must be non-negative and finite, got %g", noun, s, (double)r);
      return true;
    }
    if (max_bodies != 0 && r > 0.0f && n > max_bodies) {
      std::snprintf(msg, msg_len, "system %zu has %zu bodies: a hierarchy is examined in systems of at most %d (its %s "
                    "radius must be 0, got %g)", s, n, (int)max_bodies, noun, (double)r);
      return true;
    }
    *positive = *positive || r > 0.0f;
  }
  return false;
}

// one radius per body of the layout (null: none), non-negative and finite (the events)
inline bool batch_bad_body_radii(const float* radii_or_null, const size_t* offsets, size_t n_systems, char* msg, size_t msg_len) {
  if (!radii_or_null) return false;
  for (size_t s = 0; s < n_systems; s++)
    for (size_t i = offsets[s]; i < offsets[s + 1]; i++) {
      const float r = radii_or_null[i];
      if (!(r >= 0.0f) || !batch_finite(r)) {
        std::snprintf(msg, msg_len, "the radius of body %zu (body %zu of system %zu) must be non-negative and finite, got %g",
                      i, i - offsets[s], s, (double)r);
        return true;
      }
    }
  return false;
}

}  // namespace nbh
