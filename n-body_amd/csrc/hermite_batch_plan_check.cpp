// hermite_batch_plan_check.cpp -- the host decisions of the ensemble integrator (hermite_batch_plan.h) on a CPU, under
// AddressSanitizer and UBSan (make batch_plan_check): the advance plan against a literal restatement of the three-branch
// choice nbody_hip_hermite_batch_advance carried, the recording rule of BatchFeatures::turn against the ran_eagerly lines
// of the four configuration calls over every short sequence of calls from every state, and the shared argument checks
// against the loops they replace, code and message.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hermite_batch_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    checked++;                           \
    if (!(cond)) {                       \
      if (failures++ < 40) {             \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

// ---------------------------------------------------------------------------------------
// the handle's fields and lines as they stood before the plan
// ---------------------------------------------------------------------------------------
struct Old {
  bool ev_on = false, out_on = false, hier_on = false, mrg_on = false;
  unsigned int ev_flags = 0u, out_flags = 0u, hier_flags = 0u;
  float hier_kappa = 0.f;
  bool ran_eagerly = false, mrg_ran_eagerly = false;
};

// nbody_hip_hermite_batch_advance: 1 batch_resident_kernel, 2 batch_outcomes_kernel, 3 batch_hierarchy_kernel; what E, O
// and H hold: E 0 {}, 1 {nullptr, nullptr, events, 0u}, 2 {radii, limits, events, ev_flags}; O, H: 0 {} or none, 1 full
struct Launch {
  int kernel, E, O, H;
  bool flag;  // the third template argument
  unsigned int e_flags, o_flags, h_flags;
  float kappa;
};
static Launch restated_advance(const Old* h) {
  Launch l{0, 0, 0, 0, false, 0u, 0u, 0u, 0.f};
  const int E = h->ev_on ? 2 : 0;
  if (h->hier_on) {
    const int EO = h->ev_on ? E : 1;
    const int O = h->out_on ? 1 : 0;
    l = Launch{3, EO, O, 1, h->ev_on, EO == 2 ? h->ev_flags : 0u, O ? h->out_flags : 0u, h->hier_flags, h->hier_kappa};
  } else if (h->out_on) {
    const int EO = h->ev_on ? E : 1;
    l = Launch{2, EO, 1, 0, h->ev_on, EO == 2 ? h->ev_flags : 0u, h->out_flags, 0u, 0.f};
  } else {
    l = Launch{1, E, 0, 0, h->ev_on, E == 2 ? h->ev_flags : 0u, 0u, 0u, 0.f};
  }
  return l;
}
static Launch planned_advance(const BatchFeatures& f) {
  const BatchAdvancePlan p = batch_advance_plan(f);
  Launch l{0, 0, 0, 0, false, 0u, 0u, 0u, 0.f};
  l.kernel = p.form == BatchForm::Resident ? 1 : p.form == BatchForm::Outcomes ? 2 : 3;
  l.E = p.E == BatchEventBlock::Full ? 2 : p.E == BatchEventBlock::Records ? 1 : 0;
  l.flag = p.track;
  // (what hermite_batch.hip does with the plan: a block is filled only where the plan says so, and only passed to a kernel
  // that has the argument)
  l.O = p.O_full && l.kernel != 1 ? 1 : 0;
  l.H = p.H_full && l.kernel == 3 ? 1 : 0;
  l.e_flags = l.E == 2 ? f.flags[kFeatEvents] : 0u;
  l.o_flags = l.O ? f.flags[kFeatOutcomes] : 0u;
  l.h_flags = l.H ? f.flags[kFeatHierarchy] : 0u;
  l.kappa = l.H ? f.kappa : 0.f;
  return l;
}

// the last lines of the four configuration calls, off path and on path
static void restated_set(Old* h, int feature, bool on, unsigned int flags, float kappa) {
  switch (feature) {
    case 0:
      if (!on) {
        if (h->ev_on) h->ran_eagerly = false;
        h->ev_on = false;
        h->ev_flags = 0u;
        return;
      }
      if (!h->ev_on) h->ran_eagerly = false;
      h->ev_on = true;
      h->ev_flags = flags;
      return;
    case 1:
      if (!on) {
        if (h->out_on) h->ran_eagerly = false;
        h->out_on = false;
        h->out_flags = 0u;
        return;
      }
      if (!h->out_on) h->ran_eagerly = false;
      h->out_on = true;
      h->out_flags = flags;
      return;
    case 2:
      if (!on) {
        if (h->hier_on) h->ran_eagerly = false;
        h->hier_on = false;
        h->hier_flags = 0u;
        h->hier_kappa = 0.f;
        return;
      }
      if (!h->hier_on) h->ran_eagerly = false;
      h->hier_on = true;
      h->hier_flags = flags;
      h->hier_kappa = kappa;
      return;
    default:
      if (!on) {
        h->mrg_on = false;
        h->mrg_ran_eagerly = false;
        return;
      }
      if (!h->mrg_on) h->mrg_ran_eagerly = false;
      h->mrg_on = true;
      return;
  }
}
// ... and what hermite_batch.hip writes now
static void planned_set(BatchFeatures* f, int feature, bool on, unsigned int flags, float kappa) {
  f->turn((BatchFeature)feature, on);
  if (on && feature != kFeatMergers) f->flags[feature] = flags;
  if (on && feature == kFeatHierarchy) f->kappa = kappa;
}
static void restated_set_layout(Old* h) {
  h->ev_on = false;
  h->ev_flags = 0u;
  h->out_on = false;
  h->out_flags = 0u;
  h->hier_on = false;
  h->hier_flags = 0u;
  h->hier_kappa = 0.f;
  h->mrg_on = false;
}

static bool same(const Old& o, const BatchFeatures& f) {
  return o.ev_on == f.on[kFeatEvents] && o.out_on == f.on[kFeatOutcomes] && o.hier_on == f.on[kFeatHierarchy] &&
         o.mrg_on == f.on[kFeatMergers] && o.ev_flags == f.flags[kFeatEvents] && o.out_flags == f.flags[kFeatOutcomes] &&
         o.hier_flags == f.flags[kFeatHierarchy] && o.hier_kappa == f.kappa && o.ran_eagerly == f.ran_eagerly &&
         o.mrg_ran_eagerly == f.mrg_ran_eagerly;
}
static bool same(const Launch& a, const Launch& b) {
  return a.kernel == b.kernel && a.E == b.E && a.O == b.O && a.H == b.H && a.flag == b.flag && a.e_flags == b.e_flags &&
         a.o_flags == b.o_flags && a.h_flags == b.h_flags && a.kappa == b.kappa;
}

static void state_from_bits(int bits, Old* o, BatchFeatures* f) {
  *o = Old{};
  *f = BatchFeatures{};
  o->ev_on = f->on[kFeatEvents] = bits & 1;
  o->out_on = f->on[kFeatOutcomes] = bits & 2;
  o->hier_on = f->on[kFeatHierarchy] = bits & 4;
  o->mrg_on = f->on[kFeatMergers] = bits & 8;
  o->ran_eagerly = f->ran_eagerly = bits & 16;
  o->mrg_ran_eagerly = f->mrg_ran_eagerly = bits & 32;
  // (a feature that is on carries flags; one that is off carries none)
  if (o->ev_on) o->ev_flags = f->flags[kFeatEvents] = 3u;
  if (o->out_on) o->out_flags = f->flags[kFeatOutcomes] = 1u;
  if (o->hier_on) {
    o->hier_flags = f->flags[kFeatHierarchy] = 1u;
    o->hier_kappa = f->kappa = 2.5f;
  }
}

static void check_advance_plan() {
  for (int bits = 0; bits < 8; bits++)
    for (unsigned int ef = 0; ef < 4; ef++)
      for (unsigned int of = 0; of < 2; of++)
        for (unsigned int hf = 0; hf < 2; hf++) {
          Old o;
          BatchFeatures f;
          o.ev_on = f.on[kFeatEvents] = bits & 1;
          o.out_on = f.on[kFeatOutcomes] = bits & 2;
          o.hier_on = f.on[kFeatHierarchy] = bits & 4;
          o.ev_flags = f.flags[kFeatEvents] = ef;
          o.out_flags = f.flags[kFeatOutcomes] = of;
          o.hier_flags = f.flags[kFeatHierarchy] = hf;
          o.hier_kappa = f.kappa = 1.5f;
          const Launch a = restated_advance(&o), b = planned_advance(f);
          EXPECT(same(a, b), "on %d flags %u %u %u: kernel %d/%d E %d/%d O %d/%d H %d/%d", bits, ef, of, hf, a.kernel, b.kernel,
                 a.E, b.E, a.O, b.O, a.H, b.H);
          // the hierarchy form alone must see an EMPTY O: the kernel reads O.r_esc != nullptr
          if (o.hier_on && !o.out_on) EXPECT(b.O == 0 && !batch_advance_plan(f).O_full, "O must be empty");
        }
}

// an operation of a sequence: 0 .. 7 a configuration call (feature, on / off), 8 an eager advance, 9 an eager merger
// pass, 10 a new layout
constexpr int kOps = 11;
static void apply_op(int op, int step, Old* o, BatchFeatures* f) {
  if (op < 8) {
    const int feature = op >> 1;
    const bool on = op & 1;
    const unsigned int flags = feature == 0 ? 1u + (unsigned int)(step & 1) : (unsigned int)(step & 1);  // (they vary while on)
    const float kappa = 1.0f + (float)step;
    restated_set(o, feature, on, flags, kappa);
    planned_set(f, feature, on, flags, kappa);
  } else if (op == 8) {
    o->ran_eagerly = f->ran_eagerly = true;
  } else if (op == 9) {
    o->mrg_ran_eagerly = f->mrg_ran_eagerly = true;
  } else {
    restated_set_layout(o);
    f->reset();
  }
}
static void check_sequences() {
  for (int start = 0; start < 64; start++)
    for (int len = 1; len <= 4; len++) {
      int total = 1;
      for (int k = 0; k < len; k++) total *= kOps;
      for (int code = 0; code < total; code++) {
        Old o;
        BatchFeatures f;
        state_from_bits(start, &o, &f);
        int c = code;
        bool ok = true;
        for (int k = 0; k < len && ok; k++, c /= kOps) {
          apply_op(c % kOps, k, &o, &f);
          ok = same(o, f) && same(restated_advance(&o), planned_advance(f));
        }
        EXPECT(ok, "start %d, sequence %d of length %d", start, code, len);
      }
    }
}

// ---------------------------------------------------------------------------------------
// the argument checks as the configuration calls carried them: the code (0, or 1 for NBODY_HIP_ERR_VALIDATION) and the
// message
// ---------------------------------------------------------------------------------------
static char g_msg[512];
static int restated_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return 1;
}
static bool finite_f(float v) { return v - v == 0.0f; }
constexpr int kHierarchyMax = 64;  // NBODY_HIP_BATCH_HIERARCHY_MAX

static int restated_event_flags(int flags) {
  const int known = 1 | 2;
  if ((flags & ~known) != 0)
    return restated_fail("unknown event flag bits 0x%x (known: TRACK_CLOSEST 1, STOP_ON_CONTACT 2)", (unsigned int)(flags & ~known));
  return 0;
}
static int restated_outcome_flags(int flags) {
  const int known = 1;
  if ((flags & ~known) != 0)
    return restated_fail("unknown outcome flag bits 0x%x (known: STOP_ON_ESCAPE 1)", (unsigned int)(flags & ~known));
  return 0;
}
static int restated_hierarchy_flags(int flags) {
  const int known = 1;
  if ((flags & ~known) != 0)
    return restated_fail("unknown hierarchy flag bits 0x%x (known: STOP_ON_RESOLVED 1)", (unsigned int)(flags & ~known));
  return 0;
}
static int restated_merger_flags(int flags) {
  if ((flags & ~1) != 0) return restated_fail("unknown merger flag bits 0x%x (known: MERGERS_ON 1)", (unsigned int)(flags & ~1));
  return 0;
}
static int restated_event_radii(const float* radii_host_or_null, const std::vector<size_t>& offsets) {
  const size_t B = offsets.size() - 1;
  if (radii_host_or_null)
    for (size_t s = 0; s < B; s++)
      for (size_t i = offsets[s]; i < offsets[s + 1]; i++) {
        const float r = radii_host_or_null[i];
        if (!(r >= 0.0f) || !finite_f(r))
          return restated_fail("the radius of body %zu (body %zu of system %zu) must be non-negative "
                               "and finite, got %g", i, i - offsets[s], s, (double)r);
      }
  return 0;
}
static int restated_escape_radii(const float* escape_radii_host_or_null, const std::vector<size_t>& offsets, bool* out) {
  const size_t B = offsets.size() - 1;
  bool positive = false;
  if (escape_radii_host_or_null)
    for (size_t s = 0; s < B; s++) {
      const float r = escape_radii_host_or_null[s];
      if (!(r >= 0.0f) || !finite_f(r))
        return restated_fail("the escape radius of system %zu must be non-negative and finite, got %g", s, (double)r);
      positive = positive || r > 0.0f;
    }
  *out = positive;
  return 0;
}
static int restated_separation_radii(const float* sep_radii_host_or_null, const std::vector<size_t>& offsets, bool* out) {
  const size_t B = offsets.size() - 1;
  bool positive = false;
  if (sep_radii_host_or_null)
    for (size_t s = 0; s < B; s++) {
      const float r = sep_radii_host_or_null[s];
      const size_t n = offsets[s + 1] - offsets[s];
      if (!(r >= 0.0f) || !finite_f(r))
        return restated_fail("the separation radius of system %zu must be non-negative and finite, "
                             "got %g", s, (double)r);
      if (r > 0.0f && n > (size_t)kHierarchyMax)
        return restated_fail("system %zu has %zu bodies: a hierarchy is examined in systems of at most "
                             "%d (its separation radius must be 0, got %g)", s, n, kHierarchyMax, (double)r);
      positive = positive || r > 0.0f;
    }
  *out = positive;
  return 0;
}

static void check_flags() {
  char msg[kBatchMsg];
  const int values[] = {0, 1, 2, 3, 4, 5, 8, 0x40000000, -1, -2, std::numeric_limits<int>::min()};
  for (int flags : values) {
    struct { int (*old)(int); int known; const char *noun, *names; } calls[] = {
        {restated_event_flags, 1 | 2, "event", "TRACK_CLOSEST 1, STOP_ON_CONTACT 2"},
        {restated_outcome_flags, 1, "outcome", "STOP_ON_ESCAPE 1"},
        {restated_hierarchy_flags, 1, "hierarchy", "STOP_ON_RESOLVED 1"},
        {restated_merger_flags, 1, "merger", "MERGERS_ON 1"}};
    for (auto& c : calls) {
      g_msg[0] = msg[0] = 0;
      const int a = c.old(flags);
      const int b = batch_unknown_flags(flags, c.known, c.noun, c.names, msg, sizeof(msg)) ? 1 : 0;
      EXPECT(a == b && (a == 0 || std::strcmp(g_msg, msg) == 0), "%s flags %d: %d '%s' / %d '%s'", c.noun, flags, a, g_msg, b, msg);
    }
  }
}

static void check_radii() {
  const float values[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                          -std::numeric_limits<float>::infinity(), -0.0f, -1e-6f, 0.0f,
                          std::numeric_limits<float>::denorm_min(), 1.5f};
  const int V = (int)(sizeof(values) / sizeof(values[0]));
  char msg[kBatchMsg];
  for (size_t B : {(size_t)1, (size_t)3}) {
    // per system: every combination of the values, over system sizes 64 and 65 (and 2)
    int combos = 1;
    for (size_t s = 0; s < B; s++) combos *= V;
    for (int sizes = 0; sizes < (B == 1 ? 3 : 27); sizes++) {
      std::vector<size_t> offsets(1, 0);
      for (size_t s = 0, c = (size_t)sizes; s < B; s++, c /= 3) offsets.push_back(offsets.back() + (c % 3 == 0 ? 64 : c % 3 == 1 ? 65 : 2));
      for (int code = -1; code < combos; code++) {  // (-1: a null array)
        std::vector<float> r(B);
        for (size_t s = 0, c = (size_t)(code < 0 ? 0 : code); s < B; s++, c /= (size_t)V) r[s] = values[c % (size_t)V];
        const float* arr = code < 0 ? nullptr : r.data();
        bool pa = false, pb = false;
        g_msg[0] = msg[0] = 0;
        int a = restated_escape_radii(arr, offsets, &pa);
        int b = batch_bad_system_radii(arr, offsets.data(), B, "escape", 0, &pb, msg, sizeof(msg)) ? 1 : 0;
        EXPECT(a == b && (a ? std::strcmp(g_msg, msg) == 0 : pa == pb), "escape B %zu sizes %d code %d: %d '%s' / %d '%s'", B, sizes,
               code, a, g_msg, b, msg);
        g_msg[0] = msg[0] = 0;
        a = restated_separation_radii(arr, offsets, &pa);
        b = batch_bad_system_radii(arr, offsets.data(), B, "separation", (size_t)kHierarchyMax, &pb, msg, sizeof(msg)) ? 1 : 0;
        EXPECT(a == b && (a ? std::strcmp(g_msg, msg) == 0 : pa == pb), "separation B %zu sizes %d code %d: %d '%s' / %d '%s'", B,
               sizes, code, a, g_msg, b, msg);
      }
    }
    // per body: systems of 2 (B = 1) or of 1, 2 and 1 bodies (B = 3)
    std::vector<size_t> offsets = B == 1 ? std::vector<size_t>{0, 2} : std::vector<size_t>{0, 1, 3, 4};
    const size_t n = offsets.back();
    combos = 1;
    for (size_t i = 0; i < n; i++) combos *= V;
    for (int code = -1; code < combos; code++) {
      std::vector<float> r(n);
      for (size_t i = 0, c = (size_t)(code < 0 ? 0 : code); i < n; i++, c /= (size_t)V) r[i] = values[c % (size_t)V];
      const float* arr = code < 0 ? nullptr : r.data();
      g_msg[0] = msg[0] = 0;
      const int a = restated_event_radii(arr, offsets);
      const int b = batch_bad_body_radii(arr, offsets.data(), B, msg, sizeof(msg)) ? 1 : 0;
      EXPECT(a == b && (a == 0 || std::strcmp(g_msg, msg) == 0), "bodies B %zu code %d: %d '%s' / %d '%s'", B, code, a, g_msg, b, msg);
    }
  }
}

int main() {
  check_advance_plan();
  check_sequences();
  check_flags();
  check_radii();
  if (failures) {
    std::printf("hermite_batch_plan_check: %d FAILED of %lld\n", failures, checked);
    return 1;
  }
  std::printf("hermite_batch_plan_check: ok (%lld checks)\n", checked);
  return 0;
}
