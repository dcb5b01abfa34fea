// hop_check.cpp -- the arithmetic and the host decisions of the density-peak groups (hop_common.h, hop_plan.h) on a CPU,
// under AddressSanitizer and UBSan (make hop_check): `better` as a strict order over NaN, signed zeros, infinities and
// ties, live and viable, the slot rule, the boundary value and the order of its bits, the edge key's round trip, the
// attachment choice against a written-out scan, every validation rule, the passes of the pointer jumping against a
// simulation of the worst chain, and the three workspace tables (regions in order, aligned, disjoint, large enough) at
// 1, 2 and 2^30 bodies.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "hop_common.h"
#include "hop_plan.h"

using namespace nbh;

static int failures = 0;
static long long checked = 0;
#define EXPECT(cond, ...)              \
  do {                                 \
    checked++;                         \
    if (!(cond)) {                     \
      if (failures++ < 40) {           \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

static HopParams legal() {
  HopParams p;
  p.n_hop = 4;
  p.n_merge = 2;
  p.min_members = 1;
  p.delta_outer = 1.0;
  p.delta_saddle = 2.5;
  p.delta_peak = 3.0;
  return p;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double tiny = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();

  // ---- better: a strict order on (rho, index) without NaN; a NaN is never better and never beaten
  const std::vector<double> values = {-inf, -big, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, std::nextafter(1.0, 2.0), big, inf, nan};
  const int nv = (int)values.size();
  for (int a = 0; a < nv; a++)
    for (int ia = 0; ia < 3; ia++)
      for (int b = 0; b < nv; b++)
        for (int ib = 0; ib < 3; ib++) {
          const double ra = values[a], rb = values[b];
          const bool ab = hop_better(ra, ia, rb, ib), ba = hop_better(rb, ib, ra, ia);
          if (std::isnan(ra) || std::isnan(rb)) {
            EXPECT(!ab && !ba, "a NaN is never better and never beaten (%g, %g)", ra, rb);
            continue;
          }
          EXPECT(!(ab && ba), "asymmetric (%g,%d) (%g,%d)", ra, ia, rb, ib);
          const bool same = ra == rb && ia == ib;
          EXPECT(same ? (!ab && !ba) : (ab || ba), "total off the diagonal, irreflexive on it (%g,%d) (%g,%d)", ra, ia, rb, ib);
          EXPECT(ab == (ra > rb || (ra == rb && ia < ib)), "the written rule");
          for (int c = 0; c < nv; c++)
            for (int ic = 0; ic < 3; ic++) {
              const double rc = values[c];
              if (std::isnan(rc)) continue;
              if (ab && hop_better(rb, ib, rc, ic)) EXPECT(hop_better(ra, ia, rc, ic), "transitive");
            }
        }
  EXPECT(hop_better(0.0, 1, -0.0, 2) && !hop_better(-0.0, 2, 0.0, 1), "-0 and +0 are equal densities: the lower index wins");
  EXPECT(hop_better(inf, 5, big, 0) && !hop_better(inf, 5, inf, 4) && hop_better(inf, 3, inf, 4), "+inf is a density like any other");

  // ---- live, viable, the slot rule, the status
  EXPECT(hop_live(1.0, 1.0) && !hop_live(std::nextafter(1.0, 0.0), 1.0) && !hop_live(nan, 0.0) && hop_live(-0.0, 0.0) &&
             hop_live(inf, 1.0), "live is >=, false for a NaN");
  EXPECT(hop_viable(3.0, 1.0, 3.0) && !hop_viable(std::nextafter(3.0, 0.0), 1.0, 3.0) && !hop_viable(nan, 0.0, 0.0) &&
             hop_viable(0.0, 0.0, 0.0), "viable is live and >= delta_peak");
  EXPECT(hop_slot(-1, 5) == 0 && hop_slot(-2147483647 - 1, 5) == 0 && hop_slot(0, 5) == 1 && hop_slot(4, 5) == 1 &&
             hop_slot(5, 5) == 2 && hop_slot(2147483647, 5) == 2, "the slot rule");
  EXPECT(hop_status(0) == 0 && hop_status(1) == 1 && hop_status(7) == 1, "the status");

  // ---- the boundary value: two roundings; its bits order as the values do; -0 counts as +0
  {
    const double a = 1.0, b = std::nextafter(3.0, 0.0);
    EXPECT(hop_boundary(a, b) == std::nextafter(2.0, 0.0), "(1 + below(3)) / 2 is below(2)");
    const double c = std::nextafter(2.0, 0.0);  // 2 + below(2) rounds to 4 (a tie, to even): the sum is rounded before the product
    EXPECT(hop_boundary(2.0, c) == 2.0, "the sum is rounded on its own");
    EXPECT(hop_boundary(big, big) == inf, "an overflowing sum is +inf, not big");
    EXPECT(hop_boundary_bits(-0.0) == 0ull && hop_boundary_bits(0.0) == 0ull, "-0 counts as +0");
    EXPECT(hop_boundary_from_bits(hop_boundary_bits(1.5)) == 1.5 && hop_boundary_from_bits(hop_boundary_bits(inf)) == inf, "round trip");
    const std::vector<double> nonneg = {0.0, tiny, 2 * tiny, std::numeric_limits<double>::min(), 0.5, 1.0, std::nextafter(1.0, 2.0), 2.0, 1e300, big, inf};
    for (size_t i = 0; i < nonneg.size(); i++)
      for (size_t j = 0; j < nonneg.size(); j++)
        EXPECT((nonneg[i] < nonneg[j]) == (hop_boundary_bits(nonneg[i]) < hop_boundary_bits(nonneg[j])), "bits order as values %zu %zu", i, j);
    std::mt19937_64 rng(99);
    std::uniform_real_distribution<double> u(0.0, 1e6);
    for (int t = 0; t < 100000; t++) {
      const double x = u(rng), y = u(rng);
      const double bx = hop_boundary(x, y), by = hop_boundary(y, x);
      EXPECT(hop_boundary_bits(bx) == hop_boundary_bits(by), "the boundary of a pair is the same from either side");
      const long double exact = ((long double)x + (long double)y) * 0.5L;
      EXPECT(std::fabs((double)(exact - (long double)bx)) <= std::ldexp(std::fabs(bx), -52), "within an ulp of the exact mean");
    }
  }

  // ---- the edge key: round trip, order by (P, Q), the bits the sort has to order
  EXPECT(hop_bits_for(1) == 0 && hop_bits_for(2) == 1 && hop_bits_for(3) == 2 && hop_bits_for(4) == 2 && hop_bits_for(5) == 3 &&
             hop_bits_for(kHopMaxCount) == 30, "bits_for at its first values and at the largest count");
  for (long long count : {1LL, 2LL, 3LL, 255LL, 256LL, 257LL, 1025LL, 4194304LL, kHopMaxCount - 1, kHopMaxCount}) {
    const int qb = hop_bits_for(count);
    EXPECT(((count - 1) >> qb) == 0, "the largest index %lld fits %d bits", count - 1, qb);
    EXPECT(2 * qb <= 60, "the key fits 64 bits");
    std::mt19937_64 rng((unsigned long long)count);
    std::uniform_int_distribution<long long> u(0, count - 1);
    unsigned long long k_prev = 0;
    int p_prev = -1, q_prev = -1;
    for (int t = 0; t < 2000; t++) {
      const int P = t == 0 ? (int)(count - 1) : (int)u(rng), Q = t == 1 ? (int)(count - 1) : (int)u(rng);
      const unsigned long long key = hop_edge_key(P, Q, qb);
      EXPECT(hop_key_p(key, qb) == P && hop_key_q(key, qb) == Q, "round trip (%d, %d) at %lld bodies", P, Q, count);
      EXPECT(qb == 0 || (key >> (2 * qb)) == 0, "nothing above bit 2 qbits");
      if (t > 0) {
        const bool less = P < p_prev || (P == p_prev && Q < q_prev);
        EXPECT(less == (key < k_prev), "keys order as (P, Q)");
      }
      k_prev = key;
      p_prev = P;
      q_prev = Q;
    }
  }

  // ---- the attachment choice: fed in ascending Q, the greatest S, ties to the lowest Q
  {
    std::mt19937_64 rng(5);
    for (int t = 0; t < 20000; t++) {
      const int n = 1 + (int)(rng() % 6);
      std::vector<unsigned long long> s((size_t)n);
      for (auto& v : s) v = rng() % 4;
      bool have = false;
      unsigned long long best = 0;
      int q = -1;
      for (int i = 0; i < n; i++)
        if (hop_attach_take(have, best, s[(size_t)i])) {
          have = true;
          best = s[(size_t)i];
          q = i;
        }
      const auto top = std::max_element(s.begin(), s.end());  // (the first of the greatest)
      EXPECT(have && q == (int)(top - s.begin()) && best == *top, "the choice among %d edges", n);
    }
  }

  // ---- the validation, rule by rule
  {
    const HopParams ok = legal();
    EXPECT(hop_args_check(1, 4, ok) == 0 && hop_args_check(kHopMaxCount, 32, ok) == 0, "legal calls");
    EXPECT(hop_args_check(0, 4, ok) == 1 && hop_args_check(-1, 4, ok) == 1, "count 0");
    EXPECT(hop_args_check(kHopMaxCount + 1, 4, ok) == 2, "count above 2^30");
    EXPECT(hop_args_check(10, 0, ok) == 3 && hop_args_check(10, 33, ok) == 3, "k out of range");
    HopParams p = ok;
    p.n_hop = 0;
    EXPECT(hop_args_check(10, 4, p) == 4, "n_hop 0");
    p.n_hop = 5;
    EXPECT(hop_args_check(10, 4, p) == 4, "n_hop above k");
    p = ok;
    p.n_hop = 4;
    p.n_merge = 0;
    EXPECT(hop_args_check(10, 4, p) == 0, "n_merge 0 is legal");
    p.n_merge = -1;
    EXPECT(hop_args_check(10, 4, p) == 5, "n_merge negative");
    p.n_merge = 5;
    EXPECT(hop_args_check(10, 4, p) == 5, "n_merge above k");
    p = ok;
    p.min_members = 0;
    EXPECT(hop_args_check(10, 4, p) == 6, "min_members 0");
    for (int which = 0; which < 3; which++)
      for (double bad : {nan, inf, -inf}) {
        p = ok;
        (which == 0 ? p.delta_outer : which == 1 ? p.delta_saddle : p.delta_peak) = bad;
        EXPECT(hop_args_check(10, 4, p) == 7, "threshold %d not finite", which);
      }
    p = ok;
    p.delta_outer = -1.0;
    EXPECT(hop_args_check(10, 4, p) == 8, "negative delta_outer");
    p = ok;
    p.delta_saddle = 0.5;
    EXPECT(hop_args_check(10, 4, p) == 8, "delta_saddle below delta_outer");
    p = ok;
    p.delta_peak = 2.0;
    EXPECT(hop_args_check(10, 4, p) == 8, "delta_peak below delta_saddle");
    p = ok;
    p.delta_outer = p.delta_saddle = p.delta_peak = 0.0;
    EXPECT(hop_args_check(10, 4, p) == 0, "all thresholds equal, and zero");
    p.delta_outer = -0.0;
    EXPECT(hop_args_check(10, 4, p) == 0, "-0 is 0");
    for (int why = 1; why <= 8; why++) EXPECT(hop_args_message(why)[0] != 0, "a message for rule %d", why);
    EXPECT(hop_args_message(0)[0] == 0, "no message without a fault");
    EXPECT(hop_read_slots(3, 5) == 5 && hop_read_slots(5, 0) == 5 && hop_read_slots(1, 1) == 1, "the slots a call reads");
  }

  // ---- the passes of the pointer jumping: the worst chain (one line of count bodies), every pointer advanced by the
  // least the kernel guarantees -- 64 hops of the pointers as they stood when the pass began
  EXPECT(hop_jump_passes(1) == 1 && hop_jump_passes(2) == 1 && hop_jump_passes(65) == 1 && hop_jump_passes(66) == 2 &&
             hop_jump_passes(4097) == 2 && hop_jump_passes(4098) == 3 && hop_jump_passes(5000) == 3 &&
             hop_jump_passes(kHopMaxCount) == 5, "passes at the edges");
  for (int count : {1, 2, 64, 65, 66, 255, 256, 257, 1025, 4096, 4097, 4098, 5000, 100000}) {
    std::vector<int> next((size_t)count), after((size_t)count);
    for (int i = 0; i < count; i++) next[(size_t)i] = i + 1 < count ? i + 1 : i;
    for (int pass = 0; pass < hop_jump_passes(count); pass++) {
      for (int i = 0; i < count; i++) {
        int cur = next[(size_t)i];
        for (int s = 1; s < kHopJumpSteps && next[(size_t)cur] != cur; s++) cur = next[(size_t)cur];
        after[(size_t)i] = cur;
      }
      next = after;
    }
    bool done = true;
    for (int i = 0; i < count; i++) done = done && next[(size_t)i] == count - 1;
    EXPECT(done, "every pointer at the peak after %d passes over %d bodies", hop_jump_passes(count), count);
  }

  // ---- the workspace tables
  for (long long count : {1LL, 2LL, 257LL, 4194304LL, kHopMaxCount}) {
    for (size_t tmp : {(size_t)0, (size_t)1, (size_t)1000003}) {
      const HopBodyPlan p = hop_body_plan(count, tmp);
      const size_t n = (size_t)count;
      struct Region { size_t off, bytes; };
      const Region r[] = {{p.off_words, kHopWords * 8}, {p.off_select_count, 4}, {p.off_edge_count, 4}, {p.off_catalogue_counts, 16},
                          {p.off_next, n * 4}, {p.off_nrec, (n + 1) * 4}, {p.off_rstart, (n + 1) * 8}, {p.off_root, n * 4},
                          {p.off_anchor, n * 4}, {p.off_estart, n * 4}, {p.off_cand_flags, n}, {p.off_cand, n * 4},
                          {p.off_labels, n * 4}, {p.off_sizes, n * 4}, {p.off_best_rho, n * 8}, {p.off_best_peak, n * 4},
                          {p.off_keys_a, n * 4}, {p.off_keys_b, n * 4}, {p.off_body, n * 4}, {p.off_tmp, tmp}};
      size_t at = 0;
      for (const Region& x : r) {
        EXPECT(x.off % 256 == 0 && x.off >= at, "body region at %zu: aligned, after the one before (%zu)", x.off, at);
        at = x.off + x.bytes;
      }
      EXPECT(p.bytes >= at && p.bytes % 256 == 0, "the body workspace holds its last region");
      EXPECT(p.qbits == hop_bits_for(count) && p.jump_passes == hop_jump_passes(count) && p.scan_count == n + 1, "the plan's numbers");
      EXPECT((long long)p.body_blocks * kHopThreads >= count && ((long long)p.body_blocks - 1) * kHopThreads < count, "one lane per body");
      EXPECT((long long)p.scan_blocks * kHopThreads >= count + 1 && ((long long)p.scan_blocks - 1) * kHopThreads < count + 1,
             "one lane per scan entry");
    }
    const HopCataloguePlan c = hop_catalogue_plan(count);
    const size_t n = (size_t)count;
    EXPECT(c.off_offsets == 0 && c.off_members >= (n + 1) * 4 && c.off_group_peak >= c.off_members + n * 4 &&
               c.bytes >= c.off_group_peak + n * 4 && c.off_members % 256 == 0 && c.off_group_peak % 256 == 0, "the catalogue table");
  }
  for (long long records : {0LL, 1LL, 2LL, 255LL, 256LL, 257LL, 1024LL, 1025LL, kHopMaxRecords}) {
    const HopRecordPlan p = hop_record_plan(records, 12, 777);
    const size_t r = (size_t)records * 8;
    EXPECT(p.key_bits == 24 && p.off_keys_in == 0 && p.off_vals_in >= r && p.off_keys_out >= p.off_vals_in + r &&
               p.off_vals_out >= p.off_keys_out + r && p.off_tmp >= p.off_vals_out + r && p.bytes >= p.off_tmp + 777,
           "the record table at %lld records", records);
    EXPECT(p.off_vals_in % 256 == 0 && p.off_keys_out % 256 == 0 && p.off_vals_out % 256 == 0 && p.off_tmp % 256 == 0, "aligned");
    EXPECT((long long)p.record_blocks * kHopThreads >= records && (records == 0 ? p.record_blocks == 0
                                                                                 : ((long long)p.record_blocks - 1) * kHopThreads < records),
           "one lane per record");
  }

  if (failures) {
    std::printf("hop_check: %d FAILURES in %lld checks\n", failures, checked);
    return 1;
  }
  std::printf("hop_check: ok, %lld checks\n", checked);
  return 0;
}
