// hop_groups.hip -- density-peak (HOP) groups from neighbour lists and densities, with saddle regrouping (no reference
// counterpart).  The model is in include/nbody_hip_hop.h and DESIGN.md section 4.29; the order, live / viable, the
// boundary value, the edge key and the attachment choice are hop_common.h, which the CPU program hop_check.cpp runs too;
// the argument checks, the launch sizes, the passes of the pointer jumping and the workspace tables are hop_plan.h.  This
// file is built with -ffp-contract=off (Makefile): the boundary value is an add and a multiply, two roundings.
//
// Six stages, integer work but for the compares and the one boundary value:
//   HOP        hop_next_kernel       one lane per body: its row, the gathers of rho, next; the bad-index flag
//   PEAKS      hop_jump_kernel       hop_jump_passes launches: every lane follows up to 64 pointers and stores where it got
//   RECORDS    hop_count_kernel      one lane per body: its directed records; peaks and candidates counted per wave
//              rocprim scan / select records before every body; the live non-viable peaks, ascending
//              (the host reads the flag and the three counts, and sizes the record workspace)
//              hop_fill_kernel       (P, Q) and (Q, P) of every boundary pair, both with bits(b)
//   SORT, FOLD rocprim::radix_sort_pairs   ONE stable sort of the 64-bit keys over bits [0, 2 qbits)
//              rocprim::reduce_by_key      the segmented maximum: unique edges, ascending (P, Q), and S
//              hop_estart_kernel     where every peak's edges begin
//   REGROUP    hop_unite_kernel      viable pairs with S >= delta_saddle through the union-find of grid_groups.inc
//              hop_flatten_kernel    root[P] of every viable peak
//              hop_round_kernel      one launch per round, one lane per candidate peak over its own edge segment; the
//                                    host reads one word per round: the peaks it anchored
//   CATALOGUE  hop_label_kernel, hop_keys_kernel, the sort / heads / scan / offsets of grid_groups.inc,
//              hop_group_peak_kernel
// Atomics: integer atomicOr / atomicAdd / atomicMax / atomicMin and the CAS hooks of the union-find; the result of each
// is independent of the order they arrive in.  No index read from the lists is used before hop_slot has passed it; a
// record position is checked against the record count before it is written.

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"
#include "body_sort.h"
#include "hop_common.h"
#include "hop_plan.h"
#include "nbody_hip_hop.h"

// the union-find, the size count and the head / offset kernels of the friends-of-friends search: its shared part
#define NBH_GROUPS_SHARED_PART_ONLY
#include "grid_groups.inc"
#undef NBH_GROUPS_SHARED_PART_ONLY

namespace nbh {

static_assert(kHopThreads == kBlock, "the catalogue kernels of grid_groups.inc are launched with the same grid");
static_assert(kHopMaxK == NBODY_HIP_HOP_MAX_K, "plan and header");
static_assert(NBODY_HIP_HOP_STAGES == 6, "six stages, seven boundaries (nbody_hip_ctx::hop_events)");
static_assert(sizeof(nbody_hip_hop_params_t) == 40, "nbody_hip_hop_params_t is 40 bytes (include/nbody_hip_hop.h)");

using HopSort = BodySort<unsigned int, false, false>;  // the catalogue's (key, body index) pairs: the public sort alone
using u64 = unsigned long long;
constexpr int kHopNoPeak = 0x7fffffff;

struct HopArgs {
  const int* index;
  const double* rho;
  int count, k, n_hop, n_merge, read_slots, min_members, qbits;
  double delta_outer, delta_saddle, delta_peak;
  long long n_records;
  u64* words;
  unsigned int* edge_count;
  int *next, *nrec, *root, *anchor, *estart, *cand, *labels, *sizes, *best_peak, *body;
  long long* rstart;
  char* cand_flags;
  u64* best_rho;
  unsigned int *keys_a, *keys_b;
  u64 *keys_in, *vals_in, *keys_out, *vals_out;  // keys_in / vals_in: after the fold, the unique edges and S
  int *labels_out, *peak_out;                    // the caller's, either may be null
  int *offsets, *members, *group_peak;           // the catalogue
};

__device__ __forceinline__ int hop_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hop_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one add per wave: the number of lanes with `flag` (every lane of the wave calls this)
__device__ __forceinline__ void hop_wave_count(bool flag, u64* word) {
  const u64 m = __ballot(flag);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(word, (u64)__popcll(m));
}

__global__ __launch_bounds__(kHopThreads) void hop_next_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (i >= A.count) return;
  const int* row = A.index + i * A.k;
  int b = (int)i;
  double rb = A.rho[i];
  bool bad = false;
  for (int s = 0; s < A.read_slots; s++) {
    const int j = row[s];
    const int what = hop_slot(j, A.count);
    if (what == 2) bad = true;
    if (what != 1 || s >= A.n_hop) continue;
    const double rj = A.rho[j];
    if (hop_better(rj, j, rb, b)) {
      b = j;
      rb = rj;
    }
  }
  if (bad) atomicOr(A.words + kHopWordBad, 1ull);
  A.next[i] = b;
  A.root[i] = (int)i;
  A.anchor[i] = -1;
  A.estart[i] = -1;
  A.sizes[i] = 0;
  A.best_rho[i] = 0ull;
  A.best_peak[i] = kHopNoPeak;
  A.body[i] = (int)i;
}

// Whatever next[x] holds is a body further along x's chain (or x, at a peak); a lane writes its own word alone.
__global__ __launch_bounds__(kHopThreads) void hop_jump_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (i >= A.count) return;
  int cur = hop_load(A.next + i);
  if (cur == (int)i) return;
  for (int s = 1; s < kHopJumpSteps; s++) {
    const int nx = hop_load(A.next + cur);
    if (nx == cur) break;
    cur = nx;
  }
  hop_store(A.next + i, cur);
}

// the boundary pairs of body i, in slot order: f(j) for every one
template <class F>
__device__ __forceinline__ void hop_boundary_pairs(const HopArgs& A, long long i, int P, F&& f) {
  const int* row = A.index + i * A.k;
  for (int s = 0; s < A.n_merge; s++) {
    const int j = row[s];
    if (hop_slot(j, A.count) != 1) continue;
    const double rj = A.rho[j];
    if (hop_live(rj, A.delta_outer) && A.next[j] != P) f(j, rj);
  }
}

__global__ __launch_bounds__(kHopThreads) void hop_count_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  const bool valid = i < A.count;
  bool is_peak = false, cand = false;
  int c = 0;
  if (valid) {
    const int P = A.next[i];  // peak[i]: the pointer jumping has ended
    const double ri = A.rho[i];
    const bool live = hop_live(ri, A.delta_outer);
    is_peak = P == (int)i;
    if (is_peak) {
      const bool viable = hop_viable(ri, A.delta_outer, A.delta_peak);
      if (viable) A.anchor[i] = 0;
      cand = live && !viable;
    }
    A.cand_flags[i] = cand ? 1 : 0;
    if (live) hop_boundary_pairs(A, i, P, [&c](int, double) { c += 2; });
  }
  if (i <= A.count) A.nrec[i] = c;  // (the scan's last entry: the records of the call)
  hop_wave_count(is_peak, A.words + kHopWordPeaks);
  hop_wave_count(cand, A.words + kHopWordCandidates);
}

__global__ __launch_bounds__(kHopThreads) void hop_fill_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (i >= A.count) return;
  const double ri = A.rho[i];
  if (!hop_live(ri, A.delta_outer)) return;
  const int P = A.next[i];
  long long at = A.rstart[i];
  hop_boundary_pairs(A, i, P, [&](int j, double rj) {
    if (at >= 0 && at + 1 < A.n_records) {  // (always, while the caller's arrays are what the count kernel read)
      const int Q = A.next[j];
      const u64 bits = hop_boundary_bits(hop_boundary(ri, rj));
      A.keys_in[at] = hop_edge_key(P, Q, A.qbits);
      A.vals_in[at] = bits;
      A.keys_in[at + 1] = hop_edge_key(Q, P, A.qbits);
      A.vals_in[at + 1] = bits;
    }
    at += 2;
  });
}

__device__ __forceinline__ long long hop_edges(const HopArgs& A) {
  const long long e = *A.edge_count;
  return e < A.n_records ? e : A.n_records;
}

__global__ __launch_bounds__(kHopThreads) void hop_estart_kernel(const HopArgs A) {
  const long long e = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (e >= hop_edges(A)) return;
  const int P = hop_key_p(A.keys_in[e], A.qbits);
  if ((unsigned int)P >= (unsigned int)A.count) return;
  if (e == 0 || hop_key_p(A.keys_in[e - 1], A.qbits) != P) A.estart[P] = (int)e;
}

__global__ __launch_bounds__(kHopThreads) void hop_unite_kernel(const HopArgs A) {
  const long long e = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (e >= hop_edges(A)) return;
  const u64 key = A.keys_in[e];
  const int P = hop_key_p(key, A.qbits), Q = hop_key_q(key, A.qbits);
  // every edge is here twice: the (P < Q) copy unites
  if ((unsigned int)P >= (unsigned int)Q || (unsigned int)Q >= (unsigned int)A.count) return;
  if (A.anchor[P] != 0 || A.anchor[Q] != 0) return;                // both viable
  if (hop_boundary_from_bits(A.vals_in[e]) >= A.delta_saddle) group_unite(A.root, P, Q);
}

__global__ __launch_bounds__(kHopThreads) void hop_flatten_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (i >= A.count || A.anchor[i] != 0) return;
  const int r = group_find(A.root, (int)i);
  atomicMin(A.root + i, r);  // (the root is the lowest ancestor: root[i] = r from here on)
}

// Round `round` >= 1.  anchor[Q] of another candidate may be written while this lane reads it, but only ever to `round`,
// which the test below refuses like the -1 it replaces; root[Q] is read of peaks anchored in an earlier launch alone.
__global__ __launch_bounds__(kHopThreads) void hop_round_kernel(const HopArgs A, int n_cand, int round) {
  const long long c = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  bool did = false;
  if (c < n_cand) {
    const int P = A.cand[c];
    const long long n_edges = hop_edges(A);
    long long e = A.estart[P];
    if (hop_load(A.anchor + P) < 0 && e >= 0) {
      bool have = false;
      u64 s_best = 0;
      int q_best = -1;
      for (; e < n_edges; e++) {
        const u64 key = A.keys_in[e];
        if (hop_key_p(key, A.qbits) != P) break;
        const int Q = hop_key_q(key, A.qbits);
        if ((unsigned int)Q >= (unsigned int)A.count) continue;
        const int aq = hop_load(A.anchor + Q);
        if (aq < 0 || aq >= round) continue;
        const u64 s = A.vals_in[e];
        if (hop_attach_take(have, s_best, s)) {
          have = true;
          s_best = s;
          q_best = Q;
        }
      }
      if (have) {
        A.root[P] = A.root[q_best];
        hop_store(A.anchor + P, round);
        did = true;
      }
    }
  }
  hop_wave_count(did, A.words + kHopWordAnchored);
}

__global__ __launch_bounds__(kHopThreads) void hop_label_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  const bool valid = i < A.count;
  int lab = -1;
  if (valid) {
    const int P = A.next[i];
    const double ri = A.rho[i];
    const bool anchored = A.anchor[P] >= 0;
    if (hop_live(ri, A.delta_outer) && anchored) lab = A.root[P];
    A.labels[i] = lab;
    if (A.labels_out) A.labels_out[i] = lab;
    if (A.peak_out) A.peak_out[i] = P;
    if (P == (int)i && lab >= 0) atomicMax(A.best_rho + lab, hop_boundary_bits(ri));  // (an anchored peak: live, so >= 0)
  }
  group_size_add(valid && lab >= 0, lab, A.sizes);
}

__global__ __launch_bounds__(kHopThreads) void hop_keys_kernel(const HopArgs A) {
  const long long i = (long long)blockIdx.x * kHopThreads + threadIdx.x;
  if (i >= A.count) return;
  const int lab = A.labels[i];
  A.keys_a[i] = lab >= 0 && A.sizes[lab] >= A.min_members ? (unsigned int)lab : (unsigned int)A.count;
  // group_peak: among the anchored peaks of a root, those of the greatest density; of these the lowest index
  if (lab >= 0 && A.next[i] == (int)i && hop_boundary_bits(A.rho[i]) == A.best_rho[lab]) atomicMin(A.best_peak + lab, (int)i);
}

__global__ __launch_bounds__(kHopThreads) void hop_group_peak_kernel(const HopArgs A, const int* __restrict__ ord) {
  const int j = (int)(blockIdx.x * kHopThreads + threadIdx.x);
  if (j >= A.count) return;
  if (group_head(A.keys_b, j, A.count)) A.group_peak[ord[j]] = A.best_peak[A.keys_b[j]];
}

static hipError_t hop_record_scan(void* tmp, size_t& bytes, int* in, long long* out, size_t n, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, 0LL, n, rocprim::plus<long long>(), st);
}
static hipError_t hop_head_scan(void* tmp, size_t& bytes, int* in, int* out, size_t n, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, 0, n, rocprim::plus<int>(), st);
}
static hipError_t hop_select(void* tmp, size_t& bytes, char* flags, int* out, unsigned int* n_out, size_t n, hipStream_t st) {
  return rocprim::select(tmp, bytes, rocprim::make_counting_iterator<int>(0), flags, out, n_out, n, st);
}
static hipError_t hop_catalogue_sort(void* tmp, size_t& bytes, unsigned int* keys_in, unsigned int* keys_out, int* body_in,
                                     int* members, size_t n, hipStream_t st) {
  return HopSort::run(SortImpl::Public, tmp, bytes, keys_in, keys_out, nullptr, nullptr, body_in, members, n, 0u,
                      (unsigned)hop_bits_for((long long)n + 1), st);
}
static hipError_t hop_record_sort(void* tmp, size_t& bytes, u64* keys_in, u64* keys_out, u64* vals_in, u64* vals_out, size_t n,
                                  int bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, (unsigned)bits, st);
}
static hipError_t hop_fold(void* tmp, size_t& bytes, u64* keys, u64* vals, size_t n, u64* ukeys, u64* maxima,
                           unsigned int* n_out, hipStream_t st) {
  return rocprim::reduce_by_key(tmp, bytes, keys, vals, n, ukeys, maxima, n_out, rocprim::maximum<u64>(),
                                rocprim::equal_to<u64>(), st);
}

static int hop_groups_run(nbody_hip_ctx* ctx, int count, int k, const int* index_dev, const double* rho_dev,
                          const HopParams& hp, int* labels_dev, int* peak_dev, long long* counts_host) {
  NBH_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  const size_t n = (size_t)count;
  size_t tmp_bytes = 0;
  {
    size_t b = 0;  // (size queries: no launch)
    NBH_HIP(hop_record_scan(nullptr, b, nullptr, nullptr, n + 1, st));
    tmp_bytes = std::max(tmp_bytes, b);
    NBH_HIP(hop_head_scan(nullptr, b = 0, nullptr, nullptr, n, st));
    tmp_bytes = std::max(tmp_bytes, b);
    NBH_HIP(hop_select(nullptr, b = 0, nullptr, nullptr, nullptr, n, st));
    tmp_bytes = std::max(tmp_bytes, b);
    NBH_HIP(hop_catalogue_sort(nullptr, b = 0, nullptr, nullptr, nullptr, nullptr, n, st));
    tmp_bytes = std::max(tmp_bytes, b);
  }
  const HopBodyPlan p = hop_body_plan(count, tmp_bytes);
  if (int rc = ctx->hop.reserve(p.bytes)) return rc;
  char* const ws = static_cast<char*>(ctx->hop.ptr);
  auto ints = [ws](size_t off) { return reinterpret_cast<int*>(ws + off); };
  HopArgs A{};
  A.index = index_dev;
  A.rho = rho_dev;
  A.count = count;
  A.k = k;
  A.n_hop = hp.n_hop;
  A.n_merge = hp.n_merge;
  A.read_slots = hop_read_slots(hp.n_hop, hp.n_merge);
  A.min_members = hp.min_members;
  A.qbits = p.qbits;
  A.delta_outer = hp.delta_outer;
  A.delta_saddle = hp.delta_saddle;
  A.delta_peak = hp.delta_peak;
  A.words = reinterpret_cast<u64*>(ws + p.off_words);
  A.edge_count = reinterpret_cast<unsigned int*>(ws + p.off_edge_count);
  A.next = ints(p.off_next);
  A.nrec = ints(p.off_nrec);
  A.rstart = reinterpret_cast<long long*>(ws + p.off_rstart);
  A.root = ints(p.off_root);
  A.anchor = ints(p.off_anchor);
  A.estart = ints(p.off_estart);
  A.cand_flags = ws + p.off_cand_flags;
  A.cand = ints(p.off_cand);
  A.labels = ints(p.off_labels);
  A.sizes = ints(p.off_sizes);
  A.best_rho = reinterpret_cast<u64*>(ws + p.off_best_rho);
  A.best_peak = ints(p.off_best_peak);
  A.keys_a = reinterpret_cast<unsigned int*>(ws + p.off_keys_a);
  A.keys_b = reinterpret_cast<unsigned int*>(ws + p.off_keys_b);
  A.body = ints(p.off_body);
  A.labels_out = labels_dev;
  A.peak_out = peak_dev;
  unsigned int* const select_count = reinterpret_cast<unsigned int*>(ws + p.off_select_count);
  long long* const catalogue_counts = reinterpret_cast<long long*>(ws + p.off_catalogue_counts);
  void* const tmp = ws + p.off_tmp;
  const dim3 block(kHopThreads), body_grid(p.body_blocks);

  // the stage boundaries (nbody_hip_hop_stage_times): 0 start, 1 hop, 2 peaks, 3 records, 4 sort and fold, 5 regroup, 6 catalogue
  ctx->hop_stages_valid = false;
  for (hipEvent_t& e : ctx->hop_events)
    if (!e) NBH_HIP(hipEventCreate(&e));
  auto mark = [ctx, st](int boundary) { return hipEventRecord(ctx->hop_events[boundary], st); };

  // HOP, PEAKS, and the count of the records
  NBH_HIP(mark(0));
  NBH_HIP(hipMemsetAsync(A.words, 0, kHopWords * sizeof(u64), st));
  NBH_HIP(hipMemsetAsync(A.edge_count, 0, sizeof(unsigned int), st));
  hipLaunchKernelGGL(hop_next_kernel, body_grid, block, 0, st, A);
  NBH_HIP(mark(1));
  for (int pass = 0; pass < p.jump_passes; pass++) hipLaunchKernelGGL(hop_jump_kernel, body_grid, block, 0, st, A);
  NBH_HIP(mark(2));
  hipLaunchKernelGGL(hop_count_kernel, dim3(p.scan_blocks), block, 0, st, A);
  NBH_LAUNCH_CHECK();
  size_t tb = tmp_bytes;
  NBH_HIP(hop_record_scan(tmp, tb, A.nrec, A.rstart, p.scan_count, st));
  NBH_HIP(hop_select(tmp, tb = tmp_bytes, A.cand_flags, A.cand, select_count, n, st));
  u64 words[kHopWords] = {};
  long long n_records = 0;
  NBH_HIP(hipMemcpyAsync(words, A.words, sizeof(words), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipMemcpyAsync(&n_records, A.rstart + n, sizeof(n_records), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  const int status = hop_status(words[kHopWordBad] != 0);
  if (n_records < 0 || n_records > kHopMaxRecords)
    return NBH_FAIL(NBODY_HIP_ERR_RESOURCE, "%lld directed boundary records: more than 2^31 - 1 (lower n_merge or raise delta_outer)",
                    n_records);
  const int n_cand = (int)words[kHopWordCandidates];

  // the record workspace and the catalogue: from here on the earlier catalogue is gone
  size_t rec_tmp = 0;
  if (status == 0 && n_records > 0) {
    size_t b = 0;
    NBH_HIP(hop_record_sort(nullptr, b, nullptr, nullptr, nullptr, nullptr, (size_t)n_records, 2 * p.qbits, st));
    rec_tmp = std::max(rec_tmp, b);
    NBH_HIP(hop_fold(nullptr, b = 0, nullptr, nullptr, (size_t)n_records, nullptr, nullptr, nullptr, st));
    rec_tmp = std::max(rec_tmp, b);
  }
  const HopRecordPlan rp = hop_record_plan(status == 0 ? n_records : 0, p.qbits, rec_tmp);
  if (rp.bytes > 0)
    if (int rc = ctx->hop_records.reserve(rp.bytes)) return rc;
  const HopCataloguePlan cp = hop_catalogue_plan(count);
  ctx->hop_count = -1;
  if (int rc = ctx->hop_catalogue.reserve(cp.bytes)) return rc;
  char* const cat = static_cast<char*>(ctx->hop_catalogue.ptr);
  A.offsets = reinterpret_cast<int*>(cat + cp.off_offsets);
  A.members = reinterpret_cast<int*>(cat + cp.off_members);
  A.group_peak = reinterpret_cast<int*>(cat + cp.off_group_peak);

  if (status != 0) {  // an index at or past count: no group, every label and peak -1
    if (labels_dev) NBH_HIP(hipMemsetAsync(labels_dev, 0xff, n * sizeof(int), st));
    if (peak_dev) NBH_HIP(hipMemsetAsync(peak_dev, 0xff, n * sizeof(int), st));
    NBH_HIP(hipMemsetAsync(A.offsets, 0, sizeof(int), st));
    NBH_HIP(hipStreamSynchronize(st));
    ctx->hop_count = count;
    ctx->hop_groups = ctx->hop_members = 0;
    counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
    counts_host[4] = status;
    return NBODY_HIP_OK;
  }

  // RECORDS, SORT AND FOLD, the viable components
  A.n_records = n_records;
  if (n_records > 0) {
    char* const rw = static_cast<char*>(ctx->hop_records.ptr);
    A.keys_in = reinterpret_cast<u64*>(rw + rp.off_keys_in);
    A.vals_in = reinterpret_cast<u64*>(rw + rp.off_vals_in);
    A.keys_out = reinterpret_cast<u64*>(rw + rp.off_keys_out);
    A.vals_out = reinterpret_cast<u64*>(rw + rp.off_vals_out);
    const dim3 record_grid(rp.record_blocks);
    hipLaunchKernelGGL(hop_fill_kernel, body_grid, block, 0, st, A);
    NBH_LAUNCH_CHECK();
    NBH_HIP(mark(3));
    size_t rb = rec_tmp;
    NBH_HIP(hop_record_sort(rw + rp.off_tmp, rb, A.keys_in, A.keys_out, A.vals_in, A.vals_out, (size_t)n_records, rp.key_bits, st));
    NBH_HIP(hop_fold(rw + rp.off_tmp, rb = rec_tmp, A.keys_out, A.vals_out, (size_t)n_records, A.keys_in, A.vals_in,
                     A.edge_count, st));
    hipLaunchKernelGGL(hop_estart_kernel, record_grid, block, 0, st, A);
    NBH_HIP(mark(4));
    hipLaunchKernelGGL(hop_unite_kernel, record_grid, block, 0, st, A);
    hipLaunchKernelGGL(hop_flatten_kernel, body_grid, block, 0, st, A);
    NBH_LAUNCH_CHECK();
  } else {
    NBH_HIP(mark(3));
    NBH_HIP(mark(4));
  }

  // the attachment rounds: a peak without an edge is never anchored, so without records the first round is the last
  long long rounds = 0, left = n_records > 0 ? n_cand : 0;
  for (;;) {
    rounds++;
    if (left == 0) break;  // (nothing is left to anchor: this round anchors nothing)
    u64 anchored = 0;
    NBH_HIP(hipMemsetAsync(A.words + kHopWordAnchored, 0, sizeof(u64), st));
    hipLaunchKernelGGL(hop_round_kernel, dim3(hop_blocks(n_cand)), block, 0, st, A, n_cand, (int)rounds);
    NBH_LAUNCH_CHECK();
    NBH_HIP(hipMemcpyAsync(&anchored, A.words + kHopWordAnchored, sizeof(anchored), hipMemcpyDeviceToHost, st));
    NBH_HIP(hipStreamSynchronize(st));
    if (anchored == 0 || (long long)anchored > left) break;
    left -= (long long)anchored;
  }

  // CATALOGUE
  NBH_HIP(mark(5));
  hipLaunchKernelGGL(hop_label_kernel, body_grid, block, 0, st, A);
  hipLaunchKernelGGL(hop_keys_kernel, body_grid, block, 0, st, A);
  NBH_LAUNCH_CHECK();
  NBH_HIP(hop_catalogue_sort(tmp, tb = tmp_bytes, A.keys_a, A.keys_b, A.body, A.members, n, st));
  // (the unsorted keys and the sizes are dead from here: their arrays take the head flags and the scan's result)
  int* const flags = reinterpret_cast<int*>(A.keys_a);
  int* const ord = A.sizes;
  hipLaunchKernelGGL(group_heads_kernel, body_grid, block, 0, st, count, A.keys_b, flags);
  NBH_LAUNCH_CHECK();
  NBH_HIP(hop_head_scan(tmp, tb = tmp_bytes, flags, ord, n, st));
  hipLaunchKernelGGL(group_offsets_kernel, body_grid, block, 0, st, count, A.keys_b, ord, A.offsets, catalogue_counts);
  hipLaunchKernelGGL(hop_group_peak_kernel, body_grid, block, 0, st, A, ord);
  NBH_LAUNCH_CHECK();
  NBH_HIP(mark(6));
  long long cc[2] = {0, 0};
  NBH_HIP(hipMemcpyAsync(cc, catalogue_counts, sizeof(cc), hipMemcpyDeviceToHost, st));
  NBH_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < NBODY_HIP_HOP_STAGES; s++)
    NBH_HIP(hipEventElapsedTime(&ctx->hop_stage_ms[s], ctx->hop_events[s], ctx->hop_events[s + 1]));
  ctx->hop_stages_valid = true;
  ctx->hop_count = count;
  ctx->hop_groups = cc[0];
  ctx->hop_members = cc[1];
  counts_host[0] = cc[0];
  counts_host[1] = cc[1];
  counts_host[2] = (long long)words[kHopWordPeaks];
  counts_host[3] = rounds;
  counts_host[4] = 0;
  return NBODY_HIP_OK;
}

}  // namespace nbh

using namespace nbh;

extern "C" int nbody_hip_hop_groups(nbody_hip_ctx* ctx, int count, int k, const int* index_dev, const double* rho_dev,
                                    const nbody_hip_hop_params_t* params, int* labels_dev, int* peak_dev,
                                    long long* counts_host) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  NBH_NOT_CAPTURABLE(ctx, "a density-peak group search");
  if (!index_dev || !rho_dev) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null neighbour index or density array");
  if (!params) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null parameters");
  if (!counts_host) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null counts_host");
  HopParams hp;
  hp.n_hop = params->n_hop;
  hp.n_merge = params->n_merge;
  hp.min_members = params->min_members;
  hp.delta_outer = params->delta_outer;
  hp.delta_saddle = params->delta_saddle;
  hp.delta_peak = params->delta_peak;
  if (const int why = hop_args_check(count, k, hp)) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "%s", hop_args_message(why));
  if (params->reserved != 0) return NBH_FAIL(NBODY_HIP_ERR_VALIDATION, "the reserved word of the parameters must be 0");
  return hop_groups_run(ctx, count, k, index_dev, rho_dev, hp, labels_dev, peak_dev, counts_host);
}

extern "C" int nbody_hip_hop_stage_times(nbody_hip_ctx* ctx, float* ms_host) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  if (!ms_host) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null ms_host");
  if (!ctx->hop_stages_valid)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "no stage times: the last nbody_hip_hop_groups on this context did not end with status 0");
  for (int s = 0; s < NBODY_HIP_HOP_STAGES; s++) ms_host[s] = ctx->hop_stage_ms[s];
  return NBODY_HIP_OK;
}

extern "C" int nbody_hip_hop_groups_copy(nbody_hip_ctx* ctx, int* offsets_dev, int* members_dev, int* group_peak_dev) {
  if (!ctx) return NBH_FAIL(NBODY_HIP_ERR_STATE, "null context");
  NBH_NOT_CAPTURABLE(ctx, "a density-peak catalogue copy");
  if (ctx->hop_count < 0)
    return NBH_FAIL(NBODY_HIP_ERR_STATE, "no density-peak catalogue: call nbody_hip_hop_groups on this context first");
  NBH_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  const HopCataloguePlan cp = hop_catalogue_plan(ctx->hop_count);
  const char* const cat = static_cast<const char*>(ctx->hop_catalogue.ptr);
  if (offsets_dev)
    NBH_HIP(hipMemcpyAsync(offsets_dev, cat + cp.off_offsets, (size_t)(ctx->hop_groups + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (members_dev && ctx->hop_members > 0)
    NBH_HIP(hipMemcpyAsync(members_dev, cat + cp.off_members, (size_t)ctx->hop_members * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (group_peak_dev && ctx->hop_groups > 0)
    NBH_HIP(hipMemcpyAsync(group_peak_dev, cat + cp.off_group_peak, (size_t)ctx->hop_groups * sizeof(int), hipMemcpyDeviceToDevice, st));
  return NBODY_HIP_OK;
}
