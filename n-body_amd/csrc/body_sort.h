// SPDX-License-Identifier: MIT
// body_sort.h -- the one front end of the stable radix sort that bins the bodies, for the Barnes-Hut build (Morton keys,
// index payload) and the spatial-hash build (cell ids, float4 body + index payload) alike.  Three sorts stand behind it:
//   SortImpl::Driver  rocPRIM's Onesweep device functions under the driver of onesweep.h (fenced: rocPRIM version +
//                     self-test) -- the default while the fence holds: 172 us for the two passes of BASELINE config 5;
//   SortImpl::Own     the hand-written sort of radix_sort.h (no rocPRIM): 207 us -- what runs when the fence does not
//                     hold, or with NBH_SORT=own;
//   SortImpl::Public  rocprim::radix_sort_pairs (public API): NBH_SORT=public, and every size below the crossover.
// What the callers keep: their key kernel (which clears BodySort::clear_words words of the temporary storage and counts
// BodySort::hist_places digit places with DigitHistogram<radix::kBits>), their buffers, and WHEN the self-test and the
// error word come to life.  What they no longer know: rocPRIM's iterators, the temporary-storage layouts, the fallback
// order.  This is the only file on the product path that names one of the three sorts.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/zip_iterator.hpp>

#include "common.h"
#include "onesweep.h"
#include "radix_sort.h"

namespace nbh {

enum class SortImpl { Public, Driver, Own };

// NBH_SORT in the environment (read when a tree / grid is made, after the self-test): own | public | driver; anything
// else: the driver while it is compiled in and its self-test holds, else the hand-written sort
inline SortImpl sort_impl_from_env() {
  const char* e = std::getenv("NBH_SORT");
  if (e && std::strcmp(e, "own") == 0) return SortImpl::Own;
  if (e && std::strcmp(e, "public") == 0) return SortImpl::Public;
  if (e && std::strcmp(e, "driver") == 0 && NBH_ONESWEEP_AVAILABLE) return SortImpl::Driver;
  return NBH_ONESWEEP_AVAILABLE && driver_sort_verdict.usable() ? SortImpl::Driver : SortImpl::Own;
}

// The radix sorts of our own take over from kOwnSortFromTree bodies in the Barnes-Hut build (63-bit keys, index payload)
// and from kOwnSortFromGrid in the spatial hash (32-bit keys, float4 + index payload, where rocPRIM's merge sort is
// dearer) -- profiles/r03_sort_crossover.txt.  NBH_OWN_SORT_FROM in the environment overrides both when a tree / grid is
// created (the hook tools/sort_crossover.py measures with, not an interface).
constexpr size_t kOwnSortFromTree = 250000, kOwnSortFromGrid = 120000;
inline size_t own_sort_from(size_t compiled_default) {
  if (const char* e = std::getenv("NBH_OWN_SORT_FROM")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end != e && v >= 0) return (size_t)v;
  }
  return compiled_default;
}

// The sticky word the hand-written sort raises when a look-back gives up (radix_sort.h): mapped host memory, so the
// host reads it without a copy.  The builds look at it when they START (a build refuses after an earlier one's sort
// gave up); without a device address the hand-written sort is not used.
struct SortErrorWord {
  unsigned int* host = nullptr;
  unsigned int* dev = nullptr;
  void alloc() {
    if (host) return;
    if (hipHostMalloc(reinterpret_cast<void**>(&host), 64, hipHostMallocMapped) == hipSuccess) {
      *host = 0u;
      if (hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0) != hipSuccess) dev = nullptr;
    } else {
      host = nullptr;
    }
    (void)hipGetLastError();
  }
  void release() {
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
  }
  bool raised() const { return host && *host; }
};
constexpr const char* kSortGaveUp = "the radix sort of an earlier build gave up in its look-back (csrc/radix_sort.h)";

// The sort that runs for `n` bodies when `requested` was asked for: the public sort below the crossover; a driver that
// is absent or failed its self-test -> the hand-written sort; that one failed or without its error word -> public.
inline SortImpl effective_sort(SortImpl requested, size_t n, size_t crossover, const SortErrorWord& err) {
  SortImpl impl = n >= crossover ? requested : SortImpl::Public;
  if (impl == SortImpl::Driver && !(NBH_ONESWEEP_AVAILABLE && driver_sort_verdict.usable())) impl = SortImpl::Own;
  if (impl == SortImpl::Own && (!own_sort_verdict.usable() || !err.dev)) impl = SortImpl::Public;
  return impl;
}

// BODY: the values are (float4 body, index of the input element) and only the bodies come in (grid); otherwise
// idx_in -> idx_out (tree).  RADIX = false: the public sort alone, with rocPRIM's default tiles (the tree's 30-bit keys:
// a request for anything but SortImpl::Public is not made there, and no other sort is instantiated).
template <class Key, bool BODY, bool RADIX = true>
struct BodySort {
  static constexpr unsigned kBits = radix::kBits;  // THE digit width: the driver's, the hand-written sort's, the key kernels'
  static constexpr bool kDriver = RADIX && NBH_ONESWEEP_AVAILABLE;
  using Hist = onesweep::DigitHistogram<kBits>;
  // rocPRIM's tiles for the public path: 10-bit digits (the 19 cell-id bits of BASELINE config 5 are two passes instead
  // of three, 60 Morton bits six instead of eight: tree build 0.59 -> 0.54 ms at N = 2^20; 11 bits do not fit the LDS of
  // rocPRIM's histogram kernel), and the merge sort up to kSortMergeLimit keys
  using Tiles = std::conditional_t<
      RADIX, rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<1024, 8>, kBits,
                                                 rocprim::block_radix_rank_algorithm::match>,
      rocprim::default_config>;
  using Config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, Tiles, kSortMergeLimit>;

  // the two numbers the kernel that writes the keys needs: the 32-bit words at the front of the temporary storage it
  // has to zero, and the digit places it has to count into the caller's histogram (0: none)
  static size_t clear_words(SortImpl impl, size_t n, unsigned begin_bit, unsigned end_bit) {
    return impl == SortImpl::Driver ? onesweep::clear_words<kBits>(n, begin_bit, end_bit) : 0;
  }
  static int hist_places(SortImpl impl, int bits) { return impl != SortImpl::Public ? (bits + (int)kBits - 1) / (int)kBits : 0; }

  // One stable sort of bits [begin_bit, end_bit) with `impl` (the EFFECTIVE one: effective_sort).  tmp == nullptr:
  // size query for that sort.  cleared: the caller zeroed clear_words() words of tmp; hist: it counted hist_places()
  // digit places there, in Hist::kCopies replicas hist_stride words apart (nullptr: the sort counts).  err_dev:
  // SortErrorWord::dev.  The inputs are not modified.
  static hipError_t run(SortImpl impl, void* tmp, size_t& tmp_bytes, Key* keys_in, Key* keys_out, const float4* body_in,
                        float4* body_out, int* idx_in, int* idx_out, size_t n, unsigned begin_bit, unsigned end_bit,
                        hipStream_t st, unsigned int* err_dev = nullptr, bool cleared = false, unsigned int* hist = nullptr,
                        unsigned int hist_stride = 0) {
    auto with_values = [&](auto vin, auto vout) -> hipError_t {
      if constexpr (kDriver)
        if (impl == SortImpl::Driver)
          return onesweep::sort_pairs<kBits>(tmp, tmp_bytes, static_cast<const Key*>(keys_in), keys_out, vin, vout, n,
                                             begin_bit, end_bit, st, cleared, hist, Hist::kCopies, hist_stride);
      if constexpr (RADIX)
        if (impl != SortImpl::Public)  // (a driver request without the driver compiled in: the hand-written sort)
          return radix::sort_pairs<Key, BODY>(tmp, tmp_bytes, static_cast<const Key*>(keys_in), keys_out, body_in, body_out,
                                              idx_in, idx_out, n, begin_bit, end_bit, st, err_dev, hist,
                                              hist ? Hist::kCopies : 1, hist ? hist_stride : 0u);
      return rocprim::radix_sort_pairs<Config>(tmp, tmp_bytes, keys_in, keys_out, vin, vout, n, begin_bit, end_bit, st);
    };
    if constexpr (BODY)
      return with_values(rocprim::make_zip_iterator(rocprim::make_tuple(body_in, rocprim::make_counting_iterator<int>(0))),
                         rocprim::make_zip_iterator(rocprim::make_tuple(body_out, idx_out)));
    else
      return with_values(idx_in, idx_out);
  }

  // temporary storage that serves every sort that could run
  static hipError_t temp_bytes(size_t& bytes, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t st) {
    bytes = 0;
    for (SortImpl impl : {SortImpl::Public, SortImpl::Driver, SortImpl::Own}) {
      if ((impl == SortImpl::Driver && !kDriver) || (impl == SortImpl::Own && !RADIX)) continue;
      size_t b = 0;
      hipError_t e = run(impl, nullptr, b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, begin_bit, end_bit, st);
      if (e != hipSuccess) return e;
      bytes = std::max(bytes, b);
    }
    return hipSuccess;
  }

  // Run-time half of the dependency fence of onesweep.h, and the same question put to the hand-written sort: ONE buffer
  // of 200,000 keys key_of(0), key_of(1), ... (clustered, so that equal keys show stability) through every sort that
  // is compiled in; keys and values must agree word for word with the public sort's, whose keys must be in order.
  // Once per process and instantiation; the verdicts go to driver_sort_verdict / own_sort_verdict.
  template <class KeyOf>
  static void self_test(hipStream_t st, const char* who, unsigned begin_bit, unsigned end_bit, KeyOf key_of) {
    static std::atomic<bool> done{false};
    if (done.exchange(true)) return;
    const size_t n = 200000;
    std::vector<Key> hk(n);
    std::vector<float4> hb(BODY ? n : 0);
    std::vector<int> hi(BODY ? 0 : n);
    for (size_t i = 0; i < n; i++) {
      hk[i] = key_of(i);
      if constexpr (BODY) hb[i] = make_float4((float)i, (float)hk[i], 0.f, 1.f);
      else hi[i] = (int)i;
    }
    constexpr int kV = 3, kRef = 1;
    const SortImpl impl[kV] = {SortImpl::Driver, SortImpl::Public, SortImpl::Own};
    const bool have[kV] = {kDriver, true, true};
    struct Result {
      Key* k = nullptr;
      float4* b = nullptr;
      int* i = nullptr;
      std::vector<Key> hk;
      std::vector<float4> hb;
      std::vector<int> hi;
    } out[kV];
    std::vector<void*> owned;
    hipError_t e = hipSuccess;
    auto device = [&](auto** p, size_t count) {
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(**p));
      if (e == hipSuccess) owned.push_back(*p);
    };
    auto to_host = [&](auto& h, const auto* d) {
      h.resize(n);
      if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, n * sizeof(*d), hipMemcpyDeviceToHost, st);
    };
    Key* k_in = nullptr;
    float4* b_in = nullptr;
    int* i_in = nullptr;
    char* tmp = nullptr;
    size_t tmp_bytes = 0;
    SortErrorWord err;
    device(&k_in, n);
    if constexpr (BODY) device(&b_in, n);
    else device(&i_in, n);
    err.alloc();
    if (e == hipSuccess && !err.dev) e = hipErrorMapFailed;
    for (int v = 0; v < kV; v++) {
      device(&out[v].k, n);
      if constexpr (BODY) device(&out[v].b, n);
      device(&out[v].i, n);
    }
    if (e == hipSuccess) e = temp_bytes(tmp_bytes, n, begin_bit, end_bit, st);
    device(&tmp, tmp_bytes > 0 ? tmp_bytes : 16);
    if (e == hipSuccess) e = hipMemcpyAsync(k_in, hk.data(), n * sizeof(Key), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && BODY) e = hipMemcpyAsync(b_in, hb.data(), n * sizeof(float4), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !BODY) e = hipMemcpyAsync(i_in, hi.data(), n * sizeof(int), hipMemcpyHostToDevice, st);
    for (int v = 0; v < kV && e == hipSuccess; v++) {
      if (!have[v]) continue;
      size_t tb = tmp_bytes;
      e = run(impl[v], tmp, tb, k_in, out[v].k, b_in, out[v].b, i_in, out[v].i, n, begin_bit, end_bit, st, err.dev);
    }
    for (int v = 0; v < kV; v++) {
      if (!have[v]) continue;
      to_host(out[v].hk, out[v].k);
      if constexpr (BODY) to_host(out[v].hb, out[v].b);
      to_host(out[v].hi, out[v].i);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    const bool ran = e == hipSuccess;
    bool same[kV] = {false, true, false};
    if (ran) {
      const Result& ref = out[kRef];
      bool sorted = true;
      for (size_t i = 1; sorted && i < n; i++) sorted = (ref.hk[i - 1] >> begin_bit) <= (ref.hk[i] >> begin_bit);
      for (int v = 0; v < kV; v++) {
        if (v == kRef) continue;
        same[v] = have[v] && sorted && std::memcmp(out[v].hk.data(), ref.hk.data(), n * sizeof(Key)) == 0 &&
                  std::memcmp(out[v].hi.data(), ref.hi.data(), n * sizeof(int)) == 0;
        if constexpr (BODY) same[v] = same[v] && std::memcmp(out[v].hb.data(), ref.hb.data(), n * sizeof(float4)) == 0;
      }
      if (err.raised()) same[2] = false;  // (a look-back of the hand-written sort gave up)
    }
    (void)hipGetLastError();
    for (void* p : owned) (void)hipFree(p);
    err.release();
    if (have[0]) driver_sort_verdict.report(same[0], who);
    own_sort_verdict.report(same[2], who);
  }
};

}  // namespace nbh
