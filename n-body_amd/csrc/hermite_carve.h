// hermite_carve.h -- one allocation carved into 256-byte aligned regions, in the order they are added: the device state
// of the block-step Hermite handles (hermite_block.hip, hermite_batch.hip).  Add the regions, read total(), allocate,
// place(base): every pointer that was added then points at its region.  Plain C++ with no device and no HIP header, so
// that hermite_handle_check.cpp can run it on a CPU under a sanitizer.
#pragma once

#include <cassert>
#include <cstddef>

namespace nbh {

class Carve {
 public:
  static constexpr size_t kAlign = 256;
  static constexpr int kMaxRegions = 16;

  // a region of `count` elements of `elem` bytes (an empty one takes no room): its offset from the base
  size_t reserve(size_t count, size_t elem) {
    const size_t at = total_;
    total_ += (count * elem + kAlign - 1) & ~(kAlign - 1);
    return at;
  }
  // the same for `count` T, and *slot is set by place() (at most kMaxRegions pointers)
  template <class T>
  void add(T** slot, size_t count) {
    assert(n_ < kMaxRegions);
    regions_[n_++] = Region{slot, &assign<T>, reserve(count, sizeof(T))};
  }
  size_t total() const { return total_; }
  void place(void* base) const {
    for (int k = 0; k < n_; k++) regions_[k].assign(regions_[k].slot, static_cast<char*>(base) + regions_[k].offset);
  }

 private:
  struct Region {
    void* slot;
    void (*assign)(void* slot, char* at);
    size_t offset;
  };
  template <class T>
  static void assign(void* slot, char* at) {
    *static_cast<T**>(slot) = reinterpret_cast<T*>(at);
  }
  Region regions_[kMaxRegions] = {};
  size_t total_ = 0;
  int n_ = 0;
};

}  // namespace nbh
