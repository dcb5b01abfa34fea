// device_arrays.h -- a set of device arrays as a table of {pointer, bytes, cleared or not}, and the routine that
// replaces such a set as a whole.  Plain C++17, no HIP include: the allocator, the release and the clear are passed in, so
// tree_plan_check.cpp and grid_plan_check.cpp run it on a CPU with malloc and an allocator that fails at a chosen step.
// Shared by tree_plan.h (barnes_hut.hip) and grid_plan.h (spatial_hash.hip).
#pragma once

#include <cstddef>

namespace nbh {

struct ArraySlot {
  void** ptr;
  size_t bytes;
  bool zero;  // cleared after the allocation
};
template <class T>
inline ArraySlot array_slot(T** p, size_t count, bool zero = false) {
  return ArraySlot{reinterpret_cast<void**>(p), count * sizeof(T), zero};
}

// free and null every array; the capacity they were sized for is void
template <class Free>
inline void release_arrays(const ArraySlot* slots, int count, int* capacity, Free&& release) {
  for (int k = 0; k < count; k++) {
    if (*slots[k].ptr) release(*slots[k].ptr);
    *slots[k].ptr = nullptr;
  }
  if (capacity) *capacity = 0;
}

// free, null, allocate, zero.  allocate(void**, bytes) and zero(void*, bytes) return 0 or an error code; the first
// error is returned with EVERYTHING freed and nulled and the capacity 0 -- a capacity is only ever written beside a
// full set of arrays.
template <class Alloc, class Free, class Zero>
inline int replace_arrays(const ArraySlot* slots, int count, int* capacity, int new_capacity, Alloc&& allocate,
                          Free&& release, Zero&& zero) {
  release_arrays(slots, count, capacity, release);
  for (int k = 0; k < count; k++) {
    int e = allocate(slots[k].ptr, slots[k].bytes > 0 ? slots[k].bytes : (size_t)16);
    if (e == 0 && slots[k].zero) e = zero(*slots[k].ptr, slots[k].bytes);
    if (e != 0) {
      release_arrays(slots, count, capacity, release);
      return e;
    }
  }
  if (capacity) *capacity = new_capacity;
  return 0;
}

}  // namespace nbh
