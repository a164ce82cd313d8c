// Host-side glue every unit shares: the owner of a call's device scratch and the one conversion
// of a HIP error into the C ABI's code and message.  Host only: nothing here is seen by device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>
#include <vector>

#include "zkfl.h"

namespace zkfl {

// Device allocations that live as long as one call: freed on every exit path.  An object that
// outlives the call takes its buffer out with keep() and frees it in its own release function.
struct DevBufs {
  std::vector<void*> p;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() {
    for (void* q : p) (void)hipFree(q);
  }
  // count elements of T plus pad_bytes; a zero count still gets one element, since callers hand
  // such pointers to zero-work launches.  *out is null on failure.
  template <class T>
  hipError_t get(T** out, size_t count, size_t pad_bytes = 0) {
    *out = nullptr;
    const hipError_t e = hipMalloc((void**)out, (count ? count : 1) * sizeof(T) + pad_bytes);
    if (e == hipSuccess) p.push_back(*out);
    return e;
  }
  // hands q over to the caller: it is no longer freed here
  template <class T>
  T* keep(T* q) {
    for (size_t i = 0; i < p.size(); i++)
      if (p[i] == q) {
        p.erase(p.begin() + i);
        break;
      }
    return q;
  }
};

// err = "<where>: <HIP's text>"; returns ZKFL_E_OOM for an allocation failure, else ZKFL_E_DEVICE.
inline int hip_rc(hipError_t e, const char* where, std::string& err) {
  err = std::string(where) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? ZKFL_E_OOM : ZKFL_E_DEVICE;
}

}  // namespace zkfl

// HIP_TRY (objects.h) for the units that report through a std::string& and not the thread's string.
#define HIP_TRY_ERR(x, where, err)                                   \
  do {                                                               \
    hipError_t _e = (x);                                             \
    if (_e != hipSuccess) return ::zkfl::hip_rc(_e, where, err);     \
  } while (0)
