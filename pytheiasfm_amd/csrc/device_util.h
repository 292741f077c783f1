// device_util.h -- the host scaffolding every entry point of libtheia_hip.so shares: the two families of HIP error macros,
// the plain hipMalloc owner, and the small launch / timing helpers.
#pragma once
#include "theia_hip_internal.h"

#include <algorithm>
#include <chrono>

// A HIP error inside a call that had its device and its memory: THEIA_HIP_ERR_INTERNAL.
#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return thip::set_error(THEIA_HIP_ERR_INTERNAL, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// A HIP error where the resources are what fails (the BA handle, RANSAC): THEIA_HIP_ERR_OUT_OF_MEMORY or
// THEIA_HIP_ERR_NO_DEVICE, with the place of the call.
#define HIP_TRYR(expr)                                                                                          \
  do {                                                                                                          \
    hipError_t e_ = (expr);                                                                                     \
    if (e_ != hipSuccess)                                                                                       \
      return thip::set_error(e_ == hipErrorOutOfMemory ? THEIA_HIP_ERR_OUT_OF_MEMORY : THEIA_HIP_ERR_NO_DEVICE, \
                             "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);        \
  } while (0)

namespace thip {

// Owner of one hipMalloc block, freed with the object.  (ba_handle.h's PoolBuf and pools.h's DBuf draw from the
// library's device cache instead.)
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  // n == 0 still allocates one element, so that p is a valid kernel argument.  A failure is reported here and cleared,
  // so that a later hipGetLastError() of an unrelated call does not find it.
  int alloc(size_t n) {
    if (hipMalloc((void**)&p, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return set_error(THEIA_HIP_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) failed", n * sizeof(T));
    }
    return 0;
  }
  // alloc(n), then the n elements of src (none when src is null: an output buffer)
  int up(const void* src, size_t n) {
    int rc = alloc(n);
    if (rc) return rc;
    if (n && src && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      return set_error(THEIA_HIP_ERR_INTERNAL, "hipMemcpy H2D failed");
    return 0;
  }
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// workgroups of `threads` that cover n items, at least one
inline int grid_of(size_t n, int threads) { return (int)std::max<size_t>(1, (n + threads - 1) / threads); }

// The loop of a stage whose stopping test runs on the device: every kernel of an iteration returns at once while the
// device state's `done` is set, so the host enqueues `chunk` iterations at a time and reads the state once per chunk.
// enqueue(): one iteration's launches; returns 0 or an error code.  Starts nothing when hs->done is already set; reads
// the state back after every chunk; returns a HIP error as HIP_TRY would.
template <class State, class Enqueue>
int run_until_done(int max_iterations, int chunk, const State* d_state, State* hs, Enqueue&& enqueue) {
  for (int enqueued = 0; !hs->done && enqueued < max_iterations;) {
    const int now = std::min(chunk, max_iterations - enqueued);
    for (int c = 0; c < now; ++c)
      if (int rc = enqueue()) return rc;
    enqueued += now;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(hs, d_state, sizeof(State), hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // namespace thip
