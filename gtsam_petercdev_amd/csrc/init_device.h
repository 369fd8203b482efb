// init_device.h — what the device parts of the initializers (initialize.hip: InitializePose3, lago.hip: lago) share: the
// HIP error mapping, owners that free on every return path, stream-time spans, and the ordered internal handle.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "gsx_internal.h"

namespace gsx {
namespace initdev {

constexpr int kThreads = 256;

// a failed allocation is GSX_E_NOMEM, every other HIP failure GSX_E_NO_DEVICE (as HIPCHK of handle.h; there is no
// handle here to carry an error text)
#define HIPTRY(expr)                                                            \
  do {                                                                          \
    const hipError_t e__ = (expr);                                              \
    if (e__ != hipSuccess) {                                                    \
      (void)hipGetLastError();                                                  \
      return e__ == hipErrorOutOfMemory ? GSX_E_NOMEM : GSX_E_NO_DEVICE;        \
    }                                                                           \
  } while (0)

struct EventPair {  // a span of stream time; read after the stream was synchronised
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st = nullptr;
  void begin(hipStream_t s) {
    st = s;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    hipEventRecord(a, st);
  }
  void end() {
    if (b) hipEventRecord(b, st);
  }
  double ms() {
    float t = 0;
    if (!a || !b || hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&t, a, b) != hipSuccess) {
      (void)hipGetLastError();
      return 0.0;
    }
    return (double)t;
  }
  ~EventPair() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
};
inline double host_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <class T>
struct Dev {  // device allocation freed on every return path
  T* p = nullptr;
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)); }
  hipError_t upload(const std::vector<T>& v, hipStream_t st) {
    hipError_t e = alloc(v.size());
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
  }
  ~Dev() {
    if (p) hipFree(p);
  }
};
struct Handle {  // internal handle destroyed on every return path
  gsx_handle h = nullptr;
  ~Handle() {
    if (h) gsx_destroy(h);
  }
};
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) {
      hipStreamSynchronize(s);
      hipStreamDestroy(s);
    }
  }
};

inline int blocks_for(int64_t n) { return (int)((n + kThreads - 1) / kThreads); }

inline gsx_status check_device(int32_t device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n || hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    return GSX_E_NO_DEVICE;
  }
  return GSX_OK;
}

inline int64_t desc_state_size(const gsx_problem_desc* d, std::vector<int>* state_off) {
  int64_t n = 0;
  if (state_off) state_off->assign(d->n_vars, 0);
  for (int v = 0; v < d->n_vars; ++v) {
    if (state_off) (*state_off)[v] = (int)n;
    switch (d->var_types[v]) {
      case GSX_VAR_POSE2: n += 3; break;
      case GSX_VAR_POSE3: n += 12; break;
      case GSX_VAR_CAMERA: n += 17; break;
      case GSX_VAR_ROT3: n += 9; break;
      case GSX_VAR_UNIT3: n += 3; break;
      case GSX_VAR_ESSENTIAL: n += 12; break;
      default: n += d->var_dims[v];
    }
  }
  return n;
}

inline gsx_status create_ordered(const OwnedDesc& D, int32_t device, Handle& H) {
  const gsx_problem_desc v = D.view();
  gsx_status st = gsx_create(&v, device, &H.h);
  if (st != GSX_OK) return st;
  std::vector<uint64_t> ord(D.keys.size());
  st = gsx_compute_ordering(H.h, D.keys.size() > 2000 ? GSX_ORDER_ND : GSX_ORDER_MINDEGREE, ord.data());
  if (st != GSX_OK) return st;
  return gsx_set_ordering(H.h, ord.data(), (int32_t)ord.size());
}

}  // namespace initdev
}  // namespace gsx
