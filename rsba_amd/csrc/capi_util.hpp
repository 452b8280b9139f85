// What the C-ABI entry points share on the host (capi.hip, pnp_capi.hip, match_capi.hip, tracks_capi.hip, filter_capi.hip, through
// pair_capi_util.hpp epipolar_capi.hip and homography_capi.hip, and, through solver.hpp, the solver's units): a HIP error turned into the library's error code and message, the check of the device
// ordinal, the device buffers of a stateless call and the copy of its accepted results to the caller.  Host-side glue only; private to the
// library: nothing here is part of its surface.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "handle.hpp"

// returns from the calling function with RSBA_ERR_OUT_OF_MEMORY / RSBA_ERR_HIP and "<expr>: <HIP's text>" as the message
#define RSBA_HIP_TRY(expr)                                                                            \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return rsba_set_error(e_ == hipErrorOutOfMemory ? RSBA_ERR_OUT_OF_MEMORY : RSBA_ERR_HIP,        \
                            (std::string(#expr) + ": " + hipGetErrorString(e_)).c_str());             \
  } while (0)

#pragma GCC visibility push(hidden)

// the device ordinal names a device: the check alone, for the calls whose arena sets the device itself
inline int32_t rsba_check_device(int32_t device) {
  int32_t ndev = 0;
  int32_t rc = rsba_device_count(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev) return rsba_set_error(RSBA_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  return RSBA_OK;
}

inline int32_t rsba_select_device(int32_t device) {
  int32_t rc = rsba_check_device(device);
  if (rc) return rc;
  RSBA_HIP_TRY(hipSetDevice(device));
  return RSBA_OK;
}

namespace rsba {

// device allocations of one stateless call, freed when it returns
struct DeviceBuffers {
  std::vector<void*> ptrs;
  ~DeviceBuffers() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> hipError_t upload(const T** out, const T* src, size_t count) {
    T* p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return e;
    ptrs.push_back(p);
    *out = p;
    return count ? hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
  template <class T> hipError_t alloc(T** out, size_t count) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(out), (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) ptrs.push_back(*out);
    return e;
  }
};

// What a hypothesis kernel left on the device, to the caller's arrays: the status bytes d_status [num_tasks] to status (and to st), and of
// d_values [num_tasks][width] the slots of the accepted tasks (status != 0) to values_out; declined slots are left as they are.  With d_status
// null, st already holds the status bytes (a second array of the same tasks) and only the values are copied.
inline int32_t download_accepted(const uint8_t* d_status, const double* d_values, int width, int32_t num_tasks, uint8_t* status, double* values_out,
                                 std::vector<uint8_t>& st) {
  std::vector<double> values((size_t)num_tasks * width);
  RSBA_HIP_TRY(hipMemcpy(values.data(), d_values, values.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (d_status) {
    st.resize((size_t)num_tasks);
    RSBA_HIP_TRY(hipMemcpy(st.data(), d_status, st.size(), hipMemcpyDeviceToHost));
  }
  for (size_t t = 0; t < (size_t)num_tasks; ++t) {
    if (d_status) status[t] = st[t];
    if (st[t]) for (int k = 0; k < width; ++k) values_out[t * width + k] = values[t * width + k];
  }
  return RSBA_OK;
}

}  // namespace rsba

#pragma GCC visibility pop
