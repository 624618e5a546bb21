// wpt_launch.h — what the two kernel units (wpt_render.hip, wpt_post.hip)
// share: the error macro of their host functions, the block of the one-lane-
// per-element kernels and of the scans, and the rgb3 <-> float4 staging of the
// hooks. Internal: nothing here is part of an interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "wpt_math.h"

// In a function that returns bool and has a std::string& err.
#define HIP_OK(expr)                                                     \
  do {                                                                   \
    hipError_t e_ = (expr);                                              \
    if (e_ != hipSuccess) {                                              \
      err = std::string(#expr " failed: ") + hipGetErrorString(e_);      \
      return false;                                                      \
    }                                                                    \
  } while (0)

namespace wpt {

constexpr uint32_t kBlock = 256;
using u64 = unsigned long long;

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// The scans (u32: wpt_adaptive.h, u64: wpt_guided.h) run in chunks of
// kScanChunk elements, kScanPer per lane.
constexpr uint32_t kScanPer = 4;
constexpr uint32_t kScanChunk = kBlock * kScanPer;

__device__ __forceinline__ void st3(float* p, V3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}

// n host rgb triples as float4 (w = 0) to dst, queued on s from `stage`, which
// the caller keeps until it has waited for s.
inline hipError_t upload_rgb3(hipStream_t s, const float* rgb3, size_t n, std::vector<float4>& stage, float4* dst) {
  stage.resize(n);
  for (size_t i = 0; i < n; i++) stage[i] = make_float4(rgb3[3 * i], rgb3[3 * i + 1], rgb3[3 * i + 2], 0.0f);
  return hipMemcpyAsync(dst, stage.data(), sizeof(float4) * n, hipMemcpyHostToDevice, s);
}

// The xyz of n device float4 into host rgb triples: queued on s, then waits
// for s (and with it for the copies the caller queued before). A null rgb3
// only waits.
inline hipError_t download_rgb3(hipStream_t s, const float4* src, size_t n, float* rgb3) {
  std::vector<float4> a(rgb3 ? n : 0);
  if (rgb3) {
    const hipError_t e = hipMemcpyAsync(a.data(), src, sizeof(float4) * n, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
  }
  const hipError_t e = hipStreamSynchronize(s);
  for (size_t i = 0; i < a.size(); i++) {
    rgb3[3 * i] = a[i].x;
    rgb3[3 * i + 1] = a[i].y;
    rgb3[3 * i + 2] = a[i].z;
  }
  return e;
}

}  // namespace wpt
