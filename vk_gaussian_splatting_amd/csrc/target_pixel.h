// target_pixel.h — a pixel of the frame image in its target format (device_types.h: kTargetF32, kTargetF16, kTargetU8): the one load
// and the one store of every kernel that reads or writes the image, with a compile-time format (k_light) or a run-time one.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace mgs {

// RGBA16F widens exactly; RGBA8 UNORM is value / 255
__device__ __forceinline__ float4 loadPixel(const void* image, int fmt, size_t o)
{
  if(fmt == kTargetF16)
  {
    const uint2  pk = reinterpret_cast<const uint2*>(image)[o];
    const float2 lo = __half22float2(*reinterpret_cast<const __half2*>(&pk.x)), hi = __half22float2(*reinterpret_cast<const __half2*>(&pk.y));
    return make_float4(lo.x, lo.y, hi.x, hi.y);
  }
  if(fmt == kTargetU8)
  {
    const uint32_t pk = reinterpret_cast<const uint32_t*>(image)[o];
    return make_float4((float)(pk & 255u) / 255.0f, (float)((pk >> 8) & 255u) / 255.0f, (float)((pk >> 16) & 255u) / 255.0f, (float)(pk >> 24) / 255.0f);
  }
  return reinterpret_cast<const float4*>(image)[o];
}

// RGBA16F rounds to nearest even; RGBA8 UNORM clamps, scales and rounds to nearest
__device__ __forceinline__ void storePixel(void* image, int fmt, size_t o, float r, float g, float b, float a)
{
  if(fmt == kTargetF16)
  {
    const __half2 lo = __floats2half2_rn(r, g), hi = __floats2half2_rn(b, a);
    uint2         pk;
    pk.x = *reinterpret_cast<const uint32_t*>(&lo);
    pk.y = *reinterpret_cast<const uint32_t*>(&hi);
    reinterpret_cast<uint2*>(image)[o] = pk;
  }
  else if(fmt == kTargetU8)
  {
    auto q8 = [](float v) { return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); };
    reinterpret_cast<uint32_t*>(image)[o] = q8(r) | (q8(g) << 8) | (q8(b) << 16) | (q8(a) << 24);
  }
  else
    reinterpret_cast<float4*>(image)[o] = make_float4(r, g, b, a);
}

}  // namespace mgs
