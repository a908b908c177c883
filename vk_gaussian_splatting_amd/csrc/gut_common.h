// gut_common.h — the arithmetic helpers both 3DGUT units (k_project_gut.hip, k_composite_gut.hip) use.
#pragma once
#include "kernels_common.h"

namespace mgs {

// This pipeline's arithmetic has a tolerance (>= 50 dB vs the oracle), no bit-exact part except the keys of phase 1: reciprocals
// and square roots are the 1-ulp hardware instructions, not hipcc's correctly rounded expansions (10 instructions each; the
// front end had ~30 divisions per splat, the compositor one per fragment).
__device__ __forceinline__ float gRcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float gSqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// threedgut_camera_projections.h.slang:32-44
__device__ __forceinline__ float gutStableNorm2(float x, float y)
{
  const float ax = fabsf(x), ay = fabsf(y);
  const float mn = fminf(ax, ay), mx = fmaxf(ax, ay);
  if(mx <= 0.0f)
    return 0.0f;
  const float r = mn * gRcp(mx);
  return mx * gSqrt(1.0f + r * r);
}

}  // namespace mgs
