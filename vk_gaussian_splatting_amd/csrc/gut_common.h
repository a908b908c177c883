// gut_common.h — what the 3DGUT units share: the arithmetic helpers of k_project_gut.hip and k_composite_gut.hip (and of the traced
// pipeline, which evaluates the same particles), and the text the two compositors of k_composite_gut.hip have in common: the
// pixel's ray, the lens sample and the compaction of a staging round (their deferred shading stays written out: k_composite_gut.hip).
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

// particleRayMaxKernelResponse<KERNEL_DEGREE> (threedgrt.h.slang:83-127); its argument is the SQUARED canonical distance
__device__ __forceinline__ float kernelResponse(int degree, float dist2)
{
  switch(degree)
  {
    case 8: return __expf(-0.000685871056241f * (dist2 * dist2) * (dist2 * dist2));
    case 5: return __expf(-0.0185185185185f * dist2 * dist2 * sqrtf(dist2));
    case 4: return __expf(-0.0555555555556f * dist2 * dist2);
    case 3: return __expf(-0.166666666667f * dist2 * sqrtf(dist2));
    case 1: return __expf(-1.5f * sqrtf(dist2));
    case 0: return fmaxf(1.0f + -0.329630334487f * sqrtf(dist2), 0.0f);
    default: return __expf(-0.5f * dist2);
  }
}

// ---- shared by k_composite_gut and k_composite_gut2 -----------------------------------------------------------------------------
// world-space ray direction of the pixel whose centre is (pcx, pcy) (threedgut_raster.frag.slang:101-111); false: outside the
// fisheye's field of view (the fragment is discarded)
__device__ __forceinline__ bool gutPixelRay(const FrameConst& F, float pcx, float pcy, float& dxw, float& dyw, float& dzw)
{
  const float* Vi = F.viewInv;
  float        cx, cy, cz;
  bool         rayOk = true;
  if(F.cameraModel == 1)
  {  // generateFisheyeRay(position.xy, viewport, fovRad, principal 0, viewInverse), cameras.h.slang:46-82
    const float u = (pcx / ((float)F.width - 1.0f)) * 2.0f - 1.0f, v = (pcy / ((float)F.height - 1.0f)) * 2.0f - 1.0f;
    const float r = sqrtf(u * u + v * v);
    rayOk         = !(r > 1.0f);
    float phiCos  = fabsf(r) > 1e-9f ? u / r : 0.0f;
    phiCos        = fminf(fmaxf(phiCos, -1.0f), 1.0f);
    float phi     = acosf(phiCos);
    phi           = v < 0.0f ? -phi : phi;
    const float theta = r * F.fovRad * 0.5f;
    cx = cosf(phi) * sinf(theta);
    cy = -sinf(phi) * sinf(theta);
    cz = -cosf(theta);
  }
  else
  {  // generatePinholeRay(position.xy, float2(0.5), ...): the 0.5 is added to SV_Position, as the reference writes it
    const float ux = ((pcx + 0.5f) / (float)F.width) * 2.0f - 1.0f, uy = ((pcy + 0.5f) / (float)F.height) * 2.0f - 1.0f;
    const float* Pi = F.projInv;
    cx = Pi[0] * ux + Pi[4] * uy + Pi[8] + Pi[12];
    cy = Pi[1] * ux + Pi[5] * uy + Pi[9] + Pi[13];
    cz = Pi[2] * ux + Pi[6] * uy + Pi[10] + Pi[14];
  }
  dxw = Vi[0] * cx + Vi[4] * cy + Vi[8] * cz;
  dyw = Vi[1] * cx + Vi[5] * cy + Vi[9] * cz;
  dzw = Vi[2] * cx + Vi[6] * cy + Vi[10] * cz;
  const float l = rsqrtf(dxw * dxw + dyw * dyw + dzw * dzw);
  dxw *= l; dyw *= l; dzw *= l;
  return rayOk;
}

// depth of field (frag.slang:104-109, cameras.h.slang:85-108): one lens sample per pixel and frame.  The ray (dx, dy, dz) leaves
// the random lens point (lx, ly, lz) and still passes through the focal point of the pinhole ray.  HW_SQRT: the 1-ulp square root
// (k_composite_gut2) or the correctly rounded one (k_composite_gut) — each kernel keeps the one its frames were made with.
template <bool HW_SQRT>
__device__ __forceinline__ void gutLensSample(const FrameConst& F, uint32_t seed, float& lx, float& ly, float& lz, float& dx, float& dy, float& dz)
{
  const float r1 = rngRand(seed) * 6.28318530717958647692f, r2 = rngRand(seed) * F.aperture;
  const float* Vi = F.viewInv;  // camRight = mul(float4(1,0,0,0), viewInverse), camUp = mul(float4(0,1,0,0), viewInverse)
  const float c = cosf(r1), sn = sinf(r1), sq = HW_SQRT ? gSqrt(r2) : sqrtf(r2);
  lx = (c * Vi[0] + sn * Vi[4]) * sq;
  ly = (c * Vi[1] + sn * Vi[5]) * sq;
  lz = (c * Vi[2] + sn * Vi[6]) * sq;
  const float fx = dx * F.focusDist - lx, fy = dy * F.focusDist - ly, fz = dz * F.focusDist - lz;
  const float l  = rsqrtf(fx * fx + fy * fy + fz * fz);
  dx = fx * l; dy = fy * l; dz = fz * l;
}

// A staging round's survivors (ok) compacted in list order: the slot of this thread's record (meaningful where ok) and the
// round's count.  Every thread of the 256-thread workgroup calls it (one barrier); s_wc: four words of LDS, lane / w: the
// thread's lane and wave.
__device__ __forceinline__ uint32_t gutCompactSlot(bool ok, uint32_t (&s_wc)[4], int lane, int w, uint32_t& fill)
{
  const uint64_t bal = __ballot(ok);
  if(lane == 0)
    s_wc[w] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t base = 0;
  if(w > 0) base += s_wc[0];
  if(w > 1) base += s_wc[1];
  if(w > 2) base += s_wc[2];
  fill = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
  return base + lanesBelow(bal);
}

}  // namespace mgs
