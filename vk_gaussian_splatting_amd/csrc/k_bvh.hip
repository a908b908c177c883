// k_bvh.hip — the hierarchy of the traced pipeline (mgs_render_traced) for gfx950, built on the device.
//
// Replaces
//   shaders/particle_as_build.comp.slang:74-87,109-   kernelScale and the per-particle proxy the reference hands to the acceleration
//                                                     structure build (an icosahedron or a unit box instanced per particle)
//   the BLAS / TLAS builds of the acceleration-structure managers (fixed-function; no counterpart to restate)
// Structure ("Ray-traced splats"): an implicit complete 8-ary tree over leaves sorted by the 30-bit Morton code of the
// leaf centre.  No pointers, no atomics, no flags, no waiting on another workgroup: every kernel below is a plain map over its
// output, the sort in between is the library's own (key, value) sort, and the result is bit-reproducible.
#include "kernels_common.h"
#include "launchers.h"
#include "trace_common.h"

namespace mgs {

__device__ __forceinline__ uint32_t mortonSpread10(uint32_t v)
{
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// One thread per global (storage) splat: the exact AABB of the affine image of the proxy ellipsoid.  With A = mat3(transform) R
// diag(r exp(scale)) the half extent on axis a is sqrt(sum_j A_aj^2); r is the canonical radius at which the response reaches the
// proxy threshold (trace_common.h: proxyThreshold / proxyRadius).  Inflated by 8 ulps of the half extent plus 2 ulps of the centre's
// magnitude, which covers the rounding of the nine products, the sum, the square root and the centre's transform (each below 1 ulp
// relative to the quantity it rounds).  No leaf: density <= alphaCullThreshold (particleProcessHit rejects every hit,
// threedgrt.h.slang:166-170), a non-finite bound.
__global__ __launch_bounds__(256) void k_bvh_leaves(BvhBuildArgs a)
{
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if(g >= a.totalSplats)
    return;
  const FrameArgs* Ap = a.frame;
  int              k  = 0;
  for(int i = 1; i < Ap->f.nInstances; ++i)  // bound: kMaxInstances
    if(g >= Ap->inst[i].globalOffset)
      k = i;
  const InstanceConst& I  = Ap->inst[k];
  const uint32_t       li = g - I.globalOffset;
  const float          density = I.alpha[li];
  float                R[9], s[3], p[3];
  loadParticle(I, li, R, s, p);
  const float  r = proxyRadius(a.proxy, proxyThreshold(a.proxy, density));
  const float* M = I.model;
  float        h[3];
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
  {
    float sum = 0.0f;
#pragma unroll
    for(int j = 0; j < 3; ++j)
    {  // (mat3(M) R)_{ax, j} * r * s_j
      const float mr = M[ax] * R[j] + M[4 + ax] * R[3 + j] + M[8 + ax] * R[6 + j];
      const float e  = mr * (r * s[j]);
      sum += e * e;
    }
    h[ax] = sqrtf(sum);
  }
  float c[3];
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
    c[ax] = M[ax] * p[0] + M[4 + ax] * p[1] + M[8 + ax] * p[2] + M[12 + ax];
  bool   ok = density > a.proxy.alphaCull;
  float4 lo, hi;
  float  q[3];
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
  {
    const float hh = h[ax] * (1.0f + 8.0f * 1.1920929e-7f) + fabsf(c[ax]) * (2.0f * 1.1920929e-7f);
    const float l = c[ax] - hh, u = c[ax] + hh;
    ok = ok && isfinite(l) && isfinite(u) && hh >= 0.0f;
    (&lo.x)[ax] = l;
    (&hi.x)[ax] = u;
    q[ax]       = fminf(fmaxf((c[ax] - a.sceneLo[ax]) * a.sceneInvExt[ax], 0.0f), 1.0f) * 1023.0f;
  }
  lo.w = __uint_as_float(g);
  hi.w = 0.0f;
  uint32_t key = kTraceInvalid;
  if(ok)
    key = mortonSpread10((uint32_t)q[0]) | (mortonSpread10((uint32_t)q[1]) << 1) | (mortonSpread10((uint32_t)q[2]) << 2);
  a.keys[g]            = key;
  a.vals[g]            = g;
  a.leafBox[2 * (size_t)g]     = lo;
  a.leafBox[2 * (size_t)g + 1] = hi;
}

// the number of valid leaves = the position of the first invalid key in the sorted array (Morton codes have 30 bits, the invalid
// key is all ones): exactly one thread finds the boundary.  *countOut is zeroed by the caller (all keys invalid: stays 0).
__global__ __launch_bounds__(256) void k_bvh_count(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ countOut)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n || keys[i] == kTraceInvalid)
    return;
  if(i + 1u == n || keys[i + 1u] == kTraceInvalid)
    *countOut = i + 1u;
}

__global__ __launch_bounds__(256) void k_bvh_gather(const uint32_t* __restrict__ vals, const float4* __restrict__ leafBox,
                                                    float4* __restrict__ level0, uint32_t nLeaves)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= nLeaves)
    return;
  const uint32_t g = vals[i];
  level0[2 * (size_t)i]     = leafBox[2 * (size_t)g];
  level0[2 * (size_t)i + 1] = leafBox[2 * (size_t)g + 1];
}

// node i of this level = the union of the children [8i, 8i + 8) of the level below (min / max: exact, no rounding)
__global__ __launch_bounds__(256) void k_bvh_level(const float4* __restrict__ below, uint32_t nBelow, float4* __restrict__ level,
                                                   uint32_t nLevel)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= nLevel)
    return;
  const uint32_t c0 = 8u * i, c1 = min(c0 + 8u, nBelow);
  float4         lo = below[2 * (size_t)c0], hi = below[2 * (size_t)c0 + 1];
  for(uint32_t c = c0 + 1u; c < c1; ++c)  // bound: 8 children
  {
    const float4 l = below[2 * (size_t)c], u = below[2 * (size_t)c + 1];
    lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z);
    hi.x = fmaxf(hi.x, u.x); hi.y = fmaxf(hi.y, u.y); hi.z = fmaxf(hi.z, u.z);
  }
  lo.w = 0.0f;
  hi.w = 0.0f;
  level[2 * (size_t)i]     = lo;
  level[2 * (size_t)i + 1] = hi;
}

void launchBvhLeaves(hipStream_t stream, const BvhBuildArgs& a)
{
  if(a.totalSplats)
    hipLaunchKernelGGL(k_bvh_leaves, dim3((a.totalSplats + 255u) / 256u), dim3(256), 0, stream, a);
}
void launchBvhCount(hipStream_t stream, const uint32_t* sortedKeys, uint32_t n, uint32_t* countOut)
{
  if(n)
    hipLaunchKernelGGL(k_bvh_count, dim3((n + 255u) / 256u), dim3(256), 0, stream, sortedKeys, n, countOut);
}
void launchBvhGather(hipStream_t stream, const uint32_t* sortedVals, const float4* leafBox, float4* level0, uint32_t nLeaves)
{
  if(nLeaves)
    hipLaunchKernelGGL(k_bvh_gather, dim3((nLeaves + 255u) / 256u), dim3(256), 0, stream, sortedVals, leafBox, level0, nLeaves);
}
void launchBvhLevel(hipStream_t stream, const float4* below, uint32_t nBelow, float4* level, uint32_t nLevel)
{
  if(nLevel)
    hipLaunchKernelGGL(k_bvh_level, dim3((nLevel + 255u) / 256u), dim3(256), 0, stream, below, nBelow, level, nLevel);
}

}  // namespace mgs
