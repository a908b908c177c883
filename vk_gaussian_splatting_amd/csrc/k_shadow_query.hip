// k_shadow_query.hip — shadow and light queries (mgs_trace_shadow_rays, mgs_shade_points and their _device variants) for gfx950: what
// the light pass of a lit frame computes for a splat-surface pixel, for shadow rays and surface points of the caller's own.
//
// Replaces, for rays and points that do not come from the library's frames,
//   shaders/threedgrt_raytrace.rgen.slang:1344-1464   traceShadowRayParticle (trace_shadow.h, the code of k_trace_light.hip)
//   shaders/threedgrt_raytrace.rgen.slang:1082-1144   evaluateLightingAndShadingParticles at the caller's position: material, loop
//                                                     over the lights, headlight
//   shaders/wavefront.h.slang:33-70,233-280,388-403   computeLightToSurfaceVector, wavefrontComputeShadingDirectOnly (shade_direct.h)
// Structure: one ray or point per lane, 256 lanes per workgroup; lane i of workgroup b takes the item at perm[b * 256 + i], or
// b * 256 + i in the caller's order (the scheme of k_trace_rays.hip).  The K-buffer lives in registers (three instantiations: 4, 18,
// 32 slots), the traversal's stack in TraceLds; a point is lit by the loop of trace_lights.h (no meshes, hard shadows, the headlight at
// the call's camera position); the lights and the call's knobs are read through wave-uniform loads, a point's
// material through one lane-indexed 64-byte record.  Every loop is bounded: lights by kMaxLights, the traversal by 2 * nodes + 2
// steps, the walk by samples_per_pass, children by 8.  No flags, nothing waits on another lane, wave or workgroup, and no lane
// returns: a tail workgroup's spare lanes and the invalid items skip the work.  The counters are integer atomics at the end.
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "shade_direct.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_lights.h"
#include "trace_shadow.h"
#include "trace_traverse.h"

namespace mgs {

__device__ __forceinline__ bool finite3(const float4& v)
{
  const float big = 3.4028234664e38f;
  return fabsf(v.x) <= big && fabsf(v.y) <= big && fabsf(v.z) <= big;  // (a NaN fails it)
}

// KB: K-buffer slots in registers (>= samples_per_pass)
template <int KB>
__global__ __launch_bounds__(256) void k_shadow_rays(ShadowQueryArgs q)
{
  __shared__ TraceLds S;
  const TraceArgs& a   = q.t;
  const int        tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  const uint32_t slot = blockIdx.x * 256u + (uint32_t)tid;
  const bool     live = slot < q.count;
  const uint32_t idx  = live ? (q.perm ? q.perm[slot] : slot) : 0u;
  const bool     mine = live && idx < q.count;  // (a permutation is the library's own; the bound keeps a stray index from leaving the arrays)
  float4         ro = make_float4(0.f, 0.f, 0.f, 1.f), rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if(mine)
  {
    ro = q.items[2 * (size_t)idx];
    rd = q.items[2 * (size_t)idx + 1];
  }
  const bool rayOk = mine && rayValid(ro, rd);
  TraceRay   ray;
  ray.o[0] = ro.x; ray.o[1] = ro.y; ray.o[2] = ro.z;
  ray.d[0] = rd.x; ray.d[1] = rd.y; ray.d[2] = rd.z;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];

  V3                 T    = {1.0f, 1.0f, 1.0f};
  uint32_t           hits = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  const bool         traced = rayOk && a.nLevels > 0;
  if(traced)
  {  // t_max plays lightDist; the slab test starts at the origin: a ray has no hits behind it
    const ShadowKnobs knobs = {q.shFormat, q.shadowThreshold, q.shadowColorStrength};
    T = traceShadowRayParticle<KB>(a, S, tid, ray, fmaxf(ro.w, 0.0f), rd.w, knobs, hits, nodeVisits, candTests);
  }
  if(mine)
  {
    q.results[idx] = make_float4(T.x, T.y, T.z, __uint_as_float(hits));
    // statistics: integer sums, so the totals do not depend on the order of arrival
    if(traced)
    {
      atomicAdd(&a.ctr->nodeVisits, nodeVisits);
      atomicAdd(&a.ctr->candidateTests, candTests);
      atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hits);
      atomicMax(&a.ctr->maxPassesUsed, 1u);  // one collection, no second pass
    }
    else if(!rayOk)
      atomicAdd(q.invalid, 1u);
  }
}

template <int KB>
__global__ __launch_bounds__(256) void k_shade_points(ShadowQueryArgs q)
{
  __shared__ TraceLds S;
  const TraceArgs& a   = q.t;
  const int        tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  const uint32_t slot = blockIdx.x * 256u + (uint32_t)tid;
  const bool     live = slot < q.count;
  const uint32_t idx  = live ? (q.perm ? q.perm[slot] : slot) : 0u;
  const bool     mine = live && idx < q.count;
  float4         p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0, p3 = p0;
  if(mine)
  {  // all four in flight before the first is used
    p0 = q.items[4 * (size_t)idx];
    p1 = q.items[4 * (size_t)idx + 1];
    p2 = q.items[4 * (size_t)idx + 2];
    p3 = q.items[4 * (size_t)idx + 3];
  }
  const uint32_t matId = __float_as_uint(p0.w);
  const bool     ok    = mine && finite3(p0) && finite3(p1) && finite3(p2) && finite3(p3) && matId < q.matCount;

  V3         color = {0.0f, 0.0f, 0.0f};
  ShadowSums sums;
  if(ok)
  {
    const V3 worldPos = {p0.x, p0.y, p0.z};
    const V3 rayDir   = {p2.x, p2.y, p2.z};
    V3       normal   = {p1.x, p1.y, p1.z};
    if(sqrtf(dot3(normal, normal)) <= 0.2f)  // surfaceFinalFiltering's fallback (rgen.slang:991-1009)
      normal = -rayDir;
    normal = normalize3(normal);
    const Mat mat = splatMaterial(q.mats[matId], V3{p3.x, p3.y, p3.z});
    color         = mat.emission;
    if(mat.needShading != 0)
    {  // no meshes; hard shadows
      const LightLoopArgs g = {q.table, q.shadowsMode, q.shadowOffset, {q.shFormat, q.shadowThreshold, q.shadowColorStrength}, q.cameraPos};
      uint32_t            noSeed = 0u;
      (void)shadeLights<KB, false, false>(g, a, S, nullptr, nullptr, tid, mat, worldPos, normal, rayDir, noSeed, color, sums);
    }
  }
  if(mine)
  {
    q.results[idx] = make_float4(color.x, color.y, color.z, __uint_as_float(sums.shadowHits));
    if(ok)
    {
      atomicAdd(&q.lctr->shadowRays, sums.shadowRays);
      atomicAdd(&q.lctr->nodeVisits, sums.nodeVisits);
      atomicAdd(&q.lctr->candidateTests, sums.candTests);
      atomicAdd(&q.lctr->acceptedHits, (unsigned long long)sums.shadowHits);
    }
    else
      atomicAdd(q.invalid, 1u);
  }
}

void launchShadowRays(hipStream_t stream, const ShadowQueryArgs& a)
{
  if(a.count == 0)
    return;
  const uint32_t groups = (a.count + 255u) / 256u;
  withKBuffer("launchShadowRays", a.t.samplesPerPass,
              [&](auto kb) { hipLaunchKernelGGL((k_shadow_rays<decltype(kb)::value>), dim3(groups), dim3(256), 0, stream, a); });
}

void launchShadePoints(hipStream_t stream, const ShadowQueryArgs& a)
{
  if(a.count == 0)
    return;
  const uint32_t groups = (a.count + 255u) / 256u;
  withKBuffer("launchShadePoints", a.t.samplesPerPass,
              [&](auto kb) { hipLaunchKernelGGL((k_shade_points<decltype(kb)::value>), dim3(groups), dim3(256), 0, stream, a); });
}

}  // namespace mgs
