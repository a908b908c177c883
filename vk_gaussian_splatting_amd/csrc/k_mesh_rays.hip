// k_mesh_rays.hip — mesh ray queries (mgs_trace_mesh_rays, mgs_trace_mesh_rays_device) for gfx950: the caller's rays against the
// scene's triangle meshes, closest hit or occlusion.
//
// Replaces, for rays the caller supplies,
//   shaders/threedgrt_raytrace.rgen.slang:495-553     traceBounceRayMeshes: the closest mesh hit of a ray
//   shaders/threedgrt_raytrace.rchit.slang:31-67      the closest-hit shader: barycentrics, world position, world normal, ids
//   shaders/threedgrt_raytrace.rgen.slang:1295-1341   traceShadowRayMesh: is anything hit in the window
// and the fixed-function ray/triangle test behind them.
// Structure: one ray per lane, 256 lanes per workgroup; lane i of workgroup b takes ray perm[b * 256 + i], or b * 256 + i in the
// caller's order.  The walk is traverseProxies of trace_traverse.h as it stands (slabHit, one LDS word per level, nearest children
// first, a cut the candidate lowers); the existing kernels are not routed through anything new.  Every loop is bounded: the
// traversal by 2 * nodes + 2 steps, children by 8.  Nothing waits on another lane, wave or workgroup, and no lane returns early.
#include "kernels_common.h"
#include "launchers.h"
#include "mesh_traverse.h"
#include "trace_common.h"
#include "trace_traverse.h"

namespace mgs {

// MODE 0: closest hit (t, ids, barycentrics, world position and normal); MODE 1: occlusion (the hit flag alone; the walk's cut drops
// below every entry distance at the first hit, so nothing more is opened)
template <int MODE>
__global__ __launch_bounds__(256) void k_mesh_rays(MeshRayArgs q)
{
  __shared__ TraceLds S;
  const TraceArgs&    a   = q.t;
  const int           tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  const uint32_t slot = blockIdx.x * 256u + (uint32_t)tid;
  const bool     live = slot < q.count;
  const uint32_t idx  = live ? (q.perm ? q.perm[slot] : slot) : 0u;
  const bool     inRange = live && idx < q.count;  // (a permutation is the library's own; the bound keeps a stray index inside the arrays)
  float4         ro = make_float4(0.f, 0.f, 0.f, 1.f), rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if(inRange)
  {
    ro = q.rays[2 * (size_t)idx];
    rd = q.rays[2 * (size_t)idx + 1];
  }
  const bool rayOk = inRange && rayValid(ro, rd);
  TraceRay   ray;
  ray.o[0] = ro.x; ray.o[1] = ro.y; ray.o[2] = ro.z;
  ray.d[0] = rd.x; ray.d[1] = rd.y; ray.d[2] = rd.z;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];
  const float INF  = __builtin_huge_valf();
  const float tMin = fmaxf(ro.w, 0.0f), tMax = rd.w;  // the window (tMin, tMax), both ends open

  MeshBest           best;
  unsigned long long nodeVisits = 0, triTests = 0;

  if(rayOk && a.nLevels > 0)
    best = meshWalk<MODE>(a, S, tid, q.tris, q.table, ray, tMin, tMax, nodeVisits, triTests);

  if(inRange)
  {
    const bool hit = best.t < INF;
    float4     h0 = meshMissRecord();
    float4     h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2 = h1;
    if(MODE == 0 && hit)
      meshHitRecord(q.table, best, h0, h1, h2);
    float4* H = q.hits + 4 * (size_t)idx;
    H[0] = h0;
    H[1] = h1;
    H[2] = h2;
    H[3] = make_float4(__uint_as_float(hit ? 1u : 0u), 0.f, 0.f, 0.f);
    // statistics: integer sums, so the totals do not depend on the order of arrival
    if(rayOk)
    {
      atomicAdd(&q.ctr->nodeVisits, nodeVisits);
      atomicAdd(&q.ctr->triangleTests, triTests);
      if(hit)
        atomicAdd(&q.ctr->hits, 1ull);
    }
    else
      atomicAdd(&q.ctr->invalidRays, 1u);
  }
}

void launchMeshRays(hipStream_t stream, const MeshRayArgs& a, int mode)
{
  if(a.count == 0)
    return;
  const uint32_t groups = (a.count + 255u) / 256u;
  if(mode == 1)
    hipLaunchKernelGGL(k_mesh_rays<1>, dim3(groups), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(k_mesh_rays<0>, dim3(groups), dim3(256), 0, stream, a);
}

}  // namespace mgs
