// trace_lights.h — lighting a surface point with the scene's lights and their shadow rays, once: the light pass of the lit and hybrid
// frames (k_trace_light.hip), the lit mesh composite (k_trace_mesh.hip), both shading sites of a bounce (k_trace_bounce.hip) and the
// light queries (k_shadow_query.hip) call it.
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:1113-1143,1179-1255   the loops over the lights of evaluateLightingAndShading{Particles,Meshes}, headlight
//   shaders/threedgrt_raytrace.rgen.slang:1262-1341   traceShadowRayForLight: the meshes first (traceShadowRayMesh), then the particles
// Per light: the light vector (hard, or under SOFT the disk sample of shade_direct.h), under MESH the opaque occlusion walk over the
// triangle hierarchy (mesh_traverse.h) from the un-offset origin with the window (0.001, lightDist - 0.001), then the shadow ray
// through the particles (trace_shadow.h) from the offset origin, the < 0.001 in-shadow test and shadeDirectT<true>.  A light out of
// range is skipped before anything happens, ambient term included.  With it: the small pieces every site needs around the loop (the
// lane's integer sums, the instance of a splat id, the material of a mesh hit record, the shadow ray's set-up); the materials and
// the headlight are shade_direct.h's, which the raster passes share.  Bounded: lights by kMaxLights, instances by kMaxInstances, the
// walks as their headers say.  Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include "mesh_traverse.h"
#include "shade_direct.h"
#include "trace_shadow.h"
#include "trace_traverse.h"

namespace mgs {

namespace {

// the integer sums of a lane's shadow rays: the particle rays' (TraceLightCounters) and the mesh occlusion rays' (MeshRayCounters)
struct ShadowSums
{
  uint32_t           shadowHits = 0;
  unsigned long long shadowRays = 0, nodeVisits = 0, candTests = 0, meshNodeVisits = 0, meshTriTests = 0, meshOccluded = 0;
};

// what the loop reads of a frame's or a query's arguments
struct LightLoopArgs
{
  const LightTable* table;
  int32_t           shadowsMode;  // MGS_SHADOWS_*: 0 traces nothing
  float             shadowOffset;
  ShadowKnobs       knobs;
  const float*      cameraPos;  // [3] the headlight's position
};
__device__ __forceinline__ LightLoopArgs lightLoopArgs(const TraceLightArgs& L, const FrameConst& F)
{
  return {L.table, L.shadowsMode, L.shadowOffset, {L.shFormat, L.shadowThreshold, L.shadowColorStrength}, F.cameraPos};
}

// the instance that owns a global splat id: the last one whose first global id is not above it
__device__ __forceinline__ int splatInstance(const FrameArgs* Ap, uint32_t id)
{
  int inst = 0;
  for(int i = 1; i < Ap->f.nInstances; ++i)  // bound: kMaxInstances
    if(id >= Ap->inst[i].globalOffset)
      inst = i;
  return inst;
}

// the material of a mesh hit record's first word (t, instance, primitive, material), unweighted
__device__ __forceinline__ Mat meshMaterial(const MeshTable* table, const float4& h0)
{
  return material(table->inst[__float_as_uint(h0.y)].mats[__float_as_uint(h0.w)]);
}

// the ray from a point along a direction (not necessarily of unit length: t runs along it) with its three reciprocals
__device__ __forceinline__ TraceRay shadowRay(V3 from, V3 dir)
{
  TraceRay r;
  r.o[0] = from.x; r.o[1] = from.y; r.o[2] = from.z;
  r.d[0] = dir.x; r.d[1] = dir.y; r.d[2] = dir.z;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    r.inv[c] = 1.0f / r.d[c];
  return r;
}

// KB: K-buffer slots in registers of the particle shadow rays (>= samples_per_pass); MESH: meshes are in the traced scene, every
// shadow ray asks them first (m, SM: the triangle hierarchy and its LDS block, read under MESH only; null otherwise); SOFT: MGS_SHADOWS_SOFT, the lights
// with a radius are sampled on their disk from the pixel's random state `seed`, which the hard instantiation never reads.  a, S: the
// splat hierarchy and its LDS block.  Adds the lights' terms to `color` and the rays' counts to `sums`.  Returns whether a light
// shaded the point: one in range, or the headlight.
template <int KB, bool MESH, bool SOFT>
__device__ __forceinline__ bool shadeLights(const LightLoopArgs& g, const TraceArgs& a, TraceLds& S, const TraceMeshArgs* m, TraceLds* SM, int tid,
                                            const Mat& mat, V3 worldPos, V3 normal, V3 rayDir, uint32_t& seedIo, V3& colorIo, ShadowSums& sumsIo)
{
  // the three in-out values live in locals over the loop and are written back once: updated through the references, the inlined
  // loop takes more VGPRs than the loop written out at the site (profiles/light_loop_kernel_digest.txt)
  uint32_t   seed  = seedIo;
  V3         color = colorIo;
  ShadowSums sums  = sumsIo;
  const int  count = g.table->count;
  bool       any   = count == 0;
  for(int l = 0; l < count; ++l)  // bound: kMaxLights
  {
    const LightDev& light = g.table->lights[l];
    V3    lightDir;
    float lightDist;
    if(!(SOFT ? lightToSurfaceSoft(light, worldPos, seed, lightDir, lightDist) : lightToSurface(light, worldPos, lightDir, lightDist)))
      continue;  // culled before anything happens: no ambient term either (rgen.slang:1120-1121, :1186-1187, :1230-1231)
    any = true;
    V3   shadowT  = {1.0f, 1.0f, 1.0f};
    bool inShadow = false;
    if(g.shadowsMode != 0)
    {  // traceShadowRayForLight (:1262-1292)
      TraceRay sr;
      bool     occluded = false;
      if constexpr(MESH)
      {  // traceShadowRayMesh (:1295-1341): from the un-offset origin, window (0.001, lightDist - 0.001)
        sr = shadowRay(worldPos, lightDir);
        const MeshBest mb = meshWalk<1>(m->h, *SM, tid, m->tris, m->table, sr, 0.001f, lightDist - 0.001f, sums.meshNodeVisits, sums.meshTriTests);
        occluded = mb.t < __builtin_huge_valf();
      }
      if(occluded)
      {  // opaque: the particles are not asked (:1285)
        ++sums.meshOccluded;
        shadowT  = {0.0f, 0.0f, 0.0f};
        inShadow = true;
      }
      else if(a.nLevels > 0)
      {  // traceShadowRayParticle (:1344-1464; trace_shadow.h) from the offset origin, TMin 0
        ++sums.shadowRays;
        const V3 from = worldPos + lightDir * g.shadowOffset;
        if constexpr(MESH)
        {  // the mesh ray re-aimed: its direction and reciprocals stay (the form the composite and the bounce had)
          sr.o[0] = from.x; sr.o[1] = from.y; sr.o[2] = from.z;
        }
        else
          sr = shadowRay(from, lightDir);
        shadowT  = traceShadowRayParticle<KB>(a, S, tid, sr, 0.0f, lightDist, g.knobs, sums.shadowHits, sums.nodeVisits, sums.candTests);
        inShadow = fmaxf(fmaxf(shadowT.x, shadowT.y), shadowT.z) < 0.001f;  // :1127, :1236
      }
    }
    shadeDirectT<true>(light, worldPos, normal, mat, rayDir, shadowT, inShadow, color);
  }
  if(count == 0)  // never shadowed (:1137-1143, :1246-1252)
    shadeDirect(headlight(g.cameraPos), worldPos, normal, mat, rayDir, color);
  seedIo  = seed;
  colorIo = color;
  sumsIo  = sums;
  return any;
}

}  // namespace

}  // namespace mgs
