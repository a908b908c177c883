// k_trace_mesh.hip — triangle meshes in the traced frames (mgs_frame_set_trace_meshes; mgs_render_traced, mgs_render_traced_lit)
// for gfx950: every pixel's closest mesh hit in front of the particle walk, and the mesh's pixel behind it.
//
// Replaces, at bounce 0,
//   shaders/threedgrt_raytrace.rgen.slang:495-553     traceBounceRayMeshes: the closest mesh hit of the primary ray
//   shaders/threedgrt_raytrace.rgen.slang:1058-1075   the mesh parts of evaluateLightingAndShadingForBounce: the unlit composite
//   shaders/threedgrt_raytrace.rgen.slang:1148-1165,1222-1255   evaluateLightingAndShadingMeshes, direct mode
//   shaders/threedgrt_raytrace.rgen.slang:1262-1341   traceShadowRayForLight: meshes first, then the particles
//   shaders/threedgrt_raytrace.rgen.slang:1490-1502   the depth of a pixel whose primary hit is a mesh
// Structure: a lane per pixel in k_trace's tiling (a wave64 = an 8 x 8 pixel tile, a workgroup = a 16 x 16 tile, strip rows
// honoured).  k_trace_mesh_primary runs the closest walk of mesh_traverse.h on the ray k_trace traces (trace_primary_ray.h) and
// leaves the pixel's 64-byte hit record and its t; k_trace cuts its walk there and leaves float(T); k_trace_mesh_composite adds the
// mesh's radiance to the fp32 pixel k_trace (unlit) or the light pass (lit) left and stores the pixel again.  In a lit frame it
// lights the mesh's surface point with the loop of trace_lights.h: per light the mesh occlusion ray, then the shadow ray through the
// particles.  Every loop is bounded: lights by kMaxLights, the traversals by 2 * nodes + 2 steps, the walk by samples_per_pass, children
// by 8.  No flags, nothing waits on another lane, wave or workgroup; the counters are integer atomics at the end.
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "mesh_traverse.h"
#include "shade_direct.h"
#include "target_pixel.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_lights.h"
#include "trace_primary_ray.h"
#include "trace_traverse.h"

namespace mgs {

__global__ __launch_bounds__(256) void k_trace_mesh_primary(TraceMeshArgs m, const FrameArgs* __restrict__ Ap)
{
  __shared__ TraceLds S;
  const FrameConst&   F   = Ap->f;
  const int           tid = threadIdx.x;
  traceLdsInit(S, m.h, tid);
  int px, py;
  tilePixel(F, tid, px, py);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;

  TraceRay   ray;
  const bool rayOk = primaryRayAsTraced(F, px, py, ray.o, ray.d);
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];

  MeshBest           best;
  unsigned long long nodeVisits = 0, triTests = 0;
  if(rayOk && m.h.nLevels > 0)  // the window of rgen.slang:521-522; epsT = 1e-9 vanishes in fp32
    best = meshWalk<0>(m.h, S, tid, m.tris, m.table, ray, 0.001f, 10000.0f, nodeVisits, triTests);

  const bool hit = best.t < __builtin_huge_valf();
  float4     h0 = meshMissRecord();
  float4     h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2 = h1;
  if(hit)
    meshHitRecord(m.table, best, h0, h1, h2);
  float4* H = m.hits + 4 * pix;
  H[0] = h0;
  H[1] = h1;
  H[2] = h2;
  H[3] = make_float4(__uint_as_float(hit ? 1u : 0u), 0.f, 0.f, 0.f);
  m.meshT[pix] = best.t;
  // statistics: integer sums, so the totals do not depend on the order of arrival
  if(rayOk)
  {
    atomicAdd(&m.ctr[0].nodeVisits, nodeVisits);
    atomicAdd(&m.ctr[0].triangleTests, triTests);
    if(hit)
      atomicAdd(&m.ctr[0].hits, 1ull);
  }
  else
    atomicAdd(&m.ctr[0].invalidRays, 1u);
}

// KB: K-buffer slots in registers of the particle shadow rays (>= samples_per_pass; 4 in an unlit frame, which traces none);
// LIT: the mesh shading of mgs_render_traced_lit, otherwise the unlit composite of mgs_render_traced; SOFT (LIT only):
// MGS_SHADOWS_SOFT, the lights with a radius are sampled on their disk (lightToSurfaceSoft).  The pixel's random state is ONE for
// both light loops of a pixel (rgen.slang:1054, :1061, the same inout seed): the mesh loop continues where the splat surface's loop
// in k_trace_light ended.  That loop draws two numbers per point or spot light with a radius, culled or not, so its end state is
// recomputed here from the light table and the light pass's own conditions for running its loop; no per-pixel word is carried.
// HYBRID (LIT, not SOFT): the composite of a hybrid frame with meshes (mgs_frame_set_hybrid_meshes).  The base colour and T are the
// hand-over's (k_hybrid.hip), which has already applied discardSplatContribution and splatIsClosest to the raster surface: the traced
// frame's rule below would be wrong for its settled pixels, whose ray parameter is negative and whose colour and T are their own
template <int KB, bool LIT, bool SOFT, bool HYBRID = false>
__global__ __launch_bounds__(256) void k_trace_mesh_composite(TraceLightMeshArgs args)
{
  const TraceLightArgs& L = args.l;
  __shared__ TraceLds S;
  __shared__ TraceLds SM;
  const TraceArgs&  a  = L.t;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x;
  if constexpr(LIT)
    traceLdsInit(S, a, tid);
  traceLdsInit(SM, args.m.h, tid);
  int px, py;
  tilePixel(F, tid, px, py);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;

  const float4 h0 = args.m.hits[4 * pix];
  const float  tMesh = h0.x;
  if(!(tMesh < __builtin_huge_valf()))
    return;  // no mesh behind this pixel: what k_trace or the light pass stored stays
  const float4   h1 = args.m.hits[4 * pix + 1], h2 = args.m.hits[4 * pix + 2];
  const float4   base   = L.radiance[pix];
  float          walkT  = args.m.walkT[pix];
  const uint32_t pickId = a.outId != nullptr ? a.outId[pix] : (LIT ? L.pickId[pix] : kTraceInvalid);
  TraceRay   ray;
  (void)primaryRayAsTraced(F, px, py, ray.o, ray.d);  // the ray that found the hit (a mesh hit: the ray is valid)
  const V3 rayDir = {ray.d[0], ray.d[1], ray.d[2]};

  if(a.outDepth != nullptr && pickId == kTraceInvalid)
  {  // ndc z of primaryHitPos = origin + t_mesh * direction (:547-551, :1490-1494); an iso pick, nearer, keeps its own
    const float  hx = ray.o[0] + tMesh * ray.d[0], hy = ray.o[1] + tMesh * ray.d[1], hz = ray.o[2] + tMesh * ray.d[2];
    const float *V = F.view, *P = F.proj;
    const float  v0 = V[0] * hx + V[4] * hy + V[8] * hz + V[12], v1 = V[1] * hx + V[5] * hy + V[9] * hz + V[13],
                v2 = V[2] * hx + V[6] * hy + V[10] * hz + V[14], v3 = V[3] * hx + V[7] * hy + V[11] * hz + V[15];
    const float cz = P[2] * v0 + P[6] * v1 + P[10] * v2 + P[14] * v3, cw = P[3] * v0 + P[7] * v1 + P[11] * v2 + P[15] * v3;
    a.outDepth[pix] = cz / cw;
  }

  V3   color = {base.x, base.y, base.z};
  bool splatShaded = false;  // SOFT: the light pass reached its loop over the lights on this pixel
  if constexpr(LIT && !HYBRID)
  {  // surfaceFinalFiltering and splatIsClosest as the light pass decided them: a discarded splat surface is radiance 0, T = 1
    const float isoDist = L.isoDist[pix];
    if(pickId == kTraceInvalid || !(isoDist > 0.0f) || !(isoDist < tMesh))
    {
      color = {0.0f, 0.0f, 0.0f};
      walkT = (double)1.0f > (double)args.m.minT ? 1.0f : -1.0f;
    }
    else if constexpr(SOFT)
      splatShaded = L.table->mats[splatInstance(Ap, pickId)].needShading != 0;  // as k_trace_light reads it (rgen.slang:1091-1095 returns before the loop)
  }
  if(walkT < 0.0f)
    return;  // T > min_mesh_composite_transmittance failed (:1058-1059, :1065-1066): the mesh is not composited

  const Mat  mm = meshMaterial(args.m.table, h0);
  ShadowSums sums;
  if constexpr(!LIT)
    color = color + (mm.emission + mm.ambient + mm.diffuse) * walkT;  // :1073-1074
  else
  {
    color = color + mm.emission;  // unweighted, as written (:1159)
    if(mm.needShading != 0)
    {
      // wavefrontComputeShadingDirectOnly weights the ambient and the (diffuse + specular) terms with float(T) (wavefront.h.slang:249,
      // :279): the material goes in weighted
      const Mat mat      = weightedMaterial(mm, V3{walkT, walkT, walkT});
      const V3  worldPos = {h1.x, h1.y, h1.z}, normal = {h2.x, h2.y, h2.z};  // meshHitWorldPos, meshHitWorldNrm: the closest hit's
      const int count    = L.table->count;
      uint32_t  seedRayPass = SOFT ? rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId) : 0u;  // :228
      if constexpr(SOFT)
        if(splatShaded)
          for(int l = 0; l < count; ++l)  // bound: kMaxLights.  The splat surface's loop: two draws per light with a disk
            if(L.table->lights[l].type != MGS_LIGHT_DIRECTIONAL && L.table->lights[l].radius > 0.0f)
            {
              (void)rngPcg(seedRayPass);
              (void)rngPcg(seedRayPass);
            }
      (void)shadeLights<KB, true, SOFT>(lightLoopArgs(L, F), a, S, &args.m, &SM, tid, mat, worldPos, normal, rayDir, seedRayPass, color, sums);
    }
    L.shadowHits[pix] += sums.shadowHits;  // (this lane's own word: the light pass wrote it)
  }
  storePixel(a.image, a.fmt, pix, color.x, color.y, color.z, 1.0f);  // the mesh is opaque
  if constexpr(LIT)
  {  // statistics: integer sums, so the totals do not depend on the order of arrival
    atomicAdd(&L.lctr->shadowRays, sums.shadowRays);
    atomicAdd(&L.lctr->nodeVisits, sums.nodeVisits);
    atomicAdd(&L.lctr->candidateTests, sums.candTests);
    atomicAdd(&L.lctr->acceptedHits, (unsigned long long)sums.shadowHits);
    atomicAdd(&args.m.ctr[1].nodeVisits, sums.meshNodeVisits);
    atomicAdd(&args.m.ctr[1].triangleTests, sums.meshTriTests);
    atomicAdd(&args.m.ctr[1].hits, sums.meshOccluded);
  }
}

void launchTraceMeshPrimary(hipStream_t stream, const TraceMeshArgs& m, const FrameArgs* frame, const FrameConst& F)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  hipLaunchKernelGGL(k_trace_mesh_primary, dim3(tiles), dim3(256), 0, stream, m, frame);
}

void launchTraceMeshComposite(hipStream_t stream, const TraceLightMeshArgs& L, const FrameConst& F, bool lit)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  if(!lit)
  {
    hipLaunchKernelGGL((k_trace_mesh_composite<4, false, false>), dim3(tiles), dim3(256), 0, stream, L);
    return;
  }
  withKBuffer("launchTraceMeshComposite", L.l.t.samplesPerPass, [&](auto kb) {
    if(L.l.shadowsMode == MGS_SHADOWS_SOFT)
      hipLaunchKernelGGL((k_trace_mesh_composite<decltype(kb)::value, true, true>), dim3(tiles), dim3(256), 0, stream, L);
    else
      hipLaunchKernelGGL((k_trace_mesh_composite<decltype(kb)::value, true, false>), dim3(tiles), dim3(256), 0, stream, L);
  });
}

void launchHybridMeshComposite(hipStream_t stream, const TraceLightMeshArgs& L, const FrameConst& F)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  withKBuffer("launchHybridMeshComposite", L.l.t.samplesPerPass,
              [&](auto kb) { hipLaunchKernelGGL((k_trace_mesh_composite<decltype(kb)::value, true, false, true>), dim3(tiles), dim3(256), 0, stream, L); });
}

}  // namespace mgs
