// k_trace_bounce.hip — reflection and refraction bounces off mesh materials (mgs_render_traced_indirect) for gfx950: the
// reference's LIGHTING_INDIRECT for trace strategy 0.
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:230-337     the bounce loop
//   shaders/threedgrt_raytrace.rgen.slang:505-573     the bounce ray's closest mesh hit, the reset of the iso surface
//   shaders/threedgrt_raytrace.rgen.slang:615-763     traceRayParticlesInsertionSort with the carried radiance and double3 transmittance
//   shaders/threedgrt_raytrace.rgen.slang:1037-1062   evaluateLightingAndShadingForBounce
//   shaders/threedgrt_raytrace.rgen.slang:1082-1144   evaluateLightingAndShadingParticles on radiance - radianceBeforeParticles
//   shaders/threedgrt_raytrace.rgen.slang:1148-1219   evaluateLightingAndShadingMeshes, indirect mode
//   shaders/wavefront.h.slang:282-376                 wavefrontComputeShading: the direct light term, then illum's new ray
// Structure: a lane per pixel in k_trace's tiling.  Bounce 0 is the lit mesh frame's launches as they are (k_trace_mesh_primary,
// k_trace<., ., true>, k_trace_light<., true>) followed by k_trace_bounce_primary, the lit mesh composite in the indirect mode, which
// also writes the pixel's bounce state.  Every bounce b >= 1 is ONE launch of k_trace_bounce: the closest mesh walk on the stored
// ray, the particle pass walk below that hit, the light pass of the splat surface, the mesh's indirect shading, the next ray (both
// shading sites light their point with the loop of trace_lights.h; the bounce alone reads whether a light shaded it).  The
// three stages share no register state beyond the ray, the radiance and T, so the compiler reuses the K-buffer's registers for the
// shadow walks; a split into three kernels would carry the hit record, the pick and the normal through memory as well.  A lane
// whose pixel is not live returns after the flag read.  The host enqueues max_bounces launches; nothing is read back in between.
// Every loop is bounded: lights by kMaxLights, the traversals by 2 * nodes + 2 steps, passes by max_passes, the walk by
// samples_per_pass, bounces by kMaxBounces (host).  No flags, nothing waits on another lane, wave or workgroup; the counters are
// integer atomics at the end.  LDS: the two TraceLds blocks of the lit mesh kernels.
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "mesh_traverse.h"
#include "sh_eval.h"
#include "shade_direct.h"
#include "target_pixel.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_lights.h"
#include "trace_primary_ray.h"
#include "trace_shade.h"
#include "trace_traverse.h"

namespace mgs {

namespace {

struct D3
{
  double x, y, z;
};
__device__ __forceinline__ double maxComponent(D3 t) { return fmax(fmax(t.x, t.y), t.z); }

__device__ __forceinline__ BounceMatDev bounceMaterial(const TraceBounceArgs& B, uint32_t inst, uint32_t mat)
{
  BounceMatDev m{};
  m.ior = 1.0f;
  if(mat < B.btab->count[inst])  // ids >= count, and an instance never set: illum 0
  {
    const float4* p  = reinterpret_cast<const float4*>(&B.bmats[B.btab->offset[inst] + mat]);
    const float4  q0 = p[0], q1 = p[1];
    m.transmittance[0] = q0.x; m.transmittance[1] = q0.y; m.transmittance[2] = q0.z;
    m.ior   = q0.w;
    m.illum = __float_as_int(q1.x);
  }
  return m;
}

// evaluateLightingAndShadingMeshes in the indirect mode (rgen.slang:1148-1219) at the closest hit (h0, h1, h2: its record) of the
// ray along rayDir.  weight = float3(T).  Every light in range is shaded with the T the function was entered with (:1191-1197),
// and what wavefrontComputeShading leaves of T and the ray does not depend on the light: it is applied once, when a light shaded.
// Returns done == 0: T and (newO, newD) are the next bounce's.
template <int KB>
__device__ __forceinline__ bool shadeMeshIndirect(const TraceBounceArgs& B, TraceLds& S, TraceLds& SM, int tid, const FrameConst& F, const float4& h0,
                                                  const float4& h1, const float4& h2, V3 rayDir, V3 weight, D3& T, V3& color, V3& newO, V3& newD,
                                                  ShadowSums& sums)
{
  const TraceMeshArgs& M    = B.g.m;
  const uint32_t       inst = __float_as_uint(h0.y), matId = __float_as_uint(h0.w);
  const Mat            mm   = meshMaterial(M.table, h0);
  color = color + mm.emission;  // unweighted, as written (:1159)
  if(mm.needShading == 0)
    return false;  // needShading != 1: no lighting interaction, no bounce (:1162-1165)
  // the light term weights ambient and (diffuse + specular) with float3(T) (wavefront.h.slang:303, :332): the material goes in weighted
  const Mat mat      = weightedMaterial(mm, weight);
  const V3  worldPos = {h1.x, h1.y, h1.z}, normal = {h2.x, h2.y, h2.z};
  uint32_t  noSeed   = 0u;  // (hard shadows only: the loop never reads the random state)
  if(!shadeLights<KB, true, false>(lightLoopArgs(B.g.l, F), B.g.l.t, S, &M, &SM, tid, mat, worldPos, normal, rayDir, noSeed, color, sums))
    return false;  // every light out of range: nothing is called, done stays 1 (:1186-1187)
  const BounceMatDev bm = bounceMaterial(B, inst, matId);
  if(bm.illum <= 0)
  {
    T = {0.0, 0.0, 0.0};
    return false;
  }
  newO = worldPos;
  const float dn = dot3(rayDir, normal);
  if(bm.illum == 1)
  {  // reflection (wavefront.h.slang:340-346)
    T.x *= (double)mm.specular.x;
    T.y *= (double)mm.specular.y;
    T.z *= (double)mm.specular.z;
    newD = rayDir - normal * (2.0f * dn);
    return true;
  }
  T.x *= (double)bm.transmittance[0];
  T.y *= (double)bm.transmittance[1];
  T.z *= (double)bm.transmittance[2];
  float eta = 1.0f / bm.ior;
  V3    N   = normal;
  if(dn > 0.0f)
  {  // inside the object: flip normal and eta (:357-362)
    N   = -normal;
    eta = bm.ior;
  }
  const float ni = dot3(N, rayDir);
  const float k  = 1.0f - eta * eta * (1.0f - ni * ni);  // refract
  V3          r  = {0.0f, 0.0f, 0.0f};
  if(!(k < 0.0f))
    r = rayDir * eta - N * (eta * ni + sqrtf(k));
  const float rl = sqrtf(dot3(r, r));
  if(rl > 0.0f)
    newD = r * (1.0f / rl);
  else
    newD = rayDir - N * (2.0f * ni);  // total internal reflection (:370-374)
  return true;
}

__device__ __forceinline__ void storeBounceState(const TraceBounceArgs& B, size_t pix, V3 o, V3 d, V3 rad, D3 T)
{
  float*       r = B.ray + pix;
  const size_t n = B.pixels;
  r[0] = o.x; r[n] = o.y; r[2 * n] = o.z;
  r[3 * n] = d.x; r[4 * n] = d.y; r[5 * n] = d.z;
  r[6 * n] = rad.x; r[7 * n] = rad.y; r[8 * n] = rad.z;
  double* t = B.T + pix;
  t[0] = T.x; t[n] = T.y; t[2 * n] = T.z;
}

}  // namespace

// Bounce 0's hand-over, behind k_trace_mesh_composite<KB, true> (k_trace_mesh.hip): the mesh shading in the indirect mode for the
// pixels whose material bounces.  Every pixel of the strip gets its live word; a live one its ray, radiance and T.  A frame whose
// materials are all illum 0 therefore keeps the lit mesh frame's pixels bit for bit.
template <int KB>
__global__ __launch_bounds__(256) void k_trace_bounce_primary(TraceBounceArgs B)
{
  const TraceLightMeshArgs& args = B.g;
  const TraceLightArgs&     L    = args.l;
  __shared__ TraceLds S;
  __shared__ TraceLds SM;
  const TraceArgs&  a  = L.t;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x;
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
  {
    B.live[pix] = 0u;
    return;  // no mesh behind this pixel: what the light pass stored stays
  }
  const float4   h1 = args.m.hits[4 * pix + 1], h2 = args.m.hits[4 * pix + 2];
  const float4   base   = L.radiance[pix];
  float          walkT  = args.m.walkT[pix];
  const uint32_t pickId = a.outId != nullptr ? a.outId[pix] : L.pickId[pix];
  TraceRay   ray;
  (void)primaryRayAsTraced(F, px, py, ray.o, ray.d);  // the ray that found the hit (a mesh hit: the ray is valid)
  const V3 rayDir = {ray.d[0], ray.d[1], ray.d[2]};

  V3 color = {base.x, base.y, base.z};  // (the side outputs, the depth of a mesh pixel included, are the lit composite's)
  {  // surfaceFinalFiltering and splatIsClosest as the light pass decided them: a discarded splat surface is radiance 0, T = 1
    const float isoDist = L.isoDist[pix];
    if(pickId == kTraceInvalid || !(isoDist > 0.0f) || !(isoDist < tMesh))
    {
      color = {0.0f, 0.0f, 0.0f};
      walkT = (double)1.0f > (double)args.m.minT ? 1.0f : -1.0f;
    }
  }
  if(walkT < 0.0f)
  {
    B.live[pix] = 0u;
    return;  // T > min_mesh_composite_transmittance failed (:1058-1059): the mesh is not shaded, done stays 1
  }
  // The lit composite has shaded this pixel already, and a pixel that does not bounce keeps its bits: only a mirror or glass
  // pixel is shaded again here, in fp32 for the carried radiance (its shadow rays are the composite's, traced a second time: they
  // are not counted again).
  if(bounceMaterial(B, __float_as_uint(h0.y), __float_as_uint(h0.w)).illum <= 0)
  {
    B.live[pix] = 0u;
    return;
  }
  D3         T = {(double)walkT, (double)walkT, (double)walkT};  // (the walk's T as k_trace left it: rounded once to fp32)
  ShadowSums sums;
  V3         newO = {0.0f, 0.0f, 0.0f}, newD = {0.0f, 0.0f, 1.0f};
  const bool live = shadeMeshIndirect<KB>(B, S, SM, tid, F, h0, h1, h2, rayDir, V3{walkT, walkT, walkT}, T, color, newO, newD, sums);
  B.live[pix] = live ? 1u : 0u;
  if(live)
  {
    storePixel(a.image, a.fmt, pix, color.x, color.y, color.z, 1.0f);  // the mesh is opaque
    storeBounceState(B, pix, newO, newD, color, T);
  }
}

// One bounce b >= 1 of every live pixel.  SHF: SH storage format; KB: K-buffer slots in registers (>= samples_per_pass).
template <int SHF, int KB>
__global__ __launch_bounds__(256) void k_trace_bounce(TraceBounceArgs B)
{
  const TraceLightMeshArgs& args = B.g;
  const TraceLightArgs&     L    = args.l;
  __shared__ TraceLds S;
  __shared__ TraceLds SM;
  const TraceArgs&  a  = L.t;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  traceLdsInit(SM, args.m.h, tid);
  int px, py;
  tilePixel(F, tid, px, py);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;
  if(B.live[pix] == 0u)
    return;
  B.live[pix] = 0u;  // done = 1 (:335) until the mesh's shading says otherwise

  const size_t n = B.pixels;
  TraceRay     ray;
  {
    const float* r = B.ray + pix;
    ray.o[0] = r[0]; ray.o[1] = r[n]; ray.o[2] = r[2 * n];
    ray.d[0] = r[3 * n]; ray.d[1] = r[4 * n]; ray.d[2] = r[5 * n];
  }
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];
  float cr = B.ray[pix + 6 * n], cg = B.ray[pix + 7 * n], cb = B.ray[pix + 8 * n];
  D3    T  = {B.T[pix], B.T[pix + n], B.T[pix + 2 * n]};
  const V3 rayDir = {ray.d[0], ray.d[1], ray.d[2]};

  // ---- the closest mesh hit of the bounce ray (:505-552); the window of :521-522, epsT vanishes in fp32 ----
  unsigned long long meshNodeVisits = 0, meshTriTests = 0;
  const MeshBest best = meshWalk<0>(args.m.h, SM, tid, args.m.tris, args.m.table, ray, 0.001f, 10000.0f, meshNodeVisits, meshTriTests);
  const bool     hit  = best.t < __builtin_huge_valf();
  float4         h0 = meshMissRecord(), h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2 = h1;
  if(hit)
    meshHitRecord(args.m.table, best, h0, h1, h2);

  // ---- the pass walk with the carried radiance, T and hit count (:568-573, :615-763) ----
  const int       K       = a.samplesPerPass;
  const bool      noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  constexpr float epsT    = 1e-9f;
  const float     br = cr, bg = cg, bb = cb;  // radianceBeforeParticles (:289)
  float           nx = 0.f, ny = 0.f, nz = 0.f, isoDist = 0.0f;
  uint32_t        hitCount = 0, pickId = kTraceInvalid, passesUsed = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  float       tMin = 0.001f;
  const float tMax = fminf(best.t, 10000.0f);
  if(a.nLevels > 0)
    for(int pass = 0; pass < a.maxPasses; ++pass)  // bound: max_passes
    {
      if(!(tMin <= tMax) || !(maxComponent(T) > (double)a.minTransmittance))
        break;
      ++passesUsed;
      NearestK<KB> N = collectNearest<KB>(a, S, tid, ray, tMin + epsT, tMax + epsT, K);
      nodeVisits += N.nodeVisits;
      candTests += N.candTests;
      if(N.kid[0] == kTraceInvalid)
        break;  // no more hits (:661-667)
      for(int slot = 0; slot < K; ++slot)  // bound: samples_per_pass
      {
        uint32_t g;
        float    dist;
        popNearest<KB>(N, dist, g);
        if(g == kTraceInvalid)
          break;
        if(!(maxComponent(T) > (double)a.minTransmittance))
          continue;
        ParticleEval E;
        evalParticle(a, g, ray, E);
        float      alpha  = fminf(F.alphaClamp, E.resp * E.density);
        const bool accept = E.density > F.alphaCull && alpha > F.alphaCull && E.resp > F.kernelMinResponse;
        if(accept)
        {
          if(noGauss)
            alpha = 1.0f;
          const InstanceConst& I   = Ap->inst[E.k];
          const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[E.li];
          float vx = E.p[0] - E.om[0], vy = E.p[1] - E.om[1], vz = E.p[2] - E.om[2];
          const float vl = rsqrtf(vx * vx + vy * vy + vz * vz);
          vx *= vl; vy *= vl; vz *= vl;
          float r = shOnly ? 0.5f : col.x, gg = shOnly ? 0.5f : col.y, b = shOnly ? 0.5f : col.z;
          const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
          if(deg > 0)
            addShRadiance<SHF>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
          // particleIntegrate, threedgrt.h.slang:226-235: weight = alpha * float3(T)
          const float wx = alpha * (float)T.x, wy = alpha * (float)T.y, wz = alpha * (float)T.z;
          cr += r * wx;
          cg += gg * wy;
          cb += b * wz;
          const double keep = 1.0 - (double)alpha;
          T.x *= keep;
          T.y *= keep;
          T.z *= keep;
          ++hitCount;
          float nw[3];
          hitNormalWorld(a, F, E, nw);
          nx += nw[0] * wx;  // integratedNormal + normalWorld * weight, a float3 product (:725)
          ny += nw[1] * wy;
          nz += nw[2] * wz;
          if(isoDist == 0.0f && T.x < (double)a.depthIsoThreshold)
          {  // the x channel, as written (:729)
            isoDist = dist;
            pickId  = g;
          }
        }
        tMin = fmaxf(tMin, dist);
      }
    }

  // ---- evaluateLightingAndShadingForBounce (:1037-1062) ----
  ShadowSums sums;
  if(pickId != kTraceInvalid && isoDist > 0.0f && isoDist < best.t)
  {  // the splat surface, on radiance - radianceBeforeParticles (:1053-1055); no surfaceFinalFiltering: the raw integrated normal
    const Mat mat = splatMaterial(L.table->mats[splatInstance(Ap, pickId)], V3{cr - br, cg - bg, cb - bb});
    V3 color = mat.emission;
    if(mat.needShading != 0)
    {
      const V3 worldPos = {ray.o[0] + isoDist * ray.d[0], ray.o[1] + isoDist * ray.d[1], ray.o[2] + isoDist * ray.d[2]};
      uint32_t noSeed = 0u;
      (void)shadeLights<KB, true, false>(lightLoopArgs(L, F), a, S, &args.m, &SM, tid, mat, worldPos, V3{nx, ny, nz}, rayDir, noSeed, color, sums);
    }
    cr = color.x + br;
    cg = color.y + bg;
    cb = color.z + bb;
  }
  bool live = false;
  V3   color = {cr, cg, cb};
  V3   newO = {0.0f, 0.0f, 0.0f}, newD = {0.0f, 0.0f, 1.0f};
  if(hit && maxComponent(T) > (double)args.m.minT)
    live = shadeMeshIndirect<KB>(B, S, SM, tid, F, h0, h1, h2, rayDir, V3{(float)T.x, (float)T.y, (float)T.z}, T, color, newO, newD, sums);

  a.hitCount[pix] += hitCount;  // (this lane's own words: bounce 0 wrote them)
  L.shadowHits[pix] += sums.shadowHits;
  storePixel(a.image, a.fmt, pix, color.x, color.y, color.z, 1.0f);  // a live pixel is a mesh pixel of bounce 0: alpha 1
  if(live)
  {
    B.live[pix] = 1u;
    storeBounceState(B, pix, newO, newD, color, T);
  }
  else
  {  // the radiance alone: nothing else of the state is read again
    B.ray[pix + 6 * n] = color.x;
    B.ray[pix + 7 * n] = color.y;
    B.ray[pix + 8 * n] = color.z;
  }
  // statistics: integer sums, so the totals do not depend on the order of arrival
  const int slot = B.bounce - 1;
  atomicAdd(&B.bctr->rays[slot], 1ull);
  if(hit)
    atomicAdd(&B.bctr->meshHits[slot], 1ull);
  atomicAdd(&B.bctr->particleHits, (unsigned long long)hitCount);
  atomicAdd(&a.ctr->nodeVisits, nodeVisits);
  atomicAdd(&a.ctr->candidateTests, candTests);
  atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hitCount);
  atomicMax(&a.ctr->maxPassesUsed, passesUsed);
  atomicAdd(&L.lctr->shadowRays, sums.shadowRays);
  atomicAdd(&L.lctr->nodeVisits, sums.nodeVisits);
  atomicAdd(&L.lctr->candidateTests, sums.candTests);
  atomicAdd(&L.lctr->acceptedHits, (unsigned long long)sums.shadowHits);
  atomicAdd(&args.m.ctr[1].nodeVisits, sums.meshNodeVisits);
  atomicAdd(&args.m.ctr[1].triangleTests, sums.meshTriTests);
  atomicAdd(&args.m.ctr[1].hits, sums.meshOccluded);
}

void launchTraceBouncePrimary(hipStream_t stream, const TraceBounceArgs& B, const FrameConst& F)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  withKBuffer("launchTraceBouncePrimary", B.g.l.t.samplesPerPass,
              [&](auto kb) { hipLaunchKernelGGL((k_trace_bounce_primary<decltype(kb)::value>), dim3(tiles), dim3(256), 0, stream, B); });
}

void launchTraceBounce(hipStream_t stream, const TraceBounceArgs& B, const FrameConst& F, int shFormat)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  withShFormatAndKBuffer("launchTraceBounce", shFormat, B.g.l.t.samplesPerPass, [&](auto shf, auto kb) {
    hipLaunchKernelGGL((k_trace_bounce<decltype(shf)::value, decltype(kb)::value>), dim3(tiles), dim3(256), 0, stream, B);
  });
}

}  // namespace mgs
