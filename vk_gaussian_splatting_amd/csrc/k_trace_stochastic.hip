// k_trace_stochastic.hip — the two stochastic trace strategies of the traced pipeline (mgs_render_traced with
// MgsTraceParams::trace_strategy 1 or 2) for gfx950.  The sorted strategy (0) is k_trace.hip and is not touched by this file.
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:615-819    traceRayParticlesInsertionSort<kStochasticPass>: the passes of k_trace.hip with
//                                                    Russian roulette on every pass's opacity (:669-673, :684-687, :765-801)
//   shaders/threedgrt_raytrace.rgen.slang:823-961    traceRayParticlesStochasticSort with PARTICLES_SPP == 1 (gaussian_splatting.cpp:1693)
//   shaders/threedgrt_raytrace.rahit.slang:94-150    the any-hit that keeps a hit with probability alpha
//   shaders/threedgrt_raytrace.rgen.slang:228        seedRayPass = xxhash32(pixel, frameSampleId), apart from the lens's seed (:193)
// Structure as k_trace.hip: one ray per lane, a wave64 = an 8 x 8 pixel tile, a workgroup = a 16 x 16 tile; the ray, the particle
// evaluation, the K-buffer and the walk through the hierarchy are trace_traverse.h, the per-hit shading is trace_shade.h.  Every loop
// is bounded: passes by max_passes, the walk by samples_per_pass, a traversal by 2 * nodes + 2 steps, children by 8.  Nothing waits
// on another lane, wave or workgroup.  All register arrays are indexed by unrolled loops only.
#include <cstdio>
#include <cstdlib>

#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "sh_eval.h"
#include "target_pixel.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_shade.h"
#include "trace_traverse.h"

namespace mgs {

// the pixel and the frame's statistics, as k_trace.hip writes them (writeToGBuffers, rgen.slang:1466-1502)
__device__ __forceinline__ void writeStochasticPixel(const TraceArgs& a, const FrameConst& F, const TraceRay& ray, size_t pix, float cr, float cg, float cb,
                                                     float alphaOut, uint32_t hitCount, uint32_t pickId, float pickDist, float nx, float ny, float nz,
                                                     float nw, unsigned long long nodeVisits, unsigned long long candTests, uint32_t passesUsed)
{
  a.hitCount[pix] = hitCount;
  if(a.outDepth != nullptr)
  {
    a.outDepth[pix]  = pickId != kTraceInvalid ? pickedNdcZ(F, ray, pickDist) : 0.0f;  // "none" is 0 in this library
    a.outId[pix]     = pickId;
    a.outNormal[pix] = make_float4(nx, ny, nz, nw);
  }
  storePixel(a.image, a.fmt, pix, cr, cg, cb, alphaOut);
  atomicAdd(&a.ctr->nodeVisits, nodeVisits);
  atomicAdd(&a.ctr->candidateTests, candTests);
  atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hitCount);
  atomicMax(&a.ctr->maxPassesUsed, passesUsed);
}

// ---- strategy 1: pass-stochastic.  SHF: SH storage format; KB: K-buffer slots in registers (>= samples_per_pass) ----
// The pixel state before a pass (oldPixel, :671) is always the untouched pixel here: there are no meshes and no hand-over from a
// raster pass, a rejected pass restores the snapshot and an accepted one ends the ray.  So a rejection RESETS the state instead of
// copying it back; tMin is no part of the pixel and keeps advancing.
template <int SHF, int KB>
__global__ __launch_bounds__(256) void k_trace_pass_stochastic(TraceArgs a)
{
  __shared__ TraceLds S;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  int px, py;
  tilePixel(F, tid, px, py);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;

  TraceRay   ray;
  const bool rayOk = primaryRay(F, px, py, ray);

  const int       K       = a.samplesPerPass;
  const bool      surf    = a.outDepth != nullptr;
  const bool      noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  constexpr float epsT    = 1e-9f;  // rgen.slang:157

  double   T = 1.0;
  float    cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, wsum = 0.f, isoDist = 0.0f;
  uint32_t hitCount = 0, pickId = kTraceInvalid, passesUsed = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  float       tMin = 0.001f;
  const float tMax = 10000.0f;
  uint32_t    seedRayPass = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);  // :228

  if(rayOk && a.nLevels > 0)
    for(int pass = 0; pass < a.maxPasses; ++pass)  // bound: max_passes
    {
      if(!(tMin <= tMax) || !(T > (double)a.minTransmittance))
        break;
      ++passesUsed;
      NearestK<KB> N = collectNearest<KB>(a, S, tid, ray, tMin + epsT, tMax + epsT, K);
      nodeVisits += N.nodeVisits;
      candTests += N.candTests;
      if(N.kid[0] == kTraceInvalid)
        break;  // no more hits (:661-667): no draw
      uint32_t lastId   = N.kid[0];  // payload slot lastValidHitIdx, which starts at slot 0 (:672)
      float    lastDist = N.kd[0];
      for(int slot = 0; slot < K; ++slot)  // bound: samples_per_pass
      {
        uint32_t g;
        float    dist;
        popNearest<KB>(N, dist, g);
        if(g == kTraceInvalid)
          break;
        if(!(T > (double)a.minTransmittance))
          continue;
        lastId   = g;  // valid and walked, accepted or not (:684-687)
        lastDist = dist;
        ParticleEval E;
        evalParticle(a, g, ray, E);
        float alpha, r, gg, b;
        if(shadeHit<SHF>(Ap, E, noGauss, shOnly, alpha, r, gg, b))
        {
          const float weight = alpha * (float)T;  // particleIntegrate, threedgrt.h.slang:226-235
          cr += r * weight;
          cg += gg * weight;
          cb += b * weight;
          T *= (1.0 - (double)alpha);
          ++hitCount;
          if(surf)
          {
            float nw[3];
            hitNormalWorld(a, F, E, nw);
            nx += nw[0] * weight;
            ny += nw[1] * weight;
            nz += nw[2] * weight;
            wsum += weight;
            if(isoDist == 0.0f && T < (double)a.depthIsoThreshold)
            {
              isoDist = dist;
              pickId  = g;
            }
          }
        }
        tMin = fmaxf(tMin, dist);  // :761
      }
      // ---- Russian roulette on the pass's opacity (:765-801) ----
      const float opacity = (float)(1.0 - T);
      if(rngRand(seedRayPass) < opacity)
      {
        cr = cr / opacity;
        cg = cg / opacity;
        cb = cb / opacity;
        if(surf && isoDist == 0.0f)
        {  // no iso-surface found: the farthest walked slot
          isoDist = lastDist;
          pickId  = lastId;
        }
        T = 0.0;
        break;
      }
      // rejected: the pixel returns to the snapshot, which is the untouched pixel (see above)
      T  = 1.0;
      cr = cg = cb = nx = ny = nz = wsum = isoDist = 0.0f;
      hitCount = 0;
      pickId   = kTraceInvalid;
    }

  float alphaOut = 1.0f - (float)T;
  if(!rayOk)
    alphaOut = 1.0f;  // rgen.slang:185
  writeStochasticPixel(a, F, ray, pix, cr, cg, cb, alphaOut, hitCount, pickId, isoDist, nx, ny, nz, wsum, nodeVisits, candTests, passesUsed);
}

// ---- strategy 2: stochastic any-hit.  One traversal, one payload slot ----
// Every candidate at or before the slot is evaluated; an accepted one is kept with probability alpha, by a draw that depends on the
// pixel, the sample, the particle (caller's id) and the bits of its t alone, so the kept set does not depend on the order of
// traversal and the slot ends as the nearest kept hit; equal t: the lower caller's id.
template <int SHF>
__global__ __launch_bounds__(256) void k_trace_anyhit_stochastic(TraceArgs a)
{
  __shared__ TraceLds S;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  int px, py;
  tilePixel(F, tid, px, py);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;

  TraceRay   ray;
  const bool rayOk = primaryRay(F, px, py, ray);

  const bool      surf    = a.outDepth != nullptr;
  const bool      noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  constexpr float epsT    = 1e-9f;
  const float     t0 = 0.001f + epsT, t1 = 10000.0f + epsT;
  const uint32_t  rngSeed = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);  // :848

  float    slotT = __builtin_huge_valf();  // the payload: distance, id, colour, normal
  uint32_t slotId = kTraceInvalid, slotCaller = kTraceInvalid;
  float    sr = 0.f, sg = 0.f, sb = 0.f, snx = 0.f, sny = 0.f, snz = 0.f;
  unsigned long long nodeVisits = 0, candTests = 0;

  auto candidate = [&](uint32_t g) {
    ++candTests;
    ParticleEval E;
    evalParticle(a, g, ray, E);
    if(!(E.t > t0 && E.t < t1) || !(E.resp > proxyThreshold(a.proxy, E.density)))
      return;
    const uint32_t caller = a.callerId[g];
    if(!(E.t < slotT || (E.t == slotT && caller < slotCaller)))  // rahit.slang:101; equal t: the lower caller's id
      return;
    float alpha, r, gg, b;
    if(!shadeHit<SHF>(Ap, E, noGauss, shOnly, alpha, r, gg, b))
      return;
    uint32_t seed = rngXxhash32(rngSeed, caller ^ __float_as_uint(E.t), 0u);  // rahit.slang:131-133, slot 0
    if(!(rngRand(seed) < alpha))
      return;
    slotT      = E.t;
    slotId     = g;
    slotCaller = caller;
    sr = r; sg = gg; sb = b;
    if(surf)
    {
      float nw[3];
      hitNormalWorld(a, F, E, nw);
      snx = nw[0]; sny = nw[1]; snz = nw[2];
    }
  };
  const bool traced = rayOk && a.nLevels > 0;
  if(traced)
    traverseProxies(a, S, tid, ray, t0, t1, slotT, candidate, nodeVisits);

  // ---- the pixel (rgen.slang:951-960 with one sample: transmittance 1 times the sample, then transmittance 0) ----
  const bool kept = slotId != kTraceInvalid;
  float      nl   = sqrtf(snx * snx + sny * sny + snz * snz);
  nl              = nl > 0.0f ? 1.0f / nl : 0.0f;
  writeStochasticPixel(a, F, ray, pix, sr, sg, sb, (kept || !rayOk) ? 1.0f : 0.0f, kept ? 1u : 0u, slotId, slotT, snx * nl, sny * nl, snz * nl,
                       kept ? 1.0f : 0.0f, nodeVisits, candTests, traced ? 1u : 0u);
}

void launchTraceStochastic(hipStream_t stream, const TraceArgs& a, const FrameConst& F, int shFormat, int strategy)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  if(strategy == 2)
    withShFormat(shFormat, [&](auto shf) {
      hipLaunchKernelGGL((k_trace_anyhit_stochastic<decltype(shf)::value>), dim3(tiles), dim3(256), 0, stream, a);
    });
  else if(strategy == 1)
    withShFormatAndKBuffer("launchTraceStochastic", shFormat, a.samplesPerPass, [&](auto shf, auto kb) {
      hipLaunchKernelGGL((k_trace_pass_stochastic<decltype(shf)::value, decltype(kb)::value>), dim3(tiles), dim3(256), 0, stream, a);
    });
  else
  {
    std::fprintf(stderr, "launchTraceStochastic: no instantiation for strategy %d\n", strategy);
    std::abort();
  }
}

}  // namespace mgs
