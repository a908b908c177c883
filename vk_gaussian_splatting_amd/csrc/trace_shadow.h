// trace_shadow.h — the shadow ray through the particles, once: the loop over the lights of every traced shading site
// (trace_lights.h) and the shadow queries (k_shadow_rays, k_shadow_query.hip) call it.
//
// Replaces (hard shadows, no mesh in the traced scene)
//   shaders/threedgrt_raytrace.rgen.slang:1344-1464   traceShadowRayParticle: one collection, the walk, the ramp and the tint
//   shaders/threedgrt.h.slang:166-235                 particleProcessHit<false>, particleIntegrate
// One collection of the samples_per_pass nearest hits in (tMin, lightDist - 0.001) (trace_traverse.h: the code of the primary rays),
// no second pass and no epsT; the slots are walked in order, a slot with t >= lightDist is skipped; the transmittance is a double;
// after each slot a transmittance below the threshold becomes 0 and ends the walk.  SH is evaluated only when the colour strength
// is not 0, through a runtime switch on the storage format (the walk is short and latency-bound; three more instantiations per
// K-buffer size would triple the code for a branch that is wave-uniform).  Bounded: the traversal by 2 * nodes + 2 steps, the walk
// by samples_per_pass.  Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include "sh_eval.h"
#include "shade_direct.h"
#include "trace_traverse.h"

namespace mgs {

// the knobs of MgsTraceLightParams the shadow ray reads, and the SH storage format
struct ShadowKnobs
{
  int32_t shFormat;
  float   threshold, colorStrength;
};

// KB: K-buffer slots in registers (>= samples_per_pass).  sr: the ray as traced (origin already offset; the direction need not be
// of unit length: t runs along it); tMin >= 0; lightDist: the ray parameter of the light.  Returns the transmittance the light's
// colour is multiplied by; adds the accepted hits and the traversal's counts to the caller's sums.
template <int KB>
__device__ __forceinline__ V3 traceShadowRayParticle(const TraceArgs& a, TraceLds& S, int tid, const TraceRay& sr, float tMin, float lightDist,
                                                     const ShadowKnobs& k, uint32_t& shadowHits, unsigned long long& nodeVisits,
                                                     unsigned long long& candTests)
{
  const FrameArgs*  Ap      = a.frame;
  const FrameConst& F       = Ap->f;
  const int         K       = a.samplesPerPass;
  const bool        noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  const bool        tint    = k.colorStrength != 0.0f;
  NearestK<KB> N = collectNearest<KB>(a, S, tid, sr, tMin, lightDist - 0.001f, K);  // no second pass
  nodeVisits += N.nodeVisits;
  candTests += N.candTests;
  double T  = 1.0;
  float  sr_ = 0.0f, sg_ = 0.0f, sb_ = 0.0f;  // shadowRadiance
  for(int slot = 0; slot < K; ++slot)  // bound: samples_per_pass
  {
    uint32_t g;
    float    dist;
    popNearest<KB>(N, dist, g);
    if(g == kTraceInvalid)
      break;  // the slots are sorted: nothing valid behind an empty one
    if(dist >= lightDist)
      continue;
    ParticleEval E;
    evalParticle(a, g, sr, E);
    // particleProcessHit<false>, threedgrt.h.slang:166-201
    float      alpha  = fminf(F.alphaClamp, E.resp * E.density);
    const bool accept = E.density > F.alphaCull && alpha > F.alphaCull && E.resp > F.kernelMinResponse;
    if(accept)
    {
      if(noGauss)
        alpha = 1.0f;
      const float weight = alpha * (float)T;
      if(tint)
      {  // the hit's radiance feeds only the tint (:1456-1460)
        const InstanceConst& I   = Ap->inst[E.k];
        const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[E.li];
        float vx = E.p[0] - E.om[0], vy = E.p[1] - E.om[1], vz = E.p[2] - E.om[2];
        const float vl = rsqrtf(vx * vx + vy * vy + vz * vz);
        vx *= vl; vy *= vl; vz *= vl;
        float r = shOnly ? 0.5f : col.x, gg = shOnly ? 0.5f : col.y, b = shOnly ? 0.5f : col.z;
        const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
        if(deg > 0)
        {
          if(k.shFormat == 0)
            addShRadiance<0>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
          else if(k.shFormat == 1)
            addShRadiance<1>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
          else
            addShRadiance<2>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
        }
        sr_ += r * weight;
        sg_ += gg * weight;
        sb_ += b * weight;
      }
      T *= (1.0 - (double)alpha);
      ++shadowHits;
    }
    if(T < (double)k.threshold)
    {  // :1444-1448
      T = 0.0;
      break;
    }
  }
  // the ramp and the tint (:1453-1460)
  const float Tf      = fminf(fmaxf((float)T, 0.0f), 1.0f);
  const float thr     = k.threshold;
  const float scaledT = fminf(fmaxf((Tf - thr) / (1.0f - thr), 0.0f), 1.0f);
  const float maxRad  = fmaxf(fmaxf(sr_, sg_), sb_);
  V3          nc      = {1.0f, 1.0f, 1.0f};
  if(maxRad > 0.001f)
    nc = {sr_ / maxRad, sg_ / maxRad, sb_ / maxRad};
  const float u = k.colorStrength * (1.0f - scaledT);
  auto        sat = [](float v) { return fminf(fmaxf(v, 0.0f), 1.0f); };
  return {sat(scaledT * (1.0f + (nc.x - 1.0f) * u)), sat(scaledT * (1.0f + (nc.y - 1.0f) * u)), sat(scaledT * (1.0f + (nc.z - 1.0f) * u))};
}

}  // namespace mgs
