// k_trace.hip — the traversal of the traced pipeline (mgs_render_traced) for gfx950: primary rays of PIPELINE_RTX (3DGRT).
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:159-341    ray generation, depth of field, the pixel's outputs (writeToGBuffers :1466-1502)
//   shaders/threedgrt_raytrace.rgen.slang:615-819    traceRayParticlesInsertionSort: passes of PARTICLES_SPP nearest hits
//   shaders/threedgrt_raytrace.rahit.slang:71-75,152-173   the any-hit insertion into the sorted payload and its distance cut
//   shaders/threedgrt_raytrace.rint.slang:159-172    particleDensityHitInstance: t of the maximum response, in the particle's frame
//   shaders/threedgrt.h.slang:57-235                 canonical ray, response, particleProcessHit, particleIntegrate
// Structure: one ray per lane, a wave64 = an 8 x 8 pixel tile (a workgroup = the 16 x 16 tile of the raster pipelines), so the lanes of
// a wave walk nearly the same nodes.  The K-buffer (distance + id) lives in registers (KB = 4, 18 or 32 slots, the smallest that holds
// samples_per_pass); the ray, the particle evaluation and the collection of the K nearest hits are trace_traverse.h, shared with the
// shadow rays of k_trace_light.hip.  Every loop is bounded: passes by max_passes, the walk by samples_per_pass, the traversal by
// 2 * nodes + 2 steps, children by 8.  Nothing waits on another lane, wave or workgroup.
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

// SHF: SH storage format; KB: K-buffer slots in registers (>= samples_per_pass); MESH: a frame with mesh hits
// (mgs_frame_set_trace_meshes): the pixel's closest mesh hit, which k_trace_mesh_primary left, is the upper end of its walk
// (rgen.slang:539), and the walk's transmittance is left for the mesh composite.  The triangle walk itself is not in here.
template <int SHF, int KB, bool MESH>
__global__ __launch_bounds__(256) void k_trace(std::conditional_t<MESH, TraceWalkMeshArgs, TraceArgs> args)
{
  const TraceArgs& a = [&]() -> const TraceArgs& {
    if constexpr(MESH)
      return args.t;
    else
      return args;
  }();
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

  const int      K       = a.samplesPerPass;
  const bool     surf    = a.outDepth != nullptr;
  const bool     noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  constexpr float epsT   = 1e-9f;  // rgen.slang:157

  double   T = 1.0;  // pixel.transmittance: kept in double like the reference (one fp64 multiply per accepted hit)
  float    cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, wsum = 0.f, isoDist = 0.0f;
  uint32_t hitCount = 0, pickId = kTraceInvalid, passesUsed = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  float    tMin = 0.001f;
  float       tMaxPixel = 10000.0f;
  if constexpr(MESH)
    tMaxPixel = fminf(args.meshT[pix], 10000.0f);  // a hit lies inside (0.001, 10000); +inf = none
  const float tMax = MESH ? tMaxPixel : 10000.0f;

  if(rayOk && a.nLevels > 0)
    for(int pass = 0; pass < a.maxPasses; ++pass)  // bound: max_passes
    {
      if(!(tMin <= tMax) || !(T > (double)a.minTransmittance))
        break;
      ++passesUsed;
      // ---- collect the K nearest hits of (tMin + epsT, tMax + epsT) ----
      NearestK<KB> N = collectNearest<KB>(a, S, tid, ray, tMin + epsT, tMax + epsT, K);
      nodeVisits += N.nodeVisits;
      candTests += N.candTests;
      if(N.kid[0] == kTraceInvalid)
        break;  // no more hits (rgen.slang:661-667)

      // ---- walk them in order (rgen.slang:676-763) ----
      for(int slot = 0; slot < K; ++slot)  // bound: samples_per_pass
      {
        uint32_t g;
        float    dist;
        popNearest<KB>(N, dist, g);
        if(g == kTraceInvalid)
          break;  // the slots are sorted: nothing valid behind an empty one
        if(!(T > (double)a.minTransmittance))
          continue;
        ParticleEval E;
        evalParticle(a, g, ray, E);
        // particleProcessHit, threedgrt.h.slang:166-185 (written out here although trace_shade.h has it as shadeHit for the stochastic
        // strategies: calling that costs k_trace<0, 4> and k_trace<0, 18> a VGPR each and changes every instantiation's code)
        float      alpha  = fminf(F.alphaClamp, E.resp * E.density);
        const bool accept = E.density > F.alphaCull && alpha > F.alphaCull && E.resp > F.kernelMinResponse;
        if(accept)
        {
          if(noGauss)
            alpha = 1.0f;
          const InstanceConst& I   = Ap->inst[E.k];
          const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[E.li];
          float vx = E.p[0] - E.om[0], vy = E.p[1] - E.om[1], vz = E.p[2] - E.om[2];  // normalize(position - modelRayOrigin), :193
          const float vl = rsqrtf(vx * vx + vy * vy + vz * vz);
          vx *= vl; vy *= vl; vz *= vl;
          float r = shOnly ? 0.5f : col.x, gg = shOnly ? 0.5f : col.y, b = shOnly ? 0.5f : col.z;
          const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
          if(deg > 0)
            addShRadiance<SHF>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
          // particleIntegrate, :226-235
          const float weight = alpha * (float)T;
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
            {  // rgen.slang:729-741
              isoDist = dist;
              pickId  = g;
            }
          }
        }
        tMin = fmaxf(tMin, dist);  // "we move on in any case", :761
      }
    }

  // ---- the pixel (writeToGBuffers, rgen.slang:1466-1502; alpha = 1 - T here, 1.0 in the reference) ----
  float alphaOut = 1.0f - (float)T;
  if(!rayOk)
    alphaOut = 1.0f;  // rgen.slang:185
  a.hitCount[pix] = hitCount;
  if constexpr(MESH)  // rgen.slang:1058-1059, :1065-1066: the comparison in double; the weight is float(T)
    args.outWalkT[pix] = T > (double)args.meshMinT ? (float)T : -1.0f;
  if(surf)
  {
    float z = 0.0f;  // "none" is 0 in this library (the reference clears to 1.0)
    if(pickId != kTraceInvalid)
    {  // ndc z of primaryHitPos = origin + dist * direction (:735-740, :1490-1494)
      const float  hx = ray.o[0] + isoDist * ray.d[0], hy = ray.o[1] + isoDist * ray.d[1], hz = ray.o[2] + isoDist * ray.d[2];
      const float *V = F.view, *P = F.proj;
      const float  v0 = V[0] * hx + V[4] * hy + V[8] * hz + V[12], v1 = V[1] * hx + V[5] * hy + V[9] * hz + V[13],
                  v2 = V[2] * hx + V[6] * hy + V[10] * hz + V[14], v3 = V[3] * hx + V[7] * hy + V[11] * hz + V[15];
      const float cz = P[2] * v0 + P[6] * v1 + P[10] * v2 + P[14] * v3, cw = P[3] * v0 + P[7] * v1 + P[11] * v2 + P[15] * v3;
      z = cz / cw;
    }
    a.outDepth[pix]  = z;
    a.outId[pix]     = pickId;
    a.outNormal[pix] = make_float4(nx, ny, nz, wsum);
  }
  if(a.outIsoDist != nullptr)
  {  // what the light pass of a lit frame (k_trace_light.hip) reads besides the side outputs; null for every other frame
    a.outIsoDist[pix]  = isoDist;
    a.outRadiance[pix] = make_float4(cr, cg, cb, alphaOut);
  }
  storePixel(a.image, a.fmt, pix, cr, cg, cb, alphaOut);
  // statistics: integer sums, so the totals do not depend on the order of arrival
  atomicAdd(&a.ctr->nodeVisits, nodeVisits);
  atomicAdd(&a.ctr->candidateTests, candTests);
  atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hitCount);
  atomicMax(&a.ctr->maxPassesUsed, passesUsed);
}

void launchTrace(hipStream_t stream, const TraceArgs& a, const FrameConst& F, int shFormat)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  withShFormatAndKBuffer("launchTrace", shFormat, a.samplesPerPass, [&](auto shf, auto kb) {
    hipLaunchKernelGGL((k_trace<decltype(shf)::value, decltype(kb)::value, false>), dim3(tiles), dim3(256), 0, stream, a);
  });
}

void launchTraceWithMeshes(hipStream_t stream, const TraceWalkMeshArgs& a, const FrameConst& F, int shFormat)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  withShFormatAndKBuffer("launchTraceWithMeshes", shFormat, a.t.samplesPerPass, [&](auto shf, auto kb) {
    hipLaunchKernelGGL((k_trace<decltype(shf)::value, decltype(kb)::value, true>), dim3(tiles), dim3(256), 0, stream, a);
  });
}

}  // namespace mgs
