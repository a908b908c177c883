// k_trace_rays.hip — ray queries (mgs_trace_rays, mgs_trace_rays_device, mgs_trace_generate_rays) for gfx950: the caller's rays through
// the splat hierarchy, with the walk of the traced frames' strategy 0.
//
// Replaces, for rays that do not come from the library's cameras,
//   shaders/threedgrt_raytrace.rgen.slang:615-819    traceRayParticlesInsertionSort: passes of PARTICLES_SPP nearest hits
//   shaders/threedgrt.h.slang:166-235                particleProcessHit, particleIntegrate
// and, in k_rays_generate, writes out the rays of rgen.slang:165-196 instead of tracing them (primaryRayAsTraced, trace_primary_ray.h: primaryRay
// of trace_traverse.h with the roundings it has inside k_trace).
// Structure: one ray per lane, 256 lanes per workgroup; lane i of workgroup b takes ray perm[b * 256 + i], or b * 256 + i in the
// caller's order.  The K-buffer, the collection and the particle evaluation are trace_traverse.h, as for k_trace.hip.  Every loop is
// bounded as there: passes by max_passes, the walk by samples_per_pass, the traversal by 2 * nodes + 2 steps, children by 8.  Nothing
// waits on another lane, wave or workgroup, and no lane returns: a tail workgroup's spare lanes and the invalid rays skip the work.
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "sh_eval.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_primary_ray.h"
#include "trace_shade.h"
#include "trace_traverse.h"

namespace mgs {

// every pixel's primary ray, row-major, as k_trace would trace it: (origin, 0.001), (direction, 10000); a fisheye pixel outside the
// image circle gets the window (1, 0), which a ray query refuses
__global__ __launch_bounds__(256) void k_rays_generate(const FrameArgs* __restrict__ Ap, float4* __restrict__ rays)
{
  const FrameConst& F = Ap->f;
  const uint32_t    i = blockIdx.x * 256u + threadIdx.x;
  if(i >= (uint32_t)F.width * (uint32_t)F.height)
    return;
  float      o[3], d[3];
  const int  px = (int)(i % (uint32_t)F.width), py = (int)(i / (uint32_t)F.width);
  bool       ok;
  if(F.sensor.bound != 0)
  {  // the handle's sensor model: the ray the 3DGUT compositors give this pixel (gut_common.h), lens sample included
    ok   = gutPixelRay(F, (float)px + 0.5f, (float)py + 0.5f, d[0], d[1], d[2]);
    o[0] = F.viewInv[12]; o[1] = F.viewInv[13]; o[2] = F.viewInv[14];
    if(F.dofMode != 0)
    {
      float lx, ly, lz;
      gutLensSample<false>(F, rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId), lx, ly, lz, d[0], d[1], d[2]);
      o[0] += lx; o[1] += ly; o[2] += lz;
    }
  }
  else
    ok = primaryRayAsTraced(F, px, py, o, d);
  rays[2 * (size_t)i]     = make_float4(o[0], o[1], o[2], ok ? 0.001f : 1.0f);
  rays[2 * (size_t)i + 1] = make_float4(d[0], d[1], d[2], ok ? 10000.0f : 0.0f);
}

__device__ __forceinline__ uint32_t raySpread7(uint32_t v)
{  // 7 bits to every third bit
  v = (v | (v << 8)) & 0x0000700Fu;
  v = (v | (v << 4)) & 0x000430C3u;
  v = (v | (v << 2)) & 0x00049249u;
  return v;
}

// 21 bits of Morton code of a position's cell in the scene box, 128 cells per axis (positions outside are clamped)
__device__ __forceinline__ uint32_t mortonCell21(const float4& o, const float (&lo)[3], const float (&invExt)[3])
{
  const float oc[3] = {o.x, o.y, o.z};
  uint32_t    q[3];
#pragma unroll
  for(int c = 0; c < 3; ++c)
    q[c] = (uint32_t)fminf(fmaxf((oc[c] - lo[c]) * invExt[c], 0.0f) * 128.0f, 127.0f);
  return raySpread7(q[0]) | (raySpread7(q[1]) << 1) | (raySpread7(q[2]) << 2);
}

// coherence key of a ray: 21 bits of Morton code of the origin's cell in the scene box (origins outside are clamped), the direction's
// octant, and 4 + 4 bits of |d.x| and |d.y| over the direction's 1-norm.  Nothing but the ray and the scene box enters; an invalid
// ray gets the largest key.
__global__ __launch_bounds__(256) void k_rays_key(RayKeyArgs a)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= a.count)
    return;
  const float4 o = a.rays[2 * (size_t)i], d = a.rays[2 * (size_t)i + 1];
  uint32_t     key = 0xFFFFFFFFu;
  if(rayValid(o, d))
  {
    const float    ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const float    m  = fmaxf(fmaxf(ax, ay), az);  // (scaled by the largest component first: the 1-norm of a huge direction would overflow)
    const float    sx = ax / m, sy = ay / m, sz = az / m, n1 = sx + sy + sz;
    const uint32_t qx = (uint32_t)fminf(sx / n1 * 16.0f, 15.0f), qy = (uint32_t)fminf(sy / n1 * 16.0f, 15.0f);
    const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
    const uint32_t mort = mortonCell21(o, a.sceneLo, a.sceneInvExt);
    key = min((mort << 11) | (oct << 8) | (qx << 4) | qy, 0xFFFFFFFEu);
  }
  a.keys[i] = key;
  a.idx[i]  = i;
}

// the key kernel's second entry, for a batch of surface points (mgs_shade_points): the position's Morton cell alone, in the bits the
// rays' keys keep it in; a point with a non-finite position gets the largest key (the shading kernel decides what is invalid)
__global__ __launch_bounds__(256) void k_points_key(PointKeyArgs a)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= a.count)
    return;
  const float4 o   = a.points[4 * (size_t)i];
  const float  big = 3.4028234664e38f;
  uint32_t     key = 0xFFFFFFFFu;
  if(fabsf(o.x) <= big && fabsf(o.y) <= big && fabsf(o.z) <= big)
    key = mortonCell21(o, a.sceneLo, a.sceneInvExt) << 11;
  a.keys[i] = key;
  a.idx[i]  = i;
}

// SHF: SH storage format; KB: K-buffer slots in registers (>= samples_per_pass)
template <int SHF, int KB>
__global__ __launch_bounds__(256) void k_trace_rays(TraceRaysArgs q)
{
  __shared__ TraceLds S;
  const TraceArgs&  a  = q.t;
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int         tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  const uint32_t slot = blockIdx.x * 256u + (uint32_t)tid;
  const bool     live = slot < q.count;
  const uint32_t idx  = live ? (q.perm ? q.perm[slot] : slot) : 0u;
  float4         ro = make_float4(0.f, 0.f, 0.f, 1.f), rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if(live && idx < q.count)  // (a permutation is the library's own; the bound keeps a stray index from leaving the arrays)
  {
    ro = q.rays[2 * (size_t)idx];
    rd = q.rays[2 * (size_t)idx + 1];
  }
  const bool rayOk = live && idx < q.count && rayValid(ro, rd);
  TraceRay   ray;
  ray.o[0] = ro.x; ray.o[1] = ro.y; ray.o[2] = ro.z;
  ray.d[0] = rd.x; ray.d[1] = rd.y; ray.d[2] = rd.z;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];

  const int       K       = a.samplesPerPass;
  const bool      surf    = q.surf != 0;
  const bool      noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  constexpr float epsT    = 1e-9f;  // rgen.slang:157

  double   T = 1.0;
  float    cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, wsum = 0.f, isoDist = 0.0f;
  uint32_t hitCount = 0, pickId = kTraceInvalid, passesUsed = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  float       tMin = fmaxf(ro.w, 0.0f);  // the slab test starts at the origin: a ray has no hits behind it
  const float tMax = rd.w;

  // (the pick stays inside `if(surf)` as in k_trace.hip: taken out of it, the compiler contracts this walk's arithmetic differently
  // and the results stop being the traced frame's bit for bit; a caller who wants t_iso and id sets surface_outputs)
  // the pass loop of k_trace.hip with the ray's own window, written out again: k_trace's instantiations are held to their registers
  // (k_trace.hip's walk has the same note for shadeHit), so the walk is not moved into a shared header.  Tried as a whole too: one
  // force-inlined template over <SHF, KB> with this statement order and the accumulators in a struct taken by reference gave all
  // eighteen instantiations of the two kernels other code (0 to 8 VGPRs fewer, 30 to 60 instructions shorter: other roundings are
  // possible, and test_gpu_rays.py's bit-for-bit comparison is what holds the two walks together).  A fix to one is a fix to both.
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
        break;  // no more hits (rgen.slang:661-667)
      for(int s = 0; s < K; ++s)  // bound: samples_per_pass
      {
        uint32_t g;
        float    dist;
        popNearest<KB>(N, dist, g);
        if(g == kTraceInvalid)
          break;
        if(!(T > (double)a.minTransmittance))
          continue;
        ParticleEval E;
        evalParticle(a, g, ray, E);
        // particleProcessHit, threedgrt.h.slang:166-185
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

  if(live && idx < q.count)
  {
    const uint32_t id = pickId != kTraceInvalid ? a.callerId[pickId] : kTraceInvalid;
    float4*        R  = q.results + 3 * (size_t)idx;
    R[0] = make_float4(cr, cg, cb, (float)T);
    R[1] = make_float4(isoDist, __uint_as_float(id), __uint_as_float(hitCount), __uint_as_float(passesUsed));
    R[2] = make_float4(nx, ny, nz, wsum);
    // statistics: integer sums, so the totals do not depend on the order of arrival
    if(rayOk)
    {
      atomicAdd(&a.ctr->nodeVisits, nodeVisits);
      atomicAdd(&a.ctr->candidateTests, candTests);
      atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hitCount);
      atomicMax(&a.ctr->maxPassesUsed, passesUsed);
    }
    else
      atomicAdd(q.invalid, 1u);
  }
}

void launchRaysGenerate(hipStream_t stream, const FrameArgs* dArgs, float4* rays, uint32_t pixels)
{
  if(pixels)
    hipLaunchKernelGGL(k_rays_generate, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, dArgs, rays);
}

void launchRaysKey(hipStream_t stream, const RayKeyArgs& a)
{
  if(a.count)
    hipLaunchKernelGGL(k_rays_key, dim3((a.count + 255u) / 256u), dim3(256), 0, stream, a);
}

void launchPointsKey(hipStream_t stream, const PointKeyArgs& a)
{
  if(a.count)
    hipLaunchKernelGGL(k_points_key, dim3((a.count + 255u) / 256u), dim3(256), 0, stream, a);
}

void launchTraceRays(hipStream_t stream, const TraceRaysArgs& a, int shFormat)
{
  if(a.count == 0)
    return;
  const uint32_t groups = (a.count + 255u) / 256u;
  withShFormatAndKBuffer("launchTraceRays", shFormat, a.t.samplesPerPass, [&](auto shf, auto kb) {
    hipLaunchKernelGGL((k_trace_rays<decltype(shf)::value, decltype(kb)::value>), dim3(groups), dim3(256), 0, stream, a);
  });
}

}  // namespace mgs
