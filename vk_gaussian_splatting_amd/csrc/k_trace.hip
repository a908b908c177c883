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
// samples_per_pass); the traversal stack is ONE packed word per tree level in LDS (the children of the node open at that level
// that are still to visit, nearest first), so its depth is the tree's depth.  Every loop is bounded: passes by max_passes, the walk
// by samples_per_pass, the traversal by 2 * nodes + 2 steps (a node is entered once and left once), children by 8.  Nothing waits
// on another lane, wave or workgroup.
#include <cstdio>
#include <cstdlib>

#include "composite_common.h"
#include "gut_common.h"
#include "kernels_common.h"
#include "launchers.h"
#include "sh_eval.h"
#include "trace_common.h"

namespace mgs {

struct TraceRay
{
  float o[3], d[3], inv[3];
};

// slab test of a node against the ray: entry distance (clamped to 0) and whether [entry, exit] meets [t0, t1].  The exit is
// widened by 4 ulps (the products' rounding); NaNs of 0 * inf drop out of fminf / fmaxf, which is the conservative side.
__device__ __forceinline__ bool slabHit(const TraceRay& r, const float4& lo, const float4& hi, float t0, float t1, float& tEntry)
{
  const float ax = (lo.x - r.o[0]) * r.inv[0], bx = (hi.x - r.o[0]) * r.inv[0];
  const float ay = (lo.y - r.o[1]) * r.inv[1], by = (hi.y - r.o[1]) * r.inv[1];
  const float az = (lo.z - r.o[2]) * r.inv[2], bz = (hi.z - r.o[2]) * r.inv[2];
  const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
  const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * (1.0f + 4.0f * 1.1920929e-7f);
  tEntry         = tn * (1.0f - 4.0f * 1.1920929e-7f);
  return tEntry <= tf && tf >= t0 && tEntry <= t1;
}

// a particle against a ray: everything particleDensityHitInstance and particleProcessHit derive from the two
struct ParticleEval
{
  float    t, resp, density;
  int      k;        // instance
  uint32_t li;       // local (storage) index
  float    om[3], dmN[3];  // model-space ray: origin, normalised direction
  float    oc[3], dc[3];   // canonical ray: origin, UNNORMALISED direction (rint.slang:166-168)
  float    R[9], s[3], p[3];
};
__device__ __forceinline__ void evalParticle(const TraceArgs& a, uint32_t g, const TraceRay& ray, ParticleEval& E)
{
  const FrameArgs* Ap = a.frame;
  int              k  = 0;
  for(int i = 1; i < Ap->f.nInstances; ++i)  // bound: kMaxInstances
    if(g >= Ap->inst[i].globalOffset)
      k = i;
  const InstanceConst& I = Ap->inst[k];
  E.k  = k;
  E.li = g - I.globalOffset;
  loadParticle(I, E.li, E.R, E.s, E.p);
  E.density = I.alpha[E.li];
  // rgen.slang:697-698: origin through transformInverse, direction through transformRotScaleInverse (normalised for the response;
  // the intersection's t uses the unnormalised one, so that it is the WORLD ray's parameter)
  const float* Mi = I.modelInv;
  const float* Ri = a.inst->inst[k].rsInv;
  float        dm[3];
#pragma unroll
  for(int r = 0; r < 3; ++r)
  {
    E.om[r] = Mi[r] * ray.o[0] + Mi[4 + r] * ray.o[1] + Mi[8 + r] * ray.o[2] + Mi[12 + r];
    dm[r]   = Ri[r] * ray.d[0] + Ri[3 + r] * ray.d[1] + Ri[6 + r] * ray.d[2];
  }
  const float dl = rsqrtf(dm[0] * dm[0] + dm[1] * dm[1] + dm[2] * dm[2]);
  const float x0 = E.om[0] - E.p[0], x1 = E.om[1] - E.p[1], x2 = E.om[2] - E.p[2];
#pragma unroll
  for(int c = 0; c < 3; ++c)
  {  // mul(v, invRotation) = R^T v, then 1 / scale (threedgrt.h.slang:65-73)
    const float is = 1.0f / E.s[c];
    E.oc[c]  = (x0 * E.R[c] + x1 * E.R[3 + c] + x2 * E.R[6 + c]) * is;
    E.dc[c]  = (dm[0] * E.R[c] + dm[1] * E.R[3 + c] + dm[2] * E.R[6 + c]) * is;
    E.dmN[c] = dm[c] * dl;
  }
  const float dd = E.dc[0] * E.dc[0] + E.dc[1] * E.dc[1] + E.dc[2] * E.dc[2];
  E.t            = -(E.oc[0] * E.dc[0] + E.oc[1] * E.dc[1] + E.oc[2] * E.dc[2]) / dd;
  const float kx = E.dc[1] * E.oc[2] - E.dc[2] * E.oc[1], ky = E.dc[2] * E.oc[0] - E.dc[0] * E.oc[2],
              kz = E.dc[0] * E.oc[1] - E.dc[1] * E.oc[0];
  const float dist2 = (kx * kx + ky * ky + kz * kz) / dd;  // |cross(normalize(dc), oc)|^2, :77-81
  E.resp            = kernelResponse(a.proxy.kernelDegree, dist2);
}

// model-space normal of an accepted hit (computeEllipsoidNormalMaxDensityPlane :358-418, computeEllipsoidNormal :423-496), to world
// space as particleProcessHit does (:218): normalize(transpose(transformRotScaleInverse)-product), i.e. the inverse transpose
__device__ __forceinline__ void hitNormalWorld(const TraceArgs& a, const FrameConst& F, const ParticleEval& E, float (&nw)[3])
{
  const float l0 = E.om[0] - E.p[0], l1 = E.om[1] - E.p[1], l2 = E.om[2] - E.p[2];
  const bool  iso = F.normalMethod == 1;
  const float th  = iso ? fmaxf(0.02f * fmaxf(fmaxf(E.s[0], E.s[1]), E.s[2]), F.thinParticleThreshold) : F.thinParticleThreshold;
  const bool  t0 = E.s[0] < th, t1 = E.s[1] < th, t2 = E.s[2] < th;
  const int   smallCount = (t0 ? 1 : 0) + (t1 ? 1 : 0) + (t2 ? 1 : 0);
  const float* R = E.R;
  float        n0 = -E.dmN[0], n1 = -E.dmN[1], n2 = -E.dmN[2];  // two or more degenerate axes, or no surface point: -rayDirection
  if(smallCount == 0 && !iso)
  {
    const float c0 = (l0 * R[0] + l1 * R[3] + l2 * R[6]) * (1.0f / (E.s[0] * E.s[0]));
    const float c1 = (l0 * R[1] + l1 * R[4] + l2 * R[7]) * (1.0f / (E.s[1] * E.s[1]));
    const float c2 = (l0 * R[2] + l1 * R[5] + l2 * R[8]) * (1.0f / (E.s[2] * E.s[2]));
    const float g0 = c0 * R[0] + c1 * R[1] + c2 * R[2], g1 = c0 * R[3] + c1 * R[4] + c2 * R[5], g2 = c0 * R[6] + c1 * R[7] + c2 * R[8];
    const float rl = rsqrtf(g0 * g0 + g1 * g1 + g2 * g2);
    n0 = g0 * rl; n1 = g1 * rl; n2 = g2 * rl;
    if(n0 * l0 + n1 * l1 + n2 * l2 < 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
  }
  else if(smallCount == 0)
  {  // raySphereIntersection(canonical origin, NORMALISED canonical direction, 3, 0, inf), written around the point of closest
     // approach like the 3DGUT compositor (k_composite_gut.hip has the reason: the textbook discriminant cancels in fp32)
    const float dd = E.dc[0] * E.dc[0] + E.dc[1] * E.dc[1] + E.dc[2] * E.dc[2];
    const float tm = -(E.oc[0] * E.dc[0] + E.oc[1] * E.dc[1] + E.oc[2] * E.dc[2]) / dd;
    const float kx = E.dc[1] * E.oc[2] - E.dc[2] * E.oc[1], ky = E.dc[2] * E.oc[0] - E.dc[0] * E.oc[2],
                kz = E.dc[0] * E.oc[1] - E.dc[1] * E.oc[0];
    const float rem = 9.0f - (kx * kx + ky * ky + kz * kz) / dd;
    if(rem >= 0.0f)
    {
      const float half = sqrtf(rem / dd);
      const float tq   = (tm - half >= 0.0f) ? tm - half : tm + half;
      if(tq >= 0.0f)
      {
        float       h0 = E.oc[0] + tq * E.dc[0], h1 = E.oc[1] + tq * E.dc[1], h2 = E.oc[2] + tq * E.dc[2];
        const float hl = rsqrtf(h0 * h0 + h1 * h1 + h2 * h2);
        h0 = h0 * hl / E.s[0]; h1 = h1 * hl / E.s[1]; h2 = h2 * hl / E.s[2];
        const float g0 = R[0] * h0 + R[1] * h1 + R[2] * h2, g1 = R[3] * h0 + R[4] * h1 + R[5] * h2, g2 = R[6] * h0 + R[7] * h1 + R[8] * h2;
        const float rl = rsqrtf(g0 * g0 + g1 * g1 + g2 * g2);
        n0 = g0 * rl; n1 = g1 * rl; n2 = g2 * rl;
      }
    }
  }
  else if(smallCount == 1)
  {
    n0 = t0 ? R[0] : (t1 ? R[1] : R[2]);  // (selects: a runtime index would put the particle into scratch memory)
    n1 = t0 ? R[3] : (t1 ? R[4] : R[5]);
    n2 = t0 ? R[6] : (t1 ? R[7] : R[8]);
    if(n0 * l0 + n1 * l1 + n2 * l2 < 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
  }
  const float* Ri = a.inst->inst[E.k].rsInv;  // glm column-major: (Ri^T n)_c = sum_r Ri[3c + r] n_r
  const float  w0 = Ri[0] * n0 + Ri[1] * n1 + Ri[2] * n2, w1 = Ri[3] * n0 + Ri[4] * n1 + Ri[5] * n2, w2 = Ri[6] * n0 + Ri[7] * n1 + Ri[8] * n2;
  const float  wl = rsqrtf(w0 * w0 + w1 * w1 + w2 * w2);
  nw[0] = w0 * wl; nw[1] = w1 * wl; nw[2] = w2 * wl;
}

#define MGS_CSWAP(x, y) { const uint32_t lo_ = min(key[x], key[y]), hi_ = max(key[x], key[y]); key[x] = lo_; key[y] = hi_; }

// SHF: SH storage format; KB: K-buffer slots in registers (>= samples_per_pass)
template <int SHF, int KB>
__global__ __launch_bounds__(256) void k_trace(TraceArgs a)
{
  __shared__ uint32_t s_pend[kBvhMaxLevels][256];  // per level: the open node's children still to visit, 3 bits each, count in bits 24-27
  __shared__ uint32_t s_off[kBvhMaxLevels], s_cnt[kBvhMaxLevels];
  const FrameArgs*  Ap = a.frame;
  const FrameConst& F  = Ap->f;
  const int tid = threadIdx.x, lane = laneId(), w = tid >> 6;
#pragma unroll
  for(int l = 0; l < kBvhMaxLevels; ++l)  // (static indices: a runtime index into the argument block would copy it to scratch memory)
    if(tid == l)
    {
      s_off[l] = a.levelOffset[l];
      s_cnt[l] = a.levelCount[l];
    }
  __syncthreads();
  const int tx = (int)blockIdx.x % F.tilesX, ty = F.stripRow0 + (int)blockIdx.x / F.tilesX;
  const int px = tx * kTilePx + (w & 1) * 8 + (lane & 7), py = ty * kTilePx + (w >> 1) * 8 + (lane >> 3);
  if(px >= F.width || py >= F.height)
    return;  // (no barrier below)
  const size_t pix = (size_t)py * F.width + px;

  // ---- the ray (rgen.slang:165-196) ----
  TraceRay     ray;
  const float* Vi = F.lightViewInv;  // viewInverse / projInverse: host double, rounded once
  const float* Pi = F.lightProjInv;
  bool         rayOk = true;
  {
    float cx, cy, cz;
    if(F.cameraModel == 1)
    {  // generateFisheyeRay(launchIdFloat, ...): the pixel's integer coordinate, as written (cameras.h.slang:46-82)
      const float u = ((float)px / ((float)F.width - 1.0f)) * 2.0f - 1.0f, v = ((float)py / ((float)F.height - 1.0f)) * 2.0f - 1.0f;
      const float r = sqrtf(u * u + v * v);
      rayOk         = !(r > 1.0f);
      float phiCos  = fabsf(r) > 1e-9f ? u / r : 0.0f;
      phiCos        = fminf(fmaxf(phiCos, -1.0f), 1.0f);
      float phi     = acosf(phiCos);
      phi           = v < 0.0f ? -phi : phi;
      const float theta = r * F.fovRad * 0.5f;
      cx = cosf(phi) * sinf(theta);
      cy = -sinf(phi) * sinf(theta);
      cz = -cosf(theta);
    }
    else
    {  // generatePinholeRay(launchIdFloat, 0.5, ...), cameras.h.slang:27-44
      const float ux = (((float)px + 0.5f) / (float)F.width) * 2.0f - 1.0f, uy = (((float)py + 0.5f) / (float)F.height) * 2.0f - 1.0f;
      cx = Pi[0] * ux + Pi[4] * uy + Pi[8] + Pi[12];
      cy = Pi[1] * ux + Pi[5] * uy + Pi[9] + Pi[13];
      cz = Pi[2] * ux + Pi[6] * uy + Pi[10] + Pi[14];
    }
    float dx = Vi[0] * cx + Vi[4] * cy + Vi[8] * cz, dy = Vi[1] * cx + Vi[5] * cy + Vi[9] * cz, dz = Vi[2] * cx + Vi[6] * cy + Vi[10] * cz;
    const float l = rsqrtf(dx * dx + dy * dy + dz * dz);
    ray.d[0] = dx * l; ray.d[1] = dy * l; ray.d[2] = dz * l;
    ray.o[0] = Vi[12]; ray.o[1] = Vi[13]; ray.o[2] = Vi[14];
    if(F.dofMode != 0)
    {  // depthOfField (cameras.h.slang:85-105), seeded as rgen.slang:193
      uint32_t    seed = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);
      const float r1 = rngRand(seed) * 6.28318530717958647692f, r2 = rngRand(seed) * F.aperture;
      const float c = cosf(r1), sn = sinf(r1), sq = sqrtf(r2);
      const float lx = (c * Vi[0] + sn * Vi[4]) * sq, ly = (c * Vi[1] + sn * Vi[5]) * sq, lz = (c * Vi[2] + sn * Vi[6]) * sq;
      const float fx = ray.d[0] * F.focusDist - lx, fy = ray.d[1] * F.focusDist - ly, fz = ray.d[2] * F.focusDist - lz;
      const float fl = rsqrtf(fx * fx + fy * fy + fz * fz);
      ray.o[0] += lx; ray.o[1] += ly; ray.o[2] += lz;
      ray.d[0] = fx * fl; ray.d[1] = fy * fl; ray.d[2] = fz * fl;
    }
#pragma unroll
    for(int c = 0; c < 3; ++c)
      ray.inv[c] = 1.0f / ray.d[c];
  }

  const int      K       = a.samplesPerPass;
  const int      top     = a.nLevels - 1;
  const uint32_t maxStep = 2u * a.totalNodes + 2u;
  const bool     surf    = a.outDepth != nullptr;
  const bool     noGauss = (F.debugFlags & 4) != 0, shOnly = (F.debugFlags & 2) != 0;
  const float    INF     = __builtin_huge_valf();
  constexpr float epsT   = 1e-9f;  // rgen.slang:157

  double   T = 1.0;  // pixel.transmittance: kept in double like the reference (one fp64 multiply per accepted hit)
  float    cr = 0.f, cg = 0.f, cb = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, wsum = 0.f, isoDist = 0.0f;
  uint32_t hitCount = 0, pickId = kTraceInvalid, passesUsed = 0;
  unsigned long long nodeVisits = 0, candTests = 0;
  float    tMin = 0.001f;
  const float tMax = 10000.0f;

  if(rayOk && a.nLevels > 0)
    for(int pass = 0; pass < a.maxPasses; ++pass)  // bound: max_passes
    {
      if(!(tMin <= tMax) || !(T > (double)a.minTransmittance))
        break;
      ++passesUsed;
      float    kd[KB];
      uint32_t kid[KB];
#pragma unroll
      for(int i = 0; i < KB; ++i)
      {
        kd[i]  = INF;
        kid[i] = kTraceInvalid;
      }
      float       kth = INF;  // distance in slot K - 1
      const float t0 = tMin + epsT, t1 = tMax + epsT;

      // a candidate: exists for the pass when t0 < t < t1 and the proxy test passes; inserted as rahit.slang:152-167, ties in t by
      // ascending global id in the caller's order
      auto candidate = [&](uint32_t g) {
        ++candTests;
        ParticleEval E;
        evalParticle(a, g, ray, E);
        if(!(E.t > t0 && E.t < t1) || !(E.resp > proxyThreshold(a.proxy, E.density)))
          return;
        float    ct  = E.t;
        uint32_t cid = g;
#pragma unroll
        for(int i = 0; i < KB; ++i)
        {
          bool before = ct < kd[i];
          if(ct == kd[i] && cid != kTraceInvalid && kid[i] != kTraceInvalid)
            before = a.callerId[cid] < a.callerId[kid[i]];
          if(before)
          {
            const float    td = kd[i];
            const uint32_t ti = kid[i];
            kd[i]  = ct;
            kid[i] = cid;
            ct     = td;
            cid    = ti;
          }
          if(i == K - 1)
            kth = kd[i];
        }
      };
      // open node (level, idx): its children that the ray meets no farther than the K-th distance, nearest first
      auto expand = [&](int level, uint32_t idx) {
        const uint32_t nBelow = s_cnt[level - 1], base = s_off[level - 1];
        uint32_t       key[8];
#pragma unroll
        for(int c = 0; c < 8; ++c)  // bound: 8 children
        {
          const uint32_t ci = idx * 8u + (uint32_t)c;
          key[c]            = 0xFFFFFFFFu;
          if(ci < nBelow)
          {
            const float4 lo = a.nodes[2 * (size_t)(base + ci)], hi = a.nodes[2 * (size_t)(base + ci) + 1];
            float        te;
            if(slabHit(ray, lo, hi, t0, t1, te) && te <= kth)
              key[c] = (__float_as_uint(te) & ~7u) | (uint32_t)c;
          }
        }
        // sorting network of 8 (19 compare-exchanges): entry distances are >= 0, so their bits order like the values
        MGS_CSWAP(0, 1) MGS_CSWAP(2, 3) MGS_CSWAP(4, 5) MGS_CSWAP(6, 7)
        MGS_CSWAP(0, 2) MGS_CSWAP(1, 3) MGS_CSWAP(4, 6) MGS_CSWAP(5, 7)
        MGS_CSWAP(1, 2) MGS_CSWAP(5, 6) MGS_CSWAP(0, 4) MGS_CSWAP(3, 7)
        MGS_CSWAP(1, 5) MGS_CSWAP(2, 6)
        MGS_CSWAP(1, 4) MGS_CSWAP(3, 6)
        MGS_CSWAP(2, 4) MGS_CSWAP(3, 5)
        MGS_CSWAP(3, 4)
        uint32_t pend = 0, cnt = 0;
#pragma unroll
        for(int c = 0; c < 8; ++c)
          if(key[c] != 0xFFFFFFFFu)
          {
            pend |= (key[c] & 7u) << (3 * c);
            ++cnt;
          }
        s_pend[level][tid] = pend | (cnt << 24);
      };

      // ---- collect the K nearest hits of (t0, t1) ----
      if(top == 0)
      {  // a single leaf
        const float4 lo = a.nodes[0], hi = a.nodes[1];
        float        te;
        ++nodeVisits;
        if(slabHit(ray, lo, hi, t0, t1, te))
          candidate(__float_as_uint(lo.w));
      }
      else
      {
        int      level = top;
        uint32_t idx   = 0;
        expand(level, idx);
        for(uint32_t step = 0; step < maxStep; ++step)  // bound: every node is entered once and left once
        {
          const uint32_t pend = s_pend[level][tid];
          const uint32_t cnt  = pend >> 24;
          if(cnt == 0u)
          {
            if(level == top)
              break;
            ++level;
            idx >>= 3;
            continue;
          }
          s_pend[level][tid] = ((pend & 0xFFFFFFu) >> 3) | ((cnt - 1u) << 24);
          const uint32_t ci   = idx * 8u + (pend & 7u);
          const uint32_t node = s_off[level - 1] + ci;
          const float4   lo = a.nodes[2 * (size_t)node], hi = a.nodes[2 * (size_t)node + 1];
          float          te;
          ++nodeVisits;
          // the K-th distance may have come down since the node was queued (rahit.slang:75); equality still visits, so that the
          // tie order does not depend on the order of traversal
          if(!slabHit(ray, lo, hi, t0, t1, te) || !(te <= kth))
            continue;
          if(level == 1)
            candidate(__float_as_uint(lo.w));
          else
          {
            --level;
            idx = ci;
            expand(level, idx);
          }
        }
      }
      if(kid[0] == kTraceInvalid)
        break;  // no more hits (rgen.slang:661-667)

      // ---- walk them in order (rgen.slang:676-763) ----
      for(int slot = 0; slot < K; ++slot)  // bound: samples_per_pass
      {
        const uint32_t g    = kid[0];
        const float    dist = kd[0];
#pragma unroll
        for(int i = 0; i + 1 < KB; ++i)
        {
          kd[i]  = kd[i + 1];
          kid[i] = kid[i + 1];
        }
        kd[KB - 1]  = INF;
        kid[KB - 1] = kTraceInvalid;
        if(g == kTraceInvalid)
          break;  // the slots are sorted: nothing valid behind an empty one
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

  // ---- the pixel (writeToGBuffers, rgen.slang:1466-1502; alpha = 1 - T here, 1.0 in the reference) ----
  float alphaOut = 1.0f - (float)T;
  if(!rayOk)
    alphaOut = 1.0f;  // rgen.slang:185
  a.hitCount[pix] = hitCount;
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
  if(a.halfOut == 1)
  {
    const __half2 lo = __floats2half2_rn(cr, cg), hi2 = __floats2half2_rn(cb, alphaOut);
    uint2         o;
    o.x = *reinterpret_cast<const uint32_t*>(&lo);
    o.y = *reinterpret_cast<const uint32_t*>(&hi2);
    reinterpret_cast<uint2*>(a.image)[pix] = o;
  }
  else if(a.halfOut == 0)
    reinterpret_cast<float4*>(a.image)[pix] = make_float4(cr, cg, cb, alphaOut);
  else
  {
    auto q = [](float v) { return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); };
    reinterpret_cast<uint32_t*>(a.image)[pix] = q(cr) | (q(cg) << 8) | (q(cb) << 16) | (q(alphaOut) << 24);
  }
  // statistics: integer sums, so the totals do not depend on the order of arrival
  atomicAdd(&a.ctr->nodeVisits, nodeVisits);
  atomicAdd(&a.ctr->candidateTests, candTests);
  atomicAdd(&a.ctr->acceptedHits, (unsigned long long)hitCount);
  atomicMax(&a.ctr->maxPassesUsed, passesUsed);
}
#undef MGS_CSWAP

[[noreturn]] static void unlistedTrace(int v)
{
  std::fprintf(stderr, "launchTrace: no traversal instantiation for variant %d\n", v);
  std::abort();
}

void launchTrace(hipStream_t stream, const TraceArgs& a, const FrameConst& F, int shFormat)
{
  const int tiles = F.tilesX * (F.stripRow1 - F.stripRow0);
  if(tiles <= 0)
    return;
  const int shf = shFormat == 0 ? 0 : shFormat == 1 ? 1 : 2;
  const int kb  = a.samplesPerPass <= 4 ? 0 : a.samplesPerPass <= 18 ? 1 : 2;
#define MGS_TRACE(SHF, KBI, KB) case(SHF) * 3 + (KBI): hipLaunchKernelGGL((k_trace<SHF, KB>), dim3(tiles), dim3(256), 0, stream, a); break;
  switch(shf * 3 + kb)
  {
    MGS_TRACE(0, 0, 4) MGS_TRACE(0, 1, 18) MGS_TRACE(0, 2, 32)
    MGS_TRACE(1, 0, 4) MGS_TRACE(1, 1, 18) MGS_TRACE(1, 2, 32)
    MGS_TRACE(2, 0, 4) MGS_TRACE(2, 1, 18) MGS_TRACE(2, 2, 32)
    default: unlistedTrace(shf * 3 + kb);
  }
#undef MGS_TRACE
}

}  // namespace mgs
