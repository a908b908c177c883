// trace_traverse.h — what every ray of the traced pipeline does alike, primary (k_trace.hip) or shadow (k_trace_light.hip): the
// pixel's ray, a particle against a ray, and the collection of the K nearest hits of a ray's (t0, t1) window through the hierarchy.
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:165-196    ray generation, depth of field
//   shaders/threedgrt_raytrace.rahit.slang:71-75,152-173   the any-hit insertion into the sorted payload and its distance cut
//   shaders/threedgrt_raytrace.rint.slang:159-172    particleDensityHitInstance: t of the maximum response, in the particle's frame
//   shaders/threedgrt.h.slang:57-127                 canonical ray, response
// The traversal stack is ONE packed word per tree level in LDS (the children of the node open at that level that are still to
// visit, nearest first), so its depth is the tree's depth; the K-buffer (distance + id) lives in the caller's registers.  The
// traversal is bounded by 2 * nodes + 2 steps (a node is entered once and left once), children by 8.  Nothing waits on another
// lane, wave or workgroup.  Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include "gut_common.h"
#include "kernels_common.h"
#include "trace_common.h"

namespace mgs {

struct TraceRay
{
  float o[3], d[3], inv[3];
};

// the LDS of a 256-lane workgroup's traversal: per level the open node's children still to visit (3 bits each, count in bits
// 24-27), and the levels' offsets and counts
struct TraceLds
{
  uint32_t pend[kBvhMaxLevels][256];
  uint32_t off[kBvhMaxLevels], cnt[kBvhMaxLevels];
};
__device__ __forceinline__ void traceLdsInit(TraceLds& S, const TraceArgs& a, int tid)
{
#pragma unroll
  for(int l = 0; l < kBvhMaxLevels; ++l)  // (static indices: a runtime index into the argument block would copy it to scratch memory)
    if(tid == l)
    {
      S.off[l] = a.levelOffset[l];
      S.cnt[l] = a.levelCount[l];
    }
  __syncthreads();
}

// the lane's pixel in the traced pipeline's tiling: a workgroup = a 16 x 16 tile of the frame's strip, a wave64 = an 8 x 8 quarter of it
__device__ __forceinline__ void tilePixel(const FrameConst& F, int tid, int& px, int& py)
{
  const int lane = laneId(), w = tid >> 6;
  const int tx = (int)blockIdx.x % F.tilesX, ty = F.stripRow0 + (int)blockIdx.x / F.tilesX;
  px = tx * kTilePx + (w & 1) * 8 + (lane & 7);
  py = ty * kTilePx + (w >> 1) * 8 + (lane >> 3);
}

// the pixel's primary ray (rgen.slang:165-196); false: a fisheye pixel outside the image circle
__device__ __forceinline__ bool primaryRay(const FrameConst& F, int px, int py, TraceRay& ray)
{
  const float* Vi = F.lightViewInv;  // viewInverse / projInverse: host double, rounded once
  const float* Pi = F.lightProjInv;
  bool         rayOk = true;
  float        cx, cy, cz;
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
  return rayOk;
}

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

#define MGS_CSWAP(x, y) { const uint32_t lo_ = min(key[x], key[y]), hi_ = max(key[x], key[y]); key[x] = lo_; key[y] = hi_; }

// The K nearest hits of the ray inside (t0, t1), through the proxies: kd / kid come back sorted by (t, caller's id), empty slots
// hold (inf, kTraceInvalid).  KB: K-buffer slots in registers (>= K).  A candidate exists when t0 < t < t1 and the proxy test
// passes; it is inserted as rahit.slang:152-167, ties in t by ascending global id in the caller's order.
// The walk below (expand, the sorting network, the step loop) has a copy in traverseProxies, further down, which says why: a fix to
// one is a fix to both.
// The buffer is a local of the function and comes back by value: handed in by reference it stays memory until the function is inlined,
// and the traversal then allocates half as many registers again.
template <int KB>
struct NearestK
{
  float              kd[KB];
  uint32_t           kid[KB];
  unsigned long long nodeVisits, candTests;  // of this collection
};
template <int KB>
__device__ __forceinline__ NearestK<KB> collectNearest(const TraceArgs& a, TraceLds& S, int tid, const TraceRay& ray, float t0, float t1, int K)
{
  NearestK<KB>       N;
  float (&kd)[KB]     = N.kd;
  uint32_t (&kid)[KB] = N.kid;
  unsigned long long nodeVisits = 0, candTests = 0;
  const int      top     = a.nLevels - 1;
  const uint32_t maxStep = 2u * a.totalNodes + 2u;
  const float    INF     = __builtin_huge_valf();
#pragma unroll
  for(int i = 0; i < KB; ++i)
  {
    kd[i]  = INF;
    kid[i] = kTraceInvalid;
  }
  float kth = INF;  // distance in slot K - 1

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
    const uint32_t nBelow = S.cnt[level - 1], base = S.off[level - 1];
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
    S.pend[level][tid] = pend | (cnt << 24);
  };

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
      const uint32_t pend = S.pend[level][tid];
      const uint32_t cnt  = pend >> 24;
      if(cnt == 0u)
      {
        if(level == top)
          break;
        ++level;
        idx >>= 3;
        continue;
      }
      S.pend[level][tid] = ((pend & 0xFFFFFFu) >> 3) | ((cnt - 1u) << 24);
      const uint32_t ci   = idx * 8u + (pend & 7u);
      const uint32_t node = S.off[level - 1] + ci;
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
  N.nodeVisits = nodeVisits;
  N.candTests  = candTests;
  return N;
}

// The same walk with the candidate step left to the caller (the stochastic any-hit of k_trace_stochastic.hip, whose step is an
// accept-and-draw into one slot instead of the sorted insertion): candidate(g) is called for the particle of every leaf whose box
// the ray meets inside [t0, t1] no farther than `cut`, nearest children first.  `cut` is the caller's variable and is read again
// at every node, so a candidate may lower it; a box AT the cut is still visited (te <= cut, as above).  collectNearest keeps its own
// copy of the walk: routed through this function k_trace<0, 4> and k_trace<0, 18> take one more VGPR each, and the sorted
// strategy's kernels are held to their resources.
template <class Candidate>
__device__ __forceinline__ void traverseProxies(const TraceArgs& a, TraceLds& S, int tid, const TraceRay& ray, float t0, float t1, const float& cut,
                                                Candidate&& candidate, unsigned long long& nodeVisits)
{
  const int      top     = a.nLevels - 1;
  const uint32_t maxStep = 2u * a.totalNodes + 2u;
  auto expand = [&](int level, uint32_t idx) {
    const uint32_t nBelow = S.cnt[level - 1], base = S.off[level - 1];
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
        if(slabHit(ray, lo, hi, t0, t1, te) && te <= cut)
          key[c] = (__float_as_uint(te) & ~7u) | (uint32_t)c;
      }
    }
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
    S.pend[level][tid] = pend | (cnt << 24);
  };

  if(top == 0)
  {  // a single leaf
    const float4 lo = a.nodes[0], hi = a.nodes[1];
    float        te;
    ++nodeVisits;
    if(slabHit(ray, lo, hi, t0, t1, te))
      candidate(__float_as_uint(lo.w));
    return;
  }
  int      level = top;
  uint32_t idx   = 0;
  expand(level, idx);
  for(uint32_t step = 0; step < maxStep; ++step)  // bound: every node is entered once and left once
  {
    const uint32_t pend = S.pend[level][tid];
    const uint32_t cnt  = pend >> 24;
    if(cnt == 0u)
    {
      if(level == top)
        break;
      ++level;
      idx >>= 3;
      continue;
    }
    S.pend[level][tid] = ((pend & 0xFFFFFFu) >> 3) | ((cnt - 1u) << 24);
    const uint32_t ci   = idx * 8u + (pend & 7u);
    const uint32_t node = S.off[level - 1] + ci;
    const float4   lo = a.nodes[2 * (size_t)node], hi = a.nodes[2 * (size_t)node + 1];
    float          te;
    ++nodeVisits;
    if(!slabHit(ray, lo, hi, t0, t1, te) || !(te <= cut))
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
#undef MGS_CSWAP

// the first slot of a sorted K-buffer, the rest moved up by one (static indices: the buffer stays in registers)
template <int KB>
__device__ __forceinline__ void popNearest(NearestK<KB>& N, float& dist, uint32_t& g)
{
  float (&kd)[KB]     = N.kd;
  uint32_t (&kid)[KB] = N.kid;
  g    = kid[0];
  dist = kd[0];
#pragma unroll
  for(int i = 0; i + 1 < KB; ++i)
  {
    kd[i]  = kd[i + 1];
    kid[i] = kid[i + 1];
  }
  kd[KB - 1]  = __builtin_huge_valf();
  kid[KB - 1] = kTraceInvalid;
}

}  // namespace mgs
