// k_mesh.hip — the mesh pass: triangle meshes rasterised on the device into the occluder's depth and colour images.
//
// Restates shaders/threedmesh_raster.vert.slang:53-62 and threedmesh_raster.frag.slang:67-103 (the non-hybrid colour branch) around
// a software rasteriser whose rules are written down in include/mgs.h (mgs_meshes_render).  Four stages, one launch each:
//   k_mesh_clear    the visibility words of the handle's rows (all ones = depth clear, no primitive) and the counters;
//   k_mesh_setup    one primitive per lane: vertex stage, clipping, snap to 1/256 pixel, set-up record.  A (sub-)triangle whose
//                   bounding box is at most 8 x 8 pixels is walked by its own lane; a larger one is cut into chunks of 16 tiles of
//                   8 x 8 pixels that go to a work list — one wave-wide prefix sum and ONE atomic per wave, not one per lane.  The
//                   counter is never taken back: a lane whose chunks do not fit marks what it claimed as void and walks itself;
//   k_mesh_large    a fixed grid of waves strides over the work list (its length never leaves the device): a wave takes a chunk,
//                   rejects the tiles the three edge functions exclude and tests one pixel per lane in the others;
//   k_mesh_resolve  one pixel per lane: the winning record, barycentrics recomputed from the snapped vertices, the vertex stage
//                   of the primitive's three vertices, perspective-correct attributes, shading, plain stores.
// Visibility is a 64-bit unsigned atomic minimum on (depth bits << 32 | primitive << 3 | sub-triangle): LESS in primitive order,
// independent of arrival order.  Coverage is decided in 64-bit integers, so a shared edge is covered exactly once.
#include <hip/hip_runtime.h>

#include "../../include/mgs.h"
#include "launchers.h"
#include "shade_direct.h"

namespace mgs {

namespace {

constexpr float kGuard = 256.0f;  // |x|, |y| <= kGuard * w: window coordinates stay below 2^21 pixels at 8192 pixels, 2^29 in 1/256 pixel, so
                                  // that differences fit 2^30, their products 2^60 and an edge function 2^61

// mul(v, M) of the shaders on a glm column-major matrix == M * v, each component summed in the order of v's components
__device__ __forceinline__ float4 mulMat(const float* __restrict__ m, float4 v)
{
  float4 r;
  r.x = ((v.x * m[0] + v.y * m[4]) + v.z * m[8]) + v.w * m[12];
  r.y = ((v.x * m[1] + v.y * m[5]) + v.z * m[9]) + v.w * m[13];
  r.z = ((v.x * m[2] + v.y * m[6]) + v.z * m[10]) + v.w * m[14];
  r.w = ((v.x * m[3] + v.y * m[7]) + v.z * m[11]) + v.w * m[15];
  return r;
}

// the instance that owns a global primitive index: the last one whose first primitive is not above it
__device__ __forceinline__ int meshInstanceOf(const MeshTable* __restrict__ T, uint32_t prim)
{
  int lo = 0, hi = (int)T->count;
  while(hi - lo > 1)
  {
    const int mid = (lo + hi) >> 1;
    if(T->inst[mid].triBegin <= prim)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// threedmesh_raster.vert.slang:55,62: worldPos = M p, clip = P (V worldPos)
__device__ __forceinline__ V3 worldPosOf(const MeshInstDev& I, uint32_t vi)
{
  const float4 wp = mulMat(I.M, make_float4(I.pos[3 * vi], I.pos[3 * vi + 1], I.pos[3 * vi + 2], 1.0f));
  return {wp.x, wp.y, wp.z};
}
__device__ __forceinline__ float4 clipOf(const MeshPassArgs& a, V3 wp)
{
  return mulMat(a.proj, mulMat(a.view, make_float4(wp.x, wp.y, wp.z, 1.0f)));
}
// :60: normalize(mul(normal, transpose(transformRotScaleInverse)))
__device__ __forceinline__ V3 worldNrmOf(const MeshInstDev& I, uint32_t vi)
{
  const float nx = I.nrm[3 * vi], ny = I.nrm[3 * vi + 1], nz = I.nrm[3 * vi + 2];
  const float* r = I.rsInv;
  const V3     n = {(nx * r[0] + ny * r[1]) + nz * r[2], (nx * r[3] + ny * r[4]) + nz * r[5], (nx * r[6] + ny * r[7]) + nz * r[8]};
  return normalize3(n);
}

__device__ __forceinline__ bool finite4(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w); }

__device__ __forceinline__ float planeDist(int pl, float4 c)
{
  switch(pl)
  {
    case 0: return c.z;                  // near: clip z >= 0
    case 1: return c.x + kGuard * c.w;
    case 2: return kGuard * c.w - c.x;
    case 3: return c.y + kGuard * c.w;
    default: return kGuard * c.w - c.y;
  }
}

__device__ __forceinline__ float4 combine4(float b0, float b1, float b2, float4 c0, float4 c1, float4 c2)
{
  return make_float4((b0 * c0.x + b1 * c1.x) + b2 * c2.x, (b0 * c0.y + b1 * c1.y) + b2 * c2.y, (b0 * c0.z + b1 * c1.z) + b2 * c2.z,
                     (b0 * c0.w + b1 * c1.w) + b2 * c2.w);
}
__device__ __forceinline__ V3 combine3(float b0, float b1, float b2, V3 a0, V3 a1, V3 a2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// a (sub-)triangle as coverage and resolve see it
struct Geo
{
  int32_t x[3], y[3];
  float   z[3], invw[3];
};

// clip coordinates -> snapped window coordinates, window depth, 1 / w.  false: not representable (w <= 0, non-finite, outside the
// fixed-point range), the primitive is dropped
__device__ __forceinline__ bool toWindow(const MeshPassArgs& a, float4 c, int32_t& X, int32_t& Y, float& z, float& invw)
{
  if(!(c.w > 0.0f))
    return false;
  const float wx = ((c.x / c.w) * 0.5f + 0.5f) * (float)a.width;
  const float wy = ((c.y / c.w) * 0.5f + 0.5f) * (float)a.height;
  z              = c.z / c.w;
  invw           = 1.0f / c.w;
  if(!(fabsf(wx) <= 2097152.0f) || !(fabsf(wy) <= 2097152.0f) || !isfinite(z) || !isfinite(invw))
    return false;
  X = (int32_t)rintf(wx * 256.0f);  // round to nearest even
  Y = (int32_t)rintf(wy * 256.0f);
  return true;
}

// edge function of a -> b at p, exact in 64 bits (coordinates at most 2^29 in 1/256 pixel)
__device__ __forceinline__ long long edgeFn(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py)
{
  return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}
// top-left rule for an edge of a triangle oriented so that the interior has positive edge functions, in the frame's row order
// (row 0 = NDC y -1): a left edge (dy < 0: the interior lies toward larger x) or a top edge (horizontal, dx > 0: the interior lies
// toward larger row index) owns the samples on it
__device__ __forceinline__ long long edgeBias(int32_t ax, int32_t ay, int32_t bx, int32_t by)
{
  const int32_t dx = bx - ax, dy = by - ay;
  return (dy < 0 || (dy == 0 && dx > 0)) ? 0ll : -1ll;
}

// orient for a positive area (both windings are drawn): swaps vertices 1 and 2.  Returns twice the area in 1/256-pixel units
__device__ __forceinline__ long long orient(Geo& g, bool& swapped)
{
  long long area2 = edgeFn(g.x[0], g.y[0], g.x[1], g.y[1], g.x[2], g.y[2]);
  swapped         = area2 < 0;
  if(swapped)
  {
    int32_t t;
    float   f;
    t = g.x[1], g.x[1] = g.x[2], g.x[2] = t;
    t = g.y[1], g.y[1] = g.y[2], g.y[2] = t;
    f = g.z[1], g.z[1] = g.z[2], g.z[2] = f;
    f = g.invw[1], g.invw[1] = g.invw[2], g.invw[2] = f;
    area2 = -area2;
  }
  return area2;
}

// one sample: coverage, depth, the visibility minimum.  Returns 1 when a fragment was produced (covered, depth in [0, 1))
__device__ __forceinline__ uint32_t coverPixel(const MeshPassArgs& a, const Geo& g, long long area2, long long b0, long long b1, long long b2,
                                               int32_t px, int32_t py, uint32_t ref)
{
  const int32_t  sx = px * 256 + 128, sy = py * 256 + 128;  // the pixel centre
  const long long e0 = edgeFn(g.x[1], g.y[1], g.x[2], g.y[2], sx, sy);
  const long long e1 = edgeFn(g.x[2], g.y[2], g.x[0], g.y[0], sx, sy);
  const long long e2 = edgeFn(g.x[0], g.y[0], g.x[1], g.y[1], sx, sy);
  if((e0 + b0) < 0 || (e1 + b1) < 0 || (e2 + b2) < 0)
    return 0;
  const float fa = (float)area2;
  // z0 + b1 (z1 - z0) + b2 (z2 - z0): a triangle of constant depth keeps exactly that depth.  Every rounding is spelled out, so that
  // the two kernels that inline this (a strip pass may walk a triangle the full pass sends to the work list) give the same bits
  const float z = __fmaf_rn(__fdiv_rn((float)e2, fa), __fsub_rn(g.z[2], g.z[0]),
                            __fmaf_rn(__fdiv_rn((float)e1, fa), __fsub_rn(g.z[1], g.z[0]), g.z[0]));
  if(!(z >= 0.0f && z < 1.0f))  // depth clip; a fragment at exactly 1.0 fails LESS against the clear
    return 0;
  const unsigned long long word = ((unsigned long long)(__float_as_uint(z) & 0x7FFFFFFFu) << 32) | ref;
  atomicMin(&a.vis[(size_t)py * (size_t)a.width + (size_t)px], word);
  return 1;
}

}  // namespace

__global__ void __launch_bounds__(256) k_mesh_clear(const MeshPassArgs a)
{
  const uint32_t n = (uint32_t)(a.row1 - a.row0) * (uint32_t)a.width;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i == 0)
  {
    MeshCounters z{};
    *a.ctr = z;
  }
  if(i < n)
    a.vis[(size_t)a.row0 * (size_t)a.width + i] = ~0ull;
}

__global__ void __launch_bounds__(256) k_mesh_setup(const MeshPassArgs a)
{
  // polygon of the clipper: [buffer][vertex][weight][lane]; touched only by lanes whose primitive crosses a clip plane
  __shared__ float poly[2][8][3][256];
  const uint32_t tid  = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t prim = blockIdx.x * 256u + tid;
  const MeshTable* __restrict__ T = a.table;

  uint32_t nSub = 0, clipBase = kMeshNone;
  Geo      g0{};  // the primitive itself when it needs no clipping
  if(prim < T->totalTris)
  {
    const MeshInstDev& I = T->inst[meshInstanceOf(T, prim)];
    if(I.visible)
    {
      const uint32_t t  = prim - I.triBegin;
      const uint32_t i0 = I.idx[3 * t], i1 = I.idx[3 * t + 1], i2 = I.idx[3 * t + 2];
      const float4   c0 = clipOf(a, worldPosOf(I, i0)), c1 = clipOf(a, worldPosOf(I, i1)), c2 = clipOf(a, worldPosOf(I, i2));
      if(finite4(c0) && finite4(c1) && finite4(c2))
      {
        bool allIn = true, reject = false;
        for(int pl = 0; pl < 5; ++pl)
        {
          const bool in0 = planeDist(pl, c0) >= 0.0f, in1 = planeDist(pl, c1) >= 0.0f, in2 = planeDist(pl, c2) >= 0.0f;
          allIn          = allIn && in0 && in1 && in2;
          reject         = reject || !(in0 || in1 || in2);
        }
        if(allIn)
        {
          if(toWindow(a, c0, g0.x[0], g0.y[0], g0.z[0], g0.invw[0]) && toWindow(a, c1, g0.x[1], g0.y[1], g0.z[1], g0.invw[1])
             && toWindow(a, c2, g0.x[2], g0.y[2], g0.z[2], g0.invw[2]))
            nSub = 1;
        }
        else if(!reject)
        {  // Sutherland-Hodgman on the weights of the three vertices, plane after plane; an intersection is always computed from the
           // inside vertex toward the outside one
          int n = 3, src = 0;
          for(int v = 0; v < 3; ++v)
            for(int k = 0; k < 3; ++k)
              poly[0][v][k][tid] = v == k ? 1.0f : 0.0f;
          for(int pl = 0; pl < 5 && n >= 3; ++pl)
          {
            const int dst = src ^ 1;
            int       m   = 0;
            for(int v = 0; v < n; ++v)
            {
              const int   w   = v + 1 == n ? 0 : v + 1;
              const float cb0 = poly[src][v][0][tid], cb1 = poly[src][v][1][tid], cb2 = poly[src][v][2][tid];
              const float nb0 = poly[src][w][0][tid], nb1 = poly[src][w][1][tid], nb2 = poly[src][w][2][tid];
              const float dc  = planeDist(pl, combine4(cb0, cb1, cb2, c0, c1, c2));
              const float dn  = planeDist(pl, combine4(nb0, nb1, nb2, c0, c1, c2));
              const bool  inC = dc >= 0.0f, inN = dn >= 0.0f;
              if(inC && m < 8)
              {
                poly[dst][m][0][tid] = cb0, poly[dst][m][1][tid] = cb1, poly[dst][m][2][tid] = cb2;
                ++m;
              }
              if(inC != inN && m < 8)
              {
                const float di = inC ? dc : dn, dOut = inC ? dn : dc;
                const float tt = di / (di - dOut);
                const float ib0 = inC ? cb0 : nb0, ib1 = inC ? cb1 : nb1, ib2 = inC ? cb2 : nb2;
                const float ob0 = inC ? nb0 : cb0, ob1 = inC ? nb1 : cb1, ob2 = inC ? nb2 : cb2;
                poly[dst][m][0][tid] = ib0 + tt * (ob0 - ib0);
                poly[dst][m][1][tid] = ib1 + tt * (ob1 - ib1);
                poly[dst][m][2][tid] = ib2 + tt * (ob2 - ib2);
                ++m;
              }
            }
            n   = m;
            src = dst;
          }
          if(n >= 3)
          {
            const uint32_t want = (uint32_t)(n - 2);
            const uint32_t base = atomicAdd(&a.ctr->clipCount, want);  // clipped primitives are few: one atomic each
            if(base + want <= a.clipCapacity)
            {
              bool ok = true;
              for(uint32_t s = 0; s < want; ++s)
              {  // fan from the polygon's first vertex
                MeshClipRec r{};
                const int   vs[3] = {0, (int)s + 1, (int)s + 2};
                for(int k = 0; k < 3; ++k)
                {
                  const float b0 = poly[src][vs[k]][0][tid], b1 = poly[src][vs[k]][1][tid], b2 = poly[src][vs[k]][2][tid];
                  r.bary[3 * k] = b0, r.bary[3 * k + 1] = b1, r.bary[3 * k + 2] = b2;
                  ok = toWindow(a, combine4(b0, b1, b2, c0, c1, c2), r.x[k], r.y[k], r.z[k], r.invw[k]) && ok;
                }
                a.clips[base + s] = r;
              }
              if(ok)
              {
                nSub     = want;
                clipBase = base;
              }
            }
            else
              atomicOr(&a.ctr->flags, 1u);
          }
        }
      }
    }
    if(nSub != 0)
    {
      MeshTriRec r{};
      for(int k = 0; k < 3; ++k)
        r.x[k] = g0.x[k], r.y[k] = g0.y[k], r.z[k] = g0.z[k], r.invw[k] = g0.invw[k];
      r.clipBase   = clipBase;
      r.nSub       = nSub;
      a.recs[prim] = r;
    }
  }

  // coverage of the (sub-)triangles: small ones here, large ones through the work list
  uint32_t fragments = 0, rasterised = 0;
  bool     overflow  = false;
  for(uint32_t s = 0; __any(s < nSub); ++s)
  {
    bool      live = s < nSub;
    Geo       g    = g0;
    long long area2 = 0, b0 = 0, b1 = 0, b2 = 0;
    int32_t   px0 = 0, px1 = -1, py0 = 0, py1 = -1;
    if(live && clipBase != kMeshNone)
    {
      const MeshClipRec& r = a.clips[clipBase + s];
      for(int k = 0; k < 3; ++k)
        g.x[k] = r.x[k], g.y[k] = r.y[k], g.z[k] = r.z[k], g.invw[k] = r.invw[k];
    }
    if(live)
    {
      bool swapped;
      area2 = orient(g, swapped);
      const int32_t minX = min(g.x[0], min(g.x[1], g.x[2])), maxX = max(g.x[0], max(g.x[1], g.x[2]));
      const int32_t minY = min(g.y[0], min(g.y[1], g.y[2])), maxY = max(g.y[0], max(g.y[1], g.y[2]));
      // pixels whose centre (p * 256 + 128) lies inside the bounding box, clamped to the handle's rows
      px0  = max((minX - 128 + 255) >> 8, 0);
      px1  = min((maxX - 128) >> 8, a.width - 1);
      py0  = max((minY - 128 + 255) >> 8, a.row0);
      py1  = min((maxY - 128) >> 8, a.row1 - 1);
      live = area2 != 0 && px0 <= px1 && py0 <= py1;
      b0   = edgeBias(g.x[1], g.y[1], g.x[2], g.y[2]);
      b1   = edgeBias(g.x[2], g.y[2], g.x[0], g.y[0]);
      b2   = edgeBias(g.x[0], g.y[0], g.x[1], g.y[1]);
    }
    if(live)
      rasterised = 1;  // once per primitive, whichever of its sub-triangles is live
    const uint32_t ref   = (prim << 3) | s;
    const bool     large = live && (px1 - px0 >= kMeshSmallBox || py1 - py0 >= kMeshSmallBox);
    // tiles are aligned to multiples of 8 pixels
    const int32_t  tx0 = px0 >> 3, ty0 = py0 >> 3;
    const uint32_t ntx = large ? (uint32_t)((px1 >> 3) - tx0 + 1) : 0u, nty = large ? (uint32_t)((py1 >> 3) - ty0 + 1) : 0u;
    const uint32_t items = large ? (ntx * nty + kMeshChunkTiles - 1) / kMeshChunkTiles : 0u;
    bool           walk  = live && !large;
    if(__any(large))
    {  // wave-wide inclusive prefix sum of the item counts, one atomic for the wave
      uint32_t scan = items;
      for(int d = 1; d < 64; d <<= 1)
      {
        const uint32_t up = __shfl_up(scan, d);
        if((int)lane >= d)
          scan += up;
      }
      const unsigned long long total = __shfl(scan, 63);
      unsigned long long       base  = 0;
      if(lane == 0)
        base = atomicAdd(&a.ctr->workCount, total);  // 64 bits, only ever added to: a claimed range stays claimed
      base = __shfl(base, 0);
      if(large)
      {  // this lane owns [at, at + items).  Every slot below the capacity is written by its owner, so k_mesh_large reads no slot
         // that nobody wrote: with the chunks when all of them fit, otherwise with kMeshNone, which the consumer skips, and the lane
         // walks its triangle itself (slow, never wrong)
        const unsigned long long at   = base + scan - items;
        const bool               fits = at + items <= a.workCapacity;
        const uint32_t           wr   = fits ? items : at < a.workCapacity ? (uint32_t)(a.workCapacity - at) : 0u;
        for(uint32_t c = 0; c < wr; ++c)
          a.work[at + c] = fits ? make_uint2(ref, c) : make_uint2(kMeshNone, 0u);
        if(!fits)
        {
          walk     = true;
          overflow = true;
        }
      }
    }
    if(walk)
      for(int32_t py = py0; py <= py1; ++py)
        for(int32_t px = px0; px <= px1; ++px)
          fragments += coverPixel(a, g, area2, b0, b1, b2, px, py, ref);
  }
  // one atomic per wave for each statistic
  for(int d = 32; d >= 1; d >>= 1)
  {
    fragments += __shfl_xor(fragments, d);
    rasterised += __shfl_xor(rasterised, d);
  }
  if(lane == 0)
  {
    if(fragments)
      atomicAdd(&a.ctr->fragments, (unsigned long long)fragments);
    if(rasterised)
      atomicAdd(&a.ctr->trisRasterised, rasterised);
  }
  if(__any(overflow) && lane == 0)
    atomicOr(&a.ctr->flags, 2u);
}

__global__ void __launch_bounds__(256) k_mesh_large(const MeshPassArgs a)
{
  const uint32_t lane   = threadIdx.x & 63u;
  const uint32_t wave   = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);
  const uint32_t nWaves = gridDim.x * 4u;
  const uint32_t count  = (uint32_t)min(a.ctr->workCount, (unsigned long long)a.workCapacity);
  uint32_t       fragments = 0;
  for(uint32_t it = wave; it < count; it += nWaves)
  {
    const uint2    w    = a.work[it];
    const uint32_t ref  = __builtin_amdgcn_readfirstlane(w.x), chunk = __builtin_amdgcn_readfirstlane(w.y);
    if(ref == kMeshNone)  // claimed by a lane whose chunks did not all fit; it walked its triangle itself
      continue;
    const uint32_t prim = ref >> 3, s = ref & 7u;
    const MeshTriRec& R = a.recs[prim];
    Geo               g;
    if(R.clipBase != kMeshNone)
    {
      const MeshClipRec& r = a.clips[R.clipBase + s];
      for(int k = 0; k < 3; ++k)
        g.x[k] = r.x[k], g.y[k] = r.y[k], g.z[k] = r.z[k], g.invw[k] = r.invw[k];
    }
    else
      for(int k = 0; k < 3; ++k)
        g.x[k] = R.x[k], g.y[k] = R.y[k], g.z[k] = R.z[k], g.invw[k] = R.invw[k];
    bool            swapped;
    const long long area2 = orient(g, swapped);
    const int32_t   minX = min(g.x[0], min(g.x[1], g.x[2])), maxX = max(g.x[0], max(g.x[1], g.x[2]));
    const int32_t   minY = min(g.y[0], min(g.y[1], g.y[2])), maxY = max(g.y[0], max(g.y[1], g.y[2]));
    const int32_t   px0 = max((minX - 128 + 255) >> 8, 0), px1 = min((maxX - 128) >> 8, a.width - 1);
    const int32_t   py0 = max((minY - 128 + 255) >> 8, a.row0), py1 = min((maxY - 128) >> 8, a.row1 - 1);
    const long long b0 = edgeBias(g.x[1], g.y[1], g.x[2], g.y[2]), b1 = edgeBias(g.x[2], g.y[2], g.x[0], g.y[0]),
                    b2 = edgeBias(g.x[0], g.y[0], g.x[1], g.y[1]);
    const int32_t  tx0 = px0 >> 3, ty0 = py0 >> 3;
    const uint32_t ntx = (uint32_t)((px1 >> 3) - tx0 + 1), nty = (uint32_t)((py1 >> 3) - ty0 + 1);
    const uint32_t tEnd = min((chunk + 1u) * kMeshChunkTiles, ntx * nty);
    for(uint32_t t = chunk * kMeshChunkTiles; t < tEnd; ++t)
    {
      const int32_t tx = tx0 + (int32_t)(t % ntx), ty = ty0 + (int32_t)(t / ntx);
      // the tile's sample centres span [X0, X1] x [Y0, Y1]; an edge whose largest value over them is negative excludes the tile
      const int32_t X0 = tx * 2048 + 128, X1 = X0 + 7 * 256, Y0 = ty * 2048 + 128, Y1 = Y0 + 7 * 256;
      bool          out = false;
      for(int e = 0; e < 3; ++e)
      {
        const int       ia = e == 0 ? 1 : e == 1 ? 2 : 0, ib = e == 0 ? 2 : e == 1 ? 0 : 1;
        const int32_t   dx = g.x[ib] - g.x[ia], dy = g.y[ib] - g.y[ia];
        const long long hi = (long long)dx * (long long)((dx > 0 ? Y1 : Y0) - g.y[ia]) - (long long)dy * (long long)((dy > 0 ? X0 : X1) - g.x[ia]);
        out = out || hi + (e == 0 ? b0 : e == 1 ? b1 : b2) < 0;
      }
      if(out)
        continue;
      const int32_t px = tx * 8 + (int32_t)(lane & 7u), py = ty * 8 + (int32_t)(lane >> 3);
      if(px >= px0 && px <= px1 && py >= py0 && py <= py1)
        fragments += coverPixel(a, g, area2, b0, b1, b2, px, py, ref);
    }
  }
  for(int d = 32; d >= 1; d >>= 1)
    fragments += __shfl_xor(fragments, d);
  if(lane == 0 && fragments)
    atomicAdd(&a.ctr->fragments, (unsigned long long)fragments);
}

__global__ void __launch_bounds__(256) k_mesh_resolve(const MeshPassArgs a)
{
  const uint32_t W = (uint32_t)a.width;
  const uint32_t n = (uint32_t)(a.row1 - a.row0) * W;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n)
    return;
  const size_t             o    = (size_t)a.row0 * W + i;
  const unsigned long long word = a.vis[o];
  if(word == ~0ull)
  {  // the clear values: depth 1.0, transparent black, no primitive
    a.outDepth[o] = 1.0f;
    a.outColor[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    a.outPrim[o]  = kMeshNone;
    return;
  }
  const uint32_t ref = (uint32_t)word, prim = ref >> 3, s = ref & 7u;
  const float4*  rp  = reinterpret_cast<const float4*>(&a.recs[prim]);
  const float4   r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
  Geo            g;
  g.x[0] = __float_as_int(r0.x), g.x[1] = __float_as_int(r0.y), g.x[2] = __float_as_int(r0.z);
  g.y[0] = __float_as_int(r0.w), g.y[1] = __float_as_int(r1.x), g.y[2] = __float_as_int(r1.y);
  g.z[0] = r1.z, g.z[1] = r1.w, g.z[2] = r2.x;
  g.invw[0] = r2.y, g.invw[1] = r2.z, g.invw[2] = r2.w;
  const uint32_t clipBase = __float_as_uint(r3.x);
  float          bary[9]  = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if(clipBase != kMeshNone)
  {
    const float4* cp = reinterpret_cast<const float4*>(&a.clips[clipBase + s]);
    const float4  c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3], c4 = cp[4], c5 = cp[5];
    g.x[0] = __float_as_int(c0.x), g.x[1] = __float_as_int(c0.y), g.x[2] = __float_as_int(c0.z);
    g.y[0] = __float_as_int(c0.w), g.y[1] = __float_as_int(c1.x), g.y[2] = __float_as_int(c1.y);
    g.z[0] = c1.z, g.z[1] = c1.w, g.z[2] = c2.x;
    g.invw[0] = c2.y, g.invw[1] = c2.z, g.invw[2] = c2.w;
    bary[0] = c3.x, bary[1] = c3.y, bary[2] = c3.z, bary[3] = c3.w, bary[4] = c4.x, bary[5] = c4.y, bary[6] = c4.z, bary[7] = c4.w, bary[8] = c5.x;
  }
  bool            swapped;
  const long long area2 = orient(g, swapped);
  if(swapped)
    for(int k = 0; k < 3; ++k)
    {
      const float t = bary[3 + k];
      bary[3 + k]   = bary[6 + k];
      bary[6 + k]   = t;
    }
  const uint32_t  py = i / W, px = i - py * W;
  const int32_t   sx = (int32_t)px * 256 + 128, sy = ((int32_t)py + a.row0) * 256 + 128;
  const float     fa = (float)area2;
  const float     e0 = (float)edgeFn(g.x[1], g.y[1], g.x[2], g.y[2], sx, sy) / fa;
  const float     e1 = (float)edgeFn(g.x[2], g.y[2], g.x[0], g.y[0], sx, sy) / fa;
  const float     e2 = (float)edgeFn(g.x[0], g.y[0], g.x[1], g.y[1], sx, sy) / fa;
  // perspective correction: weights b_i / w_i, normalised
  const float pw0 = e0 * g.invw[0], pw1 = e1 * g.invw[1], pw2 = e2 * g.invw[2];
  const float sum = (pw0 + pw1) + pw2;

  const MeshInstDev& I  = a.table->inst[meshInstanceOf(a.table, prim)];
  const uint32_t     t  = prim - I.triBegin;
  const uint32_t     i0 = I.idx[3 * t], i1 = I.idx[3 * t + 1], i2 = I.idx[3 * t + 2];
  const V3           origin = load3(a.origin);
  const V3           p0 = worldPosOf(I, i0), p1 = worldPosOf(I, i1), p2 = worldPosOf(I, i2);
  const V3           n0 = worldNrmOf(I, i0), n1 = worldNrmOf(I, i1), n2 = worldNrmOf(I, i2);
  const V3           d0 = p0 - origin, d1 = p1 - origin, d2 = p2 - origin;
  // the (sub-)triangle's vertices as combinations of the primitive's (identity weights when it was not clipped)
  V3 P[3], N[3], D[3];
  for(int k = 0; k < 3; ++k)
  {
    P[k] = combine3(bary[3 * k], bary[3 * k + 1], bary[3 * k + 2], p0, p1, p2);
    N[k] = combine3(bary[3 * k], bary[3 * k + 1], bary[3 * k + 2], n0, n1, n2);
    D[k] = combine3(bary[3 * k], bary[3 * k + 1], bary[3 * k + 2], d0, d1, d2);
  }
  const float inv      = 1.0f / sum;
  const V3    worldPos = combine3(pw0, pw1, pw2, P[0], P[1], P[2]) * inv;
  const V3    worldNrm = combine3(pw0, pw1, pw2, N[0], N[1], N[2]) * inv;  // not renormalised, as written
  const V3    viewDir  = combine3(pw0, pw1, pw2, D[0], D[1], D[2]) * inv;

  const Mat mat = material(I.mats[I.matId[t]]);
  V3 color;
  if(a.lightingMode == MGS_LIGHTING_DISABLED)
    color = (mat.emission + mat.ambient) + mat.diffuse;  // threedmesh_raster.frag.slang:100
  else
  {
    color = mat.emission;
    if(mat.needShading != 0)
    {
      const int count = a.lights ? a.lights->count : 0;
      for(int l = 0; l < count; ++l)
        shadeDirect(a.lights->lights[l], worldPos, worldNrm, mat, viewDir, color);
      if(count == 0)
        shadeDirect(headlight(a.cameraPos), worldPos, worldNrm, mat, viewDir, color);
    }
  }
  a.outDepth[o] = __uint_as_float((uint32_t)(word >> 32));
  a.outColor[o] = make_float4(color.x, color.y, color.z, 1.0f);
  a.outPrim[o]  = prim;
}

void launchMeshPass(hipStream_t stream, const MeshPassArgs& a, uint32_t totalTris, uint32_t largeBlocks)
{
  const uint32_t n = (uint32_t)(a.row1 - a.row0) * (uint32_t)a.width;
  const dim3     block(256), pixels(n ? (n + 255u) / 256u : 1u);
  hipLaunchKernelGGL(k_mesh_clear, pixels, block, 0, stream, a);
  if(totalTris != 0 && n != 0)
  {
    hipLaunchKernelGGL(k_mesh_setup, dim3((totalTris + 255u) / 256u), block, 0, stream, a);
    hipLaunchKernelGGL(k_mesh_large, dim3(largeBlocks), block, 0, stream, a);
  }
  if(n != 0)
    hipLaunchKernelGGL(k_mesh_resolve, pixels, block, 0, stream, a);
}

}  // namespace mgs
