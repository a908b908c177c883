// k_mesh_rays.hip — mesh ray queries (mgs_trace_mesh_rays, mgs_trace_mesh_rays_device) for gfx950: the caller's rays against the
// scene's triangle meshes, closest hit or occlusion.
//
// Replaces, for rays the caller supplies,
//   shaders/threedgrt_raytrace.rgen.slang:495-553     traceBounceRayMeshes: the closest mesh hit of a ray
//   shaders/threedgrt_raytrace.rchit.slang:31-67      the closest-hit shader: barycentrics, world position, world normal, ids
//   shaders/threedgrt_raytrace.rgen.slang:1295-1341   traceShadowRayMesh: is anything hit in the window
// and the fixed-function ray/triangle test behind them.
// Structure: one ray per lane, 256 lanes per workgroup; lane i of workgroup b takes ray perm[b * 256 + i], or b * 256 + i in the
// caller's order.  The walk is traverseProxies of trace_traverse.h as it stands (slabHit, one LDS word per level, nearest children
// first, a cut the candidate lowers); the existing kernels are not routed through anything new.  Every loop is bounded: the
// traversal by 2 * nodes + 2 steps, children by 8.  Nothing waits on another lane, wave or workgroup, and no lane returns early.
#include "kernels_common.h"
#include "launchers.h"
#include "trace_common.h"
#include "trace_traverse.h"

namespace mgs {

namespace {

// The ray's shear (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013): kz = the direction's largest component,
// kx, ky the other two in an order that keeps the winding, S = (d_kx / d_kz, d_ky / d_kz, 1 / d_kz).
struct RayShear
{
  int   kx, ky, kz;
  float sx, sy, sz;
};
__device__ __forceinline__ RayShear rayShear(const TraceRay& r)
{
  RayShear    s;
  const float ax = fabsf(r.d[0]), ay = fabsf(r.d[1]), az = fabsf(r.d[2]);
  s.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  s.kx = s.kz == 2 ? 0 : s.kz + 1;
  s.ky = s.kx == 2 ? 0 : s.kx + 1;
  const float dz = s.kz == 0 ? r.d[0] : (s.kz == 1 ? r.d[1] : r.d[2]);
  if(dz < 0.0f)
  {
    const int t = s.kx;
    s.kx = s.ky;
    s.ky = t;
  }
  const float dx = s.kx == 0 ? r.d[0] : (s.kx == 1 ? r.d[1] : r.d[2]);
  const float dy = s.ky == 0 ? r.d[0] : (s.ky == 1 ? r.d[1] : r.d[2]);
  s.sx = dx / dz;
  s.sy = dy / dz;
  s.sz = 1.0f / dz;
  return s;
}

__device__ __forceinline__ float pick3(const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// One triangle against the ray, both facings.  The vertices are moved to the ray's origin and sheared into ray space; the three
// edge functions come from the sheared x and y alone.  Every product and difference is an explicit __fmul_rn / __fsub_rn: hipcc
// contracts a * b - c * d into fma(a, b, -(c * d)) by default, which rounds the two products differently, and the edge two triangles
// share would then no longer get the same magnitude with the opposite sign from both — a ray could slip between them.  As written,
// the edge (P, Q) gives fl(fl(Px Qy) - fl(Py Qx)) in one triangle and exactly its negative in the other, and a sheared vertex
// depends on the vertex and the ray alone.  Edges are inclusive (all three >= 0 or all three <= 0); when any of them is exactly 0 the
// three are recomputed in double, where the products of floats are exact and the sign of the difference is the true one.
// Returns t = T / det (no window test), the barycentrics of v1 and v2 (rchit.slang:50-51) in b1, b2.
__device__ __forceinline__ bool triangleHit(const TraceRay& ray, const RayShear& s, const float4& p0, const float4& p1, const float4& p2, float& t,
                                            float& b1, float& b2)
{
  const float okx = s.kx == 0 ? ray.o[0] : (s.kx == 1 ? ray.o[1] : ray.o[2]);
  const float oky = s.ky == 0 ? ray.o[0] : (s.ky == 1 ? ray.o[1] : ray.o[2]);
  const float okz = s.kz == 0 ? ray.o[0] : (s.kz == 1 ? ray.o[1] : ray.o[2]);
  const float az = __fsub_rn(pick3(p0, s.kz), okz), bz = __fsub_rn(pick3(p1, s.kz), okz), cz = __fsub_rn(pick3(p2, s.kz), okz);
  const float ax = __fsub_rn(__fsub_rn(pick3(p0, s.kx), okx), __fmul_rn(s.sx, az)), ay = __fsub_rn(__fsub_rn(pick3(p0, s.ky), oky), __fmul_rn(s.sy, az));
  const float bx = __fsub_rn(__fsub_rn(pick3(p1, s.kx), okx), __fmul_rn(s.sx, bz)), by = __fsub_rn(__fsub_rn(pick3(p1, s.ky), oky), __fmul_rn(s.sy, bz));
  const float cx = __fsub_rn(__fsub_rn(pick3(p2, s.kx), okx), __fmul_rn(s.sx, cz)), cy = __fsub_rn(__fsub_rn(pick3(p2, s.ky), oky), __fmul_rn(s.sy, cz));
  float u = __fsub_rn(__fmul_rn(cx, by), __fmul_rn(cy, bx));
  float v = __fsub_rn(__fmul_rn(ax, cy), __fmul_rn(ay, cx));
  float w = __fsub_rn(__fmul_rn(bx, ay), __fmul_rn(by, ax));
  if(u == 0.0f || v == 0.0f || w == 0.0f)
  {
    const double du = __dsub_rn(__dmul_rn((double)cx, (double)by), __dmul_rn((double)cy, (double)bx));
    const double dv = __dsub_rn(__dmul_rn((double)ax, (double)cy), __dmul_rn((double)ay, (double)cx));
    const double dw = __dsub_rn(__dmul_rn((double)bx, (double)ay), __dmul_rn((double)by, (double)ax));
    u = (float)du;
    v = (float)dv;
    w = (float)dw;
    if((du < 0.0 || dv < 0.0 || dw < 0.0) && (du > 0.0 || dv > 0.0 || dw > 0.0))
      return false;
  }
  else if((u < 0.0f || v < 0.0f || w < 0.0f) && (u > 0.0f || v > 0.0f || w > 0.0f))
    return false;
  const float det = __fadd_rn(__fadd_rn(u, v), w);
  if(det == 0.0f)
    return false;
  const float tz = __fmul_rn(s.sz, az), uz = __fmul_rn(s.sz, bz), vz = __fmul_rn(s.sz, cz);
  const float T  = __fadd_rn(__fadd_rn(__fmul_rn(u, tz), __fmul_rn(v, uz)), __fmul_rn(w, vz));
  t  = T / det;
  b1 = v / det;
  b2 = w / det;
  return true;
}

}  // namespace

// MODE 0: closest hit (t, ids, barycentrics, world position and normal); MODE 1: occlusion (the hit flag alone; the walk's cut drops
// below every entry distance at the first hit, so nothing more is opened)
template <int MODE>
__global__ __launch_bounds__(256) void k_mesh_rays(MeshRayArgs q)
{
  __shared__ TraceLds S;
  const TraceArgs&    a   = q.t;
  const int           tid = threadIdx.x;
  traceLdsInit(S, a, tid);
  const uint32_t slot = blockIdx.x * 256u + (uint32_t)tid;
  const bool     live = slot < q.count;
  const uint32_t idx  = live ? (q.perm ? q.perm[slot] : slot) : 0u;
  const bool     inRange = live && idx < q.count;  // (a permutation is the library's own; the bound keeps a stray index inside the arrays)
  float4         ro = make_float4(0.f, 0.f, 0.f, 1.f), rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if(inRange)
  {
    ro = q.rays[2 * (size_t)idx];
    rd = q.rays[2 * (size_t)idx + 1];
  }
  const bool rayOk = inRange && rayValid(ro, rd);
  TraceRay   ray;
  ray.o[0] = ro.x; ray.o[1] = ro.y; ray.o[2] = ro.z;
  ray.d[0] = rd.x; ray.d[1] = rd.y; ray.d[2] = rd.z;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    ray.inv[c] = 1.0f / ray.d[c];
  const float INF  = __builtin_huge_valf();
  const float tMin = fmaxf(ro.w, 0.0f), tMax = rd.w;  // the window (tMin, tMax), both ends open

  float    cut = tMax, bestT = INF, bestB1 = 0.0f, bestB2 = 0.0f;
  uint32_t bestPrim = kTraceInvalid, bestInst = kTraceInvalid, bestMat = kTraceInvalid;
  unsigned long long nodeVisits = 0, triTests = 0;

  if(rayOk && a.nLevels > 0)
  {
    const RayShear sh = rayShear(ray);
    auto candidate = [&](uint32_t leaf) {
      const float4   p0 = q.tris[3 * (size_t)leaf], p1 = q.tris[3 * (size_t)leaf + 1], p2 = q.tris[3 * (size_t)leaf + 2];
      const uint32_t inst = __float_as_uint(p1.w);
      if(q.table->inst[inst].visible == 0u)  // visibility is the device table's word, read per candidate: toggling it rebuilds nothing
        return;
      ++triTests;
      float t, b1, b2;
      if(!triangleHit(ray, sh, p0, p1, p2, t, b1, b2) || !(t > tMin && t < tMax))
        return;
      if(MODE == 1)
      {
        bestT = t;
        cut   = -1.0f;
        return;
      }
      const uint32_t prim = __float_as_uint(p0.w);
      if(t < bestT || (t == bestT && prim < bestPrim))  // ties in t: the lower global primitive id
      {
        bestT    = t;
        bestB1   = b1;
        bestB2   = b2;
        bestPrim = prim;
        bestInst = inst;
        bestMat  = __float_as_uint(p2.w);
        cut      = t;  // a node AT the cut is still visited (te <= cut), so a tie is seen whatever the order of traversal
      }
    };
    traverseProxies(a, S, tid, ray, tMin, tMax, cut, candidate, nodeVisits);
  }

  if(inRange)
  {
    const bool hit = bestT < INF;
    float4     h0 = make_float4(INF, __uint_as_float(kTraceInvalid), __uint_as_float(kTraceInvalid), __uint_as_float(kTraceInvalid));
    float4     h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2 = h1;
    if(MODE == 0 && hit)
    {
      const MeshInstDev& I  = q.table->inst[bestInst];
      const uint32_t     lt = bestPrim - I.triBegin;
      const uint32_t     i0 = I.idx[3 * (size_t)lt], i1 = I.idx[3 * (size_t)lt + 1], i2 = I.idx[3 * (size_t)lt + 2];
      const float        b0 = 1.0f - bestB1 - bestB2;  // rchit.slang:50-51
      float              pl[3], nl[3];
#pragma unroll
      for(int c = 0; c < 3; ++c)
      {  // :54, :58: v0 * b.x + v1 * b.y + v2 * b.z
        pl[c] = I.pos[3 * (size_t)i0 + c] * b0 + I.pos[3 * (size_t)i1 + c] * bestB1 + I.pos[3 * (size_t)i2 + c] * bestB2;
        nl[c] = I.nrm[3 * (size_t)i0 + c] * b0 + I.nrm[3 * (size_t)i1 + c] * bestB1 + I.nrm[3 * (size_t)i2 + c] * bestB2;
      }
      const float* M = I.M;
      const float* r = I.rsInv;  // transformRotScaleInverse, glm column-major: transpose(r) n is the mesh pass's worldNrm
      float        pw[3], nw[3];
#pragma unroll
      for(int c = 0; c < 3; ++c)
      {
        pw[c] = ((pl[0] * M[c] + pl[1] * M[4 + c]) + pl[2] * M[8 + c]) + M[12 + c];  // :55 ObjectToWorld
        nw[c] = (nl[0] * r[3 * c] + nl[1] * r[3 * c + 1]) + nl[2] * r[3 * c + 2];     // :59 WorldToObject, transposed
      }
      const float nlen = rsqrtf(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]);
      h0 = make_float4(bestT, __uint_as_float(bestInst), __uint_as_float(bestPrim), __uint_as_float(bestMat));
      h1 = make_float4(pw[0], pw[1], pw[2], bestB1);
      h2 = make_float4(nw[0] * nlen, nw[1] * nlen, nw[2] * nlen, bestB2);
    }
    float4* H = q.hits + 4 * (size_t)idx;
    H[0] = h0;
    H[1] = h1;
    H[2] = h2;
    H[3] = make_float4(__uint_as_float(hit ? 1u : 0u), 0.f, 0.f, 0.f);
    // statistics: integer sums, so the totals do not depend on the order of arrival
    if(rayOk)
    {
      atomicAdd(&q.ctr->nodeVisits, nodeVisits);
      atomicAdd(&q.ctr->triangleTests, triTests);
      if(hit)
        atomicAdd(&q.ctr->hits, 1ull);
    }
    else
      atomicAdd(&q.ctr->invalidRays, 1u);
  }
}

void launchMeshRays(hipStream_t stream, const MeshRayArgs& a, int mode)
{
  if(a.count == 0)
    return;
  const uint32_t groups = (a.count + 255u) / 256u;
  if(mode == 1)
    hipLaunchKernelGGL(k_mesh_rays<1>, dim3(groups), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(k_mesh_rays<0>, dim3(groups), dim3(256), 0, stream, a);
}

}  // namespace mgs
