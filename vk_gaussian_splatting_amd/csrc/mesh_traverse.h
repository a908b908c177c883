// mesh_traverse.h — what every ray against the scene's triangle meshes does alike, a caller's (k_mesh_rays.hip) or a traced frame's
// (k_trace_mesh.hip, k_trace_light.hip): the ray's shear, the watertight ray/triangle test, the closest-hit and the occlusion walk
// over the triangle hierarchy, and the hit's world position and normal.
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:495-553     traceBounceRayMeshes: the closest mesh hit of a ray
//   shaders/threedgrt_raytrace.rchit.slang:31-67      the closest-hit shader: barycentrics, world position, world normal, ids
//   shaders/threedgrt_raytrace.rgen.slang:1295-1341   traceShadowRayMesh: is anything hit in the window
// and the fixed-function ray/triangle test behind them.
// The walk is traverseProxies of trace_traverse.h as it stands (slabHit, one LDS word per level, nearest children first, a cut the
// candidate lowers).  Bounded: the traversal by 2 * nodes + 2 steps, children by 8.  Nothing waits on another lane, wave or
// workgroup.  Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include "kernels_common.h"
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

// what a walk leaves: t = +inf is a miss; the occlusion walk sets t alone
struct MeshBest
{
  float    t = __builtin_huge_valf(), b1 = 0.0f, b2 = 0.0f;
  uint32_t prim = kTraceInvalid, inst = kTraceInvalid, mat = kTraceInvalid;
};

// The ray against the triangle hierarchy `a` (its nodes, levels and node count; S holds that hierarchy's levels) inside the open
// window (tMin, tMax).  MODE 0: the closest hit, ties in t to the lower global primitive id; MODE 1: occlusion (the walk's cut
// drops below every entry distance at the first hit, so nothing more is opened).  The caller checks a.nLevels > 0 and the ray.
template <int MODE>
__device__ __forceinline__ MeshBest meshWalk(const TraceArgs& a, TraceLds& S, int tid, const float4* tris, const MeshTable* table, const TraceRay& ray,
                                             float tMin, float tMax, unsigned long long& nodeVisits, unsigned long long& triTests)
{
  MeshBest       best;
  float          cut = tMax;
  const RayShear sh  = rayShear(ray);
  auto candidate = [&](uint32_t leaf) {
    const float4   p0 = tris[3 * (size_t)leaf], p1 = tris[3 * (size_t)leaf + 1], p2 = tris[3 * (size_t)leaf + 2];
    const uint32_t inst = __float_as_uint(p1.w);
    if(table->inst[inst].visible == 0u)  // visibility is the device table's word, read per candidate: toggling it rebuilds nothing
      return;
    ++triTests;
    float t, b1, b2;
    if(!triangleHit(ray, sh, p0, p1, p2, t, b1, b2) || !(t > tMin && t < tMax))
      return;
    if(MODE == 1)
    {
      best.t = t;
      cut    = -1.0f;
      return;
    }
    const uint32_t prim = __float_as_uint(p0.w);
    if(t < best.t || (t == best.t && prim < best.prim))  // ties in t: the lower global primitive id
    {
      best.t    = t;
      best.b1   = b1;
      best.b2   = b2;
      best.prim = prim;
      best.inst = inst;
      best.mat  = __float_as_uint(p2.w);
      cut       = t;  // a node AT the cut is still visited (te <= cut), so a tie is seen whatever the order of traversal
    }
  };
  traverseProxies(a, S, tid, ray, tMin, tMax, cut, candidate, nodeVisits);
  return best;
}

// the hit record's three float4 of a closest hit (rchit.slang:50-59): (t, instance, primitive, material), (world position, b1),
// (world normal, b2)
__device__ __forceinline__ void meshHitRecord(const MeshTable* table, const MeshBest& best, float4& h0, float4& h1, float4& h2)
{
  const MeshInstDev& I  = table->inst[best.inst];
  const uint32_t     lt = best.prim - I.triBegin;
  const uint32_t     i0 = I.idx[3 * (size_t)lt], i1 = I.idx[3 * (size_t)lt + 1], i2 = I.idx[3 * (size_t)lt + 2];
  const float        b0 = 1.0f - best.b1 - best.b2;  // rchit.slang:50-51
  float              pl[3], nl[3];
#pragma unroll
  for(int c = 0; c < 3; ++c)
  {  // :54, :58: v0 * b.x + v1 * b.y + v2 * b.z
    pl[c] = I.pos[3 * (size_t)i0 + c] * b0 + I.pos[3 * (size_t)i1 + c] * best.b1 + I.pos[3 * (size_t)i2 + c] * best.b2;
    nl[c] = I.nrm[3 * (size_t)i0 + c] * b0 + I.nrm[3 * (size_t)i1 + c] * best.b1 + I.nrm[3 * (size_t)i2 + c] * best.b2;
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
  h0 = make_float4(best.t, __uint_as_float(best.inst), __uint_as_float(best.prim), __uint_as_float(best.mat));
  h1 = make_float4(pw[0], pw[1], pw[2], best.b1);
  h2 = make_float4(nw[0] * nlen, nw[1] * nlen, nw[2] * nlen, best.b2);
}

// a miss's first float4; the other two are 0
__device__ __forceinline__ float4 meshMissRecord()
{
  return make_float4(__builtin_huge_valf(), __uint_as_float(kTraceInvalid), __uint_as_float(kTraceInvalid), __uint_as_float(kTraceInvalid));
}

}  // namespace

}  // namespace mgs
