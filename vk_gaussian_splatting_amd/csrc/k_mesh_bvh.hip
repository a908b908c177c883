// k_mesh_bvh.hip — the triangle hierarchy of the mesh ray queries (mgs_trace_mesh_rays) for gfx950, built on the device.
//
// Replaces the mesh BLAS / TLAS builds of MeshManagerVk (src/mesh_manager_vk.cpp; fixed-function, no counterpart to restate).
// Structure ("Mesh ray queries"): the implicit complete 8-ary tree of k_bvh.hip over one leaf per valid triangle of every
// mesh instance, in world space, sorted by the 30-bit Morton code of the leaf centroid.  The two kernels below are plain maps over
// their output; the sort in between is the library's own (key, value) sort and count, gather and the upper levels are k_bvh.hip's
// kernels through their launchers.  No pointers, no atomics, no waiting on another workgroup: the result is bit-reproducible.
#include "kernels_common.h"
#include "launchers.h"

namespace mgs {

namespace {

__device__ __forceinline__ uint32_t meshMortonSpread10(uint32_t v)
{
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// the instance that owns a global primitive index: the last one whose first primitive is not above it (k_mesh.hip's rule)
__device__ __forceinline__ int instanceOfPrim(const MeshTable* __restrict__ T, uint32_t prim)
{
  int lo = 0, hi = (int)T->count;
  while(hi - lo > 1)  // bound: log2(kMaxMeshInstances) steps
  {
    const int mid = (lo + hi) >> 1;
    if(T->inst[mid].triBegin <= prim)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// worldPos = M p as the mesh pass's vertex stage writes it (k_mesh.hip: mulMat with w = 1): ((x m0 + y m4) + z m8) + m12, every
// product and sum rounded where it stands.  Contraction is off so that the leaf kernel and the record kernel, which both call this,
// give a vertex the same bits whatever code surrounds the call: the leaf's box then bounds exactly the triangle the traversal tests.
__device__ __forceinline__ void worldVertex(const MeshInstDev& I, uint32_t vi, float (&w)[3])
{
#pragma clang fp contract(off)
  const float x = I.pos[3 * (size_t)vi], y = I.pos[3 * (size_t)vi + 1], z = I.pos[3 * (size_t)vi + 2];
  const float* m = I.M;
#pragma unroll
  for(int r = 0; r < 3; ++r)
    w[r] = ((x * m[r] + y * m[4 + r]) + z * m[8 + r]) + m[12 + r];
}

struct WorldTri
{
  float    v[3][3];
  uint32_t inst, mat;
};
__device__ __forceinline__ WorldTri worldTriangle(const MeshTable* __restrict__ T, uint32_t g)
{
  WorldTri           W;
  const int          k  = instanceOfPrim(T, g);
  const MeshInstDev& I  = T->inst[k];
  const uint32_t     lt = g - I.triBegin;
#pragma unroll
  for(int c = 0; c < 3; ++c)
    worldVertex(I, I.idx[3 * (size_t)lt + c], W.v[c]);
  W.inst = (uint32_t)k;
  W.mat  = I.matId[lt];
  return W;
}

}  // namespace

// One thread per global primitive (instances concatenated in creation order, visible or not: the id mgs_meshes_download(which = 2)
// reports).  The leaf box is the min / max of the three world vertices, inflated on every axis by 4 ulps of the box's extent plus
// 2 ulps of the bound's magnitude plus 1e-37.  What the inflation is for, and what it is not:
//  - The box without inflation already holds the triangle exactly (the records carry the same vertex bits), so in real arithmetic
//    the ray's parameter at a hit point lies between the box's entry and exit on every axis.  slabHit computes each slab value as
//    (bound - o) * (1 / d): three roundings, a relative error below 1.5 ulps of the value, and it widens entry and exit by 4 ulps, so
//    rounding in the node test alone never refuses the leaf of a true hit.
//  - An axis-parallel triangle has a box of zero thickness, and a ray whose origin lies in that plane gets (bound - o) = 0 against an
//    infinite 1 / d there: 0 * inf, which slabHit drops as NaN.  The magnitude term keeps the two bounds apart, so the slab stays an
//    interval of two signed infinities; the extent term adds slack in proportion to the triangle's size.  In a coordinate plane
//    through 0 the magnitude is 0 too: a third, absolute term of 1e-37 (a normal float, lost in the sum wherever another term is not
//    0) keeps the box strictly around its triangle there as well (tests/test_gpu_hierarchy.py asserts the strict containment).
//  - It is NOT a bound on the triangle test's own t.  t = T / det loses accuracy as det goes to 0 (a ray grazing the triangle's
//    plane), by more than any fixed number of ulps, and the walk compares the leaf's entry with the window and with the cut.  A
//    grazing hit whose computed t falls inside the window while the box's entry does not is refused by the leaf: a miss in place of
//    a hit with a meaningless t, the same on every run and in every order of traversal.  Such rays have float64 barycentrics or t at
//    the fragile margins of the tests.  tests/np_mesh_rays.py runs slabHit in fp32 on the leaf of every hit its restatement accepts
//    (window, and the hit's t as the cut); on the committed cases none is refused.
// No leaf: a non-finite vertex, or zero area in float (the cross product of the two edge vectors is exactly 0 in all three
// components).
__global__ __launch_bounds__(256) void k_mesh_bvh_leaves(MeshBvhBuildArgs a)
{
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if(g >= a.totalTris)
    return;
  const WorldTri W = worldTriangle(a.table, g);
  bool           ok = true;
  float4         lo, hi;
  float          q[3], e1[3], e2[3];
  constexpr float ulp = 1.1920929e-7f, tiny = 1e-37f;
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
  {
    const float x0 = W.v[0][ax], x1 = W.v[1][ax], x2 = W.v[2][ax];
    ok = ok && isfinite(x0) && isfinite(x1) && isfinite(x2);
    const float l = fminf(fminf(x0, x1), x2), u = fmaxf(fmaxf(x0, x1), x2);
    const float ext = u - l;
    const float li = l - (ext * (4.0f * ulp) + fabsf(l) * (2.0f * ulp) + tiny), ui = u + (ext * (4.0f * ulp) + fabsf(u) * (2.0f * ulp) + tiny);
    ok = ok && isfinite(li) && isfinite(ui);
    (&lo.x)[ax] = li;
    (&hi.x)[ax] = ui;
    const float c = (x0 + x1 + x2) * (1.0f / 3.0f);
    q[ax]  = fminf(fmaxf((c - a.boxLo[ax]) * a.boxInvExt[ax], 0.0f), 1.0f) * 1023.0f;
    e1[ax] = x1 - x0;
    e2[ax] = x2 - x0;
  }
  {
#pragma clang fp contract(off)
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    ok = ok && !(cx == 0.0f && cy == 0.0f && cz == 0.0f) && isfinite(cx) && isfinite(cy) && isfinite(cz);
  }
  lo.w = __uint_as_float(g);
  hi.w = 0.0f;
  uint32_t key = kTraceInvalid;
  if(ok)
    key = meshMortonSpread10((uint32_t)q[0]) | (meshMortonSpread10((uint32_t)q[1]) << 1) | (meshMortonSpread10((uint32_t)q[2]) << 2);
  a.keys[g]                    = key;
  a.vals[g]                    = g;
  a.leafBox[2 * (size_t)g]     = lo;
  a.leafBox[2 * (size_t)g + 1] = hi;
}

// One thread per leaf, behind the sort and the gather: the triangle's record in leaf order, so that a traversal reads contiguous
// memory, and the leaf's own index into lo.w of its node (the gather left the global primitive id there).
__global__ __launch_bounds__(256) void k_mesh_bvh_records(MeshBvhRecordArgs a)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= a.leaves)
    return;
  const uint32_t g = a.sortedVals[i];
  const WorldTri W = worldTriangle(a.table, g);
  a.tris[3 * (size_t)i]     = make_float4(W.v[0][0], W.v[0][1], W.v[0][2], __uint_as_float(g));
  a.tris[3 * (size_t)i + 1] = make_float4(W.v[1][0], W.v[1][1], W.v[1][2], __uint_as_float(W.inst));
  a.tris[3 * (size_t)i + 2] = make_float4(W.v[2][0], W.v[2][1], W.v[2][2], __uint_as_float(W.mat));
  float4 lo = a.level0[2 * (size_t)i];
  lo.w      = __uint_as_float(i);
  a.level0[2 * (size_t)i] = lo;
}

void launchMeshBvhLeaves(hipStream_t stream, const MeshBvhBuildArgs& a)
{
  if(a.totalTris)
    hipLaunchKernelGGL(k_mesh_bvh_leaves, dim3((a.totalTris + 255u) / 256u), dim3(256), 0, stream, a);
}
void launchMeshBvhRecords(hipStream_t stream, const MeshBvhRecordArgs& a)
{
  if(a.leaves)
    hipLaunchKernelGGL(k_mesh_bvh_records, dim3((a.leaves + 255u) / 256u), dim3(256), 0, stream, a);
}

}  // namespace mgs
