// k_bvh.hip — the hierarchy of the traced pipeline (mgs_render_traced) for gfx950, built on the device.
//
// Replaces
//   shaders/particle_as_build.comp.slang:74-87,109-   kernelScale and the per-particle proxy the reference hands to the acceleration
//                                                     structure build (an icosahedron or a unit box instanced per particle)
//   the BLAS / TLAS builds of the acceleration-structure managers (fixed-function; no counterpart to restate)
// Structure ("Ray-traced splats"): an implicit complete 8-ary tree over leaves sorted by the 30-bit Morton code of the
// leaf centre.  No pointers, no atomics, no flags, no waiting on another workgroup: every kernel below is a plain map over its
// output, the sort in between is the library's own (key, value) sort, and the result is bit-reproducible.
#include "kernels_common.h"
#include "launchers.h"
#include "trace_common.h"

namespace mgs {

__device__ __forceinline__ uint32_t mortonSpread10(uint32_t v)
{
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// The leaf's bound in double: centre c = M p, half extent h_a = sqrt(sum_j A_aj^2) with A = mat3(M) R(q / |q|) diag(r exp(scale)), r the
// canonical radius at which the response reaches min(kernelMinResponse [/ density], 0.97f), and T_a = sum of the absolute terms of
// (M p)_a.  Every step is the fp32 inputs' exact formula evaluated in double: its error is a few 2^-53 of the terms it rounds.
__device__ __forceinline__ void leafBoundDouble(const InstanceConst& I, uint32_t li, const TraceProxy& P, float density, double (&c)[3],
                                                double (&h)[3], double (&T)[3])
{
  const float4 rq = *reinterpret_cast<const float4*>(I.rotations + 4 * (size_t)li);  // (w,x,y,z)
  const double qw = rq.x, qx = rq.y, qy = rq.z, qz = rq.w;
  const double ql = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  const double w = qw / ql, x = qx / ql, y = qy / ql, z = qz / ql;
  const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                       2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                       2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
  const double thr = fmin(P.adaptiveClamping ? (double)P.kernelMinResponse / (double)density : (double)P.kernelMinResponse, (double)0.97f);
  double       r;
  if(P.kernelDegree == 0)
    r = (1.0 - thr) / 0.329630334487;
  else
  {
    const double n = (double)P.kernelDegree;
    r = pow(log(thr) / (-4.5 / pow(3.0, n)), 1.0 / n);
  }
  double rs[3], p[3];
#pragma unroll
  for(int j = 0; j < 3; ++j)
  {
    rs[j] = r * exp((double)I.scales[3 * (size_t)li + j]);
    p[j]  = (double)I.centers[3 * (size_t)li + j];
  }
  const float* M = I.model;
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
  {
    double sum = 0.0;
#pragma unroll
    for(int j = 0; j < 3; ++j)
    {
      const double e = ((double)M[ax] * R[j] + (double)M[4 + ax] * R[3 + j] + (double)M[8 + ax] * R[6 + j]) * rs[j];
      sum += e * e;
    }
    h[ax] = sqrt(sum);
    const double t0 = (double)M[ax] * p[0], t1 = (double)M[4 + ax] * p[1], t2 = (double)M[8 + ax] * p[2], t3 = (double)M[12 + ax];
    c[ax] = t0 + t1 + t2 + t3;
    T[ax] = fabs(t0) + fabs(t1) + fabs(t2) + fabs(t3);
  }
}

// One thread per global (storage) splat: a box that contains the exact AABB of the affine image of the proxy ellipsoid.  With A =
// mat3(transform) R diag(r exp(scale)) the half extent on axis a is sqrt(sum_j A_aj^2); r is the canonical radius at which the response
// reaches the proxy threshold (trace_common.h: proxyThreshold, which the traversal tests a hit's response against).
// The box is that evaluation in double (leafBoundDouble), with h widened by 8 fp32 ulps of itself plus 2 fp32 ulps of T (the cushion
// the leaves have always had around the proxy, now around the exact one: the traversal accepts a hit on its own fp32 evaluation of
// the response, which may lie an ulp or so outside the exact ellipsoid) plus 64 * 2^-53 * (h + T), and then rounded outward to fp32:
// it contains the exact box and exceeds it by less than 8 ulps of h + 2 ulps of T + an ulp of the face's magnitude, inside the
// tests' tightness bound of 32 * 2^-24 * (h + T).  What the 64 covers: about a dozen roundings of terms no larger than h and T, and
// the one amplified error: kernelMinResponse / density rounds by 2^-53 relative, which just below the 0.97 clamp the inverse response
// amplifies by 1 / (n |ln 0.97|) = 33 / n in the radius (degree 0: 1 / (1 - 0.97) = 33), hence in h.  tests/test_hierarchy_cpu.py
// holds a float64 restatement of this path, in this order of operations, to an extended-precision reference.
// Why not fp32, as this kernel first had it (inflated by 8 ulps of h + 2 ulps of |c|): that box does not hold the exact one, and no
// count of ulps of h and T makes it.  The centre M p rounds at the magnitude of its TERMS, not of its result (x -> R (x - T0) with
// |T0| ~ 1e3 and centres near T0: |c| ~ 1, error up to 9e-5, and a half extent of 1e-5 leaves the box beside its own splat); the
// rotation matrix's entries carry an absolute error of an ulp of 1, which on an axis almost orthogonal to a long axis of a splat with
// 1e4 between its scales is more than 1e3 ulps of that axis' half extent, in either direction (too small for containment or too
// large for the tightness bound; both were seen on the device); kernelMinResponse / density just below the clamp rounds by a
// quarter ulp of 1, amplified as above to 8 / n ulps of the radius; and the squares of its terms overflow for half extents above
// about 1.8e19.  The build runs once per change of the scene, one thread per splat: double costs it little.
// The Morton key is still taken from the fp32 centre: the order of the leaves is what it was.
// No leaf: density <= alphaCullThreshold (particleProcessHit rejects every hit, threedgrt.h.slang:166-170), or a bound that is not
// finite in fp32 (a NaN anywhere, |c| + h above FLT_MAX).
__global__ __launch_bounds__(256) void k_bvh_leaves(BvhBuildArgs a)
{
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if(g >= a.totalSplats)
    return;
  const FrameArgs* Ap = a.frame;
  int              k  = 0;
  for(int i = 1; i < Ap->f.nInstances; ++i)  // bound: kMaxInstances
    if(g >= Ap->inst[i].globalOffset)
      k = i;
  const InstanceConst& I  = Ap->inst[k];
  const uint32_t       li = g - I.globalOffset;
  const float          density = I.alpha[li];
  const float*         M = I.model;
  const float          p[3] = {I.centers[3 * (size_t)li], I.centers[3 * (size_t)li + 1], I.centers[3 * (size_t)li + 2]};
  double               cd[3], hd[3], Td[3];
  leafBoundDouble(I, li, a.proxy, density, cd, hd, Td);
  bool   ok = density > a.proxy.alphaCull;
  float4 lo, hi;
  float  q[3];
#pragma unroll
  for(int ax = 0; ax < 3; ++ax)
  {
    const double ulp = 1.1920928955078125e-7;  // 2^-23
    const double hh = hd[ax] * (1.0 + 8.0 * ulp) + Td[ax] * (2.0 * ulp) + 64.0 * 1.1102230246251565e-16 * (hd[ax] + Td[ax]);
    const double xl = cd[ax] - hh, xu = cd[ax] + hh;
    float        l = (float)xl, u = (float)xu;
    if((double)l > xl)
      l = nextafterf(l, -INFINITY);
    if((double)u < xu)
      u = nextafterf(u, INFINITY);
    ok = ok && isfinite(l) && isfinite(u) && hd[ax] >= 0.0;
    (&lo.x)[ax] = l;
    (&hi.x)[ax] = u;
    const float c = M[ax] * p[0] + M[4 + ax] * p[1] + M[8 + ax] * p[2] + M[12 + ax];
    q[ax]         = fminf(fmaxf((c - a.sceneLo[ax]) * a.sceneInvExt[ax], 0.0f), 1.0f) * 1023.0f;
  }
  lo.w = __uint_as_float(g);
  hi.w = 0.0f;
  uint32_t key = kTraceInvalid;
  if(ok)
    key = mortonSpread10((uint32_t)q[0]) | (mortonSpread10((uint32_t)q[1]) << 1) | (mortonSpread10((uint32_t)q[2]) << 2);
  a.keys[g]            = key;
  a.vals[g]            = g;
  a.leafBox[2 * (size_t)g]     = lo;
  a.leafBox[2 * (size_t)g + 1] = hi;
}

// the number of valid leaves = the position of the first invalid key in the sorted array (Morton codes have 30 bits, the invalid
// key is all ones): exactly one thread finds the boundary.  *countOut is zeroed by the caller (all keys invalid: stays 0).
__global__ __launch_bounds__(256) void k_bvh_count(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ countOut)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n || keys[i] == kTraceInvalid)
    return;
  if(i + 1u == n || keys[i + 1u] == kTraceInvalid)
    *countOut = i + 1u;
}

__global__ __launch_bounds__(256) void k_bvh_gather(const uint32_t* __restrict__ vals, const float4* __restrict__ leafBox,
                                                    float4* __restrict__ level0, uint32_t nLeaves)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= nLeaves)
    return;
  const uint32_t g = vals[i];
  level0[2 * (size_t)i]     = leafBox[2 * (size_t)g];
  level0[2 * (size_t)i + 1] = leafBox[2 * (size_t)g + 1];
}

// node i of this level = the union of the children [8i, 8i + 8) of the level below (min / max: exact, no rounding)
__global__ __launch_bounds__(256) void k_bvh_level(const float4* __restrict__ below, uint32_t nBelow, float4* __restrict__ level,
                                                   uint32_t nLevel)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= nLevel)
    return;
  const uint32_t c0 = 8u * i, c1 = min(c0 + 8u, nBelow);
  float4         lo = below[2 * (size_t)c0], hi = below[2 * (size_t)c0 + 1];
  for(uint32_t c = c0 + 1u; c < c1; ++c)  // bound: 8 children
  {
    const float4 l = below[2 * (size_t)c], u = below[2 * (size_t)c + 1];
    lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z);
    hi.x = fmaxf(hi.x, u.x); hi.y = fmaxf(hi.y, u.y); hi.z = fmaxf(hi.z, u.z);
  }
  lo.w = 0.0f;
  hi.w = 0.0f;
  level[2 * (size_t)i]     = lo;
  level[2 * (size_t)i + 1] = hi;
}

void launchBvhLeaves(hipStream_t stream, const BvhBuildArgs& a)
{
  if(a.totalSplats)
    hipLaunchKernelGGL(k_bvh_leaves, dim3((a.totalSplats + 255u) / 256u), dim3(256), 0, stream, a);
}
void launchBvhCount(hipStream_t stream, const uint32_t* sortedKeys, uint32_t n, uint32_t* countOut)
{
  if(n)
    hipLaunchKernelGGL(k_bvh_count, dim3((n + 255u) / 256u), dim3(256), 0, stream, sortedKeys, n, countOut);
}
void launchBvhGather(hipStream_t stream, const uint32_t* sortedVals, const float4* leafBox, float4* level0, uint32_t nLeaves)
{
  if(nLeaves)
    hipLaunchKernelGGL(k_bvh_gather, dim3((nLeaves + 255u) / 256u), dim3(256), 0, stream, sortedVals, leafBox, level0, nLeaves);
}
void launchBvhLevel(hipStream_t stream, const float4* below, uint32_t nBelow, float4* level, uint32_t nLevel)
{
  if(nLevel)
    hipLaunchKernelGGL(k_bvh_level, dim3((nLevel + 255u) / 256u), dim3(256), 0, stream, below, nBelow, level, nLevel);
}

}  // namespace mgs
