// trace_common.h — what the hierarchy build (k_bvh.hip) and the traversal (k_trace.hip) must compute alike: the particle as the
// 3DGRT shaders fetch it and the proxy ellipsoid's threshold (its radius is the build's alone, in double: k_bvh.hip; the response itself: kernelResponse,
// gut_common.h, shared with the 3DGUT compositor); and what the ray and shadow queries must refuse alike (rayValid).
#pragma once
#include "gut_common.h"
#include "kernels_common.h"

namespace mgs {

// ThreedgrtParticle (threedgrt.h.slang:42-48): centre, exp(scale), rotation of the normalised quaternion.  R is the rotation matrix
// in row-major order (quatToMat3Transpose read as rows, quaternions.h.slang:56-73): canonical = diag(1/s) R^T (x - p).
__device__ __forceinline__ void loadParticle(const InstanceConst& I, uint32_t li, float (&R)[9], float (&s)[3], float (&p)[3])
{
  p[0] = I.centers[3 * (size_t)li];
  p[1] = I.centers[3 * (size_t)li + 1];
  p[2] = I.centers[3 * (size_t)li + 2];
  s[0] = expf(I.scales[3 * (size_t)li]);
  s[1] = expf(I.scales[3 * (size_t)li + 1]);
  s[2] = expf(I.scales[3 * (size_t)li + 2]);
  const float4 rq = *reinterpret_cast<const float4*>(I.rotations + 4 * (size_t)li);  // (w,x,y,z)
  const float  ql = sqrtf(rq.x * rq.x + rq.y * rq.y + rq.z * rq.z + rq.w * rq.w);
  const float  w = rq.x / ql, x = rq.y / ql, y = rq.z / ql, z = rq.w / ql;
  const float  xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0f - 2.0f * (yy + zz); R[1] = 2.0f * (xy - wz);        R[2] = 2.0f * (xz + wy);
  R[3] = 2.0f * (xy + wz);        R[4] = 1.0f - 2.0f * (xx + zz); R[5] = 2.0f * (yz - wx);
  R[6] = 2.0f * (xz - wy);        R[7] = 2.0f * (yz + wx);        R[8] = 1.0f - 2.0f * (xx + yy);
}

// the response the proxy ellipsoid is circumscribed around (kernelScale, particle_as_build.comp.slang:74-78)
__device__ __forceinline__ float proxyThreshold(const TraceProxy& P, float density)
{
  return fminf(P.adaptiveClamping ? P.kernelMinResponse / density : P.kernelMinResponse, 0.97f);
}

// what mgs.h calls an invalid ray; written so that a NaN anywhere fails it
__device__ __forceinline__ bool rayValid(const float4& o, const float4& d)
{
  const float big = 3.4028234664e38f;
  const bool  fin = fabsf(o.x) <= big && fabsf(o.y) <= big && fabsf(o.z) <= big && fabsf(o.w) <= big && fabsf(d.x) <= big && fabsf(d.y) <= big
                   && fabsf(d.z) <= big && fabsf(d.w) <= big;
  return fin && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f) && o.w <= d.w;
}

}  // namespace mgs
