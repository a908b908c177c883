// gut_common.h — what the 3DGUT units share: the arithmetic helpers of k_project_gut.hip and k_composite_gut.hip (and of the traced
// pipeline, which evaluates the same particles), and the text the two compositors of k_composite_gut.hip have in common: the
// pixel's ray, the lens sample and the compaction of a staging round (their deferred shading stays written out: k_composite_gut.hip).
#pragma once
#include "kernels_common.h"

namespace mgs {

// This pipeline's arithmetic has a tolerance (>= 50 dB vs the oracle), no bit-exact part except the keys of phase 1: reciprocals
// and square roots are the 1-ulp hardware instructions, not hipcc's correctly rounded expansions (10 instructions each; the
// front end had ~30 divisions per splat, the compositor one per fragment).
__device__ __forceinline__ float gRcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float gSqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// threedgut_camera_projections.h.slang:32-44
__device__ __forceinline__ float gutStableNorm2(float x, float y)
{
  const float ax = fabsf(x), ay = fabsf(y);
  const float mn = fminf(ax, ay), mx = fmaxf(ax, ay);
  if(mx <= 0.0f)
    return 0.0f;
  const float r = mn * gRcp(mx);
  return mx * gSqrt(1.0f + r * r);
}

// particleRayMaxKernelResponse<KERNEL_DEGREE> (threedgrt.h.slang:83-127); its argument is the SQUARED canonical distance
__device__ __forceinline__ float kernelResponse(int degree, float dist2)
{
  switch(degree)
  {
    case 8: return __expf(-0.000685871056241f * (dist2 * dist2) * (dist2 * dist2));
    case 5: return __expf(-0.0185185185185f * dist2 * dist2 * sqrtf(dist2));
    case 4: return __expf(-0.0555555555556f * dist2 * dist2);
    case 3: return __expf(-0.166666666667f * dist2 * sqrtf(dist2));
    case 1: return __expf(-1.5f * sqrtf(dist2));
    case 0: return fmaxf(1.0f + -0.329630334487f * sqrtf(dist2), 0.0f);
    default: return __expf(-0.5f * dist2);
  }
}

// ---- the handle's sensor model (mgs_frame_set_sensor): the OpenCV pinhole / fisheye models with their coefficients ---------------
// computeDistortion of projectPointPinhole (threedgut_camera_projections.h.slang:96-116): the distorted normalised point
// icD * uv + delta and the radial factor icD
__device__ __forceinline__ void gutSensorDistort(const SensorConst& S, float u, float v, float& du, float& dv, float& icD)
{
  const float uu = u * u, vv = v * v, r2 = uu + vv;
  const float a1 = 2.0f * u * v, a2 = r2 + 2.0f * uu, a3 = r2 + 2.0f * vv;
  const float num = 1.0f + r2 * (S.radial[0] + r2 * (S.radial[1] + r2 * S.radial[2]));
  const float den = 1.0f + r2 * (S.radial[3] + r2 * (S.radial[4] + r2 * S.radial[5]));
  icD = num * gRcp(den);
  du  = icD * u + (S.tangential[0] * a1 + S.tangential[1] * a2 + r2 * (S.thinPrism[0] + r2 * S.thinPrism[1]));
  dv  = icD * v + (S.tangential[0] * a3 + S.tangential[1] * a1 + r2 * (S.thinPrism[2] + r2 * S.thinPrism[3]));
}

// evalPolyHorner4 (:51-59)
__device__ __forceinline__ float gutHorner4(const float (&k)[4], float x) { return ((k[3] * x + k[2]) * x + k[1]) * x + k[0]; }

// projectPointWithShutter (global shutter, :189-205) + projectPoint with the full projectPointPinhole (:85-136) /
// projectPointFisheye (:149-171): gutProjectCam's sibling (k_project_gut.hip) for a frame with a sensor bound.  `cam` as there.
__device__ __forceinline__ bool gutProjectSensor(const FrameConst& F, float cx, float cy, float cz, float& ox, float& oy)
{
  const SensorConst& S = F.sensor;
  const float resx = (float)F.width, resy = (float)F.height;
  bool        ok;
  if(S.model == 1)
  {
    const float rho       = fmaxf(gutStableNorm2(cx, cy), 1e-7f);
    const float thetaFull = atan2f(rho, cz);
    const float theta     = fminf(thetaFull, S.maxAngle);
    const float theta2    = theta * theta;
    const float delta     = (theta * (gutHorner4(S.fisheye, theta2) * theta2 + 1.0f)) * gRcp(rho);
    ox                    = S.focal[0] * cx * delta + S.principal[0];
    oy                    = S.focal[1] * cy * delta + S.principal[1];
    ok                    = theta < S.maxAngle;
  }
  else
  {
    if(cz <= 0.0f)
    {
      ox = oy = 0.0f;
      return false;
    }
    const float rcz = gRcp(cz);
    const float u = cx * rcz, v = cy * rcz;
    float       du, dv, icD;
    gutSensorDistort(S, u, v, du, dv, icD);
    ok = icD > 0.8f && icD < 1.2f;  // kMinRadialDist, kMaxRadialDist
    if(ok)
    {
      ox = du * S.focal[0] + S.principal[0];
      oy = dv * S.focal[1] + S.principal[1];
    }
    else
    {  // out of limits: clipped to a viable direction outside the image (:125-133)
      const float k = S.clipRadius * rsqrtf(u * u + v * v);
      ox = k * u + S.principal[0];
      oy = k * v + S.principal[1];
    }
  }
  const float mx = resx * 0.1f, my = resy * 0.1f;  // withinResolution, GUT_IN_IMAGE_MARGIN_FACTOR
  return ok && (ox > -mx) && (oy > -my) && (ox < resx + mx) && (oy < resy + my);
}

// The sensor's ray: the view-space direction whose projection (gutProjectSensor) is the image point (pcx, pcy).  The reference has
// no inverse of these models (PARITY UNPINNED, mgs.h): Newton with kSensorNewtonIters steps, on the 2x2 Jacobian of the distorted
// normalised point from (p - c) / f (pinhole), on theta (1 + poly(theta^2) theta^2) = |(p - c) / f| from that radius (fisheye).
// false: the pixel has no ray — the iteration ends outside the model's validity (icD outside (0.8, 1.2), theta >= maxAngle), it
// misses the image point by more than kSensorTolPx (no convergence; written so that a NaN fails), or the forward map is not
// monotone there (Jacobian determinant / derivative <= 0).
__device__ __forceinline__ bool gutSensorRay(const SensorConst& S, float pcx, float pcy, float& cx, float& cy, float& cz)
{
  const float qx = (pcx - S.principal[0]) * S.rcpFocal[0], qy = (pcy - S.principal[1]) * S.rcpFocal[1];
  bool        ok;
  if(S.model == 1)
  {
    const float rq = sqrtf(qx * qx + qy * qy);
    float       th = rq, res = 0.0f, dg = 1.0f;
    for(int it = 0;; ++it)
    {
      const float t2 = th * th;
      res = th * (gutHorner4(S.fisheye, t2) * t2 + 1.0f) - rq;
      dg  = 1.0f + t2 * (3.0f * S.fisheye[0] + t2 * (5.0f * S.fisheye[1] + t2 * (7.0f * S.fisheye[2] + t2 * (9.0f * S.fisheye[3]))));
      if(it == kSensorNewtonIters)
        break;
      th -= res * gRcp(dg);
    }
    ok = th >= 0.0f && th < S.maxAngle && fabsf(res) <= S.tolNorm && dg > 0.0f;
    const float sn = sinf(th), rr = rq > 0.0f ? gRcp(rq) : 0.0f;
    cx = sn * (qx * rr);
    cy = sn * (qy * rr);
    cz = -cosf(th);
  }
  else
  {
    float u = qx, v = qy, fx = 0.0f, fy = 0.0f, det = 1.0f, icD = 1.0f;
    for(int it = 0;; ++it)
    {
      const float uu = u * u, vv = v * v, uv = u * v, r2 = uu + vv;
      const float num = 1.0f + r2 * (S.radial[0] + r2 * (S.radial[1] + r2 * S.radial[2]));
      const float den = 1.0f + r2 * (S.radial[3] + r2 * (S.radial[4] + r2 * S.radial[5]));
      const float rden = gRcp(den);
      icD = num * rden;
      fx  = icD * u + (S.tangential[0] * (2.0f * uv) + S.tangential[1] * (r2 + 2.0f * uu) + r2 * (S.thinPrism[0] + r2 * S.thinPrism[1])) - qx;
      fy  = icD * v + (S.tangential[0] * (r2 + 2.0f * vv) + S.tangential[1] * (2.0f * uv) + r2 * (S.thinPrism[2] + r2 * S.thinPrism[3])) - qy;
      // d icD / d r2, and the thin-prism polynomials' derivatives
      const float dnum = S.radial[0] + r2 * (2.0f * S.radial[1] + r2 * (3.0f * S.radial[2]));
      const float dden = S.radial[3] + r2 * (2.0f * S.radial[4] + r2 * (3.0f * S.radial[5]));
      const float dic  = (dnum - icD * dden) * rden;
      const float tp0 = S.thinPrism[0] + 2.0f * r2 * S.thinPrism[1], tp1 = S.thinPrism[2] + 2.0f * r2 * S.thinPrism[3];
      const float j00 = icD + 2.0f * (uu * dic + S.tangential[0] * v + 3.0f * S.tangential[1] * u + u * tp0);
      const float j01 = 2.0f * (uv * dic + S.tangential[0] * u + S.tangential[1] * v + v * tp0);
      const float j10 = 2.0f * (uv * dic + S.tangential[0] * u + S.tangential[1] * v + u * tp1);
      const float j11 = icD + 2.0f * (vv * dic + 3.0f * S.tangential[0] * v + S.tangential[1] * u + v * tp1);
      det = j00 * j11 - j01 * j10;
      if(it == kSensorNewtonIters)
        break;
      const float rdet = gRcp(det);
      u -= (j11 * fx - j01 * fy) * rdet;
      v -= (j00 * fy - j10 * fx) * rdet;
    }
    ok = icD > 0.8f && icD < 1.2f && fabsf(fx) <= S.tolNorm && fabsf(fy) <= S.tolNorm && det > 0.0f;
    cx = u;
    cy = v;
    cz = -1.0f;
  }
  if(!ok)
  {  // (a finite direction for what a pixel without a ray still computes)
    cx = cy = 0.0f;
    cz = -1.0f;
  }
  return ok;
}

// ---- shared by k_composite_gut and k_composite_gut2 -----------------------------------------------------------------------------
// world-space ray direction of the pixel whose centre is (pcx, pcy) (threedgut_raster.frag.slang:101-111); false: outside the
// fisheye's field of view, or no ray of the bound sensor (the fragment is discarded).  With a sensor bound (wave-uniform) the ray
// is the one whose projection is (pcx, pcy) itself: self-consistent with the front end's quad placement, where the perfect pinhole
// below adds the reference's second 0.5.
__device__ __forceinline__ bool gutPixelRay(const FrameConst& F, float pcx, float pcy, float& dxw, float& dyw, float& dzw)
{
  const float* Vi = F.viewInv;
  float        cx, cy, cz;
  bool         rayOk = true;
  if(F.sensor.bound != 0)
    rayOk = gutSensorRay(F.sensor, pcx, pcy, cx, cy, cz);
  else if(F.cameraModel == 1)
  {  // generateFisheyeRay(position.xy, viewport, fovRad, principal 0, viewInverse), cameras.h.slang:46-82
    const float u = (pcx / ((float)F.width - 1.0f)) * 2.0f - 1.0f, v = (pcy / ((float)F.height - 1.0f)) * 2.0f - 1.0f;
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
  {  // generatePinholeRay(position.xy, float2(0.5), ...): the 0.5 is added to SV_Position, as the reference writes it
    const float ux = ((pcx + 0.5f) / (float)F.width) * 2.0f - 1.0f, uy = ((pcy + 0.5f) / (float)F.height) * 2.0f - 1.0f;
    const float* Pi = F.projInv;
    cx = Pi[0] * ux + Pi[4] * uy + Pi[8] + Pi[12];
    cy = Pi[1] * ux + Pi[5] * uy + Pi[9] + Pi[13];
    cz = Pi[2] * ux + Pi[6] * uy + Pi[10] + Pi[14];
  }
  dxw = Vi[0] * cx + Vi[4] * cy + Vi[8] * cz;
  dyw = Vi[1] * cx + Vi[5] * cy + Vi[9] * cz;
  dzw = Vi[2] * cx + Vi[6] * cy + Vi[10] * cz;
  const float l = rsqrtf(dxw * dxw + dyw * dyw + dzw * dzw);
  dxw *= l; dyw *= l; dzw *= l;
  return rayOk;
}

// depth of field (frag.slang:104-109, cameras.h.slang:85-108): one lens sample per pixel and frame.  The ray (dx, dy, dz) leaves
// the random lens point (lx, ly, lz) and still passes through the focal point of the pinhole ray.  HW_SQRT: the 1-ulp square root
// (k_composite_gut2) or the correctly rounded one (k_composite_gut) — each kernel keeps the one its frames were made with.
template <bool HW_SQRT>
__device__ __forceinline__ void gutLensSample(const FrameConst& F, uint32_t seed, float& lx, float& ly, float& lz, float& dx, float& dy, float& dz)
{
  const float r1 = rngRand(seed) * 6.28318530717958647692f, r2 = rngRand(seed) * F.aperture;
  const float* Vi = F.viewInv;  // camRight = mul(float4(1,0,0,0), viewInverse), camUp = mul(float4(0,1,0,0), viewInverse)
  const float c = cosf(r1), sn = sinf(r1), sq = HW_SQRT ? gSqrt(r2) : sqrtf(r2);
  lx = (c * Vi[0] + sn * Vi[4]) * sq;
  ly = (c * Vi[1] + sn * Vi[5]) * sq;
  lz = (c * Vi[2] + sn * Vi[6]) * sq;
  const float fx = dx * F.focusDist - lx, fy = dy * F.focusDist - ly, fz = dz * F.focusDist - lz;
  const float l  = rsqrtf(fx * fx + fy * fy + fz * fz);
  dx = fx * l; dy = fy * l; dz = fz * l;
}

// A staging round's survivors (ok) compacted in list order: the slot of this thread's record (meaningful where ok) and the
// round's count.  Every thread of the 256-thread workgroup calls it (one barrier); s_wc: four words of LDS, lane / w: the
// thread's lane and wave.
__device__ __forceinline__ uint32_t gutCompactSlot(bool ok, uint32_t (&s_wc)[4], int lane, int w, uint32_t& fill)
{
  const uint64_t bal = __ballot(ok);
  if(lane == 0)
    s_wc[w] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t base = 0;
  if(w > 0) base += s_wc[0];
  if(w > 1) base += s_wc[1];
  if(w > 2) base += s_wc[2];
  fill = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
  return base + lanesBelow(bal);
}

}  // namespace mgs
