// trace_shade.h — what a walk of the traced pipeline's primary rays does with a hit, whatever the trace strategy: the hit's
// world-space normal (k_trace.hip and k_trace_stochastic.hip), and particleProcessHit's alpha, acceptance and radiance and the picked
// hit's depth (k_trace_stochastic.hip; k_trace.hip has these two written out in its walk and says why there).
//
// Replaces
//   shaders/threedgrt.h.slang:166-223                particleProcessHit: alpha, acceptance, SH radiance, the normal to world space
//   shaders/threedgrt.h.slang:358-537                computeEllipsoidNormalMaxDensityPlane, computeEllipsoidNormal, raySphereIntersection
//   shaders/threedgrt_raytrace.rgen.slang:735-740,1490-1494   the picked hit's position and its ndc z
// Device code only; every kernel file that includes it gets its own inlined copy.
#pragma once
#include "gut_common.h"
#include "kernels_common.h"
#include "sh_eval.h"
#include "trace_common.h"
#include "trace_traverse.h"

namespace mgs {

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

// particleProcessHit without the normal (threedgrt.h.slang:166-213): false = the hit is not accepted, and nothing else is set.
// noGauss / shOnly: debug flags 4 / 2.  SHF: SH storage format.
template <int SHF>
__device__ __forceinline__ bool shadeHit(const FrameArgs* Ap, const ParticleEval& E, bool noGauss, bool shOnly, float& alpha, float& r, float& gg,
                                         float& b)
{
  const FrameConst& F = Ap->f;
  alpha               = fminf(F.alphaClamp, E.resp * E.density);
  const bool accept   = E.density > F.alphaCull && alpha > F.alphaCull && E.resp > F.kernelMinResponse;
  if(!accept)
    return false;
  if(noGauss)
    alpha = 1.0f;
  const InstanceConst& I   = Ap->inst[E.k];
  const float4         col = reinterpret_cast<const float4*>(I.rgbaF32)[E.li];
  float vx = E.p[0] - E.om[0], vy = E.p[1] - E.om[1], vz = E.p[2] - E.om[2];  // normalize(position - modelRayOrigin), :193
  const float vl = rsqrtf(vx * vx + vy * vy + vz * vz);
  vx *= vl; vy *= vl; vz *= vl;
  r  = shOnly ? 0.5f : col.x;
  gg = shOnly ? 0.5f : col.y;
  b  = shOnly ? 0.5f : col.z;
  const int deg = (I.sh == nullptr) ? 0 : min(I.shDegree, F.shDegree);
  if(deg > 0)
    addShRadiance<SHF>(I.sh, E.li, deg, vx, vy, vz, r, gg, b);
  return true;
}

// ndc z of the picked hit's position origin + dist * direction (rgen.slang:735-740, :1490-1494)
__device__ __forceinline__ float pickedNdcZ(const FrameConst& F, const TraceRay& ray, float dist)
{
  const float  hx = ray.o[0] + dist * ray.d[0], hy = ray.o[1] + dist * ray.d[1], hz = ray.o[2] + dist * ray.d[2];
  const float *V = F.view, *P = F.proj;
  const float  v0 = V[0] * hx + V[4] * hy + V[8] * hz + V[12], v1 = V[1] * hx + V[5] * hy + V[9] * hz + V[13],
              v2 = V[2] * hx + V[6] * hy + V[10] * hz + V[14], v3 = V[3] * hx + V[7] * hy + V[11] * hz + V[15];
  const float cz = P[2] * v0 + P[6] * v1 + P[10] * v2 + P[14] * v3, cw = P[3] * v0 + P[7] * v1 + P[11] * v2 + P[15] * v3;
  return cz / cw;
}

}  // namespace mgs
