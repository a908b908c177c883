// trace_primary_ray.h — the pixel's primary ray with the bits k_trace traces: what k_rays_generate (k_trace_rays.hip) writes out and
// what the mesh primary rays of a traced frame (k_trace_mesh.hip) walk the triangles with, so that a frame's mesh hits are the mesh
// ray query's on the generated rays, bit for bit.  Device code only.
#pragma once
#include "gut_common.h"
#include "kernels_common.h"

namespace mgs {

// primaryRay (trace_traverse.h) with every rounding spelled out.  The source of primaryRay leaves the compiler free to fuse a
// multiply into an add or not (fp contraction), and which it does depends on the kernel the function is inlined into: in k_trace the
// packed-math vectoriser takes some products away from the fused form, in a kernel that only stores the ray it takes others.  The
// rays written here must be the bits k_trace traces, so this restates, operation for operation, what k_trace's code does (read
// from its gfx950 assembly; all nine instantiations share it): fma() is one rounding, everything else is rounded where it stands.
// test_gpu_rays.py (generated rays against the traced frame, bit for bit) holds the two together; if a compiler change moves
// k_trace's roundings, that test says so and this function follows.
__device__ __forceinline__ bool primaryRayAsTraced(const FrameConst& F, int px, int py, float (&o)[3], float (&d)[3])
{
#pragma clang fp contract(off)
  const float* Vi = F.lightViewInv;
  const float* Pi = F.lightProjInv;
  bool         rayOk = true;
  float        cx, cy, cz;
  if(F.cameraModel == 1)
  {
    const float u = __builtin_fmaf((float)px / ((float)F.width - 1.0f), 2.0f, -1.0f), v = __builtin_fmaf((float)py / ((float)F.height - 1.0f), 2.0f, -1.0f);
    const float r = sqrtf(__builtin_fmaf(u, u, v * v));
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
  {
    const float ux = __builtin_fmaf(((float)px + 0.5f) / (float)F.width, 2.0f, -1.0f), uy = __builtin_fmaf(((float)py + 0.5f) / (float)F.height, 2.0f, -1.0f);
    cx = __builtin_fmaf(Pi[0], ux, Pi[4] * uy) + Pi[8] + Pi[12];
    cy = __builtin_fmaf(Pi[1], ux, Pi[5] * uy) + Pi[9] + Pi[13];
    cz = __builtin_fmaf(Pi[2], ux, Pi[6] * uy) + Pi[10] + Pi[14];
  }
  const float dx = __builtin_fmaf(Vi[8], cz, __builtin_fmaf(Vi[4], cy, Vi[0] * cx));
  const float dy = __builtin_fmaf(Vi[5], cy, Vi[1] * cx) + Vi[9] * cz;
  const float dz = __builtin_fmaf(Vi[10], cz, __builtin_fmaf(Vi[2], cx, Vi[6] * cy));
  const float l  = rsqrtf(__builtin_fmaf(dy, dy, dx * dx) + dz * dz);
  d[0] = dx * l; d[1] = dy * l; d[2] = dz * l;
  o[0] = Vi[12]; o[1] = Vi[13]; o[2] = Vi[14];
  if(F.dofMode != 0)
  {
    uint32_t    seed = rngXxhash32((uint32_t)px, (uint32_t)py, (uint32_t)F.frameSampleId);
    const float r1 = rngRand(seed) * 6.28318530717958647692f, r2 = rngRand(seed) * F.aperture;
    const float c = cosf(r1), sn = sinf(r1), sq = sqrtf(r2);
    const float ax = __builtin_fmaf(Vi[0], c, Vi[4] * sn), ay = __builtin_fmaf(Vi[5], sn, Vi[1] * c), az = __builtin_fmaf(Vi[2], c, Vi[6] * sn);
    const float lx = sq * ax, ly = sq * ay, lz = sq * az;
    const float fx = __builtin_fmaf(d[0], F.focusDist, -lx), fy = d[1] * F.focusDist - ly, fz = __builtin_fmaf(d[2], F.focusDist, -lz);
    const float fl = rsqrtf(fz * fz + __builtin_fmaf(fy, fy, fx * fx));
    o[0] = __builtin_fmaf(sq, ax, Vi[12]);
    o[1] = Vi[13] + ly;
    o[2] = __builtin_fmaf(sq, az, Vi[14]);
    d[0] = fx * fl; d[1] = fy * fl; d[2] = fz * fl;
  }
  return rayOk;
}

}  // namespace mgs
