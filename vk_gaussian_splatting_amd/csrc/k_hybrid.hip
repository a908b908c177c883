// k_hybrid.hip — the hand-over of a hybrid frame (mgs_render_hybrid) for gfx950: the rasterised splat surface becomes the primary
// surface of the traced light pass (k_trace_light.hip), "in place of first-bounce ray tracing".
//
// Replaces
//   shaders/threedgrt_raytrace.rgen.slang:346-460   initRtxStateFromRasterPass (NEED_SURFACE_INFO, no mesh in the traced scene)
//   shaders/threedgrt_raytrace.rgen.slang:165-196   the pixel's ray (trace_traverse.h: primaryRay)
// Structure: a lane per pixel in k_trace's tiling (a wave64 = an 8 x 8 pixel tile, a workgroup = a 16 x 16 tile, strip rows honoured),
// so that the light pass behind it reads what the same lane wrote.  A streaming pass without reuse: per pixel it reads the stored
// pixel (4 / 8 / 16 B), the picked depth (4 B), the picked id (4 B) and the integrated normal (16 B), all four in flight before the
// first is used, and writes the light pass's inputs (4 + 16 + 16 B; the picked ids are read as they are).  It never writes the frame or the raster side outputs:
// a pixel the light pass must leave alone (valid depth, no picked id: rgen.slang:1047-1049) is handed on with a negative ray
// parameter.  No loop, no LDS, nothing waits on another lane.
// With the scene's meshes (mgs_frame_set_hybrid_meshes; rgen.slang:252-281, :1037-1062): k_hybrid_mesh_depth turns the hit records of
// the mesh depth pre-pass into the plane the raster pass is tested against, and the hand-over's MESH instantiations also leave the
// pixel's transmittance for the mesh composite (k_trace_mesh.hip).
#include "kernels_common.h"
#include "launchers.h"
#include "shade_direct.h"
#include "target_pixel.h"
#include "trace_common.h"
#include "trace_dispatch.h"
#include "trace_traverse.h"

namespace mgs {

// FMT: the target format (kTargetF32, kTargetF16, kTargetU8); MESH: a frame with the scene's meshes (mgs_frame_set_hybrid_meshes),
// whose raster pass ran against the mesh depth pre-pass: the pixel's transmittance goes to the mesh composite (:357-358, T = 1 for a
// discarded pixel, :468-478), and a surface with a pick that is not in front of the pixel's mesh hit fails splatIsClosest (:1047):
// it is handed on settled, with its raster colour and its own T
template <int FMT, bool MESH>
__global__ __launch_bounds__(256) void k_hybrid_surface(const std::conditional_t<MESH, HybridSurfaceMeshArgs, HybridSurfaceArgs> args)
{
  const HybridSurfaceArgs& a = [&]() -> const HybridSurfaceArgs& {
    if constexpr(MESH)
      return args.a;
    else
      return args;
  }();
  const FrameConst& F = a.frame->f;
  int px, py;
  tilePixel(F, (int)threadIdx.x, px, py);
  if(px >= F.width || py >= F.height)
    return;
  const size_t pix = (size_t)py * F.width + px;

  // all four inputs in flight before the first is used
  const float4   stored  = loadPixel(a.image, FMT, pix);
  const float    ndcZ    = a.depth[pix];
  const uint32_t splatId = a.id[pix];
  const float4   nrm     = a.normal[pix];
  TraceRay   ray;
  const bool rayOk = primaryRay(F, px, py, ray);

  const bool validDepth = ndcZ > 0.0001f;  // rgen.slang:367
  float      t = 0.0f;
  if(F.cameraModel == 1)
  {  // fisheye (:402-419): the z mapping of the pinhole projection does not depend on xy
    const float* V  = F.view;
    const float* Pi = F.lightProjInv;
    const float  dirViewZ = (ray.d[0] * V[2] + ray.d[1] * V[6]) + ray.d[2] * V[10];
    const float  vz = ndcZ * Pi[10] + Pi[14], vw = ndcZ * Pi[11] + Pi[15];
    t = (vz / vw) / dirViewZ;
  }
  else
  {  // pinhole (:378-390): reconstructWorldPos of k_light.hip, operation for operation
    const float* Pi = F.lightProjInv;
    const float* Vi = F.lightViewInv;
    const float  cx = ((float)px + 0.5f) / (float)F.width * 2.0f - 1.0f, cy = ((float)py + 0.5f) / (float)F.height * 2.0f - 1.0f;
    float        vx = ((cx * Pi[0] + cy * Pi[4]) + ndcZ * Pi[8]) + Pi[12];
    float        vy = ((cx * Pi[1] + cy * Pi[5]) + ndcZ * Pi[9]) + Pi[13];
    float        vz = ((cx * Pi[2] + cy * Pi[6]) + ndcZ * Pi[10]) + Pi[14];
    float        vw = ((cx * Pi[3] + cy * Pi[7]) + ndcZ * Pi[11]) + Pi[15];
    vx /= vw; vy /= vw; vz /= vw; vw /= vw;
    const float wx = ((vx * Vi[0] + vy * Vi[4]) + vz * Vi[8]) + vw * Vi[12];
    const float wy = ((vx * Vi[1] + vy * Vi[5]) + vz * Vi[9]) + vw * Vi[13];
    const float wz = ((vx * Vi[2] + vy * Vi[6]) + vz * Vi[10]) + vw * Vi[14];
    const float ex = wx - ray.o[0], ey = wy - ray.o[1], ez = wz - ray.o[2];
    t = sqrtf((ex * ex + ey * ey) + ez * ez);
  }
  // :448-452
  V3 normal = {0.0f, 0.0f, 0.0f};
  if(nrm.w > 0.001f)
    normal = normalize3({nrm.x, nrm.y, nrm.z});
  const bool discard = !validDepth || sqrtf(dot3(normal, normal)) < 0.001f;  // :455

  // 0: discarded (or outside the fisheye circle, where the light pass leaves the pixel alone by its ray).  The light pass reads the
  // picked id as the raster pass left it; the ray parameter alone says what becomes of the pixel.
  float outT = 0.0f;
  if(rayOk && !discard)
  {
    if(splatId == kTraceInvalid)
      outT = -1.0f;  // a surface without a picked splat keeps its raster colour, unlit (:1047-1049)
    else if(t > 0.0f)
      outT = t;  // (a ray parameter that is not positive is no surface for the light pass: k_trace_light's own rule)
  }
  if constexpr(MESH)
  {
    float4 radiance = stored;
    float  T        = 1.0f - stored.w;
    if(outT > 0.0f && !(outT < args.meshT[pix]))
      outT = -1.0f;  // behind (or at) the mesh: never the light pass's "store 0" branch
    if(rayOk && outT == 0.0f)
    {  // discardSplatContribution: the mesh or the background shows through
      radiance = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      T        = 1.0f;
    }
    args.outT[pix]     = (double)T > (double)args.minT ? T : -1.0f;
    a.outIsoDist[pix]  = outT;
    a.outNormal[pix]   = make_float4(normal.x, normal.y, normal.z, nrm.w);
    a.outRadiance[pix] = radiance;
  }
  else
  {
    a.outIsoDist[pix]  = outT;
    a.outNormal[pix]   = make_float4(normal.x, normal.y, normal.z, nrm.w);
    a.outRadiance[pix] = stored;
  }
}

// The mesh depth pre-pass's second half (rgen.slang:259-270, meshDepthOnly): the hit records k_trace_mesh_primary left become the
// depth plane the raster pass is tested against.  clip = (meshHitWorldPos * view) * proj, the plane gets clip.z / clip.w; 1.0 on a
// miss (a fisheye pixel outside the circle is one).  A lane per pixel in k_trace's tiling, no loop, no LDS.
__global__ __launch_bounds__(256) void k_hybrid_mesh_depth(const FrameArgs* __restrict__ Ap, const float4* __restrict__ hits, float* __restrict__ plane)
{
  const FrameConst& F = Ap->f;
  int px, py;
  tilePixel(F, (int)threadIdx.x, px, py);
  if(px >= F.width || py >= F.height)
    return;
  const size_t pix = (size_t)py * F.width + px;
  const float4 h0 = hits[4 * pix], h1 = hits[4 * pix + 1];
  float        z  = 1.0f;
  if(h0.x < __builtin_huge_valf())
  {
    const float  hx = h1.x, hy = h1.y, hz = h1.z;
    const float *V = F.view, *P = F.proj;
    const float  v0 = V[0] * hx + V[4] * hy + V[8] * hz + V[12], v1 = V[1] * hx + V[5] * hy + V[9] * hz + V[13],
                v2 = V[2] * hx + V[6] * hy + V[10] * hz + V[14], v3 = V[3] * hx + V[7] * hy + V[11] * hz + V[15];
    const float cz = P[2] * v0 + P[6] * v1 + P[10] * v2 + P[14] * v3, cw = P[3] * v0 + P[7] * v1 + P[11] * v2 + P[15] * v3;
    z = cz / cw;
  }
  plane[pix] = z;
}

void launchHybridSurface(hipStream_t stream, const HybridSurfaceArgs& a, const FrameConst& F, int fmt)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  if(fmt == kTargetF16)
    hipLaunchKernelGGL((k_hybrid_surface<kTargetF16, false>), dim3(tiles), dim3(256), 0, stream, a);
  else if(fmt == kTargetU8)
    hipLaunchKernelGGL((k_hybrid_surface<kTargetU8, false>), dim3(tiles), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((k_hybrid_surface<kTargetF32, false>), dim3(tiles), dim3(256), 0, stream, a);
}

void launchHybridSurfaceWithMeshes(hipStream_t stream, const HybridSurfaceMeshArgs& a, const FrameConst& F, int fmt)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  if(fmt == kTargetF16)
    hipLaunchKernelGGL((k_hybrid_surface<kTargetF16, true>), dim3(tiles), dim3(256), 0, stream, a);
  else if(fmt == kTargetU8)
    hipLaunchKernelGGL((k_hybrid_surface<kTargetU8, true>), dim3(tiles), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((k_hybrid_surface<kTargetF32, true>), dim3(tiles), dim3(256), 0, stream, a);
}

void launchHybridMeshDepth(hipStream_t stream, const FrameArgs* frame, const float4* hits, float* plane, const FrameConst& F)
{
  const int tiles = stripTiles(F);
  if(tiles <= 0)
    return;
  hipLaunchKernelGGL(k_hybrid_mesh_depth, dim3(tiles), dim3(256), 0, stream, frame, hits, plane);
}

}  // namespace mgs
