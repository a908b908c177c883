// k_light.hip — deferred lighting of the splat surface and depth consolidation.
//
// k_light restates shaders/deferred_shading.comp.slang:52-167 with the shading functions of shaders/wavefront.h.slang:104-280,388-403
// in their own order of operations: one launch per lit frame between the compositor and k_post_accumulate, one thread per pixel of
// the handle's strip.  Per pixel it reads the integrated normal (16 B), the picked depth (4 B), the picked id (4 B) and the frame's
// pixel (4 / 8 / 16 B) and rewrites the pixel: a streaming pass without reuse.  Consecutive lanes take consecutive pixels, the four
// loads are issued before the first is used, lanes without a surface (normal.w < 0.001) write nothing.  Lights are read through
// wave-uniform (scalar) loads inside the loop; a material is 64 B gathered by the pixel's instance (a table of at most 16 KB).
//
// k_depth_consolidate restates shaders/depth_consolidate.frag.slang (one depth image for what follows the splats).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "../../include/mgs.h"
#include "launchers.h"
#include "shade_direct.h"
#include "target_pixel.h"

namespace mgs {

namespace {

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

}  // namespace

// FMT: the target format (kTargetF32, kTargetF16, kTargetU8)
template <int FMT>
__global__ void __launch_bounds__(256) k_light(const LightArgs a)
{
  const uint32_t W = (uint32_t)a.width;
  const uint32_t n = (uint32_t)(a.row1 - a.row0) * W;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n)
    return;
  const size_t o = (size_t)a.row0 * W + i;
  // all four inputs in flight before the first is used
  const float4   normalData    = a.normal[o];
  const float    ndcDepth      = a.depth[o];
  const uint32_t globalSplatId = a.id[o];
  const float4   baseColor     = loadPixel(a.image, FMT, o);
  if(normalData.w < 0.001f)
    return;  // no surface: colour and alpha pass through

  const FrameConst& F      = a.frame->f;
  const V3          normal = normalize3({normalData.x, normalData.y, normalData.z});
  // reconstructWorldPos (deferred_shading.comp.slang:39-50)
  const uint32_t py = i / W, px = i - py * W;
  const float    fx = (float)px + 0.5f, fy = (float)(py + (uint32_t)a.row0) + 0.5f;
  const float4   clipPos = make_float4(fx / (float)F.width * 2.0f - 1.0f, fy / (float)F.height * 2.0f - 1.0f, ndcDepth, 1.0f);
  float4         viewPos = mulMat(F.lightProjInv, clipPos);
  viewPos = make_float4(viewPos.x / viewPos.w, viewPos.y / viewPos.w, viewPos.z / viewPos.w, viewPos.w / viewPos.w);
  const float4 wp4      = mulMat(F.lightViewInv, viewPos);
  const V3     worldPos = {wp4.x, wp4.y, wp4.z};
  const V3     cameraPos = load3(F.cameraPos);

  const V3 baseRadiance = {baseColor.x, baseColor.y, baseColor.z};
  Mat      mat;
  if(globalSplatId != 0xFFFFFFFFu)
  {  // the instance that owns the id: the last one whose first global id is not above it (instances are concatenated in creation
     // order); log2(instances) steps, the same count for every lane
    int lo = 0, hi = F.nInstances;
    while(hi - lo > 1)
    {
      const int mid = (lo + hi) >> 1;
      if(a.frame->inst[mid].globalOffset <= globalSplatId)
        lo = mid;
      else
        hi = mid;
    }
    mat = splatMaterial(a.table->mats[lo], baseRadiance);
  }
  else
  {  // the shader's default material with the base colour as diffuse
    mat.ambient     = {0.1f, 0.1f, 0.1f};
    mat.diffuse     = baseRadiance;
    mat.specular    = {0.0f, 0.0f, 0.0f};
    mat.emission    = {0.0f, 0.0f, 0.0f};
    mat.shininess   = 32.0f;
    mat.needShading = 1;
  }
  const V3 viewDir = normalize3(worldPos - cameraPos);
  V3       color   = mat.emission;
  if(mat.needShading != 0)
  {
    const int count = a.table->count;
    for(int l = 0; l < count; ++l)
      shadeDirect(a.table->lights[l], worldPos, normal, mat, viewDir, color);
    if(count == 0)
      shadeDirect(headlight(F.cameraPos), worldPos, normal, mat, viewDir, color);
  }
  storePixel(a.image, FMT, o, color.x, color.y, color.z, 1.0f);
}

// depth_consolidate.frag.slang: the picked splat depth where it is valid and in front of the geometry (depth test LESS against the
// geometry's depth, gaussian_splatting.cpp:2383), the geometry's depth (1.0 = the clear value when none is bound) elsewhere
__global__ void __launch_bounds__(256) k_depth_consolidate(const float* __restrict__ picked, const float* __restrict__ occDepth, float* __restrict__ out, uint32_t n)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n)
    return;
  const float p = picked[i];
  const float D = occDepth ? occDepth[i] : 1.0f;
  out[i]        = (p > 0.0001f && p < D) ? p : D;
}

void launchLight(hipStream_t stream, const LightArgs& a, int fmt)
{
  const uint32_t n = (uint32_t)(a.row1 - a.row0) * (uint32_t)a.width;
  if(n == 0)
    return;
  const dim3 grid((n + 255u) / 256u), block(256);
  if(fmt == kTargetF16)
    hipLaunchKernelGGL(k_light<kTargetF16>, grid, block, 0, stream, a);
  else if(fmt == kTargetU8)
    hipLaunchKernelGGL(k_light<kTargetU8>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(k_light<kTargetF32>, grid, block, 0, stream, a);
}

void launchDepthConsolidate(hipStream_t stream, const float* picked, const float* occDepth, float* out, uint32_t n)
{
  if(n)
    hipLaunchKernelGGL(k_depth_consolidate, dim3((n + 255u) / 256u), dim3(256), 0, stream, picked, occDepth, out, n);
}

}  // namespace mgs
