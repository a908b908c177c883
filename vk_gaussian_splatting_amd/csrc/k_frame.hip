// k_frame.hip — the frame's four small kernels: the sort plan's count, fill and iota of a word buffer, and the temporal
// accumulation of a finished frame.  They keep C names, as a profile lists them.
#include "kernels_common.h"
#include "launchers.h"
#include "target_pixel.h"

using namespace mgs;

extern "C" {
__global__ void k_set_plan_n(SortPlan* plan, FrameCounters* ctr, uint32_t n)
{
  plan->n         = n;
  plan->finalSel  = 0;
  plan->passesRun = 0;
  ctr->sortedCount = n;
}
__global__ void k_fill_u32(uint32_t* p, uint32_t v, uint32_t n)
{
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    p[i] = v;
}
// post.comp.slang:29-43: main = lerp(main, aux1, 1 / (frameSampleId + 1)) — aux1 is the frame just rendered, main the
// accumulated image.  Here the accumulator is a separate fp32 image and the result is written back over the frame in the
// target's format, so the caller reads the running mean where it reads every frame.
__global__ void k_post_accumulate(const FrameArgs* __restrict__ Ap, float4* __restrict__ acc, void* __restrict__ image, int fmt)
{
  const FrameConst& F  = Ap->f;
  const int         y0 = F.stripRow0 * kTilePx, y1 = min(F.stripRow1 * kTilePx, F.height);
  const size_t      n  = (size_t)(y1 - y0) * (size_t)F.width;
  const float       a  = 1.0f / (float)(F.frameSampleId + 1);
  for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
  {
    const size_t o = (size_t)y0 * F.width + i;
    const float4 c = loadPixel(image, fmt, o);
    float4       m = acc[o];
    if(F.frameSampleId <= 0)
      m = c;  // lerp(main, aux1, 1) without touching what the accumulator held (it may be uninitialised)
    else
    {  // lerp(x, y, s) = x + s * (y - x)
      m.x = m.x + a * (c.x - m.x);
      m.y = m.y + a * (c.y - m.y);
      m.z = m.z + a * (c.z - m.z);
      m.w = m.w + a * (c.w - m.w);
    }
    acc[o] = m;
    storePixel(image, fmt, o, m.x, m.y, m.z, m.w);
  }
}
__global__ void k_iota_u32(uint32_t* p, uint32_t n)
{
  for(uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    p[i] = i;
}
}  // extern "C"

namespace mgs {

void launchSetPlanN(hipStream_t stream, SortPlan* plan, FrameCounters* ctr, uint32_t n)
{
  hipLaunchKernelGGL(k_set_plan_n, dim3(1), dim3(1), 0, stream, plan, ctr, n);
}
void launchFillU32(hipStream_t stream, uint32_t* p, uint32_t v, uint32_t n)
{
  hipLaunchKernelGGL(k_fill_u32, dim3(1024), dim3(256), 0, stream, p, v, n);
}
void launchIotaU32(hipStream_t stream, uint32_t* p, uint32_t n)
{
  hipLaunchKernelGGL(k_iota_u32, dim3(1024), dim3(256), 0, stream, p, n);
}
void launchPostAccumulate(hipStream_t stream, const FrameArgs* dArgs, float4* accum, void* image, int fmt)
{
  hipLaunchKernelGGL(k_post_accumulate, dim3(2048), dim3(256), 0, stream, dArgs, accum, image, fmt);
}

}  // namespace mgs
