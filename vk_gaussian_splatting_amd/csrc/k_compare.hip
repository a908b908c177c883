// k_compare.hip — runtime image comparison: MSE / PSNR / FLIP of the handle's frame against a captured image, and the split view.
//
// Restates shaders/image_compare_metric.comp.slang and shaders/image_compare_composite.comp.slang (with the colour helpers of
// shaders/color.h.slang) in their own order of operations; floating-point contraction is off for the whole file, so a*b + c is a
// multiply and an add as in the shaders' SPIR-V.
//
//   k_cmp_metric<MODE>   one thread per capture pixel, 16 x 16 pixels per workgroup.  Squared error and (MODE 1 / 2) the FLIP powered
//                        error; each is reduced twice: truncated to the reference's 1e9 fixed point and added with ONE integer atomic
//                        per workgroup (integer addition commutes: the sum does not depend on the order), and untruncated in double
//                        into a per-workgroup partial.  MODE 1 (approx) keeps an 18 x 18 luminance tile of both images in LDS for
//                        the 3 x 3 Sobel.  MODE 2 (reference) reads the feature planes the three kernels below made.
//   k_cmp_fold           one workgroup: the partials in a fixed order, so that two calls return the same bits.
//   k_cmp_luminance      Rec.709 luminance plane of an image.
//   k_cmp_blur_rows      the reference-mode Gaussians are products of two 1-D Gaussians and interior pixels never clamp: the row
//   k_cmp_blur_cols      pass sums 2r+1 taps along x for all five channels out of one LDS row segment, the column pass sums 2r+1
//                        taps along y out of an LDS tile and finishes the feature |centre - blurred| * csf.  2 x 263 taps per pixel
//                        and image at 67 pixels per degree instead of the shader's 23 357.  The intermediate planes go through
//                        global memory (they fit the infinity cache at 1920 x 1080).
//   k_cmp_composite      one thread per output pixel, all six display modes.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "compare_types.h"
#include "target_pixel.h"

#pragma clang fp contract(off)

namespace mgs {

namespace {

struct C3
{
  float x, y, z;
};

__device__ __forceinline__ float4 cmpLoad(const CmpImage& im, int x, int y)
{
  const size_t o = (size_t)y * (size_t)im.w + (size_t)x;
  return loadPixel(im.p, im.fmt, o);
}

// Texture2D::Load outside the image: zero (robust image access)
__device__ __forceinline__ float4 cmpLoadOrZero(const CmpImage& im, int x, int y)
{
  if(x < 0 || y < 0 || x >= im.w || y >= im.h)
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return cmpLoad(im, x, y);
}

// SampleLevel(linearSampler, uv, 0): bilinear, clamp to edge (PARITY UNPINNED, see mgs.h), weights in fp32
__device__ __forceinline__ float4 cmpSample(const CmpImage& im, float u, float v)
{
  const float fx = u * (float)im.w - 0.5f, fy = v * (float)im.h - 0.5f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float tx = fx - x0f, ty = fy - y0f;
  const int   x0 = min(max((int)x0f, 0), im.w - 1), x1 = min(max((int)x0f + 1, 0), im.w - 1);
  const int   y0 = min(max((int)y0f, 0), im.h - 1), y1 = min(max((int)y0f + 1, 0), im.h - 1);
  const float4 c00 = cmpLoad(im, x0, y0), c10 = cmpLoad(im, x1, y0), c01 = cmpLoad(im, x0, y1), c11 = cmpLoad(im, x1, y1);
  const float  sx = 1.0f - tx, sy = 1.0f - ty;
  float4       r;
  r.x = (c00.x * sx + c10.x * tx) * sy + (c01.x * sx + c11.x * tx) * ty;
  r.y = (c00.y * sx + c10.y * tx) * sy + (c01.y * sx + c11.y * tx) * ty;
  r.z = (c00.z * sx + c10.z * tx) * sy + (c01.z * sx + c11.z * tx) * ty;
  r.w = (c00.w * sx + c10.w * tx) * sy + (c01.w * sx + c11.w * tx) * ty;
  return r;
}

__device__ __forceinline__ float lum709(float4 c) { return (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f; }
__device__ __forceinline__ float saturate(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// color.h.slang:44-51
__device__ __forceinline__ float srgbToLinear1(float s) { return (s <= 0.04045f) ? (s / 12.92f) : powf((s + 0.055f) / 1.055f, 2.4f); }

// srgbToFLIPColorSpace (color.h.slang:87-142): sRGB -> linear -> LMS -> Hunt -> YCxCz
__device__ __forceinline__ C3 srgbToYCxCz(float4 c, float huntFL)
{
  const float r = srgbToLinear1(c.x), g = srgbToLinear1(c.y), b = srgbToLinear1(c.z);
  float       L = (0.31670331f * r + 0.70299344f * g) + -0.01969366f * b;
  float       M = (0.10938715f * r + 0.87060437f * g) + 0.01990658f * b;
  float       S = (0.01840087f * r + 0.10476914f * g) + 0.87470614f * b;
  L *= huntFL;
  M *= huntFL;
  S *= huntFL;
  return {M, L - M, M - S};
}

// the colour term shared by computeFLIPApprox (:380-397) and computeFLIPReference (:496-512)
__device__ __forceinline__ float flipColorError(float4 ref, float4 cur, const CmpMetricArgs& a)
{
  const C3 p = srgbToYCxCz(ref, a.huntFL), q = srgbToYCxCz(cur, a.huntFL);
  return (fabsf(p.x - q.x) * a.csfY + fabsf(p.y - q.y) * a.csfC) + fabsf(p.z - q.z) * a.csfC;
}

// uint(v) of the shader, defined for every input: negative and NaN give 0, too large saturates
__device__ __forceinline__ uint32_t toFixed(float v)
{
  if(!(v > 0.0f))
    return 0u;
  if(v >= 4294967296.0f)
    return 0xFFFFFFFFu;
  return (uint32_t)v;
}

__device__ __forceinline__ float sobel(const float* t, int lx, int ly)
{  // t: 18 x 18 luminance tile, (lx, ly) the centre.  image_compare_metric.comp.slang:419-427
  const float tl = t[(ly - 1) * 18 + lx - 1], tc = t[(ly - 1) * 18 + lx], tr = t[(ly - 1) * 18 + lx + 1];
  const float ml = t[ly * 18 + lx - 1], mr = t[ly * 18 + lx + 1];
  const float bl = t[(ly + 1) * 18 + lx - 1], bc = t[(ly + 1) * 18 + lx], br = t[(ly + 1) * 18 + lx + 1];
  const float gx = ((((-tl + tr) - 2.0f * ml) + 2.0f * mr) - bl) + br;
  const float gy = ((((-tl - 2.0f * tc) - tr) + bl) + 2.0f * bc) + br;
  return sqrtf(gx * gx + gy * gy);
}

}  // namespace

// MODE: FLIPMode (0 disabled, 1 approx, 2 reference)
template <int MODE>
__global__ void __launch_bounds__(256) k_cmp_metric(const CmpMetricArgs a)
{
  __shared__ float    tile[2][18 * 18];
  __shared__ uint32_t redU[2][4];
  __shared__ double   redD[2][4];
  const int tid = (int)threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int x = (int)blockIdx.x * 16 + tx, y = (int)blockIdx.y * 16 + ty;
  const int W = a.cap.w, H = a.cap.h;

  if(MODE == 1)
  {  // luminance of both images around the workgroup's pixels; outside an image: 0 (never used: the feature is 0 there)
    for(int k = tid; k < 18 * 18; k += 256)
    {
      const int gx = (int)blockIdx.x * 16 - 1 + k % 18, gy = (int)blockIdx.y * 16 - 1 + k / 18;
      tile[0][k]   = lum709(cmpLoadOrZero(a.cap, gx, gy));
      tile[1][k]   = lum709(cmpLoadOrZero(a.cur, gx, gy));
    }
    __syncthreads();
  }

  uint32_t mseFixed = 0, flipFixed = 0;
  double   seD = 0.0, flipD = 0.0;
  if(x < W && y < H)
  {
    const bool   same = a.cur.w == W && a.cur.h == H;
    const float4 ref  = cmpLoad(a.cap, x, y);
    const float  u = ((float)x + 0.5f) / (float)W, v = ((float)y + 0.5f) / (float)H;
    const float4 cur = same ? cmpLoad(a.cur, x, y) : cmpSample(a.cur, u, v);
    const float  dx = ref.x - cur.x, dy = ref.y - cur.y, dz = ref.z - cur.z;
    const float  se = (dx * dx + dy * dy) + dz * dz;
    mseFixed        = toFixed((se / a.divider) * 1000000000.0f);
    seD             = (double)se;
    if(MODE != 0)
    {
      float total;
      if(MODE == 1)
      {  // computeFLIPApprox loads both images at the capture's coordinate
        const float4 curAt      = same ? cur : cmpLoadOrZero(a.cur, x, y);
        const float  colorError = flipColorError(ref, curAt, a);
        float        refFeature = 0.0f, curFeature = 0.0f;
        if(x > 0 && y > 0 && x < W - 1 && y < H - 1)
          refFeature = sobel(tile[0], tx + 1, ty + 1);
        if(x > 0 && y > 0 && x < a.cur.w - 1 && y < a.cur.h - 1)
          curFeature = sobel(tile[1], tx + 1, ty + 1);
        const float featureError = fabsf(refFeature - curFeature) * a.csfEdge;
        total                    = colorError + featureError * 3.83f;
      }
      else
      {
        const float  colorError = flipColorError(ref, cur, a);
        const size_t capN = (size_t)W * (size_t)H, curN = (size_t)a.cur.w * (size_t)a.cur.h;
        const size_t io = (size_t)y * (size_t)W + (size_t)x;
        size_t       co = io;
        if(!same)
        {  // int2(uv * float2(currentSize))
          const int cx = min(max((int)(u * (float)a.cur.w), 0), a.cur.w - 1), cy = min(max((int)(v * (float)a.cur.h), 0), a.cur.h - 1);
          co           = (size_t)cy * (size_t)a.cur.w + (size_t)cx;
        }
        float featureError = 0.0f;
#pragma unroll
        for(int i = 0; i < kCmpChannels; ++i)
          featureError += fabsf(a.featCap[i * capN + io] - a.featCur[i * curN + co]);
        total = colorError + featureError;
      }
      const float powered = powf(saturate(total), 3.0f);
      flipFixed           = toFixed((powered / (a.divider / 3.0f)) * 1000000000.0f);
      flipD               = (double)powered;
    }
  }

  // wave reduction, then across the four waves in wave order
#pragma unroll
  for(int off = 32; off > 0; off >>= 1)
  {
    mseFixed += __shfl_down(mseFixed, off, 64);
    flipFixed += __shfl_down(flipFixed, off, 64);
    seD += __shfl_down(seD, off, 64);
    flipD += __shfl_down(flipD, off, 64);
  }
  const int wave = tid >> 6;
  if((tid & 63) == 0)
  {
    redU[0][wave] = mseFixed;
    redU[1][wave] = flipFixed;
    redD[0][wave] = seD;
    redD[1][wave] = flipD;
  }
  __syncthreads();
  if(tid == 0)
  {
    const uint32_t m = redU[0][0] + redU[0][1] + redU[0][2] + redU[0][3];
    const uint32_t f = redU[1][0] + redU[1][1] + redU[1][2] + redU[1][3];
    if(m)
      atomicAdd(&a.fixed[0], m);
    if(MODE != 0 && f)
      atomicAdd(&a.fixed[2], f);
    const size_t b        = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    a.partials[2 * b]     = ((redD[0][0] + redD[0][1]) + redD[0][2]) + redD[0][3];
    a.partials[2 * b + 1] = ((redD[1][0] + redD[1][1]) + redD[1][2]) + redD[1][3];
  }
}

// the per-workgroup partials in a fixed order: thread t takes t, t + 256, ...; then a fixed tree
__global__ void __launch_bounds__(256) k_cmp_fold(const double* __restrict__ partials, uint32_t blocks, double* __restrict__ out2)
{
  __shared__ double red[2][256];
  double            s0 = 0.0, s1 = 0.0;
  for(uint32_t b = threadIdx.x; b < blocks; b += 256u)
  {
    s0 += partials[2 * (size_t)b];
    s1 += partials[2 * (size_t)b + 1];
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for(uint32_t w = 128; w > 0; w >>= 1)
  {
    if(threadIdx.x < w)
    {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if(threadIdx.x == 0)
  {
    out2[0] = red[0][0];
    out2[1] = red[1][0];
  }
}

__global__ void __launch_bounds__(256) k_cmp_luminance(const CmpImage img, float* __restrict__ lum)
{
  const uint32_t n = (uint32_t)img.w * (uint32_t)img.h;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if(i >= n)
    return;
  const int y = (int)(i / (uint32_t)img.w), x = (int)(i - (uint32_t)y * (uint32_t)img.w);
  lum[i]      = lum709(cmpLoad(img, x, y));
}

// Row pass.  A workgroup takes 1024 consecutive pixels of one row: the segment with a halo of the widest radius sits in LDS, every
// thread sums four outputs (t, t + 256, ...: consecutive lanes read consecutive words) so that a weight is fetched once per four
// taps.  Where x is not interior for a channel a zero is written: the column pass loads those words into its tile and discards the sums.
constexpr int kRowSeg = 1024;
__global__ void __launch_bounds__(256) k_cmp_blur_rows(const float* __restrict__ lum, float* __restrict__ rows, int W, int H, const CmpFlipTab tab)
{
  __shared__ float seg[kRowSeg + 2 * kCmpMaxRadius];
  const int        tid = (int)threadIdx.x;
  const int        y = (int)blockIdx.y, x0 = (int)blockIdx.x * kRowSeg;
  int              R = 0;
  for(int i = 0; i < kCmpChannels; ++i)
    R = max(R, tab.r[i]);  // <= kCmpMaxRadius (checked by the caller)
  const float* row = lum + (size_t)y * (size_t)W;
  for(int k = tid; k < kRowSeg + 2 * R; k += 256)
  {
    const int gx = x0 - R + k;
    seg[k]       = (gx >= 0 && gx < W) ? row[gx] : 0.0f;
  }
  __syncthreads();
  const size_t plane = (size_t)W * (size_t)H;
  for(int i = 0; i < kCmpChannels; ++i)
  {
    const int r = tab.r[i];
    float     acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for(int d = -r; d <= r; ++d)
    {
      const float w = tab.w[i][d < 0 ? -d : d];
#pragma unroll
      for(int j = 0; j < 4; ++j)
        acc[j] += seg[tid + j * 256 + R + d] * w;
    }
#pragma unroll
    for(int j = 0; j < 4; ++j)
    {
      const int x = x0 + tid + j * 256;
      if(x < W)  // within r of the left or right border the pixel is never interior: a defined value the column pass may load
        rows[i * plane + (size_t)y * (size_t)W + (size_t)x] = (x >= r && x < W - r) ? acc[j] : 0.0f;
    }
  }
}

// Column pass and feature.  A workgroup takes 64 columns x 64 rows; per channel the row-pass plane's tile with a halo of r rows sits
// in LDS (lanes = columns: conflict-free), every wave sums sixteen rows with a weight fetched once per sixteen taps.  Then the
// border rule (applyGaussianFilter, :228-234: within r of any border the blurred value is the centre's own luminance), the
// normalisation and the CSF (:290-297).
constexpr int kColTile = 64;
__global__ void __launch_bounds__(256) k_cmp_blur_cols(const float* __restrict__ rows, const float* __restrict__ lum, float* __restrict__ feat, int W, int H,
                                                       const CmpFlipTab tab)
{
  extern __shared__ float tile[];  // (kColTile + 2 * widest radius of this call) rows of 64 columns: 49.7 KB at r = 65
  const int        lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int        x = (int)blockIdx.x * 64 + lane, y0 = (int)blockIdx.y * kColTile;
  const size_t     plane = (size_t)W * (size_t)H;
  for(int i = 0; i < kCmpChannels; ++i)
  {
    const int    r = tab.r[i];
    const float* src = rows + i * plane;
    __syncthreads();  // the previous channel's tile has been read
    for(int k = wave; k < kColTile + 2 * r; k += 4)
    {
      const int gy       = y0 - r + k;
      tile[k * 64 + lane] = (gy >= 0 && gy < H && x < W) ? src[(size_t)gy * (size_t)W + (size_t)x] : 0.0f;
    }
    __syncthreads();
    float acc[16];
#pragma unroll
    for(int j = 0; j < 16; ++j)
      acc[j] = 0.0f;
    for(int d = -r; d <= r; ++d)
    {
      const float  w = tab.w[i][d < 0 ? -d : d];
      const float* t = &tile[(wave * 16 + r + d) * 64 + lane];
#pragma unroll
      for(int j = 0; j < 16; ++j)
        acc[j] += t[j * 64] * w;
    }
    const float norm = tab.norm[i], csf = tab.csf[i];
#pragma unroll
    for(int j = 0; j < 16; ++j)
    {
      const int y = y0 + wave * 16 + j;
      if(x < W && y < H)
      {
        const size_t o        = (size_t)y * (size_t)W + (size_t)x;
        const float  centre   = lum[o];
        const bool   interior = x >= r && y >= r && x < W - r && y < H - r;
        const float  blurred  = interior ? acc[j] / norm : centre;
        feat[i * plane + o]   = fabsf(centre - blurred) * csf;
      }
    }
  }
}

namespace {

// sampleImage (image_compare_composite.comp.slang:257-267)
__device__ __forceinline__ float4 sampleImage(const CmpImage& im, int x, int y, float u, float v, int outW, int outH)
{
  if(im.w == outW && im.h == outH)
    return cmpLoad(im, x, y);
  return cmpSample(im, u, v);
}

// computeMultiScaleContrast (:186-229), at the OUTPUT pixel's coordinate in the image's own size, as written
__device__ __forceinline__ float multiScaleContrast(const CmpImage& im, int x, int y)
{
  if(x < 2 || y < 2 || x >= im.w - 2 || y >= im.h - 2)
    return 0.0f;
  auto  L = [&](int ox, int oy) { return lum709(cmpLoad(im, x + ox, y + oy)); };
  float total = 0.0f;
  {
    const float gx = fabsf(L(1, 0) - L(-1, 0)), gy = fabsf(L(0, -1) - L(0, 1));
    total += sqrtf(gx * gx + gy * gy) * 0.5f;
  }
  {
    const float gx = fabsf(L(2, 0) - L(-2, 0)) * 0.5f, gy = fabsf(L(0, -2) - L(0, 2)) * 0.5f;
    total += sqrtf(gx * gx + gy * gy) * 0.3f;
  }
  {
    const float g1 = fabsf(L(1, -1) - L(-1, 1)), g2 = fabsf(L(-1, -1) - L(1, 1));
    total += sqrtf(g1 * g1 + g2 * g2) * 0.2f;
  }
  return total;
}

// rgbToOpponentColor (color.h.slang:54-78)
__device__ __forceinline__ C3 opponent(float4 srgb)
{
  const float r = srgbToLinear1(srgb.x), g = srgbToLinear1(srgb.y), b = srgbToLinear1(srgb.z);
  const float X = (r * 0.4124564f + g * 0.3575761f) + b * 0.1804375f;
  const float Y = (r * 0.2126729f + g * 0.7151522f) + b * 0.0721750f;
  const float Z = (r * 0.0193339f + g * 0.1191920f) + b * 0.9503041f;
  const float Ystar = (Y > 0.008856f) ? powf(Y, 1.0f / 3.0f) : (7.787f * Y + 16.0f / 116.0f);
  return {Ystar, (X - Y) * 0.5f, (Y - Z) * 0.3f};
}

// turboColormap (color.h.slang:148-162)
__device__ __forceinline__ C3 turbo(float x)
{
  x = saturate(x);
  const float v1 = x, v2 = x * x, v3 = x * x * x;
  const float a = v2 * v2, b = v3 * v2;
  auto        d4 = [&](float c0, float c1, float c2, float c3) { return ((1.0f * c0 + v1 * c1) + v2 * c2) + v3 * c3; };
  auto        d2 = [&](float c0, float c1) { return a * c0 + b * c1; };
  return {d4(0.13572138f, 4.61539260f, -42.66032258f, 132.13108234f) + d2(-152.94239396f, 59.28637943f),
          d4(0.09140261f, 2.19418839f, 4.84296658f, -14.18503333f) + d2(4.27729857f, 2.82956604f),
          d4(0.10667330f, 12.64194608f, -60.58204836f, 110.36276771f) + d2(-89.90310912f, 27.34824973f)};
}

__device__ float4 displayColor(const CmpCompositeArgs& a, int mode, int x, int y, float u, float v)
{
  if(mode == 0)
    return sampleImage(a.cap, x, y, u, v, a.outW, a.outH);
  if(mode == 1)
    return sampleImage(a.cur, x, y, u, v, a.outW, a.outH);
  const float4 ref = sampleImage(a.cap, x, y, u, v, a.outW, a.outH);
  const float4 cur = sampleImage(a.cur, x, y, u, v, a.outW, a.outH);
  if(mode == 2)
    return make_float4(fminf(fabsf(ref.x - cur.x) * a.amplify, 1.0f), fminf(fabsf(ref.y - cur.y) * a.amplify, 1.0f),
                       fminf(fabsf(ref.z - cur.z) * a.amplify, 1.0f), 1.0f);
  if(mode == 3 || mode == 4)
  {
    float intensity = (fabsf(ref.x - cur.x) * 0.299f + fabsf(ref.y - cur.y) * 0.587f) + fabsf(ref.z - cur.z) * 0.114f;
    intensity       = fminf(intensity * a.amplify, 1.0f);
    if(mode == 4)
      return make_float4(intensity, 0.0f, 0.0f, 1.0f);
    const float gray = (cur.x * 0.299f + cur.y * 0.587f) + cur.z * 0.114f;
    // lerp(gray, (1, 0, 0), intensity) = a + (b - a) * t
    return make_float4(gray + (1.0f - gray) * intensity, gray + (0.0f - gray) * intensity, gray + (0.0f - gray) * intensity, 1.0f);
  }
  // eFLIPError: the composite shader's own computeFLIP (:233-254)
  const float refContrast = multiScaleContrast(a.cap, x, y);
  const float curContrast = multiScaleContrast(a.cur, x, y);
  const C3    p = opponent(ref), q = opponent(cur);
  const float lumDiff = fabsf(p.x - q.x);
  const float cy = p.y - q.y, cz = p.z - q.z;
  const float chromaDiff = sqrtf(cy * cy + cz * cz);
  const float colorError = lumDiff * 0.75f + chromaDiff * 0.25f;
  const float avgContrast = (refContrast + curContrast) * 0.5f;
  const float sensitivity = 1.0f / (1.0f + avgContrast * 8.0f);
  const float edgeMasking = 1.0f - saturate(fmaxf(refContrast, curContrast) * 4.0f);
  float       e = (colorError * (0.4f + 0.6f * sensitivity)) * (0.3f + 0.7f * edgeMasking);
  e           = powf(saturate(e), 0.75f);
  const C3 h  = turbo(e);
  return make_float4(h.x, h.y, h.z, 1.0f);
}

}  // namespace

__global__ void __launch_bounds__(256) k_cmp_composite(const CmpCompositeArgs a)
{
  const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
  if(x >= a.outW || y >= a.outH)
    return;
  const int splitPos = (int)(a.split * (float)a.outW);
  const int dist     = abs(x - splitPos);
  float4    color;
  if(dist <= 2)
    color = dist <= 0 ? make_float4(1.0f, 1.0f, 1.0f, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  else
  {
    const float u = ((float)x + 0.5f) / (float)a.outW, v = ((float)y + 0.5f) / (float)a.outH;
    color         = displayColor(a, x < splitPos ? a.left : a.right, x, y, u, v);
  }
  a.out[(size_t)y * (size_t)a.outW + (size_t)x] = color;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
void launchCmpMetric(hipStream_t stream, const CmpMetricArgs& a, int flipMode, uint32_t blocksX, uint32_t blocksY)
{
  const dim3 grid(blocksX, blocksY), block(256);
  if(flipMode == 1)
    hipLaunchKernelGGL(k_cmp_metric<1>, grid, block, 0, stream, a);
  else if(flipMode == 2)
    hipLaunchKernelGGL(k_cmp_metric<2>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(k_cmp_metric<0>, grid, block, 0, stream, a);
}
void launchCmpFold(hipStream_t stream, const double* partials, uint32_t blocks, double* out2)
{
  hipLaunchKernelGGL(k_cmp_fold, dim3(1), dim3(256), 0, stream, partials, blocks, out2);
}
void launchCmpLuminance(hipStream_t stream, const CmpImage& img, float* lum)
{
  const uint32_t n = (uint32_t)img.w * (uint32_t)img.h;
  hipLaunchKernelGGL(k_cmp_luminance, dim3((n + 255u) / 256u), dim3(256), 0, stream, img, lum);
}
void launchCmpBlurRows(hipStream_t stream, const float* lum, float* rows, int w, int h, const CmpFlipTab& tab)
{
  hipLaunchKernelGGL(k_cmp_blur_rows, dim3((uint32_t)(w + kRowSeg - 1) / kRowSeg, (uint32_t)h), dim3(256), 0, stream, lum, rows, w, h, tab);
}
void launchCmpBlurCols(hipStream_t stream, const float* rows, const float* lum, float* feat, int w, int h, const CmpFlipTab& tab)
{
  int R = 0;
  for(int i = 0; i < kCmpChannels; ++i)
    R = R > tab.r[i] ? R : tab.r[i];  // <= kCmpMaxRadius (checked by the caller): at most 64 KB
  const size_t lds = (size_t)(kColTile + 2 * R) * 64 * sizeof(float);
  hipLaunchKernelGGL(k_cmp_blur_cols, dim3((uint32_t)(w + 63) / 64, (uint32_t)(h + kColTile - 1) / kColTile), dim3(256), lds, stream, rows, lum, feat, w, h, tab);
}
void launchCmpComposite(hipStream_t stream, const CmpCompositeArgs& a)
{
  hipLaunchKernelGGL(k_cmp_composite, dim3((uint32_t)(a.outW + 63) / 64, (uint32_t)(a.outH + 3) / 4), dim3(256), 0, stream, a);
}

}  // namespace mgs
