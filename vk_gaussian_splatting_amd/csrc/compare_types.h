// compare_types.h — launch arguments of the image-compare kernels (k_compare.hip), shared with api_compare.hip.
#pragma once
#include <stdint.h>

namespace mgs {

constexpr int kCmpMaxRadius = 96;  // widest FLIP reference filter this build holds in LDS (r = 65 at 67 pixels per degree)
constexpr int kCmpChannels  = 5;   // frequency channels of computeSpatialFeatures: 0.5, 1, 2, 4, 8 cycles per degree

// an image as stored: fmt 0 RGBA32F, 1 RGBA16F, 2 RGBA8 UNORM (the compositors' numbering), [h][w] pixels
struct CmpImage
{
  const void* p;
  int         w, h, fmt;
};

// what depends on pixels-per-degree only, computed once per call on the host in fp32 with the shader's operations
struct CmpFlipTab
{
  int   r[kCmpChannels];                      // ceil(3 sigma)
  float csf[kCmpChannels];                    // csfLuminance(f)
  float norm[kCmpChannels];                   // (sum of the 1-D weights)^2
  float w[kCmpChannels][kCmpMaxRadius + 1];   // gaussianWeight(|d|, sigma)
};

struct CmpMetricArgs
{
  CmpImage     cap, cur;
  float        divider;            // float(W * H * 3)
  float        csfY, csfC;         // csfLuminance(1), csfChrominance(1)
  float        csfEdge;            // csfLuminance(4)
  float        huntFL;             // huntAdjustment's factor at adaptation luminance 1
  float        csfRef[kCmpChannels];
  uint32_t*    fixed;              // [0] MSE sum, [2] FLIP sum (the reference's result buffer layout)
  double*      partials;           // [blocks][2]: per-workgroup sums of squared error and of FLIP powered error
  const float* featCap;            // reference mode: [5][cap.h][cap.w] features of the capture ...
  const float* featCur;            // ... and [5][cur.h][cur.w] of the current image
};

struct CmpCompositeArgs
{
  CmpImage cap, cur;
  float4*  out;
  int      outW, outH;
  float    split, amplify;
  int      left, right;
};

void launchCmpMetric(hipStream_t stream, const CmpMetricArgs& a, int flipMode, uint32_t blocksX, uint32_t blocksY);
void launchCmpFold(hipStream_t stream, const double* partials, uint32_t blocks, double* out2);
void launchCmpLuminance(hipStream_t stream, const CmpImage& img, float* lum);
void launchCmpBlurRows(hipStream_t stream, const float* lum, float* rows, int w, int h, const CmpFlipTab& tab);
void launchCmpBlurCols(hipStream_t stream, const float* rows, const float* lum, float* feat, int w, int h, const CmpFlipTab& tab);
void launchCmpComposite(hipStream_t stream, const CmpCompositeArgs& a);

}  // namespace mgs
