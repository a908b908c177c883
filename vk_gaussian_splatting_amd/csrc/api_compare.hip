// api_compare.hip — runtime image comparison (mgs_compare_*): orchestration of the kernels of k_compare.hip.
#include <cmath>

#include "scene_state.h"

// (ImageCompare, src/image_compare.cpp)
// The capture, the planes of the FLIP reference passes and the composite output belong to the handle; nothing here is touched by
// a frame, and a frame touches nothing here.
// (CmpImage::fmt is the compositors' output mode, targetLayout().fmt; a capture keeps its pixel size next to it)

// the handle's last complete frame as a compare image, or the reason there is none
static int cmpCurrentImage(MgsScene s, const char* who, CmpImage& img)
{
  if(!s->last.have || s->last.wasSortOnly)
  {
    setError(std::string(who) + ": no frame rendered yet");
    return MGS_ERR_STATE;
  }
  const MgsFrameParams& q = s->last.params;
  if(q.strip_row_begin != 0 || q.strip_row_end * kTilePx < q.height)
  {
    setError(std::string(who) + ": the last frame was a strip-only mgs_render; the frame buffer holds only some rows");
    return MGS_ERR_STATE;
  }
  img.p   = s->fb.image.p;
  img.w   = q.width;
  img.h   = q.height;
  img.fmt = targetLayout(q.target_format).fmt;
  return MGS_OK;
}

static int mgs_compare_capture_impl(MgsScene s)
{
  if(!s)
  {
    setError("mgs_compare_capture: null handle");
    return MGS_ERR_INVALID_ARG;
  }
  CmpImage cur{};
  if(int rc = cmpCurrentImage(s, "mgs_compare_capture", cur))
    return rc;
  HIPCHK(hipSetDevice(s->device));
  const size_t bytes = (size_t)cur.w * (size_t)cur.h * targetLayout(s->last.params.target_format).pixelBytes;
  if(bytes > s->cmp.capture.n)
    HIPCHK(hipStreamSynchronize(s->stream));  // a composite in flight may still read the copy that is about to be freed
  if(int rc = s->cmp.capture.ensure(bytes))
    return rc;
  HIPCHK(hipMemcpyAsync(s->cmp.capture.p, cur.p, bytes, hipMemcpyDeviceToDevice, s->stream));
  s->cmp.cap        = cur;
  s->cmp.cap.p      = s->cmp.capture.p;
  s->cmp.haveCapture = true;
  return MGS_OK;
}
int mgs_compare_capture(MgsScene s)
{
  return guarded("mgs_compare_capture", [&] { return mgs_compare_capture_impl(s); });
}

static int mgs_compare_capture_upload_impl(MgsScene s, const float* rgbaHost, int width, int height)
{
  if(!s || !rgbaHost || width <= 0 || height <= 0 || (uint64_t)width * (uint64_t)height > 0x7FFFFFFFull / 16)
  {
    setError(!s ? "mgs_compare_capture_upload: null handle" : "mgs_compare_capture_upload: bad argument");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  const size_t bytes = (size_t)width * (size_t)height * 16;
  HIPCHK(hipStreamSynchronize(s->stream));  // whatever still reads the previous capture
  if(int rc = s->cmp.capture.ensure(bytes))
    return rc;
  HIPCHK(hipMemcpy(s->cmp.capture.p, rgbaHost, bytes, hipMemcpyHostToDevice));
  s->cmp.cap         = CmpImage{s->cmp.capture.p, width, height, 0};
  s->cmp.haveCapture = true;
  return MGS_OK;
}
int mgs_compare_capture_upload(MgsScene s, const float* rgbaHost, int width, int height)
{
  return guarded("mgs_compare_capture_upload", [&] { return mgs_compare_capture_upload_impl(s, rgbaHost, width, height); });
}

static int mgs_compare_release_impl(MgsScene s)
{
  if(!s)
  {
    setError("mgs_compare_release: null handle");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->cmp.releaseBuffers();
  s->cmp.haveCapture = false;
  s->cmp.outW = s->cmp.outH = 0;
  return MGS_OK;
}
int mgs_compare_release(MgsScene s)
{
  return guarded("mgs_compare_release", [&] { return mgs_compare_release_impl(s); });
}

void mgs_compare_params_default(MgsCompareParams* p)
{
  if(!p)
    return;
  p->flip_mode         = MGS_FLIP_REFERENCE;  // PushConstantMetrics
  p->pixels_per_degree = 67.0f;               // image_compare.cpp:788
}

void mgs_compare_view_default(MgsCompareView* v)
{
  if(!v)
    return;
  v->split_position     = 0.5f;
  v->left               = MGS_COMPARE_SHOW_CAPTURE;
  v->right              = MGS_COMPARE_SHOW_CURRENT;
  v->difference_amplify = 5.0f;
  v->width = v->height = 0;
}

// csfLuminance (image_compare_metric.comp.slang:198-208) in fp32
static float cmpCsfLuminance(float freq)
{
  const float s = 1.0f / std::sqrt(1.0f + std::pow(freq / 4.0f, 2.0f));
  return s * std::exp(-0.5f * freq);
}

static int mgs_compare_metrics_impl(MgsScene s, const MgsCompareParams* p, MgsCompareMetrics* out)
{
  if(!s || !out)
  {
    setError(!s ? "mgs_compare_metrics: null handle" : "mgs_compare_metrics: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  MgsCompareParams q;
  mgs_compare_params_default(&q);
  if(p)
    q = *p;
  if(q.flip_mode < MGS_FLIP_DISABLED || q.flip_mode > MGS_FLIP_REFERENCE || !(q.pixels_per_degree > 0.0f) || !std::isfinite(q.pixels_per_degree))
  {
    setError("mgs_compare_metrics: flip_mode must be MGS_FLIP_DISABLED / APPROX / REFERENCE and pixels_per_degree positive");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->cmp.haveCapture)
  {
    setError("mgs_compare_metrics: no capture held (mgs_compare_capture / mgs_compare_capture_upload)");
    return MGS_ERR_STATE;
  }
  CmpImage cur{};
  if(int rc = cmpCurrentImage(s, "mgs_compare_metrics", cur))
    return rc;
  const CmpImage cap = s->cmp.cap;
  HIPCHK(hipSetDevice(s->device));

  CmpMetricArgs a{};
  a.cap     = cap;
  a.cur     = cur;
  a.divider = float(cap.w * cap.h * 3);  // image_compare.cpp:783
  a.csfY    = cmpCsfLuminance(1.0f);
  a.csfC    = a.csfY * 0.4f;  // csfChrominance
  a.csfEdge = cmpCsfLuminance(4.0f);
  {  // huntAdjustment at adaptation luminance 1 (color.h.slang:101-115)
    const float k = 5.0f * 1.0f, kCbrt = std::pow(k, 1.0f / 3.0f);
    a.huntFL = 0.2f * kCbrt * (1.0f - std::exp(-0.42f * kCbrt));
  }
  const size_t capN = (size_t)cap.w * (size_t)cap.h, curN = (size_t)cur.w * (size_t)cur.h;
  std::unique_ptr<CmpFlipTab> tab;
  if(q.flip_mode == MGS_FLIP_REFERENCE)
  {
    tab.reset(new CmpFlipTab());
    std::memset(tab.get(), 0, sizeof(CmpFlipTab));
    const float freq[kCmpChannels] = {0.5f, 1.0f, 2.0f, 4.0f, 8.0f};
    for(int i = 0; i < kCmpChannels; ++i)
    {
      float sigma = q.pixels_per_degree / (freq[i] * 6.28f);
      sigma       = std::max(sigma, 0.5f);
      const float rf = std::ceil(3.0f * sigma);
      if(!(rf <= (float)kCmpMaxRadius))
      {
        setError("mgs_compare_metrics: pixels_per_degree gives a filter radius above " + std::to_string(kCmpMaxRadius) + ", which this build does not hold");
        return MGS_ERR_UNSUPPORTED;
      }
      tab->r[i]   = (int)rf;
      tab->csf[i] = cmpCsfLuminance(freq[i]);
      float wsum  = 0.0f;
      for(int d = -tab->r[i]; d <= tab->r[i]; ++d)
      {
        const float x = (float)d;
        const float w = std::exp(-(x * x) / (2.0f * sigma * sigma));  // gaussianWeight
        tab->w[i][d < 0 ? -d : d] = w;
        wsum += w;
      }
      tab->norm[i] = wsum * wsum;
    }
    // planes: luminance of both images, the row pass's five planes (shared by the two images), five feature planes each
    const size_t need = capN + curN + kCmpChannels * std::max(capN, curN) + kCmpChannels * (capN + curN);
    if(need > s->cmp.planes.n)
      HIPCHK(hipStreamSynchronize(s->stream));
    if(int rc = s->cmp.planes.ensure(need))
      return rc;
  }
  const uint32_t bx = (uint32_t)(cap.w + 15) / 16, by = (uint32_t)(cap.h + 15) / 16;
  if(int rc = s->cmp.partials.ensure(2 * (size_t)bx * by + 2))
    return rc;
  if(int rc = s->cmp.fixed.ensure(4))
    return rc;
  if(!s->cmp.ev[0])
  {
    HIPCHK(hipEventCreate(&s->cmp.ev[0]));
    HIPCHK(hipEventCreate(&s->cmp.ev[1]));
  }
  a.fixed    = s->cmp.fixed.p;
  a.partials = s->cmp.partials.p + 2;  // [0..1]: the folded sums
  hipStream_t st = s->stream;
  HIPCHK(hipEventRecord(s->cmp.ev[0], st));
  HIPCHK(hipMemsetAsync(s->cmp.fixed.p, 0, 4 * sizeof(uint32_t), st));  // vkCmdFillBuffer, image_compare.cpp:765
  if(q.flip_mode == MGS_FLIP_REFERENCE)
  {
    float* lumCap  = s->cmp.planes.p;
    float* lumCur  = lumCap + capN;
    float* rows    = lumCur + curN;
    float* featCap = rows + kCmpChannels * std::max(capN, curN);
    float* featCur = featCap + kCmpChannels * capN;
    launchCmpLuminance(st, cap, lumCap);
    launchCmpLuminance(st, cur, lumCur);
    launchCmpBlurRows(st, lumCap, rows, cap.w, cap.h, *tab);
    launchCmpBlurCols(st, rows, lumCap, featCap, cap.w, cap.h, *tab);
    launchCmpBlurRows(st, lumCur, rows, cur.w, cur.h, *tab);
    launchCmpBlurCols(st, rows, lumCur, featCur, cur.w, cur.h, *tab);
    a.featCap = featCap;
    a.featCur = featCur;
  }
  launchCmpMetric(st, a, q.flip_mode, bx, by);
  launchCmpFold(st, a.partials, bx * by, s->cmp.partials.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(s->cmp.ev[1], st));
  uint32_t fixed[4] = {};
  double   sums[2]  = {};
  HIPCHK(hipMemcpyAsync(fixed, s->cmp.fixed.p, sizeof(fixed), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(sums, s->cmp.partials.p, sizeof(sums), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));

  std::memset(out, 0, sizeof(*out));
  HIPCHK(hipEventElapsedTime(&out->elapsed_ms, s->cmp.ev[0], s->cmp.ev[1]));
  // collectMetricsResult, image_compare.cpp:869-906
  out->mse_fixed  = fixed[0];
  out->flip_fixed = fixed[2];
  out->mse        = (float)fixed[0] / 1000000000.0f;
  out->psnr       = out->mse < 1e-10f ? 99.99f : std::min(10.0f * std::log10(1.0f / out->mse), 99.99f);
  out->flip       = (float)std::pow((double)fixed[2] / 1000000000.0, 1.0 / 3.0);
  out->mse_exact  = sums[0] / ((double)cap.w * (double)cap.h * 3.0);
  out->psnr_exact = out->mse_exact > 0.0 ? 10.0 * std::log10(1.0 / out->mse_exact) : HUGE_VAL;
  out->flip_exact = q.flip_mode == MGS_FLIP_DISABLED ? 0.0 : std::pow(sums[1] / ((double)cap.w * (double)cap.h), 1.0 / 3.0);
  return MGS_OK;
}
int mgs_compare_metrics(MgsScene s, const MgsCompareParams* p, MgsCompareMetrics* out)
{
  return guarded("mgs_compare_metrics", [&] { return mgs_compare_metrics_impl(s, p, out); });
}

static int mgs_compare_composite_impl(MgsScene s, const MgsCompareView* view, void** deviceOut, uint64_t* bytes)
{
  if(!s)
  {
    setError("mgs_compare_composite: null handle");
    return MGS_ERR_INVALID_ARG;
  }
  MgsCompareView v;
  mgs_compare_view_default(&v);
  if(view)
    v = *view;
  if(v.left < 0 || v.left > MGS_COMPARE_SHOW_FLIP || v.right < 0 || v.right > MGS_COMPARE_SHOW_FLIP || v.width < 0 || v.height < 0
     || (v.width == 0) != (v.height == 0) || !std::isfinite(v.split_position) || !std::isfinite(v.difference_amplify)
     || (uint64_t)v.width * (uint64_t)v.height > 0x7FFFFFFFull / 16)
  {
    setError("mgs_compare_composite: display modes must be MGS_COMPARE_SHOW_*, the output size non-negative (both 0 or both set)");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->cmp.haveCapture)
  {
    setError("mgs_compare_composite: no capture held (mgs_compare_capture / mgs_compare_capture_upload)");
    return MGS_ERR_STATE;
  }
  CmpImage cur{};
  if(int rc = cmpCurrentImage(s, "mgs_compare_composite", cur))
    return rc;
  HIPCHK(hipSetDevice(s->device));
  CmpCompositeArgs a{};
  a.cap  = s->cmp.cap;
  a.cur  = cur;
  a.outW = v.width ? v.width : cur.w;
  a.outH = v.height ? v.height : cur.h;
  const size_t n = (size_t)a.outW * (size_t)a.outH;
  if(n > s->cmp.out.n)
    HIPCHK(hipStreamSynchronize(s->stream));
  if(int rc = s->cmp.out.ensure(n))
    return rc;
  a.out     = s->cmp.out.p;
  a.split   = v.split_position;
  a.amplify = v.difference_amplify;
  a.left    = v.left;
  a.right   = v.right;
  launchCmpComposite(s->stream, a);
  HIPCHK(hipGetLastError());
  s->cmp.outW = a.outW;
  s->cmp.outH = a.outH;
  if(deviceOut)
    *deviceOut = s->cmp.out.p;
  if(bytes)
    *bytes = (uint64_t)n * sizeof(float4);
  return MGS_OK;
}
int mgs_compare_composite(MgsScene s, const MgsCompareView* view, void** deviceOut, uint64_t* bytes)
{
  return guarded("mgs_compare_composite", [&] { return mgs_compare_composite_impl(s, view, deviceOut, bytes); });
}

static int mgs_compare_download_composite_impl(MgsScene s, void* dst, size_t bytes)
{
  if(!s || !dst)
  {
    setError(!s ? "mgs_compare_download_composite: null handle" : "mgs_compare_download_composite: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->cmp.outW)
  {
    setError("mgs_compare_download_composite: no composite built yet (mgs_compare_composite)");
    return MGS_ERR_STATE;
  }
  const size_t n = (size_t)s->cmp.outW * (size_t)s->cmp.outH * sizeof(float4);
  if(bytes < n)
  {
    setError("mgs_compare_download_composite: destination too small");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(dst, s->cmp.out.p, n, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}
int mgs_compare_download_composite(MgsScene s, void* dst, size_t bytes)
{
  return guarded("mgs_compare_download_composite", [&] { return mgs_compare_download_composite_impl(s, dst, bytes); });
}
