// api_frameargs.hip — a frame's parameters: their defaults, and the constants the kernels read, built from them (buildFrameArgs).
#include <cmath>
#include <cstddef>
#include <string>

#include "scene_state.h"

void mgs_frame_params_default(MgsFrameParams* p)
{
  if(!p)
    return;
  std::memset(p, 0, sizeof(*p));
  const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(p->view, id, sizeof(id));
  std::memcpy(p->proj, id, sizeof(id));
  p->width                = 1920;
  p->height               = 1080;
  p->splat_scale          = 1.0f;
  p->frustum_dilation     = 0.2f;
  p->alpha_cull_threshold = 1.0f / 255.0f;
  p->sh_degree            = 3;
  p->sort_mode            = MGS_SORT_GPU_RADIX;
  p->frustum_culling      = MGS_CULL_AT_DIST;
  p->target_format        = MGS_TARGET_RGBA16F;
  p->alpha_mode           = MGS_ALPHA_COVERAGE;
  p->size_culling_min_pixels = 1.0f;
  p->cpu_lazy_sort           = 1;     // parameters.h:183
  p->thin_particle_threshold = 1e-6f; // parameters.h:163
  p->quantize_normals        = 1;     // parameters.h:195
  p->pipeline                = MGS_PIPELINE_3DGS;
  p->camera_model            = MGS_CAMERA_PINHOLE;
  p->extent_method           = MGS_EXTENT_CONIC;  // parameters.h:190 (read by the 3DGUT pipeline only)
  p->fov_rad                 = 0.0f;
  p->alpha_clamp             = 0.99f;    // shaderio.h:271
  p->kernel_min_response     = 0.0113f;  // parameters.h:216
  p->surface_outputs         = 0;
  p->depth_iso_threshold     = 0.7f;  // parameters.h:200
  p->dof_mode                = MGS_DOF_DISABLED;
  p->focus_dist              = 1.3f;    // shaderio.h:278
  p->aperture                = 0.001f;  // shaderio.h:279
  p->frame_sample_id         = 0;
  p->temporal_sampling       = 0;
  p->kernel_degree           = 2;       // parameters.h:215
  p->normal_method           = MGS_NORMAL_MAX_DENSITY_PLANE;  // parameters.h:162
  p->lighting_mode           = MGS_LIGHTING_DISABLED;
}

// inverse of a glm column-major 4x4 in double (Gauss-Jordan with partial pivoting), rounded once to fp32
void mat4InverseDouble(const float m[16], float out[16])
{
  double a[4][8];
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c)
    {
      a[r][c]     = (double)m[c * 4 + r];
      a[r][4 + c] = r == c ? 1.0 : 0.0;
    }
  for(int k = 0; k < 4; ++k)
  {
    int piv = k;
    for(int r = k + 1; r < 4; ++r)
      if(std::fabs(a[r][k]) > std::fabs(a[piv][k]))
        piv = r;
    if(piv != k)
      for(int c = 0; c < 8; ++c)
        std::swap(a[k][c], a[piv][c]);
    const double d = 1.0 / a[k][k];
    for(int c = 0; c < 8; ++c)
      a[k][c] *= d;
    for(int r = 0; r < 4; ++r)
      if(r != k)
      {
        const double f = a[r][k];
        for(int c = 0; c < 8; ++c)
          a[r][c] -= f * a[k][c];
      }
  }
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c)
      out[c * 4 + r] = (float)a[r][4 + c];
}

// ---- sensor models (mgs_frame_set_sensor) -------------------------------------------------------------------------------------
// computeMaxAngle, threedgut_camera_models.h.slang:87-119
static float sensorMaxAngle(float w, float h, const float pp[2], const float f[2])
{
  const float mdx = pp[0] > 0.5f * w ? pp[0] : w - pp[0], mdy = pp[1] > 0.5f * h ? pp[1] : h - pp[1];
  const float maxR = std::sqrt(mdx * mdx + mdy * mdy);
  return std::max(2.0f * maxR / f[0], 2.0f * maxR / f[1]) / 2.0f;
}
// frameInfo.focal of the 3DGUT pipelines (gaussian_splatting.cpp:1239-1251) and the field of view it is derived from
static void gutFocalOf(const MgsFrameParams* p, float focal[2], float* fovRad)
{
  *fovRad = p->fov_rad > 0.0f ? p->fov_rad : 2.0f * std::atan(1.0f / std::fabs(p->proj[5]));
  if(p->camera_model == MGS_CAMERA_FISHEYE && p->pipeline == MGS_PIPELINE_3DGUT)
  {
    focal[0] = (float)p->width / *fovRad;
    focal[1] = -(float)p->height / *fovRad;
  }
  else
  {
    focal[0] = p->proj[0] * 0.5f * (float)p->width;
    focal[1] = p->proj[5] * 0.5f * (float)p->height;
  }
}

int mgs_sensor_model_from_frame(const MgsFrameParams* p, MgsSensorModel* out)
{
  if(!p || !out)
  {
    setError("mgs_sensor_model_from_frame: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(p->width <= 0 || p->height <= 0 || p->width > 8192 || p->height > 8192 || p->camera_model < MGS_CAMERA_PINHOLE || p->camera_model > MGS_CAMERA_FISHEYE)
  {
    setError("mgs_sensor_model_from_frame: width/height must be in [1,8192] and camera_model one of MGS_CAMERA_*");
    return MGS_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  MgsFrameParams q = *p;
  q.pipeline       = MGS_PIPELINE_3DGUT;  // the sensor is the 3DGUT pipeline's: a fisheye frame's focal length is the fisheye one
  float fov;
  gutFocalOf(&q, out->focal_length, &fov);
  out->model              = p->camera_model == MGS_CAMERA_FISHEYE ? MGS_SENSOR_OPENCV_FISHEYE : MGS_SENSOR_OPENCV_PINHOLE;
  out->principal_point[0] = (float)p->width * 0.5f;
  out->principal_point[1] = (float)p->height * 0.5f;
  out->max_angle          = sensorMaxAngle((float)p->width, (float)p->height, out->principal_point, out->focal_length);
  return MGS_OK;
}

int mgs_frame_set_sensor(MgsScene s, const MgsSensorModel* m)
{
  if(m)
  {  // (before the handle is looked at)
    if(m->model < MGS_SENSOR_OPENCV_PINHOLE || m->model > MGS_SENSOR_OPENCV_FISHEYE)
    {
      setError("mgs_frame_set_sensor: model must be MGS_SENSOR_OPENCV_PINHOLE or MGS_SENSOR_OPENCV_FISHEYE");
      return MGS_ERR_INVALID_ARG;
    }
    if(m->shutter < 0 || m->shutter > 4)
    {
      setError("mgs_frame_set_sensor: shutter out of range");
      return MGS_ERR_INVALID_ARG;
    }
    const float* f = m->focal_length;  // the 21 floats from focal_length to max_angle are contiguous
    static_assert(offsetof(MgsSensorModel, max_angle) - offsetof(MgsSensorModel, focal_length) == 20 * sizeof(float), "float block");
    for(int i = 0; i < 21; ++i)
      if(!std::isfinite(f[i]))
      {
        setError("mgs_frame_set_sensor: every value must be finite");
        return MGS_ERR_INVALID_ARG;
      }
    if(m->focal_length[0] == 0.0f || m->focal_length[1] == 0.0f || m->max_angle < 0.0f)
    {
      setError("mgs_frame_set_sensor: focal_length must be non-zero and max_angle >= 0");
      return MGS_ERR_INVALID_ARG;
    }
    for(uint32_t r : m->reserved)
      if(r != 0u)
      {
        setError("mgs_frame_set_sensor: reserved words must be 0");
        return MGS_ERR_INVALID_ARG;
      }
    if(m->shutter != 0)
    {
      setError("mgs_frame_set_sensor: rolling shutters are not supported (the reference marks that code untested); shutter must be 0");
      return MGS_ERR_UNSUPPORTED;
    }
  }
  if(!s)
  {
    setError("mgs_frame_set_sensor: null scene");
    return MGS_ERR_INVALID_ARG;
  }
  s->sensor.bound = m != nullptr;
  if(m)
    s->sensor.model = *m;
  return MGS_OK;
}

int refuseBoundSensor(MgsScene s, const char* what, const char* why)
{
  if(!s->sensor.bound)
    return MGS_OK;
  setError(std::string(what) + ": a sensor model is bound (" + why + "); unbind it with mgs_frame_set_sensor(handle, NULL)");
  return MGS_ERR_UNSUPPORTED;
}

// the bound sensor as the 3DGUT kernels read it
static void fillSensorConst(const MgsSensorModel& m, int width, int height, SensorConst& S)
{
  S.bound = 1;
  S.model = m.model;
  std::memcpy(S.focal, m.focal_length, sizeof(S.focal));
  std::memcpy(S.principal, m.principal_point, sizeof(S.principal));
  std::memcpy(S.radial, m.radial, sizeof(S.radial));
  std::memcpy(S.tangential, m.tangential, sizeof(S.tangential));
  std::memcpy(S.thinPrism, m.thin_prism, sizeof(S.thinPrism));
  std::memcpy(S.fisheye, m.fisheye_radial, sizeof(S.fisheye));
  S.maxAngle    = m.max_angle > 0.0f ? m.max_angle : sensorMaxAngle((float)width, (float)height, m.principal_point, m.focal_length);
  S.clipRadius  = std::sqrt((float)width * (float)width + (float)height * (float)height);
  S.rcpFocal[0] = (float)(1.0 / (double)m.focal_length[0]);
  S.rcpFocal[1] = (float)(1.0 / (double)m.focal_length[1]);
  S.tolNorm     = kSensorTolPx / std::max(std::fabs(m.focal_length[0]), std::fabs(m.focal_length[1]));
}

// coarse bins (the default): stable multi-split straight into the per-bin lists, no records, no pair sort; MGS_DIRECT_BIN=0
// forces the record + pair-sort path of frames with more than 256 bins
bool directBinning(const FrameConst& F) { return tuning().directBin && directBinningSupported(F.binsX, F.binsY); }

// The bin rectangles ride through the key sort as codes in the id word's spare bits (kernels_common.h: rideEncode) when the
// frame bins directly and the GPU sorts: as many of the shapes 1x1, 2x1, 1x2, 2x2 as fit the spare bits (at most 16).
// MGS_RECT_RIDE=0: k_dbin_count gathers every rectangle by id instead (as frames without spare bits do).
static void chooseRide(MgsScene s, FrameConst& F, bool cpuMode)
{
  F.rideShift = F.rideShapes = F.rideSplit = 0;
  F.rideEscape = 0;
  if(!tuning().rectRide || cpuMode || !directBinning(F) || s->d->totalSplats == 0)
    return;
  int idBits = 1;
  while(idBits < 32 && (1ull << idBits) < (uint64_t)s->d->totalSplats)
    ++idBits;
  const int bx = F.binsX, by = F.binsY, nb = bx * by;
  const int codes[4] = {nb, nb + (bx - 1) * by, nb + (bx - 1) * by + bx * (by - 1), nb + (bx - 1) * by + bx * (by - 1) + (bx - 1) * (by - 1)};
  // Where the id word's spare bits hold all four shapes the code rides there whole.  Otherwise (round 5; 8 garden instances
  // need 26 id bits) it is split: its low 8 bits replace the KEY's low byte in the slot — the slot is grouped by that byte, so
  // the sort never looks at it again (slot_emit.h) — and only the rest rides above the id: 8 + spare bits.  MGS_RIDE_SPLIT=2:
  // always split (tests: small scenes take the split path too).
  const int spare = 32 - idBits;
  for(int pass = tuning().rideSplitAlways ? 1 : 0; pass < 2; ++pass)
  {
    const bool split    = pass == 1;
    const int  codeBits = std::min(split ? spare + 8 : spare, 16);
    if(split && spare < 1)
      break;
    for(int shapes = 4; shapes >= (split ? 1 : 4); --shapes)
      if(codeBits >= 1 && codes[shapes - 1] + 1 <= (1 << codeBits))
      {
        F.rideShift  = idBits;
        F.rideShapes = shapes;
        F.rideEscape = (1u << codeBits) - 1u;
        F.rideSplit  = split ? 1 : 0;
        return;
      }
  }
}

// the frames the adaptive bin size applies to: the default compositing mode of the 3DGS pipeline with the GPU sort
bool binPolicyEligible(const MgsFrameParams* p)
{
  return tuning().binAdapt && p->alpha_mode != MGS_ALPHA_SUM && p->pipeline == MGS_PIPELINE_3DGS && p->sort_mode == MGS_SORT_GPU_RADIX && !wantsSurface(p);
}

// bins: lists are built per (16<<shift)-pixel bin; the compositor culls per 16x16 tile on chip (needs F.tilesX / tilesY)
static int chooseBinGrid(MgsScene s, const MgsFrameParams* p, FrameConst& F)
{
  // Default 256x128 px (MGS_BIN_SHIFT="x,y" overrides, x 1..5, y 0..5; measured sweep in DESIGN.md §3.3).
  int bsx = 4, bsy = 3;  // 256x128 px
  // MGS_ALPHA_SUM has no early termination: every region walks its bin's WHOLE list, and the walk (the cull of stage A) is what
  // that mode pays for — 64 regions re-scanning a 256x128-px bin's list.  Smaller bins there, as small as the direct binning
  // allows (<= 256 bins): 128x64 px at 1080p = 255 bins; composite 6.6 -> 3.8 ms, binning +0.05 ms (profiles/r4_a_alpha_sum_sweep.log)
  if(p->alpha_mode == MGS_ALPHA_SUM && p->sort_mode != MGS_SORT_STOCHASTIC)
  {
    bsx = 3;
    bsy = 2;
  }
  else if(binPolicyEligible(p) && s->binPolicy.fine)
    bsx = bsy = 3;  // 128x128 px: this context's regions scan most of their lists (BinPolicy)
  if(tuning().binShiftSet)
  {
    bsx = tuning().binShiftX.value_or(bsx);
    bsy = tuning().binShiftY.value_or(bsy);
  }
  else
  {  // keep the frame at <= 256 bins so that the direct (record-free) binning applies: 4K -> 256x128 px bins
    // (8K UHD: 512x512 px bins)
    while(((F.tilesX + (1 << bsx) - 1) >> bsx) * ((F.tilesY + (1 << bsy) - 1) >> bsy) > 256 && (bsx < 5 || bsy < 5))
    {
      if(bsx <= bsy && bsx < 5)
        ++bsx;
      else if(bsy < 5)
        ++bsy;
      else
        ++bsx;
    }
  }
  bsx         = std::min(std::max(bsx, 1), 5);  // the compositor's 32x16-px regions must not straddle bins
  bsy         = std::min(std::max(bsy, 0), 5);
  if(((F.tilesX + (1 << bsx) - 1) >> bsx) > 256 || ((F.tilesY + (1 << bsy) - 1) >> bsy) > 256)
  {
    setError("frame: more than 256 bins along an axis (raise MGS_BIN_SHIFT)");
    return MGS_ERR_INVALID_ARG;
  }
  F.binShiftX = bsx;
  F.binShiftY = bsy;
  F.binsX     = (F.tilesX + (1 << bsx) - 1) >> bsx;
  F.binsY     = (F.tilesY + (1 << bsy) - 1) >> bsy;
  return MGS_OK;
}

// an instance's buffers and what the kernels need of its transform (offsets and blocks are the caller's running sums)
static void fillInstanceConst(const MgsFrameParams* p, const Instance& I, const DeviceSet& d, InstanceConst& C)
{
  C.centers = d.centers.p;
  C.cov6    = d.cov6.p;
  C.rgba    = d.rgba.p;
  C.sh      = d.sh.p;
  C.partBox = d.partBox.p;
  C.maxScale = d.maxScale.p;
  C.scales    = d.scales.p;
  C.alpha     = d.alpha.p;
  C.rgbaF32   = d.rgbaF32();
  C.rotations = d.rotations.p;
  {
    auto len3 = [&](int c) { return std::sqrt((I.M[4 * c] * I.M[4 * c] + I.M[4 * c + 1] * I.M[4 * c + 1]) + I.M[4 * c + 2] * I.M[4 * c + 2]); };
    C.modelAxisMax = std::max(len3(0), std::max(len3(1), len3(2)));
  }
  std::memcpy(C.model, I.M, sizeof(C.model));
  mat4Mul(p->view, I.M, C.modelView);  // mul(desc.transform, viewMatrix), mesh.slang:175
  float inv[16], cam[4] = {p->camera_pos[0], p->camera_pos[1], p->camera_pos[2], 1.0f}, cm[4];
  mat4Inverse(I.M, inv);
  std::memcpy(C.modelInv, inv, sizeof(inv));
  mat4MulVec4(inv, cam, cm);  // mesh.slang:240-241
  C.camModel[0]  = cm[0];
  C.camModel[1]  = cm[1];
  C.camModel[2]  = cm[2];
  {  // largest singular value of the 3x3: power iteration on A^T A (tiny, per frame, per instance)
    float AtA[9];
    for(int a = 0; a < 3; ++a)
      for(int b = 0; b < 3; ++b)
        AtA[3 * a + b] = I.M[4 * a] * I.M[4 * b] + I.M[4 * a + 1] * I.M[4 * b + 1] + I.M[4 * a + 2] * I.M[4 * b + 2];
    float v[3] = {0.577f, 0.577f, 0.577f}, lam = 0.f;
    for(int it = 0; it < 32; ++it)
    {
      float w[3];
      for(int a = 0; a < 3; ++a)
        w[a] = AtA[3 * a] * v[0] + AtA[3 * a + 1] * v[1] + AtA[3 * a + 2] * v[2];
      lam = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      if(!(lam > 0.f))
        break;
      for(int a = 0; a < 3; ++a)
        v[a] = w[a] / lam;
    }
    const float fro = std::sqrt(AtA[0] + AtA[4] + AtA[8]);
    C.modelScale    = std::min(fro, std::sqrt(lam) * 1.02f + 1e-6f);  // never above the Frobenius bound
    if(!(C.modelScale > 0.f))
      C.modelScale = fro;
  }
  C.count        = d.count;
  {
    static const float kId[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    C.modelIsIdentity = std::memcmp(I.M, kId, sizeof(kId)) == 0 ? 1u : 0u;  // bitwise (+0 only)
    {  // last row bitwise (+0, +0, +0, 1), moderate entries: w stays exactly 1 through M (kernels_common.h: mulMat4ExactAffineW1)
      const float    row[4] = {0.0f, 0.0f, 0.0f, 1.0f}, got[4] = {I.M[3], I.M[7], I.M[11], I.M[15]};
      bool           ok     = std::memcmp(row, got, sizeof(row)) == 0;
      for(int q = 0; q < 16 && ok; ++q)
        ok = std::fabs(I.M[q]) < 16777216.0f;  // 2^24; also false for NaN
      C.modelIsAffine = ok ? 1u : 0u;
    }
  }
}

int buildFrameArgs(MgsScene s, const MgsFrameParams* p, FrameArgs& A)
{
  if(p->width <= 0 || p->height <= 0 || p->width > 8192 || p->height > 8192)
  {
    setError("frame: width/height must be in [1,8192] (8-bit bin coordinates, bins of at least 32 pixels)");
    return MGS_ERR_INVALID_ARG;
  }
  std::memset(&A, 0, sizeof(A));
  FrameConst& F = A.f;
  std::memcpy(F.view, p->view, sizeof(F.view));
  std::memcpy(F.proj, p->proj, sizeof(F.proj));
  {  // affine view + perspective projection, bit patterns and magnitudes checked: the project kernels may drop the products with
     // the exact zeros (kernels_common.h: mulMat4ExactAffineW1 / mulPerspExactW1*).  MGS_EXACT_SHORTCUTS=0: never (A/B).
    const float vrow[4] = {p->view[3], p->view[7], p->view[11], p->view[15]}, want[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    bool        ok      = tuning().exactShortcuts && std::memcmp(vrow, want, sizeof(want)) == 0;
    static const int kZero[9] = {1, 2, 3, 4, 6, 7, 12, 13, 15};
    const float      zero     = 0.0f;
    for(int q = 0; q < 9 && ok; ++q)
      ok = std::memcmp(&p->proj[kZero[q]], &zero, 4) == 0;  // +0 bitwise
    ok = ok && p->proj[14] != 0.0f;
    for(int q = 0; q < 16 && ok; ++q)
      ok = std::fabs(p->view[q]) < 16777216.0f && std::fabs(p->proj[q]) < 16777216.0f;  // 2^24 (with |coordinate| < 2^40 and |M| < 2^24 no product of the chain P*V*M*p reaches 2^127); false for NaN
    F.perspAffine = ok ? 1 : 0;
  }
  F.focal[0] = p->proj[0] * 0.5f * (float)p->width;   // gaussian_splatting.cpp:1248-1250
  F.focal[1] = p->proj[5] * 0.5f * (float)p->height;
  F.width    = p->width;
  F.height   = p->height;
  F.tilesX   = (p->width + kTilePx - 1) / kTilePx;
  F.tilesY   = (p->height + kTilePx - 1) / kTilePx;
  int r0 = p->strip_row_begin, r1 = p->strip_row_end;
  if(r0 == 0 && r1 == 0)
    r1 = F.tilesY;
  if(r0 < 0 || r1 > F.tilesY || r0 >= r1)
  {
    setError("frame: strip rows out of range");
    return MGS_ERR_INVALID_ARG;
  }
  F.stripRow0       = r0;
  F.stripRow1       = r1;
  if(int rc = chooseBinGrid(s, p, F))
    return rc;
  F.splatScale      = p->splat_scale;
  F.frustumDilation = p->frustum_dilation;
  F.alphaCull       = p->alpha_cull_threshold;
  F.shDegree        = p->sh_degree;
  F.frontToBack     = 0;  // keys of -depth: ascending = far to near, the reference's default order
  F.cullMode        = p->frustum_culling;
  if(p->sort_mode == MGS_SORT_CPU_ASYNC && F.cullMode == MGS_CULL_AT_DIST)
    F.cullMode = MGS_CULL_AT_RASTER;  // gaussian_splatting_ui.cpp:1469-1479
  F.msAA            = p->ms_antialiasing;
  F.alphaMode       = p->alpha_mode;
  F.debugFlags      = p->debug_flags;
  F.sizeCulling     = p->size_culling;
  F.sizeCullingMinPixels = p->size_culling_min_pixels;
  F.surfaceOutputs  = wantsSurface(p) ? 1 : 0;
  F.depthIsoThreshold = p->depth_iso_threshold;
  F.thinParticleThreshold = p->thin_particle_threshold;
  F.quantizeNormals       = p->quantize_normals ? 1 : 0;
  // 3DGUT
  F.pipeline          = p->pipeline;
  F.cameraModel       = p->camera_model;
  F.extentMethod      = p->extent_method;
  F.fovRad            = p->fov_rad > 0.0f ? p->fov_rad : 2.0f * std::atan(1.0f / std::fabs(p->proj[5]));
  F.alphaClamp        = p->alpha_clamp;
  F.kernelMinResponse = p->kernel_min_response;
  F.stochastic        = p->sort_mode == MGS_SORT_STOCHASTIC ? 1 : 0;
  if(F.stochastic)
    F.alphaMode = MGS_ALPHA_COVERAGE;  // opaque writes: the pixel's alpha is "a fragment was accepted"
  F.dofMode          = p->pipeline == MGS_PIPELINE_3DGUT ? p->dof_mode : 0;
  F.focusDist        = p->focus_dist;
  F.aperture         = p->aperture;
  F.frameSampleId    = p->frame_sample_id;
  F.temporalSampling = p->temporal_sampling ? 1 : 0;
  F.kernelDegree     = p->kernel_degree;
  F.normalMethod     = p->normal_method;
  chooseRide(s, F, p->sort_mode == MGS_SORT_CPU_ASYNC);
  if(p->camera_model == MGS_CAMERA_FISHEYE && p->pipeline == MGS_PIPELINE_3DGUT)
  {  // gaussian_splatting.cpp:1239-1244: frameInfo.focal is the fisheye focal only for the 3DGUT pipelines; a fisheye camera on
     // the 3DGS pipelines keeps the pinhole focal (and dist.comp's fisheye cull then runs on that)
    F.gutFocal[0] = (float)p->width / F.fovRad;
    F.gutFocal[1] = -(float)p->height / F.fovRad;
  }
  else
  {
    F.gutFocal[0] = F.focal[0];
    F.gutFocal[1] = F.focal[1];
  }
  {  // computeMaxAngle, threedgut_camera_models.h.slang:87-118 (principal point at the viewport centre)
    const float mdx = (float)p->width * 0.5f, mdy = (float)p->height * 0.5f;
    const float maxR = std::sqrt(mdx * mdx + mdy * mdy);
    F.gutMaxAngle = std::max(2.0f * maxR / F.gutFocal[0], 2.0f * maxR / F.gutFocal[1]) / 2.0f;
  }
  mat4Inverse(p->view, F.viewInv);
  mat4Inverse(p->proj, F.projInv);
  F.lightingMode = p->lighting_mode;
  if(F.lightingMode != MGS_LIGHTING_DISABLED)
  {  // (unlit frames keep these zero)
    std::memcpy(F.cameraPos, p->camera_pos, sizeof(F.cameraPos));
    mat4InverseDouble(p->view, F.lightViewInv);
    mat4InverseDouble(p->proj, F.lightProjInv);
  }
  F.maxFocal        = std::max(std::fabs(F.gutFocal[0]), std::fabs(F.gutFocal[1]));  // frameInfo.focal (dist.comp.slang:125)
  F.targetFormat    = p->target_format;
  F.nInstances      = (int)s->d->instances.size();
  F.totalSplats     = s->d->totalSplats;
  F.totalPartitions = s->d->totalParts;
  F.partitionCull   = F.cullMode == MGS_CULL_AT_DIST ? 1 : 0;
  if(s->sensor.bound && p->pipeline == MGS_PIPELINE_3DGUT)
  {  // the handle's sensor model replaces cameraModel / fovRad for the projection and the rays; the pre-cull of partition_cull.h
     // bounds the two perfect models only
    fillSensorConst(s->sensor.model, p->width, p->height, F.sensor);
    F.partitionCull = 0;
  }
  uint32_t offset = 0, block = 0;
  for(int k = 0; k < F.nInstances; ++k)
  {
    const DeviceSet& d = s->d->sets[s->d->instances[k].set];
    InstanceConst&   C = A.inst[k];
    fillInstanceConst(p, s->d->instances[k], d, C);
    C.globalOffset = offset;
    C.blockBegin   = block;
    C.shDegree     = d.shDegree;
    C.shStride     = d.shPitch;  // kernels index by the stored pitch
    offset += d.count;
    block += (d.count + kPart - 1) / kPart;
  }
  return MGS_OK;
}
