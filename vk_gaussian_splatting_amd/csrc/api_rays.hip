// api_rays.hip — ray queries, host side: mgs_trace_rays / mgs_trace_rays_device trace the caller's rays through the scene's hierarchy
// with the walk of mgs_render_traced's strategy 0, mgs_trace_generate_rays writes out a frame's primary rays.  The range checks, the
// hierarchy and the traversal's arguments are api_trace.hip's.
#include <cmath>
#include <memory>

#include "scene_state.h"

void mgs_ray_query_params_default(MgsRayQueryParams* q)
{
  if(q)
    std::memset(q, 0, sizeof(*q));  // reorder 0: the caller's order
}

// *p with every field a ray query does not read set to a value that is in range and reads no memory: the caller's camera, frame
// size, strip rows, lens, sample and target are neither read nor checked
MgsFrameParams withoutCamera(const MgsFrameParams& p)
{
  MgsFrameParams q = p;
  std::memset(q.view, 0, sizeof(q.view));
  std::memset(q.proj, 0, sizeof(q.proj));
  std::memset(q.camera_pos, 0, sizeof(q.camera_pos));
  q.view[0] = q.view[5] = q.view[10] = q.view[15] = 1.0f;
  q.proj[0] = q.proj[5] = q.proj[10] = q.proj[15] = 1.0f;
  q.width = q.height  = kTilePx;
  q.strip_row_begin   = 0;
  q.strip_row_end     = 0;
  q.target_format     = MGS_TARGET_RGBA32F;
  q.camera_model      = MGS_CAMERA_PINHOLE;
  q.fov_rad           = 0.0f;
  q.dof_mode          = MGS_DOF_DISABLED;
  q.frame_sample_id   = 0;
  q.temporal_sampling = 0;
  return q;
}

namespace {
struct RayBatch
{
  const MgsRay* rays    = nullptr;  // device
  MgsRayResult* results = nullptr;  // device
  uint64_t      count   = 0;
};
}  // namespace

// the checks that need no device, in the order of the other traced entry points
int validateRays(const MgsFrameParams* p, const MgsTraceParams& t, const MgsRayQueryParams& q, const void* rays, const void* results, uint64_t count,
                 bool onDevice, const char* what, const char* items)
{
  const std::string w = std::string(what) + ": ", n(items);
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null params");
  const MgsFrameParams v = withoutCamera(*p);
  if(int rc = validateTrace(&v, t))
    return rc;
  if(t.trace_strategy != MGS_TRACE_STRATEGY_FULL_ANYHIT)
    return failTrace(MGS_ERR_UNSUPPORTED, std::string(what) + ": the stochastic trace strategies are mgs_render_traced's, their seeds are per pixel "
                                                              "(trace_strategy must be 0)");
  if(q.reorder != 0 && q.reorder != 1)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": reorder must be 0 or 1");
  if(count > 0 && (!rays || !results))
    return failTrace(MGS_ERR_INVALID_ARG, w + "null " + n + " or results with count > 0");
  if(count > 0x7FFFFFFFull)
    return failTrace(MGS_ERR_UNSUPPORTED, w + "at most 2^31 - 1 " + n + " per call");
  if(onDevice && (((uintptr_t)rays | (uintptr_t)results) & 15u))
    return failTrace(MGS_ERR_INVALID_ARG, w + n + " and results must be 16-byte aligned");
  return MGS_OK;
}

// the batch on the device, on the handle's stream; waits only for `out`
static int traceRaysOnDevice(MgsScene s, const RayBatch& b, const MgsFrameParams* p, const MgsTraceParams& t, const MgsRayQueryParams& qp,
                             MgsRayQueryOut* out, const char* what)
{
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null scene");
  if(out)
    std::memset(out, 0, sizeof(*out));
  if(b.count == 0)
    return MGS_OK;
  // the frame's constants as mgs_render_traced builds them, without a camera (so without the rays' inverses)
  MgsFrameParams q      = withoutCamera(*p);
  q.lighting_mode       = MGS_LIGHTING_DISABLED;
  q.depth_iso_threshold = t.depth_iso_threshold;
  std::unique_ptr<FrameArgs> A;
  int                        rc;
  if((rc = traceFrameArgs(s, q, what, false, A))) return rc;
  SceneData&      d  = *s->d;
  TracePassState& ts = s->trace;
  if((rc = ensureTraceEvents(ts))) return rc;
  if((rc = ts.ctr.ensure(1))) return rc;
  if((rc = ts.rayInvalid.ensure(1))) return rc;
  const uint32_t n = (uint32_t)b.count;
  if(qp.reorder)
  {
    if((rc = ts.rayKeys.ensure(n))) return rc;
    if((rc = ts.rayIdx.ensure(n))) return rc;
  }
  if((rc = uploadFrameState(s, *A, s->stream))) return rc;
  const TraceProxy proxy   = traceProxy(*p, t);
  float            buildMs = 0.0f;
  uint32_t         rebuilt = 0;
  if((rc = ensureHierarchy(s, *A, proxy, &buildMs, &rebuilt))) return rc;
  hipStream_t st = s->stream;
  if(qp.reorder)
  {
    HIPCHK(hipEventRecord(ts.ev[kEvReorderBegin], st));
    RayKeyArgs K{};
    K.rays  = reinterpret_cast<const float4*>(b.rays);
    K.keys  = ts.rayKeys.p;
    K.idx   = ts.rayIdx.p;
    K.count = n;
    sceneBox(d, K.sceneLo, K.sceneInvExt);
    launchRaysKey(st, K);
    HIPCHK(hipGetLastError());
    // the library's own (key, value) sort: stable, so rays with equal keys keep the caller's order
    if((rc = mgs_radix_sort_u32(s, ts.rayKeys.p, ts.rayIdx.p, n, 0, 32, nullptr))) return rc;
    HIPCHK(hipEventRecord(ts.ev[kEvReorderEnd], st));
  }
  HIPCHK(hipMemsetAsync(ts.ctr.p, 0, sizeof(TraceCounters), st));
  HIPCHK(hipMemsetAsync(ts.rayInvalid.p, 0, 4, st));
  HIPCHK(hipEventRecord(ts.ev[kEvTraverseBegin], st));
  TraceRaysArgs L{};
  L.t       = traceArgs(s, proxy, t, 0);
  L.t.image = nullptr;  // a ray query writes results only: the handle's frame, side outputs and hit counts stay as they are
  L.rays    = reinterpret_cast<const float4*>(b.rays);
  L.results = reinterpret_cast<float4*>(b.results);
  L.perm    = qp.reorder ? ts.rayIdx.p : nullptr;
  L.count   = n;
  L.invalid = ts.rayInvalid.p;
  L.surf    = p->surface_outputs != 0 ? 1 : 0;
  launchTraceRays(st, L, d.shFormat);
  HIPCHK(hipEventRecord(ts.ev[kEvTraverseEnd], st));
  HIPCHK(hipGetLastError());
  if(out)
  {
    TraceOutRead R;
    uint32_t     invalid = 0;
    if((rc = R.begin(s))) return rc;
    HIPCHK(hipMemcpyAsync(&invalid, ts.rayInvalid.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if((rc = R.finish(s, rebuilt, buildMs, &out->trace))) return rc;
    out->invalid_rays = invalid;
    if(qp.reorder)
      HIPCHK(hipEventElapsedTime(&out->reorder_ms, ts.ev[kEvReorderBegin], ts.ev[kEvReorderEnd]));
  }
  return MGS_OK;
}

static int mgs_trace_rays_impl(MgsScene s, const void* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp,
                               const MgsRayQueryParams* qp, void* results, MgsRayQueryOut* out, bool host)
{
  const char*    what = host ? "mgs_trace_rays" : "mgs_trace_rays_device";
  const MgsTraceParams    t = traceParamsOr(tp);
  const MgsRayQueryParams q = rayQueryParamsOr(qp);
  // (before the handle is looked at; host arrays need no alignment: they are staged)
  if(int rc = validateRays(p, t, q, rays, results, count, !host, what))
    return rc;
  RayBatch b;
  b.count = count;
  if(!host)
  {
    b.rays    = static_cast<const MgsRay*>(rays);
    b.results = static_cast<MgsRayResult*>(results);
    return traceRaysOnDevice(s, b, p, t, q, out, what);
  }
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_rays: null scene");
  if(count == 0)
  {
    if(out)
      std::memset(out, 0, sizeof(*out));
    return MGS_OK;
  }
  HIPCHK(hipSetDevice(s->device));
  TracePassState& ts = s->trace;
  int             rc;
  if((rc = ts.rayStage.ensure(2 * (size_t)count))) return rc;
  if((rc = ts.resultStage.ensure(3 * (size_t)count))) return rc;
  HIPCHK(hipMemcpyAsync(ts.rayStage.p, rays, (size_t)count * sizeof(MgsRay), hipMemcpyHostToDevice, s->stream));
  b.rays    = reinterpret_cast<const MgsRay*>(ts.rayStage.p);
  b.results = reinterpret_cast<MgsRayResult*>(ts.resultStage.p);
  if((rc = traceRaysOnDevice(s, b, p, t, q, out, what)))
  {
    (void)hipStreamSynchronize(s->stream);  // the upload reads the caller's array
    return rc;
  }
  HIPCHK(hipMemcpyAsync(results, ts.resultStage.p, (size_t)count * sizeof(MgsRayResult), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}
int mgs_trace_rays(MgsScene s, const MgsRay* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsRayQueryParams* qp,
                   MgsRayResult* results, MgsRayQueryOut* out)
{
  return guarded("mgs_trace_rays", [&] { return mgs_trace_rays_impl(s, rays, count, p, tp, qp, results, out, true); });
}
int mgs_trace_rays_device(MgsScene s, const MgsRay* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp,
                          const MgsRayQueryParams* qp, MgsRayResult* results, MgsRayQueryOut* out)
{
  return guarded("mgs_trace_rays_device", [&] { return mgs_trace_rays_impl(s, rays, count, p, tp, qp, results, out, false); });
}

static int mgs_trace_generate_rays_impl(MgsScene s, const MgsFrameParams* p, MgsRay* raysDev)
{
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_generate_rays: null params");
  if(int rc = validateTrace(p, traceParamsOr(nullptr)))  // (before the handle is looked at)
    return rc;
  if(!raysDev || ((uintptr_t)raysDev & 15u))
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_generate_rays: rays must be a 16-byte aligned device pointer");
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_generate_rays: null scene");
  MgsFrameParams q = *p;  // the constants of mgs_render_traced's frame (the iso threshold, which no ray depends on, stays the caller's)
  std::unique_ptr<FrameArgs> A;
  int                        rc;
  if((rc = traceFrameArgs(s, q, "mgs_trace_generate_rays", true, A))) return rc;
  if((rc = uploadFrameState(s, *A, s->stream))) return rc;
  launchRaysGenerate(s->stream, s->fb.dArgs.p, reinterpret_cast<float4*>(raysDev), (uint32_t)A->f.width * (uint32_t)A->f.height);
  HIPCHK(hipGetLastError());
  return MGS_OK;
}
int mgs_trace_generate_rays(MgsScene s, const MgsFrameParams* p, MgsRay* raysDev)
{
  return guarded("mgs_trace_generate_rays", [&] { return mgs_trace_generate_rays_impl(s, p, raysDev); });
}
