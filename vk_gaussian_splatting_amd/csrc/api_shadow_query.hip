// api_shadow_query.hip — shadow and light queries, host side: mgs_trace_shadow_rays / mgs_trace_shadow_rays_device trace the caller's
// shadow rays as the light pass of a lit frame traces its own, mgs_shade_points / mgs_shade_points_device shade the caller's surface
// points under the scene's lights with one such ray per light.  The range checks are the ray queries' (api_rays.hip) and the light
// pass's; the frame's constants, the hierarchy, the events and the traversal's arguments are api_trace.hip's.
#include <cmath>
#include <memory>
#include <vector>

#include "scene_state.h"
#include "trace_dispatch.h"

namespace {
constexpr uint32_t kMaxQueryMaterials = 256;

struct ShadowBatch
{
  bool                points    = false;    // surface points (4 float4 each) instead of rays (2)
  const void*         items     = nullptr;  // device
  void*               results   = nullptr;  // device, one float4 each
  uint64_t            count     = 0;
  const MgsMaterial*  materials = nullptr;  // host (points)
  uint32_t            materialCount = 0;
};
}  // namespace

// the light knobs a query reads: the ranges of validateTrace's lit branch, without the frame's lighting_mode rule
static int validateShadowKnobs(const MgsTraceLightParams& lt, bool points, const char* what)
{
  const std::string w(what);
  if(lt.shadows_mode == MGS_SHADOWS_SOFT)
    return failTrace(MGS_ERR_UNSUPPORTED, w + ": soft shadows are a frame's (a query point has no pixel to seed the light's disk sample from)");
  if(points ? (lt.shadows_mode != MGS_SHADOWS_DISABLED && lt.shadows_mode != MGS_SHADOWS_HARD) : lt.shadows_mode != MGS_SHADOWS_HARD)
    return failTrace(MGS_ERR_INVALID_ARG, w + (points ? ": shadows_mode must be MGS_SHADOWS_DISABLED or MGS_SHADOWS_HARD" : ": shadows_mode must be MGS_SHADOWS_HARD"));
  if(points && (!(lt.particle_shadow_offset >= 0.0f) || !std::isfinite(lt.particle_shadow_offset)))
    return failTrace(MGS_ERR_INVALID_ARG, w + ": particle_shadow_offset must be finite and >= 0");
  if(!(lt.particle_shadow_transmittance_threshold >= 0.0f && lt.particle_shadow_transmittance_threshold < 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, w + ": particle_shadow_transmittance_threshold must be in [0, 1)");
  if(!(lt.particle_shadow_color_strength >= 0.0f && lt.particle_shadow_color_strength <= 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, w + ": particle_shadow_color_strength must be in [0, 1]");
  return MGS_OK;
}

// the batch on the device, on the handle's stream; waits only for `out` / `lout` / `invalidOut`
static int shadowQueryOnDevice(MgsScene s, const ShadowBatch& b, const MgsFrameParams* p, const MgsTraceParams& t, const MgsTraceLightParams& lt,
                               const MgsRayQueryParams& qp, MgsRayQueryOut* out, MgsTraceLightOut* lout, uint32_t* invalidOut, const char* what)
{
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null scene");
  if(out)
    std::memset(out, 0, sizeof(*out));
  if(lout)
    std::memset(lout, 0, sizeof(*lout));
  if(invalidOut)
    *invalidOut = 0;
  if(b.count == 0)
    return MGS_OK;
  // the frame's constants as a ray query builds them: no camera
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
  hipStream_t st = s->stream;
  if(b.points)
  {
    if((rc = ts.lctr.ensure(1))) return rc;
    if((rc = ensureLightTable(d))) return rc;
    if((rc = ts.queryMats.ensure(kMaxQueryMaterials))) return rc;
    // the converted table is the handle's, so the copy needs no wait: only the previous call's copy must have left it, which it has
    // long since unless the caller queues queries faster than the stream runs them
    HIPCHK(hipEventSynchronize(ts.ev[kEvMatsUploaded]));
    ts.queryMatsHost.resize(b.materialCount);
    for(uint32_t i = 0; i < b.materialCount; ++i)
      ts.queryMatsHost[i] = materialToDevice(b.materials[i]);
    HIPCHK(hipMemcpyAsync(ts.queryMats.p, ts.queryMatsHost.data(), b.materialCount * sizeof(MaterialDev), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ts.ev[kEvMatsUploaded], st));
  }
  if((rc = uploadFrameState(s, *A, st))) return rc;
  const TraceProxy proxy    = traceProxy(*p, t);
  const bool       traverse = !b.points || lt.shadows_mode != MGS_SHADOWS_DISABLED;  // pure shading needs no hierarchy
  float            buildMs  = 0.0f;
  uint32_t         rebuilt  = 0;
  if(traverse)
    if((rc = ensureHierarchy(s, *A, proxy, &buildMs, &rebuilt))) return rc;
  if(qp.reorder)
  {
    HIPCHK(hipEventRecord(ts.ev[kEvReorderBegin], st));
    if(b.points)
    {
      PointKeyArgs K{};
      K.points = static_cast<const float4*>(b.items);
      K.keys   = ts.rayKeys.p;
      K.idx    = ts.rayIdx.p;
      K.count  = n;
      sceneBox(d, K.sceneLo, K.sceneInvExt);
      launchPointsKey(st, K);
    }
    else
    {
      RayKeyArgs K{};
      K.rays  = static_cast<const float4*>(b.items);
      K.keys  = ts.rayKeys.p;
      K.idx   = ts.rayIdx.p;
      K.count = n;
      sceneBox(d, K.sceneLo, K.sceneInvExt);
      launchRaysKey(st, K);
    }
    HIPCHK(hipGetLastError());
    // the library's own (key, value) sort: stable, so items with equal keys keep the caller's order
    if((rc = mgs_radix_sort_u32(s, ts.rayKeys.p, ts.rayIdx.p, n, 0, 32, nullptr))) return rc;
    HIPCHK(hipEventRecord(ts.ev[kEvReorderEnd], st));
  }
  HIPCHK(hipMemsetAsync(ts.ctr.p, 0, sizeof(TraceCounters), st));
  HIPCHK(hipMemsetAsync(ts.rayInvalid.p, 0, 4, st));
  if(b.points)
    HIPCHK(hipMemsetAsync(ts.lctr.p, 0, sizeof(TraceLightCounters), st));
  ShadowQueryArgs L{};
  L.t = traceArgs(s, proxy, t, 0);
  L.t.image = nullptr;  // a query writes results only: the handle's frame, side outputs, hit counts and shadow hits stay as they are
  if(!traverse)
    L.t.nLevels = 0;    // (a hierarchy another call built is not walked either)
  L.items               = static_cast<const float4*>(b.items);
  L.results             = static_cast<float4*>(b.results);
  L.perm                = qp.reorder ? ts.rayIdx.p : nullptr;
  L.count               = n;
  L.invalid             = ts.rayInvalid.p;
  L.lctr                = ts.lctr.p;
  L.table               = d.lightTab.p;
  L.mats                = ts.queryMats.p;
  L.matCount            = b.materialCount;
  L.shadowsMode         = lt.shadows_mode;
  L.shFormat            = shFormatIndex(d.shFormat);
  L.shadowOffset        = lt.particle_shadow_offset;
  L.shadowThreshold     = lt.particle_shadow_transmittance_threshold;
  L.shadowColorStrength = lt.particle_shadow_color_strength;
  std::memcpy(L.cameraPos, p->camera_pos, sizeof(L.cameraPos));
  HIPCHK(hipEventRecord(ts.ev[b.points ? kEvLightBegin : kEvTraverseBegin], st));
  if(b.points)
    launchShadePoints(st, L);
  else
    launchShadowRays(st, L);
  HIPCHK(hipEventRecord(ts.ev[b.points ? kEvLightEnd : kEvTraverseEnd], st));
  HIPCHK(hipGetLastError());
  if(out || lout || invalidOut)
  {
    TraceOutRead       R;
    TraceLightCounters hc{};
    uint32_t           invalid = 0;
    if(out)
      if((rc = R.begin(s))) return rc;
    if(lout)
      HIPCHK(hipMemcpyAsync(&hc, ts.lctr.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&invalid, ts.rayInvalid.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if(out)
    {
      if((rc = R.finish(s, rebuilt, buildMs, &out->trace))) return rc;
      out->invalid_rays = invalid;
      if(qp.reorder)
        HIPCHK(hipEventElapsedTime(&out->reorder_ms, ts.ev[kEvReorderBegin], ts.ev[kEvReorderEnd]));
    }
    if(lout)
    {
      lout->shadow_rays            = hc.shadowRays;
      lout->shadow_node_visits     = hc.nodeVisits;
      lout->shadow_candidate_tests = hc.candidateTests;
      lout->shadow_accepted_hits   = hc.acceptedHits;
      HIPCHK(hipEventElapsedTime(&lout->light_ms, ts.ev[kEvLightBegin], ts.ev[kEvLightEnd]));
    }
    if(invalidOut)
      *invalidOut = invalid;
  }
  return MGS_OK;
}

// host arrays through the handle's staging buffers; waits
static int shadowQueryStaged(MgsScene s, ShadowBatch b, const void* itemsHost, void* resultsHost, const MgsFrameParams* p, const MgsTraceParams& t,
                             const MgsTraceLightParams& lt, const MgsRayQueryParams& qp, MgsRayQueryOut* out, MgsTraceLightOut* lout,
                             uint32_t* invalidOut, const char* what)
{
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null scene");
  if(b.count == 0)
    return shadowQueryOnDevice(s, b, p, t, lt, qp, out, lout, invalidOut, what);
  HIPCHK(hipSetDevice(s->device));
  TracePassState& ts    = s->trace;
  const size_t    words = b.points ? 4 : 2;
  int             rc;
  if((rc = ts.rayStage.ensure(words * (size_t)b.count))) return rc;
  if((rc = ts.resultStage.ensure((size_t)b.count))) return rc;
  HIPCHK(hipMemcpyAsync(ts.rayStage.p, itemsHost, words * (size_t)b.count * sizeof(float4), hipMemcpyHostToDevice, s->stream));
  b.items   = ts.rayStage.p;
  b.results = ts.resultStage.p;
  if((rc = shadowQueryOnDevice(s, b, p, t, lt, qp, out, lout, invalidOut, what)))
  {
    (void)hipStreamSynchronize(s->stream);  // the upload reads the caller's array
    return rc;
  }
  HIPCHK(hipMemcpyAsync(resultsHost, ts.resultStage.p, (size_t)b.count * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}

static int mgs_trace_shadow_rays_impl(MgsScene s, const MgsRay* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp,
                                      const MgsTraceLightParams* lp, const MgsRayQueryParams* qp, MgsShadowResult* results, MgsRayQueryOut* out,
                                      bool host)
{
  static_assert(sizeof(MgsShadowResult) == 16 && sizeof(MgsRay) == 32, "one and two 16-byte vectors");
  const char*             what = host ? "mgs_trace_shadow_rays" : "mgs_trace_shadow_rays_device";
  const MgsTraceParams    t    = traceParamsOr(tp);
  const MgsRayQueryParams q    = rayQueryParamsOr(qp);
  MgsTraceLightParams     lt   = traceLightParamsOr(lp);
  if(!lp)
    lt.shadows_mode = MGS_SHADOWS_HARD;  // the defaults of a call that traces nothing but shadow rays
  // (before the handle is looked at; host arrays need no alignment: they are staged)
  if(int rc = validateRays(p, t, q, rays, results, count, !host, what))
    return rc;
  if(int rc = validateShadowKnobs(lt, false, what))
    return rc;
  ShadowBatch b;
  b.count = count;
  if(host)
    return shadowQueryStaged(s, b, rays, results, p, t, lt, q, out, nullptr, nullptr, what);
  b.items   = rays;
  b.results = results;
  return shadowQueryOnDevice(s, b, p, t, lt, q, out, nullptr, nullptr, what);
}
int mgs_trace_shadow_rays(MgsScene s, const MgsRay* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp,
                          const MgsRayQueryParams* qp, MgsShadowResult* results, MgsRayQueryOut* out)
{
  return guarded("mgs_trace_shadow_rays", [&] { return mgs_trace_shadow_rays_impl(s, rays, count, p, tp, lp, qp, results, out, true); });
}
int mgs_trace_shadow_rays_device(MgsScene s, const MgsRay* rays, uint64_t count, const MgsFrameParams* p, const MgsTraceParams* tp,
                                 const MgsTraceLightParams* lp, const MgsRayQueryParams* qp, MgsShadowResult* results, MgsRayQueryOut* out)
{
  return guarded("mgs_trace_shadow_rays_device", [&] { return mgs_trace_shadow_rays_impl(s, rays, count, p, tp, lp, qp, results, out, false); });
}

static int mgs_shade_points_impl(MgsScene s, const MgsSurfacePoint* points, uint64_t count, const MgsMaterial* mats, uint32_t matCount,
                                 const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, const MgsRayQueryParams* qp,
                                 MgsShadeResult* results, MgsTraceLightOut* lout, uint32_t* invalidOut, bool host)
{
  static_assert(sizeof(MgsShadeResult) == 16 && sizeof(MgsSurfacePoint) == 64, "one and four 16-byte vectors");
  const char*               what = host ? "mgs_shade_points" : "mgs_shade_points_device";
  const MgsTraceParams      t    = traceParamsOr(tp);
  const MgsRayQueryParams   q    = rayQueryParamsOr(qp);
  const MgsTraceLightParams lt   = traceLightParamsOr(lp);
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null params");
  MgsFrameParams v = *p;
  v.lighting_mode  = MGS_LIGHTING_DISABLED;  // not read: the call is the light pass
  if(int rc = validateRays(&v, t, q, points, results, count, !host, what, "points"))
    return rc;
  if(int rc = validateShadowKnobs(lt, true, what))
    return rc;
  if(!mats || matCount < 1 || matCount > kMaxQueryMaterials)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": materials must hold 1 to 256 entries");
  if(!std::isfinite(p->camera_pos[0]) || !std::isfinite(p->camera_pos[1]) || !std::isfinite(p->camera_pos[2]))
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": camera_pos (the headlight's position) must be finite");
  if(host)
    for(uint64_t i = 0; i < count; ++i)
      if(points[i].material >= matCount)
        return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": a point's material index is not below material_count");
  ShadowBatch b;
  b.points        = true;
  b.count         = count;
  b.materials     = mats;
  b.materialCount = matCount;
  if(host)
    return shadowQueryStaged(s, b, points, results, &v, t, lt, q, nullptr, lout, invalidOut, what);
  b.items   = points;
  b.results = results;
  return shadowQueryOnDevice(s, b, &v, t, lt, q, nullptr, lout, invalidOut, what);
}
int mgs_shade_points(MgsScene s, const MgsSurfacePoint* points, uint64_t count, const MgsMaterial* mats, uint32_t matCount, const MgsFrameParams* p,
                     const MgsTraceParams* tp, const MgsTraceLightParams* lp, const MgsRayQueryParams* qp, MgsShadeResult* results, MgsTraceLightOut* lout,
                     uint32_t* invalidOut)
{
  return guarded("mgs_shade_points", [&] { return mgs_shade_points_impl(s, points, count, mats, matCount, p, tp, lp, qp, results, lout, invalidOut, true); });
}
int mgs_shade_points_device(MgsScene s, const MgsSurfacePoint* points, uint64_t count, const MgsMaterial* mats, uint32_t matCount,
                            const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, const MgsRayQueryParams* qp,
                            MgsShadeResult* results, MgsTraceLightOut* lout, uint32_t* invalidOut)
{
  return guarded("mgs_shade_points_device",
                 [&] { return mgs_shade_points_impl(s, points, count, mats, matCount, p, tp, lp, qp, results, lout, invalidOut, false); });
}
