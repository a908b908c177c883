// api_trace.hip — the traced pipeline's host side: mgs_render_traced and mgs_render_traced_lit, the lazy build of the scene's
// hierarchy, the hit-count and shadow-hit downloads; and mgs_render_hybrid, whose primary surface is a frame of mgs_render.
#include <array>
#include <cmath>
#include <memory>
#include <mutex>

#include "scene_state.h"
#include "trace_dispatch.h"

void mgs_trace_params_default(MgsTraceParams* p)
{
  if(!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->samples_per_pass         = 18;     // PARTICLES_SPP, parameters.h:218
  p->max_passes               = 200;    // shaderio.h:269
  p->min_transmittance        = 0.01f;  // shaderio.h:272
  p->kernel_adaptive_clamping = 1;      // parameters.h:217
  p->depth_iso_threshold      = 0.7f;   // depthIsoThresholdRTX, parameters.h:226
  p->trace_strategy           = MGS_TRACE_STRATEGY_FULL_ANYHIT;  // parameters.h:219
}

void mgs_trace_light_params_default(MgsTraceLightParams* p)
{
  if(!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->shadows_mode                            = MGS_SHADOWS_DISABLED;  // parameters.h:167
  p->particle_shadow_offset                  = 0.2f;                  // parameters.h:222
  p->particle_shadow_transmittance_threshold = 0.8f;                  // parameters.h:223
  p->particle_shadow_color_strength          = 0.0f;                  // parameters.h:224
}

void mgs_trace_mesh_params_default(MgsTraceMeshParams* p)
{
  if(!p)
    return;
  std::memset(p, 0, sizeof(*p));  // off; frameInfo.minMeshCompositeTransmittance = 0.0, shaderio.h:285
}

int failTrace(int code, const std::string& msg)
{
  setError(msg);
  return code;
}

// what needs no device: the ranges of MgsTraceParams and of the MgsFrameParams fields the traced pipeline reads
// (lit: the checks of mgs_render_traced_lit, whose lighting_mode rule differs; hybrid: those of mgs_render_hybrid, which has no
// primary walk and takes its surface from one of the raster pipelines)
int validateTrace(const MgsFrameParams* p, const MgsTraceParams& t, const MgsTraceLightParams* lit, bool hybrid)
{
  if(t.samples_per_pass < 1 || t.samples_per_pass > 32)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: samples_per_pass must be in [1, 32]");
  if(!hybrid && t.max_passes < 1)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: max_passes must be at least 1");
  if(!(t.min_transmittance >= 0.0f && t.min_transmittance < 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: min_transmittance must be in [0, 1)");
  if(!hybrid && !(t.depth_iso_threshold >= 0.0f && t.depth_iso_threshold <= 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: depth_iso_threshold must be in [0, 1]");
  if(t.kernel_adaptive_clamping != 0 && t.kernel_adaptive_clamping != 1)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: kernel_adaptive_clamping must be 0 or 1");
  if(t.trace_strategy < MGS_TRACE_STRATEGY_FULL_ANYHIT || t.trace_strategy > MGS_TRACE_STRATEGY_STOCHASTIC_ANYHIT)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: trace_strategy must be MGS_TRACE_STRATEGY_FULL_ANYHIT, PASS_STOCHASTIC or STOCHASTIC_ANYHIT");
  if(p->width <= 0 || p->height <= 0 || p->width > 8192 || p->height > 8192)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: width/height must be in [1,8192]");
  if(p->target_format < MGS_TARGET_RGBA16F || p->target_format > MGS_TARGET_RGBA8)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: target_format must be MGS_TARGET_RGBA16F / RGBA32F / RGBA8");
  if(p->camera_model < MGS_CAMERA_PINHOLE || p->camera_model > MGS_CAMERA_FISHEYE)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: camera_model out of range");
  // kernel_min_response = 0 would make the proxy ellipsoid infinite (no finite bound, hence no leaf)
  if(!(p->alpha_clamp > 1.0f / 255.0f && p->alpha_clamp <= 1.0f) || !(p->kernel_min_response > 0.0f && p->kernel_min_response < 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: alpha_clamp must be in (1/255, 1] and kernel_min_response in (0, 1)");
  if(!(p->alpha_cull_threshold >= 0.0f))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: alpha_cull_threshold must be >= 0");
  if(p->kernel_degree != 8 && (p->kernel_degree < 0 || p->kernel_degree > 5))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: kernel_degree must be one of 0, 1, 2, 3, 4, 5, 8 (shaderio.h:112-119)");
  if(p->normal_method != MGS_NORMAL_MAX_DENSITY_PLANE && p->normal_method != MGS_NORMAL_ISO_SURFACE)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: normal_method must be MGS_NORMAL_MAX_DENSITY_PLANE or MGS_NORMAL_ISO_SURFACE");
  if(p->dof_mode < MGS_DOF_DISABLED || p->dof_mode > MGS_DOF_FIXED_FOCUS || p->frame_sample_id < 0)
    return failTrace(MGS_ERR_INVALID_ARG, "trace: dof_mode / frame_sample_id out of range");
  if(p->dof_mode != MGS_DOF_DISABLED && (!(p->aperture >= 0.0f) || !std::isfinite(p->aperture) || !(p->focus_dist > 0.0f) || !std::isfinite(p->focus_dist)))
    return failTrace(MGS_ERR_INVALID_ARG, "trace: depth of field needs a finite aperture >= 0 and a finite focus_dist > 0");
  if(hybrid)
  {
    if(p->pipeline != MGS_PIPELINE_3DGS && p->pipeline != MGS_PIPELINE_3DGUT)
      return failTrace(MGS_ERR_INVALID_ARG, "hybrid: pipeline must be MGS_PIPELINE_3DGS or MGS_PIPELINE_3DGUT");
    // the 3DGS hybrid's rays skip the lens (rgen.slang:191), and its raster pass knows neither lens nor fisheye rays
    if(p->pipeline == MGS_PIPELINE_3DGS && p->dof_mode != MGS_DOF_DISABLED)
      return failTrace(MGS_ERR_UNSUPPORTED, "hybrid: depth of field is a feature of the 3DGUT pipeline (per-pixel rays); the 3DGS pipeline has none");
    if(p->pipeline == MGS_PIPELINE_3DGS && p->camera_model != MGS_CAMERA_PINHOLE)
      return failTrace(MGS_ERR_INVALID_ARG, "hybrid: a fisheye camera needs MGS_PIPELINE_3DGUT (the 3DGS surface is a pinhole one)");
  }
  if(lit)
  {
    // (the reference also randomises the shadow rays under the any-hit strategy, rgen.slang:1364-1400)
    if(t.trace_strategy != MGS_TRACE_STRATEGY_FULL_ANYHIT)
      return failTrace(MGS_ERR_UNSUPPORTED, hybrid ? "mgs_render_hybrid: the stochastic trace strategies are mgs_render_traced's (trace_strategy must be 0)"
                                                   : "mgs_render_traced_lit: the stochastic trace strategies are mgs_render_traced's (trace_strategy must be 0)");
    if(lit->shadows_mode < MGS_SHADOWS_DISABLED || lit->shadows_mode > MGS_SHADOWS_SOFT)
      return failTrace(MGS_ERR_INVALID_ARG, "trace: shadows_mode must be MGS_SHADOWS_DISABLED, MGS_SHADOWS_HARD or MGS_SHADOWS_SOFT");
    if(!(lit->particle_shadow_offset >= 0.0f) || !std::isfinite(lit->particle_shadow_offset))
      return failTrace(MGS_ERR_INVALID_ARG, "trace: particle_shadow_offset must be finite and >= 0");
    if(!(lit->particle_shadow_transmittance_threshold >= 0.0f && lit->particle_shadow_transmittance_threshold < 1.0f))
      return failTrace(MGS_ERR_INVALID_ARG, "trace: particle_shadow_transmittance_threshold must be in [0, 1)");
    if(!(lit->particle_shadow_color_strength >= 0.0f && lit->particle_shadow_color_strength <= 1.0f))
      return failTrace(MGS_ERR_INVALID_ARG, "trace: particle_shadow_color_strength must be in [0, 1]");
    if(p->lighting_mode == MGS_LIGHTING_INDIRECT)
      return failTrace(MGS_ERR_UNSUPPORTED, "trace: indirect lighting needs bounces, which are out of scope");
    if(p->lighting_mode != MGS_LIGHTING_DIRECT)
      return failTrace(MGS_ERR_INVALID_ARG, hybrid ? "mgs_render_hybrid: lighting_mode must be MGS_LIGHTING_DIRECT (a hybrid frame without lighting is mgs_render's)"
                                                   : "mgs_render_traced_lit: lighting_mode must be MGS_LIGHTING_DIRECT");
    // within ABI 5.1 a caller that probes MGS_SHADOWS_SOFT keeps the answer it always got unless the process opts in
    if(lit->shadows_mode == MGS_SHADOWS_SOFT && !tuning().softShadows)
      return failTrace(MGS_ERR_UNSUPPORTED, "trace: soft shadows are off in this process; start it with MGS_SOFT_SHADOWS=1 (MGS_HAS_SOFT_SHADOWS)");
  }
  else
  {
    if(p->lighting_mode < MGS_LIGHTING_DISABLED || p->lighting_mode > MGS_LIGHTING_INDIRECT)
      return failTrace(MGS_ERR_INVALID_ARG, "trace: lighting_mode out of range");
    if(p->lighting_mode != MGS_LIGHTING_DISABLED)
      return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_traced: lighting_mode != 0 is mgs_render_traced_lit's");
  }
  if(p->sort_mode == MGS_SORT_STOCHASTIC)
    return failTrace(MGS_ERR_UNSUPPORTED, "trace: sort_mode has no meaning for a traced frame (the stochastic strategies are MgsTraceParams::trace_strategy)");
  return MGS_OK;
}

// The constants of a traced entry point's frame on handle s (not null), as the raster pipelines build them: the 3DGUT fields carry
// the ray's parameters.  q: the caller's own copy of the frame's parameters (a ray query's is without a camera), which leaves here
// with the pipeline and sort mode the constants were built for; what: the entry point's name for the messages; rayInverses:
// viewInverse / projInverse of the rays, host double, rounded once (a ray query has no camera to invert).
int traceFrameArgs(MgsScene s, MgsFrameParams& q, const char* what, bool rayInverses, std::unique_ptr<FrameArgs>& A)
{
  SceneData& d     = *s->d;
  const bool empty = d.instances.empty();
  if(!empty && !d.committed)
    return failTrace(MGS_ERR_STATE, std::string(what) + ": call mgs_scene_commit first");
  HIPCHK(hipSetDevice(s->device));
  if(!empty)
    if(int wrc = ensureWorkingSet(s))
      return wrc;
  q.pipeline  = MGS_PIPELINE_3DGUT;
  q.sort_mode = MGS_SORT_GPU_RADIX;
  // (with a sensor bound to the handle, buildFrameArgs fills FrameConst::sensor and clears partitionCull for this 3DGUT frame too.  Of
  // the callers only mgs_trace_generate_rays reads it: the traced frames refuse before they get here, and the ray queries, which "do
  // not look at the binding", launch k_trace_rays, which reads neither field.)
  A           = std::make_unique<FrameArgs>();
  if(int rc = buildFrameArgs(s, &q, *A))
    return rc;
  if(rayInverses)
  {
    mat4InverseDouble(q.view, A->f.lightViewInv);
    mat4InverseDouble(q.proj, A->f.lightProjInv);
  }
  return MGS_OK;
}

// everything the hierarchy depends on, as bytes: a traced frame whose signature differs rebuilds
static std::vector<uint8_t> bvhSignature(const SceneData& d, const TraceProxy& proxy)
{
  std::vector<uint8_t> sig;
  auto put = [&](const void* p, size_t n) { sig.insert(sig.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  put(&d.epoch, sizeof(d.epoch));
  put(&proxy, sizeof(proxy));
  for(const Instance& I : d.instances)
  {
    put(&I.set, sizeof(I.set));
    put(I.M, sizeof(I.M));
  }
  return sig;
}

// the frame in which the Morton codes are quantised: the union of the instances' transformed set boxes (finite centres only)
void sceneBox(const SceneData& d, float lo[3], float invExt[3])
{
  double wl[3] = {1e300, 1e300, 1e300}, wh[3] = {-1e300, -1e300, -1e300};
  std::vector<std::array<float, 6>> setBox(d.sets.size());
  for(size_t si = 0; si < d.sets.size(); ++si)
  {
    std::array<float, 6> b = {3e38f, 3e38f, 3e38f, -3e38f, -3e38f, -3e38f};
    const auto&          pos = d.sets[si].host->positions;
    for(size_t i = 0; i + 2 < pos.size(); i += 3)
      if(std::isfinite(pos[i]) && std::isfinite(pos[i + 1]) && std::isfinite(pos[i + 2]))
        for(int a = 0; a < 3; ++a)
        {
          b[a]     = std::min(b[a], pos[i + a]);
          b[3 + a] = std::max(b[3 + a], pos[i + a]);
        }
    setBox[si] = b;
  }
  for(const Instance& I : d.instances)
  {
    const auto& b = setBox[I.set];
    if(b[0] > b[3])
      continue;
    for(int corner = 0; corner < 8; ++corner)
    {
      const double x = (corner & 1) ? b[3] : b[0], y = (corner & 2) ? b[4] : b[1], z = (corner & 4) ? b[5] : b[2];
      for(int a = 0; a < 3; ++a)
      {
        const double v = (double)I.M[a] * x + (double)I.M[4 + a] * y + (double)I.M[8 + a] * z + (double)I.M[12 + a];
        if(std::isfinite(v))
        {
          wl[a] = std::min(wl[a], v);
          wh[a] = std::max(wh[a], v);
        }
      }
    }
  }
  for(int a = 0; a < 3; ++a)
  {
    const double ext = wh[a] - wl[a];
    lo[a]            = wl[a] <= wh[a] ? (float)wl[a] : 0.0f;
    invExt[a]        = (ext > 0.0 && std::isfinite(ext)) ? (float)(1.0 / ext) : 0.0f;
  }
}

// (re)build the scene's hierarchy on handle s; the frame's constants A are already on the device (s->fb.dArgs)
static int buildBvh(MgsScene s, const FrameArgs& A, const TraceProxy& proxy, std::vector<uint8_t>&& sig, float* buildMs)
{
  SceneData&      d = *s->d;
  TraceBvhState&  B = d.bvh;
  TracePassState& t = s->trace;
  hipStream_t     st = s->stream;
  {  // the frames in flight on every context read the hierarchy this call rewrites: the rule of mgs_scene_set_lights
    std::lock_guard<std::mutex> lk(d.mtx);
    for(MgsScene_t* h : d.handles)
      if(h != s)
        HIPCHK(hipStreamSynchronize(h->stream));
  }
  B.built = false;
  const uint32_t n = d.totalSplats;
  int            rc;
  if((rc = B.inst.ensure(1))) return rc;
  if((rc = B.callerId.ensure(n))) return rc;
  if((rc = t.keys.ensure(n))) return rc;
  if((rc = t.vals.ensure(n))) return rc;
  if((rc = t.leafBox.ensure(2 * (size_t)n))) return rc;
  if((rc = t.leafCount.ensure(1))) return rc;
  {
    auto tab = std::make_unique<TraceInstTable>();
    std::memset(tab.get(), 0, sizeof(TraceInstTable));
    std::vector<uint32_t> caller(n);
    uint32_t              off = 0;
    for(size_t k = 0; k < d.instances.size(); ++k)
    {
      rotScaleInverse(d.instances[k].M, tab->inst[k].rsInv);
      const DeviceSet& ds = d.sets[d.instances[k].set];
      for(uint32_t i = 0; i < ds.count; ++i)
        caller[off + i] = off + ds.newToOld[i];
      off += ds.count;
    }
    HIPCHK(hipMemcpyAsync(B.inst.p, tab.get(), sizeof(TraceInstTable), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(B.callerId.p, caller.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // the sources are locals
  }
  HIPCHK(hipEventRecord(t.ev[kEvBuildBegin], st));
  BvhBuildArgs L{};
  L.frame = s->fb.dArgs.p;
  L.proxy = proxy;
  sceneBox(d, L.sceneLo, L.sceneInvExt);
  std::memcpy(B.sceneLo, L.sceneLo, sizeof(B.sceneLo));
  std::memcpy(B.sceneInvExt, L.sceneInvExt, sizeof(B.sceneInvExt));
  B.splats      = n;
  L.totalSplats = n;
  L.keys        = t.keys.p;
  L.vals        = t.vals.p;
  L.leafBox     = t.leafBox.p;
  launchBvhLeaves(st, L);
  HIPCHK(hipGetLastError());
  // the library's own (key, value) sort: LSD radix, stable, so equal Morton codes keep the order of the global storage ids
  if((rc = mgs_radix_sort_u32(s, t.keys.p, t.vals.p, n, 0, 32, nullptr))) return rc;
  HIPCHK(hipMemsetAsync(t.leafCount.p, 0, 4, st));
  launchBvhCount(st, t.keys.p, n, t.leafCount.p);
  uint32_t leaves = 0;
  HIPCHK(hipMemcpyAsync(&leaves, t.leafCount.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  B.nLevels    = 0;
  B.totalNodes = 0;
  B.leaves     = leaves;
  std::memset(B.levelOffset, 0, sizeof(B.levelOffset));
  std::memset(B.levelCount, 0, sizeof(B.levelCount));
  for(uint32_t c = leaves; c > 0 && B.nLevels < kBvhMaxLevels;)
  {  // level 0: the leaves; then ceil(count / 8) until a level has one node
    B.levelOffset[B.nLevels] = B.totalNodes;
    B.levelCount[B.nLevels]  = c;
    B.totalNodes += c;
    ++B.nLevels;
    if(c == 1)
      break;
    c = (c + 7u) / 8u;
  }
  if((rc = B.nodes.ensure(2 * (size_t)std::max<uint32_t>(B.totalNodes, 1u)))) return rc;
  launchBvhGather(st, t.vals.p, t.leafBox.p, B.nodes.p, leaves);
  for(int l = 1; l < B.nLevels; ++l)  // one plain kernel per level
    launchBvhLevel(st, B.nodes.p + 2 * (size_t)B.levelOffset[l - 1], B.levelCount[l - 1], B.nodes.p + 2 * (size_t)B.levelOffset[l], B.levelCount[l]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(t.ev[kEvBuildEnd], st));
  HIPCHK(hipStreamSynchronize(st));  // other contexts may trace over it as soon as this call returns
  HIPCHK(hipEventElapsedTime(buildMs, t.ev[kEvBuildBegin], t.ev[kEvBuildEnd]));
  t.keys.release(), t.vals.release(), t.leafBox.release();
  B.proxy     = proxy;
  B.signature = std::move(sig);
  B.built     = true;
  return MGS_OK;
}

// the scene's hierarchy for this frame's proxy: rebuilt when its signature differs (the frame's constants are on the device)
int ensureHierarchy(MgsScene s, const FrameArgs& A, const TraceProxy& proxy, float* buildMs, uint32_t* rebuilt)
{
  SceneData& d = *s->d;
  *buildMs = 0.0f;
  *rebuilt = 0;
  if(d.instances.empty())
    return MGS_OK;
  std::vector<uint8_t> sig = bvhSignature(d, proxy);
  if(d.bvh.built && sig == d.bvh.signature)
    return MGS_OK;
  *rebuilt = 1;
  return buildBvh(s, A, proxy, std::move(sig), buildMs);
}

int ensureTraceEvents(TracePassState& ts)
{
  if(!ts.ev[kEvBuildBegin])
    for(auto& e : ts.ev)
      HIPCHK(hipEventCreate(&e));
  return MGS_OK;
}

// a light pass's scratch and the scene's light table
static int ensureLightScratch(MgsScene s, size_t pixels)
{
  TracePassState& ts = s->trace;
  int             rc;
  if((rc = ts.isoDist.ensure(pixels))) return rc;
  if((rc = ts.radiance.ensure(pixels))) return rc;
  if((rc = ts.shadowHits.ensure(pixels))) return rc;
  if((rc = ts.lctr.ensure(1))) return rc;
  return ensureLightTable(*s->d);
}

// what every kernel of the traced pipeline receives: frame, hierarchy, proxy, the rays' knobs, the image (the outputs stay null)
TraceArgs traceArgs(MgsScene s, const TraceProxy& proxy, const MgsTraceParams& t, int fmt)
{
  SceneData& d = *s->d;
  TraceArgs  L{};
  L.frame    = s->fb.dArgs.p;
  L.nodes    = d.bvh.nodes.p;
  L.callerId = d.bvh.callerId.p;
  L.inst     = d.bvh.inst.p;
  L.ctr      = s->trace.ctr.p;
  if(!d.instances.empty())
  {
    std::memcpy(L.levelOffset, d.bvh.levelOffset, sizeof(L.levelOffset));
    std::memcpy(L.levelCount, d.bvh.levelCount, sizeof(L.levelCount));
    L.nLevels    = d.bvh.nLevels;
    L.totalNodes = d.bvh.totalNodes;
  }
  L.proxy             = proxy;
  L.samplesPerPass    = t.samples_per_pass;
  L.maxPasses         = t.max_passes;
  L.minTransmittance  = t.min_transmittance;
  L.depthIsoThreshold = t.depth_iso_threshold;
  L.image             = s->fb.image.p;
  L.fmt               = fmt;
  return L;
}

// the light pass over the surface in the handle's scratch (ray parameter, fp32 radiance), the picked ids and the given normals
static TraceLightArgs traceLightArgs(MgsScene s, const TraceArgs& L, const MgsTraceLightParams& lt, const uint32_t* pickId, const float4* normal)
{
  SceneData&      d  = *s->d;
  TracePassState& ts = s->trace;
  TraceLightArgs  G{};
  G.t                   = L;
  G.isoDist             = ts.isoDist.p;
  G.pickId              = pickId;
  G.normal              = normal;
  G.radiance            = ts.radiance.p;
  G.table               = d.lightTab.p;
  G.shadowHits          = ts.shadowHits.p;
  G.lctr                = ts.lctr.p;
  G.shadowsMode         = lt.shadows_mode;
  G.shFormat            = shFormatIndex(d.shFormat);
  G.shadowOffset        = lt.particle_shadow_offset;
  G.shadowThreshold     = lt.particle_shadow_transmittance_threshold;
  G.shadowColorStrength = lt.particle_shadow_color_strength;
  return G;
}

// the shadow rays' counters and the time between the light pass's events; waits
static int readLightOut(MgsScene s, MgsTraceLightOut* lout)
{
  TracePassState& ts = s->trace;
  std::memset(lout, 0, sizeof(*lout));
  TraceLightCounters hc{};
  HIPCHK(hipMemcpyAsync(&hc, ts.lctr.p, sizeof(hc), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  lout->shadow_rays            = hc.shadowRays;
  lout->shadow_node_visits     = hc.nodeVisits;
  lout->shadow_candidate_tests = hc.candidateTests;
  lout->shadow_accepted_hits   = hc.acceptedHits;
  HIPCHK(hipEventElapsedTime(&lout->light_ms, ts.ev[kEvLightBegin], ts.ev[kEvLightEnd]));
  return MGS_OK;
}

int TraceOutRead::begin(MgsScene s)
{
  HIPCHK(hipMemcpyAsync(&hc, s->trace.ctr.p, sizeof(hc), hipMemcpyDeviceToHost, s->stream));
  return MGS_OK;
}

int TraceOutRead::finish(MgsScene s, uint32_t rebuilt, float buildMs, MgsTraceOut* out) const
{
  const SceneData& d     = *s->d;
  const bool       empty = d.instances.empty();
  out->leaves          = empty ? 0 : d.bvh.leaves;
  out->nodes           = empty ? 0 : d.bvh.totalNodes;
  out->node_visits     = hc.nodeVisits;
  out->candidate_tests = hc.candidateTests;
  out->accepted_hits   = hc.acceptedHits;
  out->max_passes_used = hc.maxPassesUsed;
  out->bvh_rebuilt     = rebuilt;
  out->build_ms        = buildMs;
  HIPCHK(hipEventElapsedTime(&out->trace_ms, s->trace.ev[kEvTraverseBegin], s->trace.ev[kEvTraverseEnd]));
  return MGS_OK;
}

// The mesh step of a traced frame's set-up on a handle whose setting is on: the per-pixel buffers, the lazy build of the triangle
// hierarchy exactly as a mesh query runs it, and what the frame's kernels receive of it.  `hierarchy` comes back locked: the caller
// holds it to the frame's last launch, so that a rebuild on another context (which waits for every stream) never frees nodes a
// launched kernel still reads.  active: a visible instance has a leaf; without one the frame's kernels are the ones of a frame with
// the setting off, and only the (all-miss) hit records are written.
static int traceMeshSetUp(MgsScene s, size_t pixels, bool lit, std::unique_lock<std::mutex>& hierarchy, TraceMeshArgs& M, bool& active)
{
  SceneData&      d  = *s->d;
  TraceMeshState& tm = s->traceMesh;
  TracePassState& ts = s->trace;
  int             rc;
  if(!tm.ev[0])
    for(auto& e : tm.ev)
      HIPCHK(hipEventCreate(&e));
  if((rc = tm.hits.ensure(4 * pixels))) return rc;
  if((rc = tm.meshT.ensure(pixels))) return rc;
  if((rc = tm.walkT.ensure(pixels))) return rc;
  if((rc = tm.ctr.ensure(2))) return rc;
  hierarchy = std::unique_lock<std::mutex>(d.meshBvh.mtx);
  if((rc = ensureMeshHierarchyLocked(s, &tm.buildMs, &tm.rebuilt))) return rc;
  const MeshBvhState& B = d.meshBvh;
  tm.triangles = B.triangles, tm.leaves = B.leaves, tm.nodes = B.totalNodes;
  active = false;
  if(d.meshHost && B.nLevels > 0)
    for(uint32_t k = 0; k < d.meshHost->count; ++k)
      active = active || (d.meshHost->inst[k].visible != 0u && d.meshHost->inst[k].triCount > 0u);
  if(active && !lit)  // the composite adds to the fp32 pixel, which an unlit frame otherwise does not keep
  {
    if((rc = ts.isoDist.ensure(pixels))) return rc;
    if((rc = ts.radiance.ensure(pixels))) return rc;
  }
  M = TraceMeshArgs{};
  if(active)
  {  // (an inactive frame's primary kernel walks nothing: nLevels stays 0 and every record is a miss)
    M.h.nodes      = B.nodes.p;
    M.h.nLevels    = B.nLevels;
    M.h.totalNodes = B.totalNodes;
    std::memcpy(M.h.levelOffset, B.levelOffset, sizeof(M.h.levelOffset));
    std::memcpy(M.h.levelCount, B.levelCount, sizeof(M.h.levelCount));
    M.tris  = B.tris.p;
    M.table = d.meshTab.p;
  }
  M.hits  = tm.hits.p;
  M.meshT = tm.meshT.p;
  M.walkT = tm.walkT.p;
  M.ctr   = tm.ctr.p;
  M.minT  = tm.minT;
  return MGS_OK;
}

// The end of trace_ms.  A lit frame records it before its light pass, which has light_ms; an unlit frame behind the temporal
// accumulation, the last work of the frame.
static int endTraversal(TracePassState& ts, hipStream_t st)
{
  HIPCHK(hipEventRecord(ts.ev[kEvTraverseEnd], st));
  return MGS_OK;
}

// lit: the frame of mgs_render_traced_lit (lp NULL = the defaults); otherwise lp and lout are not looked at
// bounce: the frame of mgs_render_traced_indirect (a lit frame whose mesh composite is the indirect one, followed by max_bounces
// bounce launches); bout is then not looked at otherwise
static int mgs_render_traced_impl(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, MgsTraceOut* out, bool lit = false,
                                  const MgsTraceLightParams* lp = nullptr, MgsTraceLightOut* lout = nullptr,
                                  const MgsTraceBounceParams* bounce = nullptr, MgsTraceBounceOut* bout = nullptr)
{
  const bool indirect = bounce != nullptr;
  // the entry point's name for the messages that are raised in here (the other frames keep theirs as they were)
  const std::string who = indirect ? "mgs_render_traced_indirect" : "mgs_render_traced";
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, who + ": null params");
  const MgsTraceParams      t  = traceParamsOr(tp);
  const MgsTraceLightParams lt = traceLightParamsOr(lit ? lp : nullptr);
  // An indirect frame's bounce 0 IS the lit mesh frame: the lit frame's checks and the frame's constants are those of
  // MGS_LIGHTING_DIRECT (`lp0`, and `q` below); the caller's own parameters, lighting_mode included, are what the handle records.
  MgsFrameParams lp0 = *p;
  if(indirect)
    lp0.lighting_mode = MGS_LIGHTING_DIRECT;
  if(int rc = validateTrace(&lp0, t, lit ? &lt : nullptr))  // (before the handle is looked at: the ranges can be checked without a device)
    return rc;
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, who + ": null scene");
  if(s->occ.depth)
    return failTrace(MGS_ERR_UNSUPPORTED, who + ": an occluder is bound (meshes in the traced scene are out of scope); unbind it with "
                                          "mgs_frame_set_occluder(handle, NULL, NULL, 0, 0)");
  if(int rc = refuseBoundSensor(s, indirect ? "mgs_render_traced_indirect" : lit ? "mgs_render_traced_lit" : "mgs_render_traced", "the traced frames generate the perfect cameras' rays; trace the sensor's "
                                                                                         "rays with mgs_trace_generate_rays and mgs_trace_rays_device"))
    return rc;
  const bool meshOn = s->traceMesh.enabled;
  if(indirect && !meshOn)
    return failTrace(MGS_ERR_STATE, "mgs_render_traced_indirect: the handle's trace-mesh setting is off (an indirect frame bounces off mesh materials); turn "
                                    "it on with mgs_frame_set_trace_meshes");
  if(meshOn && t.trace_strategy != MGS_TRACE_STRATEGY_FULL_ANYHIT)
    return failTrace(MGS_ERR_UNSUPPORTED, who + ": the stochastic trace strategies have no mesh hits; turn the setting off with "
                                          "mgs_frame_set_trace_meshes(handle, NULL) or use trace_strategy 0");
  MgsFrameParams q      = lp0;
  q.depth_iso_threshold = t.depth_iso_threshold;
  std::unique_ptr<FrameArgs> A;
  int                        rc;
  if((rc = traceFrameArgs(s, q, who.c_str(), true, A))) return rc;
  const FrameConst& F = A->f;
  if((rc = ensureFrameImage(s, &q, F))) return rc;
  TracePassState& ts = s->trace;
  if((rc = ensureTraceEvents(ts))) return rc;
  const size_t pixels = (size_t)F.width * F.height;
  if((rc = ts.hitCount.ensure(pixels))) return rc;
  if((rc = ts.ctr.ensure(1))) return rc;
  if(lit)  // scratch
    if((rc = ensureLightScratch(s, pixels))) return rc;
  if((rc = uploadFrameState(s, *A, s->stream))) return rc;
  const TraceProxy proxy   = traceProxy(*p, t);
  float            buildMs = 0.0f;
  uint32_t         rebuilt = 0;
  if((rc = ensureHierarchy(s, *A, proxy, &buildMs, &rebuilt))) return rc;
  hipStream_t st = s->stream;
  TraceMeshState&              tm = s->traceMesh;
  std::unique_lock<std::mutex> meshHierarchy;  // held from the mesh step's signature check to the frame's last launch
  TraceMeshArgs                M{};
  bool                         meshActive = false;
  if(meshOn)
  {  // launch order: mesh primary, k_trace, the light pass, the mesh composite
    if((rc = traceMeshSetUp(s, pixels, lit, meshHierarchy, M, meshActive))) return rc;
    if(indirect && meshActive)
    {  // the per-pixel bounce state (64 B a pixel), the counters, the scene's bounce materials
      if(!tm.bounceEv[0])
        for(auto& e : tm.bounceEv)
          HIPCHK(hipEventCreate(&e));
      if((rc = tm.bounceLive.ensure(pixels))) return rc;
      if((rc = tm.bounceRay.ensure(9 * pixels))) return rc;
      if((rc = tm.bounceT.ensure(3 * pixels))) return rc;
      if((rc = tm.bounceCtr.ensure(1))) return rc;
      if((rc = ensureBounceTable(*s->d))) return rc;
    }
    HIPCHK(hipMemsetAsync(tm.ctr.p, 0, 2 * sizeof(MeshRayCounters), st));
    HIPCHK(hipEventRecord(tm.ev[kTmevPrimaryBegin], st));
    launchTraceMeshPrimary(st, M, s->fb.dArgs.p, F);
    HIPCHK(hipEventRecord(tm.ev[kTmevPrimaryEnd], st));
  }
  HIPCHK(hipMemsetAsync(ts.ctr.p, 0, sizeof(TraceCounters), st));
  HIPCHK(hipEventRecord(ts.ev[kEvTraverseBegin], st));
  TraceArgs L = traceArgs(s, proxy, t, targetLayout(p->target_format).fmt);
  L.hitCount    = ts.hitCount.p;
  L.outDepth    = F.surfaceOutputs ? s->surf.depth.p : nullptr;
  L.outId       = F.surfaceOutputs ? s->surf.id.p : nullptr;
  L.outNormal   = F.surfaceOutputs ? s->surf.normal.p : nullptr;
  L.outIsoDist  = lit ? ts.isoDist.p : nullptr;  // what the light pass reads besides the side outputs
  L.outRadiance = lit ? ts.radiance.p : nullptr;
  if(meshActive)
  {  // the composite adds to the fp32 pixel
    L.outIsoDist  = ts.isoDist.p;
    L.outRadiance = ts.radiance.p;
  }
  TraceLightMeshArgs G{};  // (read only when meshActive, except G.l: the light pass's arguments of every lit frame)
  G.l      = traceLightArgs(s, L, lt, s->surf.id.p, s->surf.normal.p);
  G.m      = M;
  G.litOut = ts.radiance.p;
  if(meshActive)
  {  // k_trace only learns its per-pixel upper end, and leaves float(T) for the composite
    TraceWalkMeshArgs Wm{};
    Wm.t        = L;
    Wm.meshT    = tm.meshT.p;
    Wm.outWalkT = tm.walkT.p;
    Wm.meshMinT = tm.minT;
    launchTraceWithMeshes(st, Wm, F, s->d->shFormat);
  }
  else if(t.trace_strategy == MGS_TRACE_STRATEGY_FULL_ANYHIT)
    launchTrace(st, L, F, s->d->shFormat);
  else
    launchTraceStochastic(st, L, F, s->d->shFormat, t.trace_strategy);
  if(lit)
  {  // launch: the light pass rewrites the frame's pixels from the fp32 radiance k_trace left
    if((rc = endTraversal(ts, st))) return rc;
    HIPCHK(hipMemsetAsync(ts.lctr.p, 0, sizeof(TraceLightCounters), st));
    HIPCHK(hipEventRecord(ts.ev[kEvLightBegin], st));
    if(meshActive)
      launchTraceLightWithMeshes(st, G, F);
    else
      launchTraceLight(st, G.l, F);
    HIPCHK(hipEventRecord(ts.ev[kEvLightEnd], st));
  }
  if(meshActive)
  {
    HIPCHK(hipEventRecord(tm.ev[kTmevCompositeBegin], st));
    TraceBounceArgs B{};
    if(indirect)
    {
      B.g      = G;
      B.btab   = s->d->bounceTab.p;
      B.bmats  = s->d->bounceMatsDev.p;
      B.live   = tm.bounceLive.p;
      B.ray    = tm.bounceRay.p;
      B.T      = tm.bounceT.p;
      B.bctr   = tm.bounceCtr.p;
      B.pixels = pixels;
      HIPCHK(hipMemsetAsync(tm.bounceCtr.p, 0, sizeof(BounceCounters), st));
    }
    launchTraceMeshComposite(st, G, F, lit);
    HIPCHK(hipEventRecord(tm.ev[kTmevCompositeEnd], st));
    if(indirect)
    {  // the hand-over of bounce 0, then max_bounces rounds, unconditionally: a round without a live pixel reads the live words and no more
      HIPCHK(hipEventRecord(tm.bounceEv[0], st));
      launchTraceBouncePrimary(st, B, F);
      for(int b = 1; b <= bounce->max_bounces && b <= kMaxBounces; ++b)  // bound: kMaxBounces
      {
        B.bounce = b;
        launchTraceBounce(st, B, F, s->d->shFormat);
      }
      HIPCHK(hipEventRecord(tm.bounceEv[1], st));
    }
  }
  if(F.temporalSampling)
    launchPostAccumulate(st, s->fb.dArgs.p, s->fb.accum.p, s->fb.image.p, L.fmt);
  if(!lit)
    if((rc = endTraversal(ts, st))) return rc;
  HIPCHK(hipGetLastError());
  if(meshHierarchy.owns_lock())
    meshHierarchy.unlock();
  tm.have        = meshOn;
  tm.composited  = meshActive;
  tm.lit         = lit;
  tm.hybridFrame = false;
  // the frame is the handle's last frame, as after mgs_render (downloads, strips, image compare); no bin lists belong to it
  // (mgs_frame_row_costs: MGS_ERR_STATE)
  recordLastFrameHead(s->last, *p, F, false, true);
  ts.w    = F.width;
  ts.h    = F.height;
  ts.have = true;
  ts.haveLit = lit;  // the shadow hits are those of the last traced frame only when that frame was lit
  if(lit && lout)  // read-back
    if((rc = readLightOut(s, lout))) return rc;
  if(out)
  {
    std::memset(out, 0, sizeof(*out));
    TraceOutRead R;
    if((rc = R.begin(s))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if((rc = R.finish(s, rebuilt, buildMs, out))) return rc;
  }
  if(indirect && bout)
  {  // all zero when no visible mesh instance has a leaf: nothing bounced
    std::memset(bout, 0, sizeof(*bout));
    if(meshActive)
    {
      BounceCounters bc{};
      HIPCHK(hipMemcpyAsync(&bc, tm.bounceCtr.p, sizeof(bc), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for(int b = 0; b < kMaxBounces; ++b)
      {
        bout->rays[b]      = bc.rays[b];
        bout->mesh_hits[b] = bc.meshHits[b];
      }
      bout->particle_hits = bc.particleHits;
      HIPCHK(hipEventElapsedTime(&bout->bounce_ms, tm.bounceEv[0], tm.bounceEv[1]));
    }
  }
  return MGS_OK;
}

void mgs_trace_bounce_params_default(MgsTraceBounceParams* p)
{
  if(!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->max_bounces = 3;  // rtxMaxBounces, shaderio.h:273
}

static int mgs_render_traced_indirect_impl(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp,
                                           const MgsTraceBounceParams* bp, MgsTraceOut* out, MgsTraceLightOut* lout, MgsTraceBounceOut* bout)
{
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_traced_indirect: null params");
  MgsTraceBounceParams b;
  mgs_trace_bounce_params_default(&b);
  if(bp)
    b = *bp;
  // (before the handle is looked at: the ranges can be checked without a device)
  if(p->lighting_mode != MGS_LIGHTING_INDIRECT)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_traced_indirect: lighting_mode must be MGS_LIGHTING_INDIRECT (direct lighting is mgs_render_traced_lit's)");
  if(b.max_bounces < 1 || b.max_bounces > kMaxBounces)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_traced_indirect: max_bounces must be in [1, 16]");
  if(b.reserved[0] != 0 || b.reserved[1] != 0 || b.reserved[2] != 0)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_traced_indirect: the reserved words of MgsTraceBounceParams must be 0");
  const MgsTraceParams      t  = traceParamsOr(tp);
  const MgsTraceLightParams lt = traceLightParamsOr(lp);
  if(t.trace_strategy == MGS_TRACE_STRATEGY_PASS_STOCHASTIC || t.trace_strategy == MGS_TRACE_STRATEGY_STOCHASTIC_ANYHIT)
    return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_traced_indirect: the stochastic strategies' bounces are out of scope (trace_strategy must be 0)");
  if(lt.shadows_mode == MGS_SHADOWS_SOFT)
    return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_traced_indirect: soft shadows need the pixel's random state carried across the bounce launches, which is not built (MGS_SHADOWS_HARD or off)");
  // bounce 0 is the lit mesh frame: its checks, its set-up and its launches, with the composite and the rounds behind it exchanged
  return mgs_render_traced_impl(s, p, &t, out, true, &lt, lout, &b, bout);
}
int mgs_render_traced_indirect(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, const MgsTraceBounceParams* bp,
                               MgsTraceOut* out, MgsTraceLightOut* lout, MgsTraceBounceOut* bout)
{
  return guarded("mgs_render_traced_indirect", [&] { return mgs_render_traced_indirect_impl(s, p, tp, lp, bp, out, lout, bout); });
}

int mgs_render_traced(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, MgsTraceOut* out)
{
  return guarded("mgs_render_traced", [&] { return mgs_render_traced_impl(s, p, tp, out); });
}

int mgs_render_traced_lit(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, MgsTraceOut* out,
                          MgsTraceLightOut* lout)
{
  return guarded("mgs_render_traced_lit", [&] { return mgs_render_traced_impl(s, p, tp, out, true, lp, lout); });
}

// ---- hybrid frames: the raster pass supplies the primary surface, the light pass of the traced pipeline shades and shadows it ----
namespace {
struct HybridTail : FrameTail
{
  MgsScene                   s = nullptr;
  const MgsFrameParams*      p = nullptr;  // the caller's
  MgsTraceParams             t;
  MgsTraceLightParams        lt;
  float                      buildMs = 0.0f;
  uint32_t                   rebuilt = 0;

  // a frame with the handle's hybrid-mesh setting on (mgs_frame_set_hybrid_meshes): what the mesh step's set-up left.  meshActive: a
  // visible instance has a leaf, the raster pass runs against the pre-pass's depth plane and the mesh kernels replace the plain ones
  bool          meshOn = false, meshActive = false;
  TraceMeshArgs M{};

  TraceProxy proxy() const { return traceProxy(*p, t); }
  int        afterUpload(const FrameArgs& A) override
  {
    TracePassState& ts = s->trace;
    int             rc;
    if((rc = ensureTraceEvents(ts))) return rc;
    const size_t pixels = (size_t)A.f.width * A.f.height;
    if((rc = ts.hybridNormal.ensure(pixels))) return rc;
    if((rc = ensureLightScratch(s, pixels))) return rc;
    if((rc = ensureHierarchy(s, A, proxy(), &buildMs, &rebuilt))) return rc;
    if(meshOn)
    {  // the mesh depth pre-pass (rgen.slang:252-281): the closest walk on the pixel's ray, then the plane the raster pass is tested against
      TraceMeshState& tm = s->traceMesh;
      hipStream_t     st = s->stream;
      HIPCHK(hipMemsetAsync(tm.ctr.p, 0, 2 * sizeof(MeshRayCounters), st));
      HIPCHK(hipEventRecord(tm.ev[kTmevPrimaryBegin], st));
      launchTraceMeshPrimary(st, M, s->fb.dArgs.p, A.f);
      if(meshActive)
        launchHybridMeshDepth(st, s->fb.dArgs.p, tm.hits.p, tm.hybridDepth.p, A.f);
      HIPCHK(hipEventRecord(tm.ev[kTmevPrimaryEnd], st));
      HIPCHK(hipGetLastError());
    }
    return MGS_OK;
  }
  // the hand-over, the light pass and, in a frame whose meshes are active, the mesh shading over the hand-over's pixels: there the
  // hand-over also leaves T and the light pass's shadow rays ask the meshes first
  int afterFrame(const FrameArgs& A, int fmt) override
  {
    TracePassState&   ts = s->trace;
    TraceMeshState&   tm = s->traceMesh;
    const FrameConst& F  = A.f;
    hipStream_t       st = s->stream;
    HIPCHK(hipMemsetAsync(ts.lctr.p, 0, sizeof(TraceLightCounters), st));
    HIPCHK(hipEventRecord(ts.ev[kEvLightBegin], st));
    HybridSurfaceMeshArgs H{};
    H.a.frame       = s->fb.dArgs.p;
    H.a.image       = s->fb.image.p;
    H.a.depth       = s->surf.depth.p;
    H.a.id          = s->surf.id.p;
    H.a.normal      = s->surf.normal.p;
    H.a.outIsoDist  = ts.isoDist.p;
    H.a.outNormal   = ts.hybridNormal.p;
    H.a.outRadiance = ts.radiance.p;
    TraceLightMeshArgs G{};
    G.l = traceLightArgs(s, traceArgs(s, proxy(), t, fmt), lt, s->surf.id.p, ts.hybridNormal.p);
    if(meshActive)
    {
      H.meshT = tm.meshT.p;
      H.outT  = tm.walkT.p;
      H.minT  = tm.hybridMinT;
      launchHybridSurfaceWithMeshes(st, H, F, fmt);
      G.m      = M;
      G.litOut = ts.radiance.p;
      launchTraceLightWithMeshes(st, G, F);
      HIPCHK(hipEventRecord(ts.ev[kEvLightEnd], st));
      HIPCHK(hipEventRecord(tm.ev[kTmevCompositeBegin], st));
      launchHybridMeshComposite(st, G, F);
      HIPCHK(hipEventRecord(tm.ev[kTmevCompositeEnd], st));
    }
    else
    {
      launchHybridSurface(st, H.a, F, fmt);
      launchTraceLight(st, G.l, F);
      HIPCHK(hipEventRecord(ts.ev[kEvLightEnd], st));
    }
    if(F.temporalSampling)  // the lit sample is what the running mean folds in
      launchPostAccumulate(st, s->fb.dArgs.p, s->fb.accum.p, s->fb.image.p, fmt);
    HIPCHK(hipGetLastError());
    return MGS_OK;
  }
};
}  // namespace

static int mgs_render_hybrid_impl(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, MgsFrameOut* out,
                                  MgsTraceLightOut* lout)
{
  if(!p)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_hybrid: null params");
  HybridTail tail;
  tail.t  = traceParamsOr(tp);
  tail.lt = traceLightParamsOr(lp);
  if(int rc = validateTrace(p, tail.t, &tail.lt, true))  // (before the handle is looked at)
    return rc;
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_render_hybrid: null scene");
  if(s->occ.depth)
    return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_hybrid: an occluder is bound (shadowing mesh pixels needs meshes in the traced scene, which are out of "
                                          "scope); unbind it with mgs_frame_set_occluder(handle, NULL, NULL, 0, 0)");
  if(int rc = refuseBoundSensor(s, "mgs_render_hybrid", "the shadow rays start from a surface unprojected through the perfect cameras"))
    return rc;
  TraceMeshState& tm     = s->traceMesh;
  const bool      meshOn = tm.hybridEnabled;
  if(!meshOn && tm.enabled)
    return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_hybrid: mesh hits are mgs_render_traced's and mgs_render_traced_lit's; a hybrid frame's meshes are "
                                          "mgs_frame_set_hybrid_meshes'.  Turn the setting off with mgs_frame_set_trace_meshes(handle, NULL)");
  if(meshOn && tail.lt.shadows_mode == MGS_SHADOWS_SOFT)
    return failTrace(MGS_ERR_UNSUPPORTED, "mgs_render_hybrid: soft shadows with mgs_frame_set_hybrid_meshes on are not built (the mesh composite continues the "
                                          "light pass's random state, whose conditions differ in a hybrid frame); MGS_SHADOWS_HARD or off");
  tail.s = s;
  tail.p = p;
  // a frame that fails below must not leave the previous frame's flags over buffers its pre-pass may already have rewritten
  tm.hybridFrame = false;
  if(meshOn)
    tm.have = false;
  std::unique_lock<std::mutex> meshHierarchy;  // held from the mesh step's signature check to the frame's last launch
  if(meshOn && s->d->committed)
  {  // (an uncommitted scene: renderFrame says so)
    HIPCHK(hipSetDevice(s->device));
    const size_t pixels = (size_t)p->width * (size_t)p->height;
    if(int rc = traceMeshSetUp(s, pixels, true, meshHierarchy, tail.M, tail.meshActive))
      return rc;
    tail.M.minT = tm.hybridMinT;
    tail.meshOn = true;
    if(tail.meshActive)
    {
      if(pixels > tm.hybridDepth.n && tm.hybridDepth.p && s->surf.lastOccDepth == tm.hybridDepth.p)
        s->surf.lastOccGone = true;  // the plane the last frame was tested against is about to be freed (mgs_frame_download_surface, which = 3)
      if(int rc = tm.hybridDepth.ensure(pixels))
        return rc;
      tail.occDepth = tm.hybridDepth.p;
    }
  }
  // step 1: exactly mgs_render's unlit frame with the surface outputs on (the deferred pass is off in hybrid mode, NEED_SURFACE_INFO on)
  MgsFrameParams q  = *p;
  q.lighting_mode   = MGS_LIGHTING_DISABLED;
  q.surface_outputs = 1;
  if(int rc = renderFrame(s, &q, out, &tail))
    return rc;
  if(meshHierarchy.owns_lock())
    meshHierarchy.unlock();
  s->last.params.lighting_mode = p->lighting_mode;  // (surface_outputs stays 1: the raster pass's outputs are there to download)
  TracePassState& ts = s->trace;
  ts.w       = p->width;
  ts.h       = p->height;
  ts.have    = false;  // no primary walk: there are no hit counts
  ts.haveLit = true;
  tm.hybridFrame = tail.meshOn;  // the pre-pass's hit records and the mesh rays' sums are this frame's
  if(tail.meshOn)
  {
    tm.have       = true;
    tm.composited = tail.meshActive;
    tm.lit        = true;
  }
  if(lout)
    return readLightOut(s, lout);
  return MGS_OK;
}
int mgs_render_hybrid(MgsScene s, const MgsFrameParams* p, const MgsTraceParams* tp, const MgsTraceLightParams* lp, MgsFrameOut* out, MgsTraceLightOut* lout)
{
  return guarded("mgs_render_hybrid", [&] { return mgs_render_hybrid_impl(s, p, tp, lp, out, lout); });
}

// one per-pixel plane of the handle's last traced frame to the host; waits.  have: the last frame wrote the plane (noFrame is the
// message when it did not); tooSmall: the message for a destination, or a plane, smaller than that frame
static int downloadTracePlane(MgsScene s, uint32_t* dst, size_t count, DevBuf<uint32_t> TracePassState::*plane, bool TracePassState::*have,
                              const char* what, const char* noFrame, const char* tooSmall)
{
  if(!s || !dst)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null argument");
  const TracePassState& ts = s->trace;
  if(!(ts.*have))
    return failTrace(MGS_ERR_STATE, noFrame);
  const size_t n = (size_t)ts.w * (size_t)ts.h;
  if(count < n || (ts.*plane).n < n)
    return failTrace(MGS_ERR_INVALID_ARG, tooSmall);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(dst, (ts.*plane).p, n * 4, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}

int mgs_trace_download_shadow_hits(MgsScene s, uint32_t* dst, size_t count)
{
  return downloadTracePlane(s, dst, count, &TracePassState::shadowHits, &TracePassState::haveLit, "mgs_trace_download_shadow_hits",
                            "mgs_trace_download_shadow_hits: the handle's last traced frame was not a lit one",
                            "mgs_trace_download_shadow_hits: destination too small, or the last traced frame was not lit at this size");
}

// (a frame that has hit counts sized their plane: only the destination can be too small)
int mgs_trace_download_hit_counts(MgsScene s, uint32_t* dst, size_t count)
{
  return downloadTracePlane(s, dst, count, &TracePassState::hitCount, &TracePassState::have, "mgs_trace_download_hit_counts",
                            "mgs_trace_download_hit_counts: no traced frame yet", "mgs_trace_download_hit_counts: destination too small");
}

// ---- mesh hits in the traced frames: the handle's setting, the last frame's hit records and its mesh rays' statistics ----
// the ranges of MgsTraceMeshParams, which can be checked without a device; `fn`: the entry point's name for the message
static int checkTraceMeshParams(const char* fn, const MgsTraceMeshParams* p)
{
  if(!p)
    return MGS_OK;
  if(p->enabled != 0 && p->enabled != 1)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(fn) + ": enabled must be 0 or 1");
  if(!(p->min_mesh_composite_transmittance >= 0.0f && p->min_mesh_composite_transmittance <= 1.0f))
    return failTrace(MGS_ERR_INVALID_ARG, std::string(fn) + ": min_mesh_composite_transmittance must be in [0, 1]");
  if(p->reserved[0] != 0 || p->reserved[1] != 0)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(fn) + ": the reserved words of MgsTraceMeshParams must be 0");
  return MGS_OK;
}

int mgs_frame_set_trace_meshes(MgsScene s, const MgsTraceMeshParams* p)
{
  return guarded("mgs_frame_set_trace_meshes", [&]() -> int {
    if(int rc = checkTraceMeshParams("mgs_frame_set_trace_meshes", p))  // (before the handle is looked at)
      return rc;
    if(!s)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_frame_set_trace_meshes: null scene");
    s->traceMesh.enabled = p != nullptr && p->enabled == 1;
    s->traceMesh.minT    = p ? p->min_mesh_composite_transmittance : 0.0f;
    return (int)MGS_OK;
  });
}

int mgs_frame_set_hybrid_meshes(MgsScene s, const MgsTraceMeshParams* p)
{
  return guarded("mgs_frame_set_hybrid_meshes", [&]() -> int {
    if(int rc = checkTraceMeshParams("mgs_frame_set_hybrid_meshes", p))  // (before the handle is looked at)
      return rc;
    if(!s)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_frame_set_hybrid_meshes: null scene");
    s->traceMesh.hybridEnabled = p != nullptr && p->enabled == 1;
    s->traceMesh.hybridMinT    = p ? p->min_mesh_composite_transmittance : 0.0f;
    return (int)MGS_OK;
  });
}

int mgs_debug_download_hybrid_depth(MgsScene s, float* dst, size_t count)
{
  return guarded("mgs_debug_download_hybrid_depth", [&]() -> int {
    if(!s || !dst)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_debug_download_hybrid_depth: null argument");
    const TraceMeshState& tm = s->traceMesh;
    if(!tm.hybridFrame || !tm.composited)
      return failTrace(MGS_ERR_STATE, "mgs_debug_download_hybrid_depth: the handle's last frame was not a hybrid frame that ran its mesh depth pre-pass "
                                      "(mgs_frame_set_hybrid_meshes on, a visible mesh instance with a leaf)");
    const size_t n = (size_t)s->trace.w * (size_t)s->trace.h;
    if(count < n || tm.hybridDepth.n < n)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_debug_download_hybrid_depth: destination too small");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpyAsync(dst, tm.hybridDepth.p, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return (int)MGS_OK;
  });
}

int mgs_trace_download_mesh_hits(MgsScene s, MgsMeshHit* dst, size_t count)
{
  return guarded("mgs_trace_download_mesh_hits", [&]() -> int {
    if(!s || !dst)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_download_mesh_hits: null argument");
    const TraceMeshState& tm = s->traceMesh;
    if(!tm.have || !(s->trace.have || tm.hybridFrame))
      return failTrace(MGS_ERR_STATE, "mgs_trace_download_mesh_hits: the handle's last traced frame did not run with mgs_frame_set_trace_meshes on (nor its last hybrid frame with mgs_frame_set_hybrid_meshes)");
    const size_t n = (size_t)s->trace.w * (size_t)s->trace.h;
    if(count < n || tm.hits.n < 4 * n)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_download_mesh_hits: destination too small");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpyAsync(dst, tm.hits.p, n * sizeof(MgsMeshHit), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return (int)MGS_OK;
  });
}

int mgs_trace_mesh_stats(MgsScene s, MgsMeshRayOut* primary, MgsMeshRayOut* shadow)
{
  return guarded("mgs_trace_mesh_stats", [&]() -> int {
    if(!s)
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_mesh_stats: null scene");
    const TraceMeshState& tm = s->traceMesh;
    if(!tm.have || !(s->trace.have || tm.hybridFrame))
      return failTrace(MGS_ERR_STATE, "mgs_trace_mesh_stats: the handle's last traced frame did not run with mgs_frame_set_trace_meshes on (nor its last hybrid frame with mgs_frame_set_hybrid_meshes)");
    HIPCHK(hipSetDevice(s->device));
    MeshRayCounters c[2] = {};
    HIPCHK(hipMemcpyAsync(c, tm.ctr.p, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    auto fill = [&](MgsMeshRayOut* o, const MeshRayCounters& k, int evBegin, int evEnd) -> int {
      std::memset(o, 0, sizeof(*o));
      o->triangles      = tm.triangles;
      o->leaves         = tm.leaves;
      o->nodes          = tm.nodes;
      o->node_visits    = k.nodeVisits;
      o->triangle_tests = k.triangleTests;
      o->hits           = k.hits;
      o->invalid_rays   = k.invalidRays;
      o->bvh_rebuilt    = tm.rebuilt;
      o->build_ms       = tm.buildMs;
      HIPCHK(hipEventElapsedTime(&o->trace_ms, tm.ev[evBegin], tm.ev[evEnd]));
      return (int)MGS_OK;
    };
    if(primary)
      if(int rc = fill(primary, c[0], kTmevPrimaryBegin, kTmevPrimaryEnd))
        return rc;
    if(shadow)
    {
      std::memset(shadow, 0, sizeof(*shadow));  // all zero after an unlit frame
      if(tm.lit && tm.composited)
        if(int rc = fill(shadow, c[1], kTmevCompositeBegin, kTmevCompositeEnd))
          return rc;
    }
    return (int)MGS_OK;
  });
}

// mgs_debug_download_hierarchy(which = 0): the splat hierarchy as the last build left it, through host memory alone
static int downloadSplatHierarchy(MgsScene s, MgsHierarchyInfo* info, float* nodes8, size_t nodeCapacity)
{
  const TraceBvhState& B = s->d->bvh;
  if(!B.built)
    return failTrace(MGS_ERR_STATE, "mgs_debug_download_hierarchy: no splat hierarchy has been built yet (a traced frame or query builds it)");
  if(nodes8 && nodeCapacity < B.totalNodes)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_debug_download_hierarchy: node_capacity is below total_nodes");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  std::memset(info, 0, sizeof(*info));
  info->levels      = (uint32_t)B.nLevels;
  info->total_nodes = B.totalNodes;
  info->leaves      = B.leaves;
  info->primitives  = B.splats;
  static_assert(sizeof(info->level_offset) == sizeof(B.levelOffset) && sizeof(info->level_count) == sizeof(B.levelCount), "MgsHierarchyInfo: kBvhMaxLevels levels");
  std::memcpy(info->level_offset, B.levelOffset, sizeof(info->level_offset));
  std::memcpy(info->level_count, B.levelCount, sizeof(info->level_count));
  std::memcpy(info->box_lo, B.sceneLo, sizeof(info->box_lo));
  std::memcpy(info->box_inv_ext, B.sceneInvExt, sizeof(info->box_inv_ext));
  if(nodes8 && B.totalNodes)
    HIPCHK(hipMemcpy(nodes8, B.nodes.p, (size_t)B.totalNodes * 32, hipMemcpyDeviceToHost));
  return MGS_OK;
}

int mgs_debug_download_hierarchy(MgsScene s, int which, MgsHierarchyInfo* info, float* nodes8, size_t nodeCapacity, float* tris12, size_t triCapacity)
{
  return guarded("mgs_debug_download_hierarchy", [&]() -> int {
    if(!s || !info || (which != 0 && which != 1))
      return failTrace(MGS_ERR_INVALID_ARG, "mgs_debug_download_hierarchy: null scene or info, or which is neither 0 (splats) nor 1 (triangles)");
    return which == 0 ? downloadSplatHierarchy(s, info, nodes8, nodeCapacity) : downloadMeshHierarchy(s, info, nodes8, nodeCapacity, tris12, triCapacity);
  });
}
