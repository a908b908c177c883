// api_frame.hip — a frame: occluder binding, mgs_render, timings, statistics and the downloads of what a frame leaves.
//
// Host orchestration replaces GaussianSplatting::processSortingOnGPU / drawSplatPrimitives
// (src/gaussian_splatting.cpp:1298-1465): everything after the parameter upload is GPU-driven —
// counts stay on the device (IndirectParams, shaders/shaderio.h:343-356) and are read back only
// for statistics, like readBackIndirectParametersIfNeeded (:1536).
#include <cmath>
#include <string>

#include "scene_state.h"

// ---- occluder: the caller's opaque geometry -----------------------------------------------------------------------------
// The reference's hybrid pipeline draws the meshes' depth first, tests the splats against it and adds the meshes' colour behind
// them (src/gaussian_splatting.cpp:697-805, 2343-2356).  The library consumes the two images such a rasterisation yields.
int mgs_frame_set_occluder(MgsScene s, const float* depthDevice, const float* colorDevice, int width, int height)
{
  if(!s)
  {
    setError("mgs_frame_set_occluder: null handle");
    return MGS_ERR_INVALID_ARG;
  }
  if(!depthDevice)
  {  // unbind both
    s->occ.depth = s->occ.color = nullptr;
    s->occ.w = s->occ.h = 0;
    return MGS_OK;
  }
  if(width <= 0 || height <= 0)
  {
    setError("mgs_frame_set_occluder: width and height must be positive");
    return MGS_ERR_INVALID_ARG;
  }
  s->occ.depth = depthDevice;
  s->occ.color = colorDevice;
  s->occ.w     = width;
  s->occ.h     = height;
  return MGS_OK;
}

static int mgs_frame_upload_occluder_impl(MgsScene s, const float* depthHost, const float* colorHost, int width, int height)
{
  if(!s)
  {
    setError("mgs_frame_upload_occluder: null handle");
    return MGS_ERR_INVALID_ARG;
  }
  if(!depthHost)
    return mgs_frame_set_occluder(s, nullptr, nullptr, 0, 0);
  if(width <= 0 || height <= 0)
  {
    setError("mgs_frame_upload_occluder: width and height must be positive");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  const size_t n = (size_t)width * (size_t)height;
  // frames in flight may still read the previous copy (and captured graphs point at it): wait before it is rewritten or moved
  HIPCHK(hipStreamSynchronize(s->stream));
  if(n > s->occ.ownDepth.n && s->surf.lastOccDepth == s->occ.ownDepth.p && s->surf.lastOccDepth)
    s->surf.lastOccGone = true;  // the copy the last frame was tested against is about to be freed (mgs_frame_download_surface, which = 3)
  if(int rc = s->occ.ownDepth.ensure(n)) return rc;
  HIPCHK(hipMemcpy(s->occ.ownDepth.p, depthHost, n * sizeof(float), hipMemcpyHostToDevice));
  if(colorHost)
  {
    if(int rc = s->occ.ownColor.ensure(n * 4)) return rc;
    HIPCHK(hipMemcpy(s->occ.ownColor.p, colorHost, n * 4 * sizeof(float), hipMemcpyHostToDevice));
  }
  return mgs_frame_set_occluder(s, s->occ.ownDepth.p, colorHost ? s->occ.ownColor.p : nullptr, width, height);
}
int mgs_frame_upload_occluder(MgsScene s, const float* depthHost, const float* colorHost, int width, int height)
{
  return guarded("mgs_frame_upload_occluder", [&] { return mgs_frame_upload_occluder_impl(s, depthHost, colorHost, width, height); });
}

// the handle's FrameState block (allocated once; its address is baked into captured frame graphs)
int ensureFrameState(MgsScene s)
{
  if(s->fb.fstate.p)
    return MGS_OK;
  int rc = s->fb.fstate.ensure(1);
  if(rc)
    return rc;
  HIPCHK(hipMemset(s->fb.fstate.p, 0, sizeof(FrameState)));
  HIPCHK(hipDeviceSynchronize());
  s->fb.ctr.p   = &s->fb.fstate.p->ctr;
  s->fb.plans.p = &s->fb.fstate.p->plans;
  s->fb.dArgs.p = &s->fb.fstate.p->args;
  return MGS_OK;
}

// A frame's first operation on its stream: counters and plans to zero, this frame's constants behind them, in one upload
// from the handle's ring of pinned buffers (a buffer is reused four uploads later, after its copy's event).
int uploadFrameState(MgsScene s, const FrameArgs& A, hipStream_t st)
{
  int rc = ensureFrameState(s);
  if(rc)
    return rc;
  const size_t head = offsetof(FrameState, args), used = offsetof(FrameArgs, inst) + (size_t)A.f.nInstances * sizeof(InstanceConst);
  const int    k    = (int)(s->up.next++ % UploadRing::kRing);
  if(!s->up.buf[k])
  {
    if(hipHostMalloc((void**)&s->up.buf[k], head + sizeof(FrameArgs)) != hipSuccess || hipEventCreateWithFlags(&s->up.ev[k], hipEventDisableTiming) != hipSuccess)
    {
      if(s->up.buf[k]) (void)hipHostFree(s->up.buf[k]);
      s->up.buf[k] = nullptr;
      setError("frame: pinned allocation for the per-frame upload failed");
      return MGS_ERR_OOM;
    }
    std::memset(s->up.buf[k], 0, head);  // the head stays zero for good
  }
  if(s->up.busy[k])
    HIPCHK(hipEventSynchronize(s->up.ev[k]));
  std::memcpy(s->up.buf[k] + head, &A, used);
  HIPCHK(hipMemcpyAsync(s->fb.fstate.p, s->up.buf[k], head + used, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(s->up.ev[k], st));
  s->up.busy[k] = true;
  return MGS_OK;
}

static int pairSortBits(int nTiles)
{
  int bits = 1;
  while((1 << bits) < nTiles)
    ++bits;
  return ((bits + 7) / 8) * 8;
}

// The frame image, side outputs and accumulator of a frame; one made by the frame graph (mgs_render) also sizes its range table
// and names the occluder depth it is tested against, one made outside it (mgs_render_traced) has neither.  Captured frames that
// point at a buffer that moved are dropped.
int ensureFrameImage(MgsScene s, const MgsFrameParams* p, const FrameConst& F, uint32_t rangeEntries, const float* occDepth)
{
  FrameBuffers& fb = s->fb;
  int           rc = MGS_OK;
  const size_t  pixels  = (size_t)F.width * F.height;
  fb.imageRowBytes      = (size_t)F.width * targetLayout(p->target_format).pixelBytes;
  fb.imageBytes         = fb.imageRowBytes * (size_t)F.height;
  const void* before[6] = {fb.ranges.p, fb.image.p, s->surf.depth.p, s->surf.id.p, s->surf.normal.p, fb.accum.p};
  if(rangeEntries)
    if((rc = fb.ranges.ensure(rangeEntries))) return rc;
  if(fb.image.n < fb.imageBytes)
  {
    if((rc = fb.image.ensure(fb.imageBytes))) return rc;
    HIPCHK(hipMemsetAsync(fb.image.p, 0, fb.imageBytes, s->stream));
  }
  if(F.surfaceOutputs)
  {
    if((rc = s->surf.depth.ensure(pixels))) return rc;
    if((rc = s->surf.id.ensure(pixels))) return rc;
    if((rc = s->surf.normal.ensure(pixels))) return rc;
  }
  if(F.temporalSampling)
    if((rc = fb.accum.ensure(pixels))) return rc;
  s->surf.have         = F.surfaceOutputs != 0;
  s->surf.lastOccDepth = occDepth;
  s->surf.lastOccGone  = false;
  const void* after[6] = {fb.ranges.p, fb.image.p, s->surf.depth.p, s->surf.id.p, s->surf.normal.p, fb.accum.p};
  if(std::memcmp(before, after, sizeof(before)) != 0 && !s->graphs.map.empty())
  {  // a buffer moved: captured frames point at the old one
    HIPCHK(hipStreamSynchronize(s->stream));
    s->graphs.drop();
  }
  return MGS_OK;
}

// ---- adaptive bin size (BinPolicy, scene_state.h) ---------------------------------------------------------------------------
// a sample taken 8 eligible frames ago is applied now
int BinPolicy::apply()
{
  if(!pending || (frames & 31u) != 24u)
    return MGS_OK;
  HIPCHK(hipEventSynchronize(ev));  // (eight frames of this context's stream ago: long done)
  const FrameStatTotals tot     = foldFrameStats(host);
  const uint64_t        scanned = tot.scanned, D = tot.listEntries;
  pending                       = false;
  if(D > 0)
  {
    lastRatio = (float)((double)scanned / ((double)D * (double)sampledRegions));
    // ... and how far a region walks in absolute terms: one stage-A round is 512 entries, and a region that saturates inside its
    // first round or two (686 entries on the benchmark scene; 1 140-2 570 on the sparse / train-sized / fog scenes) has nothing
    // to gain from a shorter list, however short the list is (a small scene's lists are a few rounds long: its ratio is high for
    // that reason alone)
    const float perRegion = (float)((double)scanned / (double)sampledRegionCount);
    // (under the finer bins a saturating region's share of its — shorter — list is about twice what it is under the coarse ones)
    fine = sampledFine ? ((lastRatio > 0.030f && perRegion > 450.0f) ? 1 : 0) : ((lastRatio > 0.025f && perRegion > 900.0f) ? 1 : 0);
  }
  return MGS_OK;
}
// every 32nd eligible frame leaves a copy of its statistics lines (4 KB) for the frame eight later
int BinPolicy::sample(const FrameConst& F, const FrameStatLine* statLines, hipStream_t st)
{
  if((frames & 31u) == 16u && !pending)
  {
    if(!host)
    {
      if(hipHostMalloc((void**)&host, kFrameStatSlots * sizeof(FrameStatLine)) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
      {
        (void)hipGetLastError();
        if(host) (void)hipHostFree(host);
        host = nullptr;
      }
    }
    if(host)
    {
      HIPCHK(hipMemcpyAsync(host, statLines, kFrameStatSlots * sizeof(FrameStatLine), hipMemcpyDeviceToHost, st));
      HIPCHK(hipEventRecord(ev, st));
      pending        = true;
      sampledFine    = (F.binShiftX == 3 && F.binShiftY == 3) ? 1 : 0;
      sampledRegions = (1 << (F.binShiftX - 1)) * (1 << F.binShiftY);
      sampledRegionCount = (uint32_t)std::max(1, ((F.tilesX + 1) / 2) * (F.stripRow1 - F.stripRow0));
    }
  }
  ++frames;
  return MGS_OK;
}

// ---- mgs_render, step by step -----------------------------------------------------------------------------------------------
// What the frame's parameters must satisfy beyond buildFrameArgs' own checks, in the order the errors win.  No side effects on
// the handle: a rejected frame leaves it as it was.
static int validateFrameParams(const MgsFrameParams* p, const FrameConst& F, const OccluderBinding& occ)
{
  auto fail = [](int code, const std::string& msg) {
    setError(msg);
    return code;
  };
  if(p->target_format < MGS_TARGET_RGBA16F || p->target_format > MGS_TARGET_RGBA8)
    return fail(MGS_ERR_INVALID_ARG, "frame: target_format must be MGS_TARGET_RGBA16F / RGBA32F / RGBA8");
  const bool gut = p->pipeline == MGS_PIPELINE_3DGUT;
  if(p->pipeline != MGS_PIPELINE_3DGS && !gut)
    return fail(MGS_ERR_INVALID_ARG, "frame: pipeline must be MGS_PIPELINE_3DGS or MGS_PIPELINE_3DGUT");
  // CAMERA_TYPE also selects the dist-stage cull of the 3DGS pipelines (dist.comp.slang:64-91)
  if(p->camera_model < MGS_CAMERA_PINHOLE || p->camera_model > MGS_CAMERA_FISHEYE)
    return fail(MGS_ERR_INVALID_ARG, "frame: camera_model out of range");
  if(gut)
  {
    if(p->extent_method < MGS_EXTENT_EIGEN || p->extent_method > MGS_EXTENT_CONIC)
      return fail(MGS_ERR_INVALID_ARG, "frame: extent_method out of range");
    // the float knobs of the particle response and the lens: values outside these ranges make every ray NaN (negative or
    // non-finite aperture, focus distance <= 0) or reject / accept every hit differently from the reference (alphaClamp <=
    // 1/255 rejects everything in threedgrt.h.slang:181-184, which the per-record cutoff of the packed compositor would not)
    if(!(p->alpha_clamp > 1.0f / 255.0f && p->alpha_clamp <= 1.0f) || !(p->kernel_min_response >= 0.0f && p->kernel_min_response < 1.0f))
      return fail(MGS_ERR_INVALID_ARG, "frame: alpha_clamp must be in (1/255, 1] and kernel_min_response in [0, 1)");
    if(p->dof_mode != MGS_DOF_DISABLED && (!(p->aperture >= 0.0f) || !std::isfinite(p->aperture) || !(p->focus_dist > 0.0f) || !std::isfinite(p->focus_dist)))
      return fail(MGS_ERR_INVALID_ARG, "frame: depth of field needs a finite aperture >= 0 and a finite focus_dist > 0");
    if(p->kernel_degree != 8 && (p->kernel_degree < 0 || p->kernel_degree > 5))
      return fail(MGS_ERR_INVALID_ARG, "frame: kernel_degree must be one of 0, 1, 2, 3, 4, 5, 8 (shaderio.h:112-119)");
    if(p->normal_method != MGS_NORMAL_MAX_DENSITY_PLANE && p->normal_method != MGS_NORMAL_ISO_SURFACE)
      return fail(MGS_ERR_INVALID_ARG, "frame: normal_method must be MGS_NORMAL_MAX_DENSITY_PLANE or MGS_NORMAL_ISO_SURFACE (shaderio.h:126-128)");
  }
  else if(p->dof_mode != MGS_DOF_DISABLED)
    return fail(MGS_ERR_UNSUPPORTED, "frame: depth of field is a feature of the 3DGUT pipeline (per-pixel rays); the 3DGS pipeline has none");
  if(p->sort_mode != MGS_SORT_GPU_RADIX && p->sort_mode != MGS_SORT_CPU_ASYNC && p->sort_mode != MGS_SORT_STOCHASTIC)
    return fail(MGS_ERR_INVALID_ARG, "frame: sort_mode must be MGS_SORT_GPU_RADIX, MGS_SORT_CPU_ASYNC or MGS_SORT_STOCHASTIC");
  if(p->dof_mode < MGS_DOF_DISABLED || p->dof_mode > MGS_DOF_FIXED_FOCUS || p->frame_sample_id < 0)
    return fail(MGS_ERR_INVALID_ARG, "frame: dof_mode / frame_sample_id out of range");
  if(p->lighting_mode < MGS_LIGHTING_DISABLED || p->lighting_mode > MGS_LIGHTING_INDIRECT)
    return fail(MGS_ERR_INVALID_ARG, "frame: lighting_mode must be MGS_LIGHTING_DISABLED, MGS_LIGHTING_DIRECT or MGS_LIGHTING_INDIRECT");
  if(p->lighting_mode != MGS_LIGHTING_DISABLED && p->sort_mode == MGS_SORT_STOCHASTIC)
    return fail(MGS_ERR_UNSUPPORTED, "frame: lighting of MGS_SORT_STOCHASTIC frames is not supported (the reference's stochastic pipeline is not front to back: "
                                     "it yields no surface to light)");
  if(F.sensor.bound && p->lighting_mode != MGS_LIGHTING_DISABLED)
    return fail(MGS_ERR_UNSUPPORTED, "frame: a sensor model is bound (the deferred lighting pass unprojects through projInverse); unbind it with "
                                     "mgs_frame_set_sensor(handle, NULL)");
  if(occ.depth)
  {
    if(occ.w != F.width || occ.h != F.height)
      return fail(MGS_ERR_INVALID_ARG, "frame: the bound occluder images are " + std::to_string(occ.w) + "x" + std::to_string(occ.h) + ", the frame is " +
                                           std::to_string(F.width) + "x" + std::to_string(F.height) + " (mgs_frame_set_occluder)");
    if(p->sort_mode == MGS_SORT_STOCHASTIC)
      return fail(MGS_ERR_UNSUPPORTED, "frame: MGS_SORT_STOCHASTIC with an occluder bound is not supported (the reference resolves it through the depth buffer "
                                       "itself, a different mechanism); unbind it with mgs_frame_set_occluder(handle, NULL, NULL, 0, 0)");
  }
  return MGS_OK;
}

// what mgs_render has settled before it issues the frame's launches
struct FramePass
{
  MgsScene              s;
  const MgsFrameParams* p;
  const FrameArgs*      A;
  int                   fmt;   // the image's format as the kernels name it (targetLayout)
  bool                  gut, lit, cpuMode;
  bool                  hybrid;  // a frame of mgs_render_hybrid: its tail folds the frame into the running mean, behind its light pass
  Occluder              occ;
  uint32_t              nTiles;  // lists (and ranges) exist per bin
};

// the buffers this frame needs beyond the working set
static int ensureFrameBuffers(const FramePass& fp)
{
  MgsScene          s  = fp.s;
  FrameBuffers&     fb = s->fb;
  const FrameConst& F  = fp.A->f;
  int               rc = MGS_OK;
  if(fp.gut && fb.recGut.n < s->d->totalSplats)
  {  // first 3DGUT frame of this scene: its record buffer (captured frames do not reference it yet)
    if((rc = fb.recGut.ensure(s->d->totalSplats))) return rc;
  }
  if(fp.lit)
    if((rc = ensureLightTable(*s->d))) return rc;
  if(!directBinning(F) && fb.pairKey0.n < fb.pairCapacity)
  {  // first frame on the record + pair-sort path (> 256 bins, or forced): its buffers
    const uint64_t cap = fb.pairCapacity;
    if((rc = fb.pairKey0.ensure(cap))) return rc;
    if((rc = fb.pairVal0.ensure(cap))) return rc;
    if((rc = fb.pairKey1.ensure(cap))) return rc;
    if((rc = fb.chunkStart.ensure(cap / kPart + 4))) return rc;
    if((rc = fb.splatOffset.ensure(s->d->totalSplats))) return rc;
  }
  return ensureFrameImage(s, fp.p, F, std::max<uint32_t>(fp.nTiles, 256u), fp.occ.depth);
}

// what both project kernels receive; mgs_sort_keys runs the 3DGS one with full = false over the whole frame
ProjectLaunch projectLaunch(MgsScene s, const FrameArgs& A, bool full, bool gpuSort)
{
  FrameBuffers& fb = s->fb;
  ProjectLaunch L{};
  L.dArgs           = fb.dArgs.p;
  L.totalPartitions = A.f.totalPartitions;
  L.full            = full;
  L.sensor          = A.f.sensor.bound != 0;
  L.ctr             = fb.ctr.p;
  L.slotPairs       = fb.pairB.p;
  L.slotCount       = fb.slotCount.p;
  L.rec             = fb.rec.p;
  L.recGut          = fb.recGut.p;
  L.rect            = fb.rect.p;
  L.slotHist2       = fb.slotHist2.p;
  L.top16Rec        = fb.top16Rec.p;
  L.top16Count      = gpuSort ? fb.top16Count.p : nullptr;
  L.osPlan          = &fb.plans.p->os;
  L.order           = fb.prjOrder.p;
  return L;
}

// the sorted ids in idsA: the GPU key sort, or what the CPU sorter has delivered so far
static int issueSort(const FramePass& fp, hipStream_t st)
{
  MgsScene s = fp.s;
  if(!fp.cpuMode)
  {
    keySort(s, st, false, &fp.A->f);
    return MGS_OK;
  }
  if(int rc = cpuSortStep(s, fp.p, fp.p->cpu_sort_blocking != 0))
    return rc;
  if(s->cpu.haveIndices && s->cpu.indices.size() == s->d->totalSplats)
  {
    s->cpu.storageIds = s->cpu.indices;  // the sorter works in the caller's id space
    mapIdsToStorage(s, s->cpu.storageIds.data(), s->cpu.storageIds.size());
    HIPCHK(hipMemcpyAsync(s->fb.idsA.p, s->cpu.storageIds.data(), (size_t)s->d->totalSplats * 4, hipMemcpyHostToDevice, st));
  }
  else  // no result yet: the reference draws with whatever the index buffer holds; we use identity order
    launchIotaU32(st, s->fb.idsA.p, s->d->totalSplats);
  launchSetPlanN(st, &s->fb.plans.p->keys, s->fb.ctr.p, s->d->totalSplats);
  return MGS_OK;
}

// sorted ids -> per-bin lists and their ranges.  binEv is recorded between the binning and the pair sort of the record path
static int issueBinning(const FramePass& fp, hipStream_t st, hipEvent_t binEv)
{
  MgsScene          s  = fp.s;
  FrameBuffers&     fb = s->fb;
  const FrameConst& F  = fp.A->f;
  SortPlan*         planK = &fb.plans.p->keys;
  SortPlan*         planP = &fb.plans.p->pairs;
  if(directBinning(F))
  {  // coarse bins (the default): stable multi-split straight into the per-bin lists, no records, no pair sort
    DirectBinLaunch L{};
    L.idsX = L.idsY = fb.idsA.p;
    L.planKeys      = planK;
    L.rect          = fb.rect.p;
    L.sortedCode16  = fb.sortedCode16.p;
    L.maskBuf       = fb.dbinMasks.p;
    L.maxSplats     = s->d->totalSplats;
    L.binHist       = fb.partHist.p;
    L.pStride       = fb.pStride;
    L.tables        = directBinTables(planP);
    L.binList       = fb.pairVal1.p;
    L.ranges        = fb.ranges.p;
    L.ctr           = fb.ctr.p;
    L.capacity      = fb.pairCapacity;
    L.binsX         = F.binsX;
    L.binsY         = F.binsY;
    L.binCost       = fb.binCost.p;
    launchDirectBinning(st, L);
    if(binEv) HIPCHK(hipEventRecord(binEv, st));
    return MGS_OK;
  }
  BinLaunch B{};
  B.idsX = B.idsY = fb.idsA.p;
  B.planKeys      = planK;
  B.rect          = fb.rect.p;
  B.blockCount    = fb.blockCount.p;
  B.maxBlocks     = (s->d->totalSplats + kPart - 1) / kPart;
  B.ctr           = fb.ctr.p;
  B.sortedRect    = fb.sortedRect.p;
  B.splatOffset   = fb.splatOffset.p;
  B.chunkStart    = fb.chunkStart.p;
  B.pairKey       = fb.pairKey0.p;
  B.pairVal       = fb.pairVal0.p;
  B.capacity      = fb.pairCapacity;
  B.binsX         = F.binsX;
  B.gatherRects   = true;
  launchBinning(st, B);
  if(binEv) HIPCHK(hipEventRecord(binEv, st));
  SortLaunch L{};
  L.keys0 = fb.pairKey0.p;
  L.vals0 = fb.pairVal0.p;
  L.keysX = fb.pairKey1.p;
  L.valsX = fb.pairVal1.p;
  L.keysY = fb.pairKey0.p;
  L.valsY = fb.pairVal0.p;
  L.nPtr      = &fb.ctr.p->pairCount;
  L.plan      = planP;
  L.partHist  = fb.partHist.p;
  L.pStride   = fb.pStride;
  L.maxElems  = fb.pairCapacity;
  L.beginBit  = 0;
  L.endBit    = pairSortBits((int)fp.nTiles);
  if(L.endBit > kPairSortMaxBits)
  {  // (cannot happen: at most 256 x 256 bins.  A third pass would leave its totals where the compositors read binOrderValid)
    setError("frame: the pair sort's key exceeds 16 bits");
    return MGS_ERR_STATE;
  }
  const bool onePass = L.endBit <= 8;  // <= 256 bins: the digit histogram IS the range table
  L.ranges    = onePass ? fb.ranges.p : nullptr;
  launchRadixSort(st, L);
  if(!onePass)
    launchTileRanges(st, fb.pairKey1.p, fb.pairKey0.p, planP, fb.ranges.p);
  return MGS_OK;
}

// The frame's launches on the handle's stream, behind the upload of its constants (counters and sort plans arrive zeroed with
// it).  withEvents: a timed frame brackets its stages with the events of its ring slot.
static int issueFrame(const FramePass& fp, bool withEvents)
{
  MgsScene          s   = fp.s;
  FrameBuffers&     fb  = s->fb;
  const FrameConst& F   = fp.A->f;
  hipStream_t       st  = s->stream;
  hipEvent_t*       fev = s->timing.evRing[s->timing.frameIndex % FrameTiming::kRing];
  if(withEvents) HIPCHK(hipEventRecord(fev[0], st));
  if(!directBinning(F))
    launchFrameInit(st, fb.ranges.p, fp.nTiles);  // record path: tiles without entries keep an empty range
  if(withEvents) HIPCHK(hipEventRecord(fev[6], st));  // MGS_STAGE_CULL ends here; it is part of MGS_STAGE_PROJECT too
  if(fp.cpuMode)  // rejected splats must look empty to the binning stage: rect with x0 > x1
    launchFillU32(st, fb.rect.p, 1u, s->d->totalSplats);
  const ProjectLaunch P = projectLaunch(s, *fp.A, true, !fp.cpuMode);
  if(fp.gut)
    launchProjectGut(st, P);
  else
    launchProject(st, P);
  if(withEvents) HIPCHK(hipEventRecord(fev[1], st));
  if(int rc = issueSort(fp, st))
    return rc;
  if(withEvents) HIPCHK(hipEventRecord(fev[2], st));
  if(int rc = issueBinning(fp, st, withEvents ? fev[3] : nullptr))
    return rc;
  if(withEvents) HIPCHK(hipEventRecord(fev[4], st));
  CompositeLaunch C{};
  C.A          = fp.A;
  C.dArgs      = fb.dArgs.p;
  C.ranges     = fb.ranges.p;
  C.valX       = fb.pairVal1.p;
  C.valY       = fb.pairVal0.p;
  C.planPairs  = &fb.plans.p->pairs;
  C.rec        = fb.rec.p;
  C.recGut     = fb.recGut.p;
  C.image      = fb.image.p;
  C.fmt        = fp.fmt;
  C.shFormat   = s->d->shFormat;
  C.ctr        = fb.ctr.p;
  C.outDepth   = F.surfaceOutputs ? s->surf.depth.p : nullptr;
  C.outSplatId = F.surfaceOutputs ? s->surf.id.p : nullptr;
  C.outNormal  = F.surfaceOutputs ? s->surf.normal.p : nullptr;
  C.instTable  = s->d->compInst.p;
  C.binCost    = fb.binCost.p;
  C.occ        = fp.occ;
  if(fp.gut)
    launchCompositeGut(st, C);
  else
    launchComposite(st, C);
  if(fp.lit)
  {  // deferred lighting: shades the fresh sample in place, before it is folded into the running mean
    if(withEvents) HIPCHK(hipEventRecord(fev[7], st));
    LightArgs L{};
    L.image  = fb.image.p;
    L.depth  = s->surf.depth.p;
    L.id     = s->surf.id.p;
    L.normal = s->surf.normal.p;
    L.table  = s->d->lightTab.p;
    L.frame  = fb.dArgs.p;
    L.width  = F.width;
    L.row0   = F.stripRow0 * kTilePx;
    L.row1   = std::min(F.stripRow1 * kTilePx, F.height);
    launchLight(st, L, fp.fmt);
    if(withEvents) HIPCHK(hipEventRecord(fev[8], st));
  }
  if(F.temporalSampling && !fp.hybrid)
    launchPostAccumulate(st, fb.dArgs.p, fb.accum.p, fb.image.p, fp.fmt);
  if(withEvents) HIPCHK(hipEventRecord(fev[5], st));
  return MGS_OK;
}

// everything the launchers receive by value, or that selects a kernel variant or a launch argument, is part of the key
static GraphCache::Key graphKey(const FramePass& fp)
{
  const FrameConst& F = fp.A->f;
  GraphCache::Key   key;
  std::memset(&key, 0, sizeof(key));
  int32_t isoBits;
  std::memcpy(&isoBits, &F.depthIsoThreshold, 4);
  // everything the compositor receives by value (CompositeArgs) must be part of the key
  const int32_t kv[16] = {F.width, F.height, F.stripRow0, F.stripRow1, F.binShiftX, F.binShiftY, F.partitionCull, F.alphaMode,
                          F.debugFlags & (2 | 4), F.surfaceOutputs, fp.fmt, F.nInstances, F.shDegree, isoBits,
                          F.pipeline, F.stochastic | (F.dofMode << 1) | (F.temporalSampling << 2) | ((F.pipeline == 1 && F.kernelDegree != 2) ? 8 : 0) |
                              ((F.pipeline == 1 && F.normalMethod == 1) ? 16 : 0) |
                              (F.lightingMode << 5) |  // 0..2: the lighting pass is a launch of its own; what it gets by value is in this key or moves with the buffers
                              (fp.hybrid ? 128 : 0) |  // a hybrid frame's graph ends before the accumulation
                              (F.rideShift << 8) | (F.rideShapes << 16) | (F.rideSplit << 24) |  // ... and everything that selects a kernel variant or a launch argument
                              (F.sensor.bound ? (1 << 25) : 0)};  // k_project_gut<true>; the sensor's constants themselves travel with the frame's upload
  std::memcpy(key.v, kv, sizeof(kv));
  key.p[0] = fp.s->fb.image.p;
  key.p[1] = fp.s->surf.depth.p;
  key.p[2] = fp.occ.depth;  // the compositors receive the occluder's pointers by value: another binding is another graph
  key.p[3] = fp.occ.color;
  return key;
}

// The frame is 17 dependent launches (18 with temporal accumulation); on the submitting thread that is ~0.15 ms of API calls.  A frame whose
// launch sequence does not depend on host-side data (GPU sort, no per-stage events) is captured ONCE per
// (resolution, strip, mode) into a hipGraph and replayed: the kernels read everything that changes from frame to
// frame through dArgs.  MGS_GRAPH=0 forces plain launches.
static int launchFrame(const FramePass& fp, bool timed)
{
  GraphCache& graphs = fp.s->graphs;
  if(tuning().useGraph && graphs.ok && !timed && !fp.cpuMode)
  {
    const GraphCache::Key key  = graphKey(fp);
    hipGraphExec_t        exec = graphs.find(key);
    if(!exec)
      exec = graphs.capture(fp.s->stream, key, [&] { return issueFrame(fp, false); });
    if(exec)
      return graphs.replay(exec, fp.s->stream);
  }
  return issueFrame(fp, timed);
}

void recordLastFrameHead(LastFrame& last, const MgsFrameParams& p, const FrameConst& F, bool timed, bool listsPartial)
{
  last.params                 = p;
  last.params.strip_row_begin = F.stripRow0;
  last.params.strip_row_end   = F.stripRow1;
  last.have         = true;
  last.timed        = timed;
  last.wasSortOnly  = false;
  last.listsPartial = listsPartial;
}

static void recordLastFrame(const FramePass& fp, bool timed)
{
  MgsScene          s = fp.s;
  const FrameConst& F = fp.A->f;
  LastFrame&        last = s->last;
  recordLastFrameHead(last, *fp.p, F, timed, false);
  last.rideShift = F.rideShift;
  last.codeBits  = rideCodeBits(F);
  last.binsX     = F.binsX;
  last.binsY     = F.binsY;
  last.gpuSorted = !fp.cpuMode;
  last.binShift[0] = F.binShiftX;
  last.binShift[1] = F.binShiftY;
  if(timed)
  {
    s->timing.litRing[s->timing.frameIndex % FrameTiming::kRing] = fp.lit;
    ++s->timing.frameIndex;
  }
}

// tail: what mgs_render_hybrid hangs onto the frame (scene_state.h), null for mgs_render
int renderFrame(MgsScene s, const MgsFrameParams* p, MgsFrameOut* out, FrameTail* tail)
{
  if(!s || !p)
  {
    setError("mgs_render: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->d->committed)
  {
    setError("mgs_render: call mgs_scene_commit first");
    return MGS_ERR_STATE;
  }
  if(int wrc = ensureWorkingSet(s))
    return wrc;
  HIPCHK(hipSetDevice(s->device));
  const bool policyFrame = binPolicyEligible(p);
  int        rc          = policyFrame ? s->binPolicy.apply() : MGS_OK;
  if(rc != MGS_OK)
    return rc;
  FrameArgs A;
  if((rc = buildFrameArgs(s, p, A))) return rc;
  const FrameConst& F = A.f;
  if((rc = validateFrameParams(p, F, s->occ))) return rc;
  if(p->pipeline == MGS_PIPELINE_3DGS)
    if((rc = refuseBoundSensor(s, "frame", "EWA splatting has no model of distortion: MGS_PIPELINE_3DGS cannot serve it"))) return rc;
  if(tail)
  {  // the rays of the tail's kernels: what a lit frame's constants carry (the raster kernels read none of it)
    std::memcpy(A.f.cameraPos, p->camera_pos, sizeof(A.f.cameraPos));
    mat4InverseDouble(p->view, A.f.lightViewInv);
    mat4InverseDouble(p->proj, A.f.lightProjInv);
  }
  FramePass fp{};
  fp.s       = s;
  fp.p       = p;
  fp.A       = &A;
  fp.fmt     = targetLayout(p->target_format).fmt;
  fp.gut     = p->pipeline == MGS_PIPELINE_3DGUT;
  fp.lit     = p->lighting_mode != MGS_LIGHTING_DISABLED;
  fp.cpuMode = p->sort_mode == MGS_SORT_CPU_ASYNC;
  fp.hybrid  = tail != nullptr;
  fp.nTiles  = (uint32_t)(F.binsX * F.binsY);
  if(s->occ.depth)
  {
    fp.occ.depth       = s->occ.depth;
    fp.occ.color       = s->occ.color;
    fp.occ.sortedByKey = p->sort_mode == MGS_SORT_GPU_RADIX;  // the CPU sorter orders by plane distance, not by the key's depth
  }
  else if(tail && tail->occDepth)
  {  // (mgs_render_hybrid refuses a caller's binding: the two never meet)
    fp.occ.depth       = tail->occDepth;
    fp.occ.sortedByKey = p->sort_mode == MGS_SORT_GPU_RADIX;
  }
  if((rc = ensureFrameBuffers(fp))) return rc;
  const bool timed = p->collect_timings != 0;
  // this frame's constants, and its counters and plans zeroed: one 18 KB upload
  if((rc = uploadFrameState(s, A, s->stream))) return rc;
  if(tail)
    if((rc = tail->afterUpload(A))) return rc;
  if((rc = launchFrame(fp, timed))) return rc;
  if(tail)
    if((rc = tail->afterFrame(A, fp.fmt))) return rc;
  if(policyFrame && directBinning(F))
    if((rc = s->binPolicy.sample(F, frameStatLines(&s->fb.plans.p->keys), s->stream))) return rc;
  // the counters stay on the device; mgs_frame_stats fetches them when somebody asks (two API calls per frame less
  // on the submitting thread, which spends ~6 us per call)
  HIPCHK(hipGetLastError());
  recordLastFrame(fp, timed);
  if(out)
  {
    std::memset(out, 0, sizeof(*out));
    out->rgba_device = s->fb.image.p;
    out->rgba_bytes  = s->fb.imageBytes;
    if(p->collect_timings == 1)
      return mgs_frame_stats(s, out);
  }
  return MGS_OK;
}
int mgs_render(MgsScene s, const MgsFrameParams* p, MgsFrameOut* out)
{
  return guarded("mgs_render", [&] { return renderFrame(s, p, out, nullptr); });
}

int mgs_timings_query(MgsScene s, uint32_t framesBack, float* stageMs)
{
  if(!s || !stageMs)
  {
    setError("mgs_timings_query: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(framesBack >= (uint32_t)FrameTiming::kRing || framesBack >= s->timing.frameIndex)
  {
    setError("mgs_timings_query: no timed frame that far back (ring of 128)");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  hipEvent_t* fev = s->timing.evRing[(s->timing.frameIndex - 1 - framesBack) % FrameTiming::kRing];
  HIPCHK(hipEventSynchronize(fev[5]));
  std::memset(stageMs, 0, sizeof(float) * MGS_STAGE_COUNT);
  float ms = 0;
  for(int i = 0; i < 5; ++i)
  {
    HIPCHK(hipEventElapsedTime(&ms, fev[i], fev[i + 1]));
    stageMs[i] = ms;
  }
  HIPCHK(hipEventElapsedTime(&ms, fev[0], fev[5]));
  stageMs[MGS_STAGE_TOTAL] = ms;
  HIPCHK(hipEventElapsedTime(&ms, fev[0], fev[6]));
  stageMs[MGS_STAGE_CULL] = ms;
  if(s->timing.litRing[(s->timing.frameIndex - 1 - framesBack) % FrameTiming::kRing])
  {
    HIPCHK(hipEventElapsedTime(&ms, fev[7], fev[8]));
    stageMs[MGS_STAGE_LIGHT] = ms;
    stageMs[MGS_STAGE_COMPOSITE] -= ms;  // (the composite bracket ends behind the pass)
  }
  return MGS_OK;
}

int mgs_frame_stats(MgsScene s, MgsFrameOut* out)
{
  if(!s || !out)
  {
    setError("mgs_frame_stats: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have)
  {
    setError("mgs_frame_stats: no frame rendered yet");
    return MGS_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  if(!s->last.wasSortOnly)
  {
    HIPCHK(hipMemcpyAsync(s->fb.hCtr, s->fb.ctr.p, sizeof(FrameCounters), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(s->fb.hPlans, s->fb.plans.p, sizeof(FramePlans), hipMemcpyDeviceToHost, s->stream));
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  std::memset(out->stage_ms, 0, sizeof(out->stage_ms));
  out->rgba_device   = s->fb.image.p;
  out->rgba_bytes    = s->fb.imageBytes;
  // (the kernels' counts live on the statistics lines, frame_state.h; after mgs_sort_keys the plans were fetched by that call)
  const FrameStatTotals tot = foldFrameStats(frameStatLines(&s->fb.hPlans->keys));
  out->frustum_count   = tot.survivors;
  out->sorted_count    = s->fb.hCtr->sortedCount;
  out->tile_pairs      = s->fb.hCtr->pairCount;
  out->error_flags     = s->fb.hCtr->errorFlags;
  out->shaded_count    = tot.staged;
  out->scanned_entries = tot.scanned;
  out->escape_count    = tot.escapes;
  if(!s->last.wasSortOnly && s->last.rideShift == 0)
    out->escape_count = out->sorted_count;  // nothing rode through the sort: every sorted splat's rectangle was stored and gathered by id
  if(s->last.timed && !s->last.wasSortOnly)
  {
    int rc = mgs_timings_query(s, 0, out->stage_ms);
    if(rc != MGS_OK)
      return rc;
  }
  if(out->error_flags & kErrPairOverflow)
  {
    setError("frame: tile-pair capacity exceeded (raise MGS_PAIR_CAPACITY); frame is incomplete");
    return MGS_ERR_OVERFLOW;
  }
  if(out->error_flags & kErrSpinTimeout)
  {  // a look-back wait of the key sort ran into its bound (k_osort_pass.hip): the sorted order, hence the frame, is not to be trusted
    setError("frame: a look-back wait of the key sort gave up (kErrSpinTimeout); the frame is invalid");
    return MGS_ERR_DEVICE;
  }
  return MGS_OK;
}

int mgs_frame_download_surface(MgsScene s, int which, void* dst, size_t bytes)
{
  if(!s || !dst || which < 0 || which > 3)
  {
    setError("mgs_frame_download_surface: bad argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have || !s->surf.have || s->last.wasSortOnly)
  {
    setError("mgs_frame_download_surface: the last frame was not rendered with surface_outputs = 1 or lighting on");
    return MGS_ERR_STATE;
  }
  const size_t n = (size_t)s->last.params.width * (size_t)s->last.params.height;
  if(bytes < n * (which == 2 ? 16 : 4))
  {
    setError("mgs_frame_download_surface: destination too small");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  if(which == 3)
  {  // depth consolidation, on demand: frames pay nothing for it
    if(s->surf.lastOccGone)
    {
      setError("mgs_frame_download_surface: the occluder depth the last frame was rendered against has been replaced since");
      return MGS_ERR_STATE;
    }
    if(int rc = s->surf.consDepth.ensure(n))
      return rc;
    launchDepthConsolidate(s->stream, s->surf.depth.p, s->surf.lastOccDepth, s->surf.consDepth.p, (uint32_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, s->surf.consDepth.p, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return MGS_OK;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  if(which == 2)
  {
    HIPCHK(hipMemcpy(dst, s->surf.normal.p, n * 16, hipMemcpyDeviceToHost));
    return MGS_OK;
  }
  HIPCHK(hipMemcpy(dst, which == 0 ? (const void*)s->surf.depth.p : (const void*)s->surf.id.p, n * 4, hipMemcpyDeviceToHost));
  if(which == 1)
  {  // the pipeline works on storage ids: hand out the caller's
    uint32_t*             ids = static_cast<uint32_t*>(dst);
    std::vector<uint32_t> hit;
    std::vector<size_t>   where;
    for(size_t i = 0; i < n; ++i)
      if(ids[i] != 0xFFFFFFFFu)
      {
        hit.push_back(ids[i]);
        where.push_back(i);
      }
    mapIdsToCaller(s, hit.data(), hit.size());
    for(size_t i = 0; i < hit.size(); ++i)
      ids[where[i]] = hit[i];
  }
  return MGS_OK;
}

int mgs_frame_download(MgsScene s, void* dst, size_t bytes)
{
  if(!s || !dst)
  {
    setError("mgs_frame_download: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have || s->last.wasSortOnly)
  {
    setError("mgs_frame_download: no frame rendered yet");
    return MGS_ERR_STATE;
  }
  if(bytes < s->fb.imageBytes)
  {
    setError("mgs_frame_download: destination too small");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(dst, s->fb.image.p, s->fb.imageBytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}

int mgs_frame_copy_strip(MgsScene s, void* dst, size_t bytes)
{
  if(!s || !dst)
  {
    setError("mgs_frame_copy_strip: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have || s->last.wasSortOnly)
  {
    setError("mgs_frame_copy_strip: no frame rendered yet");
    return MGS_ERR_STATE;
  }
  const int    y0 = s->last.params.strip_row_begin * kTilePx;
  const int    y1 = std::min(s->last.params.strip_row_end * kTilePx, s->last.params.height);
  const size_t n  = (size_t)(y1 - y0) * s->fb.imageRowBytes;
  if(bytes < n)
  {
    setError("mgs_frame_copy_strip: destination too small");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(dst, s->fb.image.p + (size_t)y0 * s->fb.imageRowBytes, n, hipMemcpyDeviceToDevice, s->stream));
  return MGS_OK;
}

// what the two record hooks below share: the checks (`what` names the hook, `pipeline` the frame it needs), the ids in storage
// space (sid) and, where wanted, the bin rectangle of every storage id (rect)
static int projectedHookBegin(MgsScene s, const char* what, int pipeline, const uint32_t* ids, size_t count, const float* out,
                              bool wantRect, std::vector<uint32_t>& sid, std::vector<uint32_t>& rect)
{
  const std::string name(what);
  if(!s || !ids || !out)
  {
    setError((name + ": null argument").c_str());
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have || s->last.wasSortOnly || s->last.params.pipeline != pipeline)
  {
    setError((name + (pipeline == MGS_PIPELINE_3DGUT ? ": no 3DGUT frame rendered yet" : ": no 3DGS frame rendered yet")).c_str());
    return MGS_ERR_STATE;
  }
  for(size_t i = 0; i < count; ++i)
    if(ids[i] >= s->d->totalSplats)
    {
      setError((name + ": id out of range").c_str());
      return MGS_ERR_INVALID_ARG;
    }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  sid.assign(ids, ids + count);
  mapIdsToStorage(s, sid.data(), count);
  if(!wantRect)
    return MGS_OK;
  rect.resize(s->d->totalSplats);
  HIPCHK(hipMemcpy(rect.data(), s->fb.rect.p, (size_t)s->d->totalSplats * 4, hipMemcpyDeviceToHost));
  if(s->last.rideShift != 0 && s->last.gpuSorted)
  {  // the rectangles rode through the key sort as codes (kernels_common.h: rideEncode): rect[id] holds the escapes only, the
     // others are rebuilt from the code at the id's sorted position (they used to come back stale)
    FrameCounters c;
    HIPCHK(hipMemcpy(&c, s->fb.ctr.p, sizeof(c), hipMemcpyDeviceToHost));
    const uint32_t        n = std::min<uint32_t>(c.sortedCount, (uint32_t)s->d->totalSplats);
    std::vector<uint32_t> sortedIds(n);
    std::vector<uint16_t> codes(n);
    if(n)
    {
      HIPCHK(hipMemcpy(sortedIds.data(), s->fb.idsA.p, (size_t)n * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(codes.data(), s->fb.sortedCode16.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    }
    const int      bx = s->last.binsX, by = s->last.binsY, nb = bx * by;
    const uint32_t escape = (1u << s->last.codeBits) - 1u;
    const uint32_t base[4] = {0u, (uint32_t)nb, (uint32_t)(nb + (bx - 1) * by), (uint32_t)(nb + (bx - 1) * by + bx * (by - 1))};
    for(uint32_t e = 0; e < n; ++e)
    {
      const uint32_t code = codes[e];
      if(code == escape || sortedIds[e] >= rect.size())
        continue;
      const uint32_t shape = code >= base[3] ? 3u : (code >= base[2] ? 2u : (code >= base[1] ? 1u : 0u));
      const uint32_t r = code - base[shape], dx = shape & 1u, dy = shape >> 1, wS = (uint32_t)bx - dx;
      const uint32_t y0 = r / wS, x0 = r - y0 * wS;
      rect[sortedIds[e]] = x0 | (y0 << 8) | ((x0 + dx) << 16) | ((y0 + dy) << 24);
    }
  }
  return MGS_OK;
}

// test/debug hook: the projected records of the last full frame for the given global ids (caller's id space)
static int mgs_frame_download_projected_impl(MgsScene s, const uint32_t* ids, size_t count, float* out10, uint32_t* rectOut)
{
  std::vector<uint32_t> sid, rect;
  const int rc = projectedHookBegin(s, "mgs_frame_download_projected", MGS_PIPELINE_3DGS, ids, count, out10, rectOut != nullptr, sid, rect);
  if(rc != MGS_OK)
    return rc;
  std::vector<SplatRec> rec(s->d->totalSplats);
  HIPCHK(hipMemcpy(rec.data(), s->fb.rec.p, (size_t)s->d->totalSplats * sizeof(SplatRec), hipMemcpyDeviceToHost));
  for(size_t i = 0; i < count; ++i)
  {
    const SplatRec& r = rec[sid[i]];
    float*          o = out10 + 10 * i;
    // p = 2 b / |b|^2  =>  b = 2 p / |p|^2
    const double n1 = (double)r.p1x * r.p1x + (double)r.p1y * r.p1y, n2 = (double)r.p2x * r.p2x + (double)r.p2y * r.p2y;
    o[0] = r.cx;
    o[1] = r.cy;
    o[2] = (float)(2.0 * r.p1x / n1);
    o[3] = (float)(2.0 * r.p1y / n1);
    o[4] = (float)(2.0 * r.p2x / n2);
    o[5] = (float)(2.0 * r.p2y / n2);
    o[6] = r.a;
    uint16_t h[2];
    std::memcpy(h, &r.exey, 4);
    o[7] = halfToFloat(h[0]);
    o[8] = halfToFloat(h[1]);
    o[9] = 0.0f;
    if(rectOut)
      rectOut[i] = rect[sid[i]];
  }
  return MGS_OK;
}
int mgs_frame_download_projected(MgsScene s, const uint32_t* ids, size_t count, float* out10, uint32_t* rectOut)
{
  return guarded("mgs_frame_download_projected", [&] { return mgs_frame_download_projected_impl(s, ids, count, out10, rectOut); });
}

// the same for a 3DGUT frame: the GutRecs of k_project_gut.hip as they are, 24 floats in struct order
static int mgs_frame_download_projected_gut_impl(MgsScene s, const uint32_t* ids, size_t count, float* out24, uint32_t* rectOut)
{
  std::vector<uint32_t> sid, rect;
  const int rc = projectedHookBegin(s, "mgs_frame_download_projected_gut", MGS_PIPELINE_3DGUT, ids, count, out24, rectOut != nullptr, sid, rect);
  if(rc != MGS_OK)
    return rc;
  if(!s->fb.recGut.p)
  {
    setError("mgs_frame_download_projected_gut: no 3DGUT frame rendered yet");
    return MGS_ERR_STATE;
  }
  static_assert(sizeof(GutRec) == 24 * sizeof(float), "out24 is the record itself");
  std::vector<GutRec> rec(s->d->totalSplats);
  HIPCHK(hipMemcpy(rec.data(), s->fb.recGut.p, (size_t)s->d->totalSplats * sizeof(GutRec), hipMemcpyDeviceToHost));
  for(size_t i = 0; i < count; ++i)
  {
    std::memcpy(out24 + 24 * i, &rec[sid[i]], sizeof(GutRec));
    if(rectOut)
      rectOut[i] = rect[sid[i]];
  }
  return MGS_OK;
}
int mgs_frame_download_projected_gut(MgsScene s, const uint32_t* ids, size_t count, float* out24, uint32_t* rectOut)
{
  return guarded("mgs_frame_download_projected_gut", [&] { return mgs_frame_download_projected_gut_impl(s, ids, count, out24, rectOut); });
}
