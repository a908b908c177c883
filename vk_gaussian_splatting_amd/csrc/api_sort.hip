// api_sort.hip — the frame's key sort as the host sees it, the CPU sorter, and the sort entry points (mgs_sort_*, mgs_radix_sort_*).
#include <chrono>
#include <cmath>
#include <execution>

#include "scene_state.h"

void CpuSorter::run()
{
  std::unique_lock<std::mutex> lk(mtx);
  for(;;)
  {
    cv.wait(lk, [&] { return state == SORTING || state == SHUTDOWN; });
    if(state == SHUTDOWN)
      return;
    lk.unlock();
    innerSort();
    lk.lock();
    if(state != SHUTDOWN)
      state = SORTED;
    cv.notify_all();
  }
}
// SplatSorterAsync::innerSort (src/splat_sorter_async.cpp:92-141): plane distance keys, then
// std::sort(par_unseq) of the index array with a comparator on the distances.
void CpuSorter::innerSort()
{
  const auto  t0 = std::chrono::high_resolution_clock::now();
  const float plane[4] = {job.dir[0], job.dir[1], job.dir[2],
                          -job.dir[0] * job.cop[0] - job.dir[1] * job.cop[1] - job.dir[2] * job.cop[2]};
  const float divider = 1.0f / std::sqrt(plane[0] * plane[0] + plane[1] * plane[1] + plane[2] * plane[2]);
  distances.resize(job.total);
  indices.resize(job.total);
  for(const auto& I : job.inst)
  {
    const float* pos = I.set->positions.data();
    parallelBatches(I.count, [&](size_t s) {
      const float v[4] = {pos[3 * s], pos[3 * s + 1], pos[3 * s + 2], 1.0f};
      float       p[4];
      mat4MulVec4(I.M, v, p);
      distances[I.offset + s] = std::fabs(plane[0] * p[0] + plane[1] * p[1] + plane[2] * p[2] + plane[3]) * divider;
      indices[I.offset + s]   = I.offset + (uint32_t)s;
    });
  }
  const auto   t1 = std::chrono::high_resolution_clock::now();
  const float* d  = distances.data();
  if(job.frontToBack)
    std::sort(std::execution::par_unseq, indices.begin(), indices.end(), [d](uint32_t i, uint32_t j) { return d[i] < d[j]; });
  else
    std::sort(std::execution::par_unseq, indices.begin(), indices.end(), [d](uint32_t i, uint32_t j) { return d[i] > d[j]; });
  const auto t2 = std::chrono::high_resolution_clock::now();
  distMs        = std::chrono::duration<double, std::milli>(t1 - t0).count();
  sortMs        = std::chrono::duration<double, std::milli>(t2 - t1).count();
}
void CpuSorter::ensureStarted()
{
  if(!started)
  {
    started = true;
    worker  = std::thread([this] { run(); });
  }
}
void CpuSorter::shutdown()
{
  if(!started)
    return;
  {
    std::lock_guard<std::mutex> lk(mtx);
    state = SHUTDOWN;
  }
  cv.notify_all();
  worker.join();
  started = false;
}

// what every launch of the key sort's kernels takes from the scene's device and tuning() (OsLaunch: required, no defaults)
static void setOsTuning(MgsScene s, OsLaunch& L)
{
  L.partMin      = tuning().osPartMin;
  L.resSlots     = s->osResSlots;
  L.flatLookback = tuning().osFlat;
}

// the frame's key sort (osort_launch.hip): slots of the project kernel -> sorted ids in idsA (keys in keysA when wanted).  Its pass
// elision (sort_plan.h) is on unless MGS_SORT_REMAP=0.  It leaves the project kernels' next dispatch order in prjOrder: fullest
// slot of this frame first (scheduling only).
void keySort(MgsScene s, hipStream_t st, bool wantKeys, const FrameConst* ride)
{
  OsLaunch L{};
  L.pairs0       = s->fb.pairB.p;
  L.prjParts     = s->d->totalParts;
  L.slotCount    = s->fb.slotCount.p;
  L.chunkSum     = s->fb.chunkSum.p;
  L.runTab       = s->fb.runTab.p;
  L.nOut         = &s->fb.ctr.p->sortedCount;
  L.prjOrderOut  = s->fb.prjOrder.p;
  L.slotHist     = s->fb.slotHist2.p;
  L.top16Rec     = s->fb.top16Rec.p;
  L.top16Count   = s->fb.top16Count.p;
  L.nPtr         = &s->fb.ctr.p->sortedCount;
  L.maxElems     = s->d->totalSplats;
  L.pairA        = s->fb.pairA.p;
  L.pairB        = s->fb.pairB.p;
  L.outVals      = s->fb.idsA.p;
  L.outKeys      = wantKeys ? s->fb.keysA.p : nullptr;
  L.plan         = &s->fb.plans.p->os;
  L.planOut      = &s->fb.plans.p->keys;
  L.status       = s->fb.osStatus.p;
  L.ctr          = s->fb.ctr.p;
  L.allowRemap   = tuning().sortRemap;
  setOsTuning(s, L);
  if(ride != nullptr && ride->rideShift != 0 && !wantKeys)
  {
    L.rideShift = (uint32_t)ride->rideShift;
    L.rideSplit = (uint32_t)ride->rideSplit;
    L.rideInfo  = (uint32_t)ride->rideShapes | ((uint32_t)rideCodeBits(*ride) << 8);
    L.outCode16 = s->fb.sortedCode16.p;
  }
  launchOsSort(st, L);
}

// CPU_ASYNC path: tryConsumeAndUploadCpuSortingResult (src/splat_set_manager_vk.cpp:3334-3416)
int cpuSortStep(MgsScene s, const MgsFrameParams* p, bool blocking)
{
  CpuSorter& c = s->cpu.sorter;
  c.ensureStarted();
  std::unique_lock<std::mutex> lk(c.mtx);
  auto submit = [&]() {
    // view direction = -Z axis of the camera in world space; centre of projection = camera position
    // (SplatSetManagerVk passes cameraManip's eye/centre; with matrices only, the third row of the
    //  view matrix is the same direction)
    c.job.dir[0] = -p->view[2];
    c.job.dir[1] = -p->view[6];
    c.job.dir[2] = -p->view[10];
    std::memcpy(c.job.cop, p->camera_pos, sizeof(float) * 3);
    c.job.frontToBack = false;
    c.job.inst.clear();
    uint32_t offset = 0;
    for(const auto& I : s->d->instances)
    {
      CpuSorter::Job::Inst ji;
      ji.set = s->d->sets[I.set].host;
      std::memcpy(ji.M, I.M, sizeof(ji.M));
      ji.offset = offset;
      ji.count  = s->d->sets[I.set].count;
      offset += ji.count;
      c.job.inst.push_back(ji);
    }
    c.job.total = offset;
    c.state     = CpuSorter::SORTING;
    c.cv.notify_all();
  };
  if(c.state == CpuSorter::SORTED)
  {
    s->cpu.indices.swap(c.indices);  // consume()
    s->cpu.distances.swap(c.distances);  // the worker resizes and rewrites its own copy on the next job
    s->cpu.haveIndices = true;
    c.state           = CpuSorter::READY;
  }
  // lazy (parameters.h:183, splat_sorter_async.h:81-97): a new sort starts only if the viewpoint changed since the
  // last one that was started (direction, centre of projection, order — instance transforms are not compared there either)
  const float dirNow[3] = {-p->view[2], -p->view[6], -p->view[10]};
  const bool  sameView  = c.haveLast && std::memcmp(dirNow, c.lastDir, sizeof(dirNow)) == 0
                        && std::memcmp(p->camera_pos, c.lastCop, sizeof(float) * 3) == 0;
  const bool  lazySkip  = p->cpu_lazy_sort != 0 && sameView && s->cpu.haveIndices;
  if(c.state == CpuSorter::READY && !lazySkip)
  {
    submit();
    std::memcpy(c.lastDir, dirNow, sizeof(dirNow));
    std::memcpy(c.lastCop, p->camera_pos, sizeof(float) * 3);
    c.haveLast = true;
  }
  if(blocking && c.state == CpuSorter::SORTING)
  {
    c.cv.wait(lk, [&] { return c.state == CpuSorter::SORTED; });
    s->cpu.indices.swap(c.indices);
    s->cpu.distances.swap(c.distances);
    s->cpu.haveIndices = true;
    c.state           = CpuSorter::READY;
  }
  s->last.sort.key_ms  = (float)c.distMs;
  s->last.sort.sort_ms = (float)c.sortMs;
  return MGS_OK;
}

// what mgs_sort_keys leaves for the queries behind it, whichever sorter ran
static int recordSortOnly(MgsScene s, const MgsFrameParams* p, const MgsSortOut* out)
{
  s->last.sort        = *out;
  s->last.wasSortOnly = true;
  s->last.have        = true;
  s->last.params      = *p;
  return MGS_OK;
}

int mgs_sort_keys(MgsScene s, const MgsFrameParams* p, MgsSortOut* out)
{
  if(!s || !p || !out)
  {
    setError("mgs_sort_keys: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->d->committed)
  {
    setError("mgs_sort_keys: call mgs_scene_commit first");
    return MGS_ERR_STATE;
  }
  if(int wrc = ensureWorkingSet(s))
    return wrc;
  HIPCHK(hipSetDevice(s->device));
  std::memset(out, 0, sizeof(*out));
  if(p->sort_mode == MGS_SORT_CPU_ASYNC)
  {
    int rc = cpuSortStep(s, p, true);
    if(rc != MGS_OK)
      return rc;
    out->count   = (uint32_t)s->cpu.indices.size();
    out->key_ms  = s->last.sort.key_ms;
    out->sort_ms = s->last.sort.sort_ms;
    return recordSortOnly(s, p, out);
  }
  FrameArgs A;
  int       rc = buildFrameArgs(s, p, A);
  if(rc != MGS_OK)
    return rc;
  hipStream_t st = s->stream;
  // the metric hook returns dist.comp.slang's stream for the whole frame: a strip set on the scene culls footprints, which is
  // the raster stage's business, so it does not apply here
  A.f.stripRow0 = 0;
  A.f.stripRow1 = A.f.tilesY;
  if((rc = s->fb.ranges.ensure(1))) return rc;
  if((rc = uploadFrameState(s, A, st))) return rc;
  HIPCHK(hipEventRecord(s->timing.ev[0], st));
  launchProject(st, projectLaunch(s, A, false, true));
  HIPCHK(hipEventRecord(s->timing.ev[1], st));
  if((rc = s->fb.keysA.ensure(s->d->totalSplats))) return rc;  // the hook returns the sorted keys too
  keySort(s, st, true);
  HIPCHK(hipEventRecord(s->timing.ev[2], st));
  HIPCHK(hipMemcpyAsync(s->fb.hCtr, s->fb.ctr.p, sizeof(FrameCounters), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(s->fb.hPlans, s->fb.plans.p, sizeof(FramePlans), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, s->timing.ev[0], s->timing.ev[1]));
  out->key_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, s->timing.ev[1], s->timing.ev[2]));
  out->sort_ms = ms;
  if(s->fb.hCtr->errorFlags & kErrSpinTimeout)
  {
    setError("mgs_sort_keys: a look-back wait of the key sort gave up (kErrSpinTimeout); the order is invalid");
    return MGS_ERR_DEVICE;
  }
  out->count   = s->fb.hCtr->sortedCount;
  out->passes  = s->fb.hPlans->keys.passesRun;
  out->reserved[0] = s->fb.hPlans->os.remapOn;     // pass 2 sorted on the rank of key >> 16
  out->reserved[1] = s->fb.hPlans->os.remapCount;  // occurring values of key >> 16
  return recordSortOnly(s, p, out);
}

int mgs_sort_download(MgsScene s, uint32_t* keys, uint32_t* ids, uint32_t capacity)
{
  if(!s || !ids)
  {
    setError("mgs_sort_download: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(!s->last.have)
  {
    setError("mgs_sort_download: nothing sorted yet");
    return MGS_ERR_STATE;
  }
  HIPCHK(hipSetDevice(s->device));
  if(s->last.params.sort_mode == MGS_SORT_CPU_ASYNC)
  {
    const size_t n = s->cpu.indices.size();
    if(capacity < n)
    {
      setError("mgs_sort_download: capacity too small");
      return MGS_ERR_INVALID_ARG;
    }
    std::memcpy(ids, s->cpu.indices.data(), n * 4);
    if(keys)  // the snapshot taken together with the indices (the worker may already be rewriting its own array)
      for(size_t i = 0; i < n; ++i)
      {
        const uint32_t g = s->cpu.indices[i];
        const float    d = g < s->cpu.distances.size() ? s->cpu.distances[g] : 0.0f;
        std::memcpy(&keys[i], &d, 4);
      }
    return MGS_OK;
  }
  if(!s->last.wasSortOnly)
  {  // after a full frame the counters are still on the device
    HIPCHK(hipMemcpyAsync(s->fb.hCtr, s->fb.ctr.p, sizeof(FrameCounters), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(s->fb.hPlans, s->fb.plans.p, sizeof(FramePlans), hipMemcpyDeviceToHost, s->stream));
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  const uint32_t n = s->fb.hCtr->sortedCount;
  if(capacity < n)
  {
    setError("mgs_sort_download: capacity too small");
    return MGS_ERR_INVALID_ARG;
  }
  if(n)
  {
    if(keys)
    {
      if(!s->last.wasSortOnly || s->fb.keysA.n < n)
      {
        setError("mgs_sort_download: the sorted keys exist after mgs_sort_keys only (a frame's last sort pass writes the ids alone)");
        return MGS_ERR_STATE;
      }
      HIPCHK(hipMemcpy(keys, s->fb.keysA.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(ids, s->fb.idsA.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    mapIdsToCaller(s, ids, n);  // the pipeline works on storage ids
  }
  return MGS_OK;
}

int mgs_radix_sort_u32(MgsScene s, void* keysDev, void* valsDev, uint32_t count, int beginBit, int endBit, float* ms)
{
  if(!s || !keysDev || !valsDev || beginBit < 0 || endBit > 32 || beginBit >= endBit)
  {
    setError("mgs_radix_sort_u32: bad argument");
    return MGS_ERR_INVALID_ARG;
  }
  HIPCHK(hipSetDevice(s->device));
  if(count == 0)
    return MGS_OK;
  // scratch of the stand-alone sort: owned by the scene (its device, its stream), released in mgs_scene_destroy
  DevBuf<uint32_t>&kX = s->rs.keys, &vX = s->rs.vals, &hist = s->rs.hist, &nDev = s->rs.count;
  DevBuf<SortPlan>& plan = s->rs.plan;
  int rc;
  const uint32_t parts = (count + kPart - 1) / kPart;
  if((rc = kX.ensure(count))) return rc;
  if((rc = vX.ensure(count))) return rc;
  if((rc = hist.ensure(256ull * parts))) return rc;
  if((rc = nDev.ensure(1))) return rc;
  if((rc = plan.ensure(1))) return rc;
  // a full-width sort runs on the frame key sort's kernels (osort_launch.hip: uniform input, four plain passes): the battery of
  // the stand-alone sort tests exercises exactly what the frame uses; partial bit ranges take the generic sort (k_sort.hip).
  // MGS_RAW_SORT=generic forces the generic one for every range.
  // (2^30 pairs or more: the look-back words of k_os_pass hold 30-bit prefixes — the generic sort has no such limit)
  const bool os = !tuning().rawSortGeneric && beginBit == 0 && endBit == 32 && (uint64_t)count < kOsMaxPairs;
  if(os)
  {
    if((rc = s->rs.pairA.ensure(count))) return rc;
    if((rc = s->rs.pairB.ensure(count))) return rc;
    if((rc = s->rs.osPlan.ensure(1))) return rc;
    // the passes keep the three sets of look-back words zeroed for each other (osort_launch.hip); the sets' offsets depend on
    // the count, so a sort of another size starts from freshly zeroed words
    const uint32_t maxParts = osSortMaxParts(count, tuning().osPartMin);
    const size_t   words    = 3u * osSortStatusWords(maxParts);
    if(s->rs.status.n < words || s->rs.statusParts != maxParts)
    {
      if((rc = s->rs.status.ensure(words))) return rc;
      HIPCHK(hipMemset(s->rs.status.p, 0, s->rs.status.n * 4u));
      HIPCHK(hipDeviceSynchronize());
      s->rs.statusParts = maxParts;
    }
  }
  hipStream_t st = s->stream;
  HIPCHK(hipMemcpyAsync(nDev.p, &count, 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventRecord(s->timing.ev[6], st));
  launchSortClearPlan(st, plan.p);
  if(os)
  {
    launchOsSortClearPlan(st, s->rs.osPlan.p);
    OsLaunch O{};
    O.keys0    = (const uint32_t*)keysDev;
    O.vals0    = (const uint32_t*)valsDev;
    O.nPtr     = nDev.p;
    O.maxElems = count;
    O.pairA    = s->rs.pairA.p;
    O.pairB    = s->rs.pairB.p;
    O.outKeys  = kX.p;
    O.outVals  = vX.p;
    O.plan     = s->rs.osPlan.p;
    O.planOut  = plan.p;  // finalSel = 0: the result is in X
    if((rc = ensureFrameState(s))) return rc;
    O.ctr      = s->fb.ctr.p;
    O.status   = s->rs.status.p;
    O.allowRemap = false;
    setOsTuning(s, O);
    HIPCHK(hipMemsetAsync(&s->fb.ctr.p->errorFlags, 0, sizeof(uint32_t), st));  // whatever an earlier frame left there is not this sort's
    launchOsSort(st, O);
  }
  else
  {
    SortLaunch L{};
    L.keys0 = (uint32_t*)keysDev;
    L.vals0 = (uint32_t*)valsDev;
    L.keysX = kX.p;
    L.valsX = vX.p;
    L.keysY = (uint32_t*)keysDev;
    L.valsY = (uint32_t*)valsDev;
    L.nPtr     = nDev.p;
    L.plan     = plan.p;
    L.partHist = hist.p;
    L.pStride  = parts;
    L.maxElems = count;
    L.beginBit = beginBit;
    L.endBit   = endBit;
    launchRadixSort(st, L);
  }
  HIPCHK(hipEventRecord(s->timing.ev[7], st));
  SortPlan hp;
  uint32_t sortFlags = 0;
  HIPCHK(hipMemcpyAsync(&hp, plan.p, sizeof(SortPlan), hipMemcpyDeviceToHost, st));
  if(os)
    HIPCHK(hipMemcpyAsync(&sortFlags, &s->fb.ctr.p->errorFlags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if(sortFlags & kErrSpinTimeout)
  {
    setError("mgs_radix_sort_u32: a look-back wait gave up (kErrSpinTimeout); the caller's arrays are untouched");
    return MGS_ERR_DEVICE;
  }
  if(ms)
    HIPCHK(hipEventElapsedTime(ms, s->timing.ev[6], s->timing.ev[7]));
  if(hp.finalSel == 0)
  {  // result is in X: bring it home (outside the timed region)
    HIPCHK(hipMemcpyAsync(keysDev, kX.p, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(valsDev, vX.p, (size_t)count * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  HIPCHK(hipGetLastError());
  return MGS_OK;
}

int mgs_radix_sort_host(MgsScene s, uint32_t* keys, uint32_t* vals, uint32_t count, int beginBit, int endBit, float* ms)
{
  if(!s || !keys || !vals)
  {
    setError("mgs_radix_sort_host: null argument");
    return MGS_ERR_INVALID_ARG;
  }
  if(count == 0)
    return MGS_OK;
  HIPCHK(hipSetDevice(s->device));
  DevBuf<uint32_t> dk, dv;  // released on every exit path
  int              rc = dk.ensure(count);
  if(rc == MGS_OK)
    rc = dv.ensure(count);
  auto copy = [&](void* dst, const void* src, hipMemcpyKind kind) {
    if(rc == MGS_OK && hipMemcpy(dst, src, (size_t)count * 4, kind) != hipSuccess)
    {
      setError("mgs_radix_sort_host: hipMemcpy failed");
      rc = MGS_ERR_DEVICE;
    }
  };
  copy(dk.p, keys, hipMemcpyHostToDevice);
  copy(dv.p, vals, hipMemcpyHostToDevice);
  if(rc == MGS_OK)
    rc = mgs_radix_sort_u32(s, dk.p, dv.p, count, beginBit, endBit, ms);
  copy(keys, dk.p, hipMemcpyDeviceToHost);
  copy(vals, dv.p, hipMemcpyDeviceToHost);
  dk.release();
  dv.release();
  return rc;
}
