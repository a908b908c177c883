// scene_state.h — what the host units of the C ABI (api_*.hip) share: the handles' state, grouped by the subsystem that owns
// it, and the few helpers more than one unit calls.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library itself is resolved with dlopen on first use (api_comm.hip)

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mgs.h"
#include "host_model.h"
#include "launchers.h"
#include "tuning.h"

using namespace mgs;

#define HIPCHK(expr)                                                                                                    \
  do                                                                                                                    \
  {                                                                                                                     \
    hipError_t e_ = (expr);                                                                                             \
    if(e_ != hipSuccess)                                                                                                \
    {                                                                                                                   \
      setError(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr);                                      \
      return MGS_ERR_DEVICE;                                                                                            \
    }                                                                                                                   \
  } while(0)

// No exception crosses the C ABI (include/mgs.h): every entry point that can allocate host memory or parse untrusted
// input runs inside this guard.
template <typename Fn>
static int guarded(const char* what, Fn&& fn) noexcept
{
  try
  {
    return fn();
  }
  catch(const std::bad_alloc&)
  {
    setError(std::string(what) + ": out of host memory");
    return MGS_ERR_OOM;
  }
  catch(const std::length_error&)
  {
    setError(std::string(what) + ": size exceeds what the host can allocate");
    return MGS_ERR_OOM;
  }
  catch(const std::exception& e)
  {
    setError(std::string(what) + ": " + e.what());
    return MGS_ERR_FORMAT;
  }
  catch(...)
  {
    setError(std::string(what) + ": unknown failure");
    return MGS_ERR_FORMAT;
  }
}

struct MgsSplatSet_t
{
  std::shared_ptr<HostSplatSet> data;
};

template <typename T>
struct DevBuf
{
  T*     p = nullptr;
  size_t n = 0;
  int    ensure(size_t count)
  {
    if(count <= n)
      return MGS_OK;
    if(p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
    if(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess)
    {
      setError("device allocation failed (" + std::to_string(count * sizeof(T)) + " bytes)");
      return MGS_ERR_OOM;
    }
    n = count;
    return MGS_OK;
  }
  void release()
  {
    if(p)
      (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  uint64_t bytes() const { return (uint64_t)n * sizeof(T); }
};

// A committed splat set on the device: the planes of PackedSplatSet (host_model.h), uploaded as they are.  Built whole or not at all
// (commitSet, api_scene.hip); `host` stays when the planes are released.
struct DeviceSet
{
  std::shared_ptr<HostSplatSet> host;
  DevBuf<float>   centers, cov6, partBox, maxScale, scales, rotations, alpha;
  DevBuf<uint8_t> rgba, sh;   // as stored: fp32 | fp16 | u8 (`sh` stays empty for a set without SH)
  DevBuf<float>   rgbaRead;   // `rgba` read back as fp32, for the formats where `rgba` itself is not that
  uint32_t count   = 0;
  int      shDegree = 0, shStride = 0, shPitch = 0;  // PackedSplatSet's
  int      shFormat = -1, rgbaFormat = -1;
  bool     built = false;
  std::vector<uint32_t> newToOld, oldToNew;  // storage order (Morton) <-> caller's order

  // [count*4] the colours as the shaders read them back
  const float* rgbaF32() const { return rgbaFormat == MGS_FORMAT_FLOAT32 ? reinterpret_cast<const float*>(rgba.p) : rgbaRead.p; }
  uint64_t bytes() const
  {
    return centers.bytes() + cov6.bytes() + partBox.bytes() + maxScale.bytes() + scales.bytes() + rotations.bytes() + alpha.bytes()
           + rgba.bytes() + sh.bytes() + rgbaRead.bytes();
  }
  void release()
  {
    centers.release(), cov6.release(), partBox.release(), maxScale.release(), scales.release(), rotations.release(), alpha.release();
    rgba.release(), sh.release(), rgbaRead.release();
    shFormat = rgbaFormat = -1;
    built = false;
  }
};
static_assert(kPackPart == kPart, "the host pack and the kernels agree on the partition size");

struct Instance
{
  int   set;  // index into sets
  float M[16];
};

// a typed window into memory somebody else owns (the members of FrameState, frame_state.h)
template <class T>
struct DevView
{
  T* p = nullptr;
};

struct MgsMesh_t
{
  std::shared_ptr<HostMesh> data;
};
// device copy of a mesh (made when its first instance is added) and the scene's mesh instances (api_mesh.hip)
struct DeviceMesh
{
  std::shared_ptr<HostMesh> host;
  DevBuf<float>             pos, nrm;
  DevBuf<uint32_t>          idx, matId;
  DevBuf<MaterialDev>       mats;
  uint64_t bytes() const { return pos.bytes() + nrm.bytes() + idx.bytes() + matId.bytes() + mats.bytes(); }
  void     release() { pos.release(), nrm.release(), idx.release(), matId.release(), mats.release(); }
};
struct MeshInstance
{
  int   mesh;  // index into SceneData::meshes
  float M[16];
  bool  visible = true;
};

// the kernels' name of a target format (device_types.h: kTargetF32 / kTargetF16 / kTargetU8, the numbering of CmpImage::fmt too; RGBA8
// is linear UNORM, rounded once at the end) and the bytes of one pixel
struct TargetLayout
{
  int    fmt;
  size_t pixelBytes;
};
inline TargetLayout targetLayout(int targetFormat)
{
  if(targetFormat == MGS_TARGET_RGBA16F)
    return {kTargetF16, 8};
  return targetFormat == MGS_TARGET_RGBA8 ? TargetLayout{kTargetU8, 4} : TargetLayout{kTargetF32, 16};
}

// bits of the bin-rectangle codes that ride through the key sort (0: nothing rides; chooseRide, api_frameargs.hip)
inline int rideCodeBits(const FrameConst& F)
{
  int codeBits = 0;
  while(F.rideShift != 0 && (1u << codeBits) - 1u < F.rideEscape)
    ++codeBits;
  return codeBits;
}

// CPU async sorter: same protocol as SplatSorterAsync (src/splat_sorter_async.h:41-48,84-128); api_sort.hip
struct CpuSorter
{
  enum State { READY, SORTING, SORTED, FAILURE, SHUTDOWN };
  std::thread             worker;
  std::mutex              mtx;
  std::condition_variable cv;
  State                   state = READY;
  bool                    started = false;
  struct Job
  {
    float dir[3], cop[3];
    bool  frontToBack;
    struct Inst
    {
      std::shared_ptr<HostSplatSet> set;
      float                         M[16];
      uint32_t                      offset, count;
    };
    std::vector<Inst> inst;
    uint32_t          total;
  } job;
  float                 lastDir[3] = {0, 0, 0}, lastCop[3] = {0, 0, 0};  // viewpoint of the last sort that was started
  bool                  haveLast   = false;
  std::vector<float>    distances;
  std::vector<uint32_t> indices;
  double                distMs = 0, sortMs = 0;

  void run();
  void innerSort();
  void ensureStarted();
  void shutdown();
};

// The hierarchy of the traced pipeline (mgs_render_traced; api_trace.hip, k_bvh.hip): all instances' particles in world space.  It
// belongs to the SCENE and is shared by its frame contexts; rebuilt lazily by the next traced frame whose inputs (`signature`: the
// commit epoch, the instances and their transforms, the proxy's parameters) differ from what it was built for.
struct TraceBvhState
{
  DevBuf<float4>         nodes;     // all levels, two float4 per node (device_types.h)
  DevBuf<uint32_t>       callerId;  // [totalSplats] storage id -> caller's id
  DevBuf<TraceInstTable> inst;
  uint32_t               levelOffset[kBvhMaxLevels] = {}, levelCount[kBvhMaxLevels] = {};
  int                    nLevels = 0;
  uint32_t               totalNodes = 0, leaves = 0, splats = 0;
  float                  sceneLo[3] = {}, sceneInvExt[3] = {};  // the Morton frame of the last build (sceneBox)
  TraceProxy             proxy{};
  std::vector<uint8_t>   signature;
  bool                   built = false;
  uint64_t bytes() const { return nodes.bytes() + callerId.bytes() + inst.bytes(); }
  void     release() { nodes.release(), callerId.release(), inst.release(); built = false; }
};

// The triangle hierarchy of the mesh ray queries (mgs_trace_mesh_rays; api_mesh_rays.hip, k_mesh_bvh.hip): every mesh instance's
// triangles in world space.  It belongs to the SCENE and is shared by its frame contexts; rebuilt lazily by the next mesh query whose
// inputs (`signature`: the mesh instances and their transforms; visibility is not part of it) differ from what it was built for.
struct MeshBvhState
{
  DevBuf<float4>       nodes;  // all levels, two float4 per node
  DevBuf<float4>       tris;   // three float4 per leaf, in leaf order (device_types.h)
  uint32_t             levelOffset[kBvhMaxLevels] = {}, levelCount[kBvhMaxLevels] = {};
  int                  nLevels = 0;
  uint32_t             totalNodes = 0, leaves = 0, triangles = 0;
  float                boxLo[3] = {}, boxInvExt[3] = {};  // the meshes' world box: the Morton frame, and the reorder keys'
  std::vector<uint8_t> signature;
  bool                 built = false;
  std::mutex           mtx;  // held by a mesh query from its signature check to its last launch (api_mesh_rays.hip)
  uint64_t bytes() const { return nodes.bytes() + tris.bytes(); }
  void     release() { nodes.release(), tris.release(); built = false; }
};

// What a commit produces: the resident splat buffers and the instance list.  ONE copy per scene, shared read-only by the scene
// handle and every frame context created from it — the reference likewise keeps one copy of the splat buffers however many
// frames are in flight, which is why processUpdateRequests waits for the device before it touches them
// (src/gaussian_splatting.cpp:1092-1111); mgs_scene_commit does the same over all contexts' streams.
struct SceneData
{
  int                    device = 0;
  std::vector<DeviceSet> sets;
  std::vector<Instance>  instances;
  bool                   committed = false;
  int                    shFormat = 0, rgbaFormat = 0;
  uint32_t               totalSplats = 0, totalParts = 0;
  std::vector<uint32_t>  instOffset;     // [instances + 1] first global id of each instance (the same in storage and caller's ids)
  DevBuf<CompositeArgs::Inst> compInst;  // SH table of all instances for the compositor (scenes with > 16 instances)
  // lights and per-instance materials of the lighting pass (mgs_scene_set_lights, mgs_instance_set_material): the host copy, and
  // the device block every context's pass reads (allocated once: its address is baked into captured frames)
  std::unique_ptr<LightTable> lightHost;
  DevBuf<LightTable>     lightTab;
  // triangle meshes of the mesh pass (mgs_mesh_instance_*): device copies, instances in creation order, and the device table every
  // handle's pass reads (allocated once, rewritten by the editing calls after they waited for the frames in flight)
  std::vector<DeviceMesh>   meshes;
  std::vector<MeshInstance> meshInstances;
  std::unique_ptr<MeshTable> meshHost;
  DevBuf<MeshTable>      meshTab;
  // bounce materials of the mesh instances (mgs_mesh_instance_set_bounce_materials): per instance the caller's array, and the device
  // copies an indirect frame reads (the flat array and each instance's slice of it), rewritten under the rule of mgs_scene_set_lights
  std::vector<std::vector<BounceMatDev>> bounceMats;
  DevBuf<BounceMatDev>   bounceMatsDev;
  DevBuf<BounceTable>    bounceTab;
  TraceBvhState          bvh;            // mgs_render_traced
  MeshBvhState           meshBvh;        // mgs_trace_mesh_rays
  uint64_t               epoch = 0;     // bumped by every commit: a context re-sizes its working set when it lags
  std::mutex             mtx;            // guards `handles`
  std::vector<MgsScene_t*> handles;      // the owning scene and its live frame contexts
  ~SceneData();
};

// ---- the groups of a handle's state, each with the entry points that own it ------------------------------------------------

// the working set of a frame (sizeWorkingSet at commit; mgs_render grows the per-resolution ones) and its pinned readback
struct FrameBuffers
{
  DevBuf<uint2>         pairA, pairB;  // ping-pong of the key sort; the project kernels leave their (key, id) pairs in B, one
                                       // slot of 2048 entries per partition
  DevBuf<uint32_t>      slotHist2, top16Rec, top16Count, osStatus;  // what the key sort needs besides (osort_launch.hip)
  DevBuf<uint32_t>      prjOrder;                    // [parts] dispatch order of the project kernels' partitions (identity until a key sort has run)
  DevBuf<uint32_t>      slotCount, chunkSum, runTab;  // pairs per slot; the tables of the sort's virtual pass 0 (k_os_prepare)
  DevBuf<uint16_t>      sortedCode16;                // the bin rectangles' codes in sorted order (they ride through the key sort)
  DevBuf<uint32_t>      binCost;                     // [256] per bin: its slowest region in the last frame -> the next frame's bin order
  DevBuf<uint32_t>      keysA, idsA;  // the sorted ids (and, for the sort-only hook, the sorted keys)
  DevBuf<uint32_t>      rect, partHist, blockCount;
  DevBuf<uint32_t>      sortedRect, splatOffset, chunkStart;
  DevBuf<uint64_t>      dbinMasks;
  DevBuf<FrameState>    fstate;      // counters + plans + this frame's constants: one block, one upload per frame (FrameState)
  DevView<FrameArgs>    dArgs;       // = &fstate->args
  DevView<FrameCounters> ctr;        // = &fstate->ctr
  DevView<FramePlans>    plans;      // = &fstate->plans
  DevBuf<float4>        accum;       // temporal accumulation (post.comp.slang): running mean of the frame samples, fp32
  DevBuf<SplatRec>      rec;
  DevBuf<GutRec>        recGut;  // 3DGUT records (96 B per splat), allocated by the first 3DGUT frame
  DevBuf<uint32_t>      pairKey0, pairVal0, pairKey1, pairVal1;
  DevBuf<uint2>         ranges;
  DevBuf<uint8_t>       image;
  uint32_t              pairCapacity = 0, pStride = 0;
  size_t                imageBytes = 0, imageRowBytes = 0;
  FrameCounters*        hCtr   = nullptr;  // pinned readback (mgs_frame_stats, mgs_sort_keys, mgs_sort_download)
  FramePlans*           hPlans = nullptr;

  template <class F>
  void eachBuffer(F&& f)  // every device buffer of the group, once: what release() frees and mgs_scene_memory_usage counts
  {
    f(pairA); f(pairB); f(prjOrder); f(slotCount); f(chunkSum); f(runTab); f(sortedCode16); f(binCost); f(slotHist2); f(top16Rec);
    f(top16Count); f(osStatus); f(keysA); f(idsA); f(rect); f(partHist); f(blockCount); f(sortedRect); f(splatOffset); f(chunkStart);
    f(dbinMasks); f(fstate); f(accum); f(rec); f(recGut); f(pairKey0); f(pairVal0); f(pairKey1); f(pairVal1); f(ranges); f(image);
  }
  void release()
  {
    eachBuffer([](auto& b) { b.release(); });
    if(hCtr) (void)hipHostFree(hCtr);
    if(hPlans) (void)hipHostFree(hPlans);
    hCtr   = nullptr;
    hPlans = nullptr;
  }
};

// The source of a frame's upload (uploadFrameState): zeros for counters and plans, then the constants.  Pinned, a ring of four
// guarded by events: the copy is asynchronous for real (nothing is staged behind the caller's back), and a buffer is rewritten
// only after the copy that read it has completed — with several frames in flight a late read would hand one frame the constants
// of another
struct UploadRing
{
  static constexpr int kRing = 4;
  uint8_t*   buf[kRing]  = {};
  hipEvent_t ev[kRing]   = {};
  bool       busy[kRing] = {};
  uint32_t   next        = 0;
  void release()
  {
    for(int k = 0; k < kRing; ++k)
      if(buf[k])
      {
        (void)hipHostFree(buf[k]);
        (void)hipEventDestroy(ev[k]);
        buf[k] = nullptr;
      }
  }
};

// Captured frames (mgs_render), one per (resolution, strip, mode): they hold buffer addresses and grid sizes, so whoever moves
// a buffer they point at, or commits, drops them
struct GraphCache
{
  struct Key
  {
    int32_t     v[16];
    const void* p[4];  // image, picked depth, occluder depth, occluder colour
    bool operator<(const Key& o) const { return std::memcmp(this, &o, sizeof(*this)) < 0; }
  };
  std::map<Key, hipGraphExec_t> map;
  bool ok = true;  // false: this runtime cannot capture the frame, stay with plain launches

  hipGraphExec_t find(const Key& key) const
  {
    const auto it = map.find(key);
    return it == map.end() ? nullptr : it->second;
  }
  // captures what issue() launches on st; null (and ok = false) when that fails
  template <class Issue>
  hipGraphExec_t capture(hipStream_t st, const Key& key, Issue&& issue)
  {
    hipGraph_t     graph = nullptr;
    hipGraphExec_t exec  = nullptr;
    bool           good  = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if(good)
    {
      const int rcI = issue();
      good          = (hipStreamEndCapture(st, &graph) == hipSuccess) && rcI == MGS_OK && graph != nullptr;
    }
    if(good)
      good = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if(graph)
      (void)hipGraphDestroy(graph);
    if(good)
      return map.emplace(key, exec).first->second;
    (void)hipGetLastError();
    ok = false;
    return nullptr;
  }
  int replay(hipGraphExec_t exec, hipStream_t st) const
  {
    HIPCHK(hipGraphLaunch(exec, st));
    return MGS_OK;
  }
  void drop()
  {
    for(auto& g : map)
      (void)hipGraphExecDestroy(g.second);
    map.clear();
  }
  void release() { drop(); }
};

// the caller's opaque geometry (mgs_frame_set_occluder): caller-owned images, or the library-owned copies
struct OccluderBinding
{
  const float*  depth = nullptr;
  const float*  color = nullptr;
  int           w = 0, h = 0;
  DevBuf<float> ownDepth, ownColor;  // mgs_frame_upload_occluder
  void release() { ownDepth.release(), ownColor.release(); }
};

// the handle's sensor model (mgs_frame_set_sensor): a copy of the caller's, validated; buildFrameArgs turns it into SensorConst
struct SensorBinding
{
  bool           bound = false;
  MgsSensorModel model{};
};

// FTB side outputs of the last frame rendered with surface_outputs (mgs_render, mgs_frame_download_surface)
struct SurfaceOutputs
{
  DevBuf<float>    depth;
  DevBuf<uint32_t> id;
  DevBuf<float4>   normal;
  DevBuf<float>    consDepth;  // consolidated depth, computed when mgs_frame_download_surface(3) asks for it
  bool             have = false;
  const float*     lastOccDepth = nullptr;  // the occluder depth the last frame was rendered against
  bool             lastOccGone  = false;    // ... was a library-owned copy that has been freed since
  template <class F>
  void eachBuffer(F&& f) { f(depth); f(id); f(normal); f(consDepth); }
  void release() { eachBuffer([](auto& b) { b.release(); }); }
};

// image comparison (mgs_compare_*): the captured image as stored, the planes of the FLIP reference passes, the sums, the split view
struct CompareState
{
  DevBuf<uint8_t>  capture;
  CmpImage         cap{};
  bool             haveCapture = false;
  DevBuf<float>    planes;
  DevBuf<uint32_t> fixed;
  DevBuf<double>   partials;
  DevBuf<float4>   out;
  int              outW = 0, outH = 0;
  hipEvent_t       ev[2] = {};
  template <class F>
  void eachBuffer(F&& f) { f(capture); f(planes); f(out); f(fixed); f(partials); }
  void releaseBuffers() { eachBuffer([](auto& b) { b.release(); }); }  // mgs_compare_release
  void release()
  {
    releaseBuffers();
    for(auto& e : ev)
      if(e) (void)hipEventDestroy(e);
  }
};

// the mesh pass (mgs_meshes_render): visibility words, set-up records, work list, counters and the primitive-id image.  The depth
// and colour images it produces are the handle's owned occluder buffers (OccluderBinding::ownDepth / ownColor)
struct MeshPassState
{
  DevBuf<unsigned long long> vis;
  DevBuf<MeshTriRec>         recs;
  DevBuf<MeshClipRec>        clips;
  DevBuf<uint2>              work;
  DevBuf<MeshCounters>       ctr;
  DevBuf<uint32_t>           prim;
  int                        w = 0, h = 0;  // size of the last pass (mgs_meshes_download)
  bool                       have = false;
  hipEvent_t                 ev[2] = {};
  template <class F>
  void eachBuffer(F&& f) { f(vis); f(recs); f(clips); f(work); f(ctr); f(prim); }
  void release()
  {
    eachBuffer([](auto& b) { b.release(); });
    for(auto& e : ev)
      if(e) (void)hipEventDestroy(e);
    ev[0] = ev[1] = nullptr;
  }
};

// the traced pipeline's per-handle state (mgs_render_traced): hit counts and counters of the last traced frame, the scratch of a
// hierarchy build this handle ran (freed when the build is done), the events around build and frame
enum TraceEvent  // TracePassState::ev: the brackets of build_ms, trace_ms, light_ms and reorder_ms; the upload of queryMatsHost
{
  kEvBuildBegin, kEvBuildEnd, kEvTraverseBegin, kEvTraverseEnd, kEvLightBegin, kEvLightEnd, kEvReorderBegin, kEvReorderEnd, kEvMatsUploaded, kEvCount
};
struct TracePassState
{
  DevBuf<uint32_t>      hitCount;
  DevBuf<TraceCounters> ctr;
  DevBuf<uint32_t>      keys, vals, leafCount;
  DevBuf<float4>        leafBox;
  // a lit frame's scratch (mgs_render_traced_lit): what k_trace leaves for the light pass, and the light pass's own outputs
  DevBuf<float>              isoDist;
  DevBuf<float4>             radiance;
  DevBuf<uint32_t>           shadowHits;
  DevBuf<TraceLightCounters> lctr;
  DevBuf<float4>             hybridNormal;  // a hybrid frame's normalised normal (mgs_render_hybrid): the raster side outputs stay as they are
  // ray queries (mgs_trace_rays, api_rays.hip): the host variant's staging of rays and results, the refused rays' counter, and a
  // reordered batch's coherence keys and ray indices (sorted in place: the indices become the permutation)
  DevBuf<float4>             rayStage, resultStage;
  DevBuf<uint32_t>           rayInvalid, rayKeys, rayIdx;
  DevBuf<MaterialDev>        queryMats;  // a light query's materials (mgs_shade_points, api_shadow_query.hip): the call's array, uploaded
  std::vector<MaterialDev>   queryMatsHost;  // ... converted: the source of that upload, rewritten only after kEvMatsUploaded
  int                   w = 0, h = 0;
  bool                  have = false, haveLit = false;
  hipEvent_t            ev[kEvCount] = {};  // indexed by TraceEvent
  template <class F>
  void eachBuffer(F&& f)
  {
    f(hitCount); f(ctr); f(keys); f(vals); f(leafCount); f(leafBox); f(isoDist); f(radiance); f(shadowHits); f(lctr); f(hybridNormal);
    f(rayStage); f(resultStage); f(rayInvalid); f(rayKeys); f(rayIdx); f(queryMats);
  }
  void release()
  {
    eachBuffer([](auto& b) { b.release(); });
    for(auto& e : ev)
    {
      if(e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// the mesh ray queries' per-handle state (mgs_trace_mesh_rays, api_mesh_rays.hip): the host variant's staging of rays and hits, the
// batch's counters, a reordered batch's coherence keys and ray indices, the scratch of a hierarchy build this handle ran (freed when
// the build is done), the events around build, reorder and traversal
struct MeshRayState
{
  DevBuf<float4>          rayStage, hitStage, leafBox;
  DevBuf<uint32_t>        keys, vals, leafCount, rayKeys, rayIdx;
  DevBuf<MeshRayCounters> ctr;
  hipEvent_t              ev[6] = {};  // build, reorder, traversal: begin and end
  template <class F>
  void eachBuffer(F&& f) { f(rayStage); f(hitStage); f(leafBox); f(keys); f(vals); f(leafCount); f(rayKeys); f(rayIdx); f(ctr); }
  void release()
  {
    eachBuffer([](auto& b) { b.release(); });
    for(auto& e : ev)
    {
      if(e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// mesh hits in the traced frames (mgs_frame_set_trace_meshes; api_trace.hip, k_trace_mesh.hip): the handle's setting, the per-pixel
// buffers of its last such frame (hit record, its t, the walk's transmittance as a float), the two counter blocks (primary mesh
// rays, mesh occlusion rays), what mgs_trace_mesh_stats reports besides them, and the events around the two new launches
enum TraceMeshEvent { kTmevPrimaryBegin, kTmevPrimaryEnd, kTmevCompositeBegin, kTmevCompositeEnd, kTmevCount };
struct TraceMeshState
{
  bool                    enabled = false;  // mgs_frame_set_trace_meshes
  float                   minT    = 0.0f;
  DevBuf<float4>          hits;
  DevBuf<float>           meshT, walkT;
  DevBuf<MeshRayCounters> ctr;
  // an indirect frame's per-pixel bounce state (mgs_render_traced_indirect, 64 B a pixel) and its counters
  DevBuf<uint32_t>        bounceLive;
  DevBuf<float>           bounceRay;   // [9][pixels]
  DevBuf<double>          bounceT;     // [3][pixels]
  DevBuf<BounceCounters>  bounceCtr;
  hipEvent_t              bounceEv[2] = {};
  bool                    have = false;       // the handle's last traced frame ran with the setting on
  bool                    composited = false, lit = false;  // ... with a visible mesh instance (the composite ran); as a lit frame
  uint32_t                rebuilt = 0;
  float                   buildMs = 0.0f;
  uint64_t                triangles = 0, leaves = 0, nodes = 0;
  hipEvent_t              ev[kTmevCount] = {};
  // meshes in the hybrid frames (mgs_frame_set_hybrid_meshes): a setting of its own, the depth plane of the mesh pre-pass (the raster
  // pass's occluder depth: never a caller's pointer), and whether the handle's last hybrid frame ran with the setting on (it then
  // left hits, ctr and the events as a lit traced frame with meshes does, though it has no primary walk)
  bool                    hybridEnabled = false;
  float                   hybridMinT    = 0.0f;
  DevBuf<float>           hybridDepth;
  bool                    hybridFrame = false;
  template <class F>
  void eachBuffer(F&& f) { f(hits); f(meshT); f(walkT); f(ctr); f(bounceLive); f(bounceRay); f(bounceT); f(bounceCtr); f(hybridDepth); }
  void release()
  {
    eachBuffer([](auto& b) { b.release(); });
    for(auto& e : ev)
    {
      if(e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    for(auto& e : bounceEv)
    {
      if(e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// scratch of the stand-alone sort (mgs_radix_sort_u32): owned by the handle (its device, its stream)
struct SortScratch
{
  DevBuf<uint32_t> keys, vals, hist, count;
  DevBuf<uint2>    pairA, pairB;
  DevBuf<uint32_t> status;
  uint32_t         statusParts = 0;  // partition bound the look-back words of the stand-alone sort are laid out for
  DevBuf<OsPlan>   osPlan;
  DevBuf<SortPlan> plan;
  template <class F>
  void eachBuffer(F&& f) { f(keys); f(vals); f(hist); f(count); f(plan); f(pairA); f(pairB); f(status); f(osPlan); }
  void release() { eachBuffer([](auto& b) { b.release(); }); }
};

// multi-GPU strips (RCCL; api_comm.hip)
struct CommState
{
  ncclComm_t           handle = nullptr;
  int                  rank = 0, world = 1;
  std::vector<int32_t> stripBounds;  // [world + 1] tile rows; empty = equal strips
};

// MGS_SORT_CPU_ASYNC: the worker and the result the handle has consumed from it (cpuSortStep)
struct CpuSortState
{
  CpuSorter             sorter;
  std::vector<float>    distances;  // distances of the consumed sort (swapped out under the sorter's lock, like the indices)
  std::vector<uint32_t> indices;    // consumed result (caller's id space)
  std::vector<uint32_t> storageIds;
  bool                  haveIndices = false;
  DevBuf<float>         distDev;
  void release()
  {
    sorter.shutdown();
    distDev.release();
  }
};

// the events of timed frames and of the sort hooks
struct FrameTiming
{
  static constexpr int kRing = 128;
  hipEvent_t ev[8] = {};              // [0..2] sort-only hook, [6..7] raw radix sort
  hipEvent_t evRing[kRing][9] = {};   // per-frame stage brackets ([6]: end of the partition cull, [7] [8]: around the lighting pass), so timed frames need no host sync
  bool       litRing[kRing] = {};     // the timed frame of that slot ran the lighting pass
  uint64_t   frameIndex = 0;          // frames rendered with collect_timings
  bool       ready = false;           // every event exists
  bool create()
  {
    ready = true;
    for(auto& e : ev)
      ready = ready && hipEventCreate(&e) == hipSuccess;
    for(auto& set : evRing)
      for(auto& e : set)
        ready = ready && hipEventCreate(&e) == hipSuccess;
    if(!ready)
      release();
    return ready;
  }
  void release()
  {
    for(auto& e : ev)
      if(e) (void)hipEventDestroy(e);
    for(auto& set : evRing)
      for(auto& e : set)
        if(e) (void)hipEventDestroy(e);
    std::memset(ev, 0, sizeof(ev));
    std::memset(evRing, 0, sizeof(evRing));
    ready = false;
  }
};

// what the last mgs_render / mgs_sort_keys / mgs_render_gathered left for the queries and downloads behind it
struct LastFrame
{
  MgsFrameParams params{};
  bool           have = false, timed = false, wasSortOnly = false;
  int            binShift[2] = {4, 3};  // the last frame's bin size (the adaptive policy may pick another one for the next frame)
  int            rideShift = 0, codeBits = 0;      // of the last frame (0: nothing rode through the key sort) ...
  int            binsX = 0, binsY = 0;             // ... its bins ...
  bool           gpuSorted = false;                // ... and whether its GPU key sort ran (mgs_frame_download_projected)
  bool           listsPartial = false;  // the last frame came from mgs_render_gathered: its bin lists cover this rank's rows only
  MgsSortOut     sort{};
};

// Adaptive bin size (round 6).  A region walks its bin's list until its pixels saturate; where regions never
// saturate (sparse or translucent scenes) every region re-scans the WHOLE list of a 256x128-px bin, and 128x128-px bins halve
// that — measured in round 5: train-sized composite 137 -> 124 us for +6 us of binning, fog -2 %, the benchmark scene +4.6 %
// (its regions stop after a few hundred entries whatever the list's length).  The signal is the fraction of the list entries
// the regions look at, scanned / (D x regions per bin): 0.008 on the benchmark scene, 0.034 fog, 0.056 sparse, 0.077 train-sized.
// Sampled every 32nd frame of a context (one 4 KB device-to-host copy of the statistics lines behind the frame), applied eight
// frames later — by frame count, not by when the copy lands, so that a sequence renders the same way every time.  Scheduling
// only: frames do not depend on the bin size (test_binning_paths_bit_identical).  MGS_BIN_ADAPT=0 turns it off; MGS_BIN_SHIFT wins.
struct BinPolicy
{
  int        fine = 0;           // 1: 128x128-px bins (where the frame allows: <= 256 bins)
  uint32_t   frames = 0;         // eligible frames rendered by this context
  bool       pending = false;    // a sample is in flight / waiting to be applied
  int        sampledFine = 0, sampledRegions = 64;
  uint32_t   sampledRegionCount = 1;  // 32x16-px regions of the sampled frame (its strip)
  hipEvent_t ev = nullptr;
  FrameStatLine* host = nullptr;  // pinned, kFrameStatSlots lines
  float      lastRatio = 0.0f;

  int  apply();                                                                     // before an eligible frame (api_frame.hip)
  int  sample(const FrameConst& F, const FrameStatLine* statLines, hipStream_t stream);  // behind an eligible frame
  void release()
  {
    if(host) (void)hipHostFree(host);
    if(ev) (void)hipEventDestroy(ev);
    host = nullptr;
    ev   = nullptr;
  }
};

struct MgsScene_t
{
  int         device = 0;
  uint32_t    osResSlots = 0;  // workgroups of a key-sort pass the device holds at once: CUs x MGS_OS_WAVES (OsLaunch::resSlots)
  hipStream_t stream = nullptr, ownStream = nullptr;

  std::shared_ptr<SceneData> d;   // shared with the frame contexts (mgs_frame_context_create)
  uint64_t    listCapacityOverride = 0;  // mgs_scene_set_list_capacity: entries of the per-bin lists (0 = 32 per splat)
  bool        isContext = false;  // a frame context: own stream, working buffers and graphs; the scene data is the parent's
  uint64_t    wsEpoch   = ~0ull;  // d->epoch the working set below was sized for

  FrameBuffers    fb;
  UploadRing      up;
  GraphCache      graphs;
  OccluderBinding occ;
  SensorBinding   sensor;
  SurfaceOutputs  surf;
  CompareState    cmp;
  MeshPassState   mesh;
  TracePassState  trace;
  MeshRayState    meshRays;
  TraceMeshState  traceMesh;
  SortScratch     rs;
  CommState       comm;
  CpuSortState    cpu;
  FrameTiming     timing;
  LastFrame       last;
  BinPolicy       binPolicy;
};

// ---- helpers more than one unit calls ---------------------------------------------------------------------------------------
int  sizeWorkingSet(MgsScene s);                                              // api_scene.hip
int  ensureLightTable(SceneData& d);                                          // api_scene.hip
int  ensureBounceTable(SceneData& d);                                         // api_mesh.hip: the bounce materials' device copies exist
MaterialDev materialToDevice(const MgsMaterial& m);                           // api_scene.hip: with needShading derived
void mapIdsToCaller(MgsScene s, uint32_t* ids, size_t n);                     // api_scene.hip: storage global id -> caller's
void mapIdsToStorage(MgsScene s, uint32_t* ids, size_t n);                    // ... and back
int  buildFrameArgs(MgsScene s, const MgsFrameParams* p, FrameArgs& A);       // api_frameargs.hip
bool directBinning(const FrameConst& F);                                      // api_frameargs.hip
bool binPolicyEligible(const MgsFrameParams* p);                              // api_frameargs.hip
int  ensureFrameState(MgsScene s);                                            // api_frame.hip
// api_frameargs.hip: MGS_ERR_UNSUPPORTED with the message every entry point without a sensor model gives while one is bound
int  refuseBoundSensor(MgsScene s, const char* what, const char* why);
// api_frame.hip: image, side outputs, accumulator; a frame of the graph also sizes its range table and names its occluder depth
int  ensureFrameImage(MgsScene s, const MgsFrameParams* p, const FrameConst& F, uint32_t rangeEntries = 0, const float* occDepth = nullptr);
void mat4InverseDouble(const float m[16], float out[16]);                     // api_frameargs.hip
void rotScaleInverse(const float M[16], float out[9]);                        // api_mesh.hip
int  uploadFrameState(MgsScene s, const FrameArgs& A, hipStream_t st);        // api_frame.hip
// What mgs_render_hybrid (api_trace.hip) hangs onto a frame of mgs_render: the frame's constants then also carry the camera position
// and the rays' inverses, temporal accumulation is left to afterFrame, and the captured graph ends at the compositor.
struct FrameTail
{
  const float* occDepth = nullptr;  // the frame's own occluder depth (a hybrid frame's mesh depth plane), without colour; set before renderFrame
  virtual int afterUpload(const FrameArgs& A) = 0;          // the constants are on the device, nothing of the frame is launched yet
  virtual int afterFrame(const FrameArgs& A, int fmt) = 0;  // behind the frame's launches on the handle's stream
  virtual ~FrameTail() = default;
};
int  renderFrame(MgsScene s, const MgsFrameParams* p, MgsFrameOut* out, FrameTail* tail);  // api_frame.hip: mgs_render's frame
// api_frame.hip: what every frame leaves in the handle's LastFrame (the caller's parameters with the strip rows it rendered); a
// raster frame adds its bins and its sort, a traced frame has none
void recordLastFrameHead(LastFrame& last, const MgsFrameParams& p, const FrameConst& F, bool timed, bool listsPartial);
// api_trace.hip, shared with the ray queries of api_rays.hip: the range checks that need no device, the frame's constants, the
// Morton frame of the hierarchy, its lazy build, the handle's events, what every traversal kernel receives and what it reports
int  failTrace(int code, const std::string& msg);
int  validateTrace(const MgsFrameParams* p, const MgsTraceParams& t, const MgsTraceLightParams* lit = nullptr, bool hybrid = false);
// the caller's optional parameter block: *p, or what the block's mgs_*_params_default fills in for NULL
template <class P>
P paramsOr(const P* p, void (*defaults)(P*))
{
  P v;
  if(p)
    v = *p;
  else
    defaults(&v);
  return v;
}
inline MgsTraceParams      traceParamsOr(const MgsTraceParams* tp) { return paramsOr(tp, mgs_trace_params_default); }
inline MgsTraceLightParams traceLightParamsOr(const MgsTraceLightParams* lp) { return paramsOr(lp, mgs_trace_light_params_default); }
inline MgsRayQueryParams   rayQueryParamsOr(const MgsRayQueryParams* qp) { return paramsOr(qp, mgs_ray_query_params_default); }
// api_rays.hip, shared with the shadow and light queries of api_shadow_query.hip: *p without the fields a query does not read, and
// the checks of a batch that need no device (`items`: what the batch holds, "rays" or "points", for the messages)
MgsFrameParams withoutCamera(const MgsFrameParams& p);
int  validateRays(const MgsFrameParams* p, const MgsTraceParams& t, const MgsRayQueryParams& q, const void* rays, const void* results,
                  uint64_t count, bool onDevice, const char* what, const char* items = "rays");
int  traceFrameArgs(MgsScene s, MgsFrameParams& q, const char* what, bool rayInverses, std::unique_ptr<FrameArgs>& A);
void sceneBox(const SceneData& d, float lo[3], float invExt[3]);
int  ensureHierarchy(MgsScene s, const FrameArgs& A, const TraceProxy& proxy, float* buildMs, uint32_t* rebuilt);
int  ensureTraceEvents(TracePassState& ts);
TraceArgs traceArgs(MgsScene s, const TraceProxy& proxy, const MgsTraceParams& t, int fmt);
// the hierarchy's proxy of a frame: every traced entry point builds it here, so that alternating between them never rebuilds
inline TraceProxy traceProxy(const MgsFrameParams& p, const MgsTraceParams& t)
{
  return TraceProxy{p.kernel_min_response, t.kernel_adaptive_clamping, p.kernel_degree, p.alpha_cull_threshold};
}
// MgsTraceOut of the walk between the traversal events: begin() enqueues the counters' copy on the handle's stream, the caller
// waits for the stream once (behind whatever else it reads back), finish() fills *out
struct TraceOutRead
{
  TraceCounters hc{};
  int begin(MgsScene s);
  int finish(MgsScene s, uint32_t rebuilt, float buildMs, MgsTraceOut* out) const;
};
// api_mesh_rays.hip: the lazy build of the triangle hierarchy on handle s, as a mesh query runs it; the caller holds
// SceneData::meshBvh.mtx from this call to its last launch that reads the hierarchy
int  ensureMeshHierarchyLocked(MgsScene s, float* buildMs, uint32_t* rebuilt);
// api_mesh_rays.hip: mgs_debug_download_hierarchy(which = 1), the triangle hierarchy's half of the hook (api_trace.hip)
int  downloadMeshHierarchy(MgsScene s, MgsHierarchyInfo* info, float* nodes8, size_t nodeCapacity, float* tris12, size_t triCapacity);
ProjectLaunch projectLaunch(MgsScene s, const FrameArgs& A, bool full, bool gpuSort);  // api_frame.hip
void keySort(MgsScene s, hipStream_t st, bool wantKeys, const FrameConst* ride = nullptr);  // api_sort.hip
int  cpuSortStep(MgsScene s, const MgsFrameParams* p, bool blocking);         // api_sort.hip

// a lit frame needs the side outputs the pass reads (needSurfaceInfo, gaussian_splatting.h:169-179)
inline bool wantsSurface(const MgsFrameParams* p) { return p->surface_outputs != 0 || p->lighting_mode != MGS_LIGHTING_DISABLED; }

// a frame context that has not seen the scene's latest commit re-sizes its working set before it renders
inline int ensureWorkingSet(MgsScene s) { return s->wsEpoch == s->d->epoch ? MGS_OK : sizeWorkingSet(s); }
