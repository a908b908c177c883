// api_mesh_rays.hip — mesh ray queries, host side: mgs_trace_mesh_rays / mgs_trace_mesh_rays_device trace the caller's rays against
// the scene's triangle meshes (closest hit or occlusion), and the lazy build of the triangle hierarchy they walk.  The hierarchy's
// structure, its count / gather / level kernels and the key sort are the splat hierarchy's (api_trace.hip, k_bvh.hip); the reorder
// is the ray queries' (api_rays.hip).  Nothing here reads the splats, the frame's constants, a bound occluder or a bound sensor.
#include <cmath>

#include "scene_state.h"

void mgs_mesh_ray_params_default(MgsMeshRayParams* p)
{
  if(p)
    std::memset(p, 0, sizeof(*p));  // MGS_MESH_RAYS_CLOSEST, the caller's order
}

static_assert(sizeof(MgsMeshHit) == 64 && sizeof(MgsRay) == 32, "a hit is four float4, a ray two");

namespace {
enum MeshRayEvent { kMevBuildBegin, kMevBuildEnd, kMevReorderBegin, kMevReorderEnd, kMevTraceBegin, kMevTraceEnd };

struct MeshRayBatch
{
  const MgsRay* rays  = nullptr;  // device
  MgsMeshHit*   hits  = nullptr;  // device
  uint64_t      count = 0;
};

// the checks that need no device, before the handle is looked at (the order of mgs_trace_rays)
int validateMeshRays(const MgsMeshRayParams& q, const void* rays, const void* hits, uint64_t count, bool onDevice, const char* what)
{
  const std::string w = std::string(what) + ": ";
  if(q.mode != MGS_MESH_RAYS_CLOSEST && q.mode != MGS_MESH_RAYS_OCCLUSION)
    return failTrace(MGS_ERR_INVALID_ARG, w + "mode must be MGS_MESH_RAYS_CLOSEST or MGS_MESH_RAYS_OCCLUSION");
  if(q.reorder != 0 && q.reorder != 1)
    return failTrace(MGS_ERR_INVALID_ARG, w + "reorder must be 0 or 1");
  if(q.reserved[0] != 0 || q.reserved[1] != 0)
    return failTrace(MGS_ERR_INVALID_ARG, w + "the reserved words of MgsMeshRayParams must be 0");
  if(count > 0 && (!rays || !hits))
    return failTrace(MGS_ERR_INVALID_ARG, w + "null rays or hits with count > 0");
  if(count > 0x7FFFFFFFull)
    return failTrace(MGS_ERR_UNSUPPORTED, w + "at most 2^31 - 1 rays per call");
  if(onDevice && (((uintptr_t)rays | (uintptr_t)hits) & 15u))
    return failTrace(MGS_ERR_INVALID_ARG, w + "rays and hits must be 16-byte aligned");
  return MGS_OK;
}

// everything the hierarchy depends on, as bytes (visibility is read at query time and is not part of it)
std::vector<uint8_t> meshBvhSignature(const SceneData& d)
{
  std::vector<uint8_t> sig;
  auto put = [&](const void* p, size_t n) { sig.insert(sig.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  for(const MeshInstance& I : d.meshInstances)
  {
    const HostMesh* m = d.meshes[I.mesh].host.get();
    put(&m, sizeof(m));
    put(I.M, sizeof(I.M));
  }
  return sig;
}

// the meshes' world box: the union of the instances' transformed local boxes (finite vertices only), in double
void meshWorldBox(const SceneData& d, float lo[3], float invExt[3])
{
  double wl[3] = {1e300, 1e300, 1e300}, wh[3] = {-1e300, -1e300, -1e300};
  for(const MeshInstance& I : d.meshInstances)
  {
    const auto& pos  = d.meshes[I.mesh].host->positions;
    float       b[6] = {3e38f, 3e38f, 3e38f, -3e38f, -3e38f, -3e38f};
    for(size_t i = 0; i + 2 < pos.size(); i += 3)
      if(std::isfinite(pos[i]) && std::isfinite(pos[i + 1]) && std::isfinite(pos[i + 2]))
        for(int a = 0; a < 3; ++a)
        {
          b[a]     = std::min(b[a], pos[i + a]);
          b[3 + a] = std::max(b[3 + a], pos[i + a]);
        }
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

int ensureMeshRayEvents(MeshRayState& ms)
{
  if(!ms.ev[0])
    for(auto& e : ms.ev)
      HIPCHK(hipEventCreate(&e));
  return MGS_OK;
}

// (re)build the scene's triangle hierarchy on handle s
int buildMeshBvh(MgsScene s, std::vector<uint8_t>&& sig, float* buildMs)
{
  SceneData&    d  = *s->d;
  MeshBvhState& B  = d.meshBvh;
  MeshRayState& ms = s->meshRays;
  hipStream_t   st = s->stream;
  {  // the queries in flight on every context read the hierarchy this call rewrites: the rule of the splat hierarchy
    std::lock_guard<std::mutex> lk(d.mtx);
    for(MgsScene_t* h : d.handles)
      if(h != s)
        HIPCHK(hipStreamSynchronize(h->stream));
  }
  B.built      = false;
  B.nLevels    = 0;
  B.totalNodes = 0;
  B.leaves     = 0;
  std::memset(B.levelOffset, 0, sizeof(B.levelOffset));
  std::memset(B.levelCount, 0, sizeof(B.levelCount));
  const uint32_t n = d.meshHost ? d.meshHost->totalTris : 0u;
  B.triangles      = n;
  meshWorldBox(d, B.boxLo, B.boxInvExt);
  if(n == 0)
  {  // no mesh instance: every ray misses, nothing is launched
    B.signature = std::move(sig);
    B.built     = true;
    return MGS_OK;
  }
  int rc;
  struct ScratchGuard  // the build's scratch goes on every way out, an error return included
  {
    MeshRayState& m;
    ~ScratchGuard() { m.keys.release(), m.vals.release(), m.leafBox.release(); }
  } scratch{ms};
  if((rc = ms.keys.ensure(n))) return rc;
  if((rc = ms.vals.ensure(n))) return rc;
  if((rc = ms.leafBox.ensure(2 * (size_t)n))) return rc;
  if((rc = ms.leafCount.ensure(1))) return rc;
  HIPCHK(hipEventRecord(ms.ev[kMevBuildBegin], st));
  MeshBvhBuildArgs L{};
  L.table = d.meshTab.p;
  std::memcpy(L.boxLo, B.boxLo, sizeof(L.boxLo));
  std::memcpy(L.boxInvExt, B.boxInvExt, sizeof(L.boxInvExt));
  L.totalTris = n;
  L.keys      = ms.keys.p;
  L.vals      = ms.vals.p;
  L.leafBox   = ms.leafBox.p;
  launchMeshBvhLeaves(st, L);
  HIPCHK(hipGetLastError());
  // the library's own (key, value) sort: LSD radix, stable, so equal Morton codes keep the order of the global primitive ids
  if((rc = mgs_radix_sort_u32(s, ms.keys.p, ms.vals.p, n, 0, 32, nullptr))) return rc;
  HIPCHK(hipMemsetAsync(ms.leafCount.p, 0, 4, st));
  launchBvhCount(st, ms.keys.p, n, ms.leafCount.p);
  uint32_t leaves = 0;
  HIPCHK(hipMemcpyAsync(&leaves, ms.leafCount.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if(leaves > n)
    return failTrace(MGS_ERR_DEVICE, "mesh hierarchy: the leaf count exceeds the triangle count");
  B.leaves = leaves;
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
  if(leaves > 0)
  {
    if((rc = B.nodes.ensure(2 * (size_t)B.totalNodes))) return rc;
    if((rc = B.tris.ensure(3 * (size_t)leaves))) return rc;
    launchBvhGather(st, ms.vals.p, ms.leafBox.p, B.nodes.p, leaves);
    MeshBvhRecordArgs R{};
    R.table      = d.meshTab.p;
    R.sortedVals = ms.vals.p;
    R.level0     = B.nodes.p;
    R.tris       = B.tris.p;
    R.leaves     = leaves;
    launchMeshBvhRecords(st, R);
    for(int l = 1; l < B.nLevels; ++l)  // one plain kernel per level
      launchBvhLevel(st, B.nodes.p + 2 * (size_t)B.levelOffset[l - 1], B.levelCount[l - 1], B.nodes.p + 2 * (size_t)B.levelOffset[l], B.levelCount[l]);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(ms.ev[kMevBuildEnd], st));
  HIPCHK(hipStreamSynchronize(st));  // other contexts may trace over it as soon as this call returns
  HIPCHK(hipEventElapsedTime(buildMs, ms.ev[kMevBuildBegin], ms.ev[kMevBuildEnd]));
  B.signature = std::move(sig);
  B.built     = true;
  return MGS_OK;
}

int ensureMeshHierarchy(MgsScene s, float* buildMs, uint32_t* rebuilt)
{
  SceneData& d = *s->d;
  *buildMs = 0.0f;
  *rebuilt = 0;
  std::vector<uint8_t> sig = meshBvhSignature(d);
  if(d.meshBvh.built && sig == d.meshBvh.signature)
    return MGS_OK;
  *rebuilt = 1;
  return buildMeshBvh(s, std::move(sig), buildMs);
}

// the batch on the device, on the handle's stream; waits only for `out` (and for a rebuild or a reorder's sort)
int meshRaysOnDevice(MgsScene s, const MeshRayBatch& b, const MgsMeshRayParams& qp, MgsMeshRayOut* out, const char* what)
{
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, std::string(what) + ": null scene");
  if(out)
    std::memset(out, 0, sizeof(*out));
  if(b.count == 0)
    return MGS_OK;
  HIPCHK(hipSetDevice(s->device));
  SceneData&    d  = *s->d;
  MeshRayState& ms = s->meshRays;
  int           rc;
  if((rc = ensureMeshRayEvents(ms))) return rc;
  if((rc = ms.ctr.ensure(1))) return rc;
  const uint32_t n = (uint32_t)b.count;
  if(qp.reorder)
  {
    if((rc = ms.rayKeys.ensure(n))) return rc;
    if((rc = ms.rayIdx.ensure(n))) return rc;
  }
  float    buildMs = 0.0f;
  uint32_t rebuilt = 0;
  MeshRayCounters c{};
  uint64_t        triangles = 0, leaves = 0, nodes = 0;
  hipStream_t     st = s->stream;
  {
  // Contexts of one scene may query from several threads: the check, a rebuild and this query's launches run under the hierarchy's
  // mutex, so a rebuild (which waits for every other handle's stream) never frees nodes a launched kernel still reads, and no query
  // reads a half-written level table.  (The build takes d.mtx inside, for the handle list: always in this order.)
  std::lock_guard<std::mutex> hierarchy(d.meshBvh.mtx);
  if((rc = ensureMeshHierarchy(s, &buildMs, &rebuilt))) return rc;
  const MeshBvhState& B = d.meshBvh;
  triangles = B.triangles, leaves = B.leaves, nodes = B.totalNodes;
  if(qp.reorder)
  {
    HIPCHK(hipEventRecord(ms.ev[kMevReorderBegin], st));
    RayKeyArgs K{};
    K.rays  = reinterpret_cast<const float4*>(b.rays);
    K.keys  = ms.rayKeys.p;
    K.idx   = ms.rayIdx.p;
    K.count = n;
    std::memcpy(K.sceneLo, B.boxLo, sizeof(K.sceneLo));
    std::memcpy(K.sceneInvExt, B.boxInvExt, sizeof(K.sceneInvExt));
    launchRaysKey(st, K);  // the ray queries' coherence key, in the meshes' world box
    HIPCHK(hipGetLastError());
    if((rc = mgs_radix_sort_u32(s, ms.rayKeys.p, ms.rayIdx.p, n, 0, 32, nullptr))) return rc;
    HIPCHK(hipEventRecord(ms.ev[kMevReorderEnd], st));
  }
  HIPCHK(hipMemsetAsync(ms.ctr.p, 0, sizeof(MeshRayCounters), st));
  HIPCHK(hipEventRecord(ms.ev[kMevTraceBegin], st));
  MeshRayArgs L{};
  L.t.nodes      = B.nodes.p;
  L.t.nLevels    = B.nLevels;
  L.t.totalNodes = B.totalNodes;
  std::memcpy(L.t.levelOffset, B.levelOffset, sizeof(L.t.levelOffset));
  std::memcpy(L.t.levelCount, B.levelCount, sizeof(L.t.levelCount));
  L.tris  = B.tris.p;
  L.table = d.meshTab.p;
  L.rays  = reinterpret_cast<const float4*>(b.rays);
  L.hits  = reinterpret_cast<float4*>(b.hits);
  L.perm  = qp.reorder ? ms.rayIdx.p : nullptr;
  L.count = n;
  L.ctr   = ms.ctr.p;
  launchMeshRays(st, L, qp.mode);
  HIPCHK(hipEventRecord(ms.ev[kMevTraceEnd], st));
  HIPCHK(hipGetLastError());
  }
  if(out)
  {
    HIPCHK(hipMemcpyAsync(&c, ms.ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out->triangles      = triangles;
    out->leaves         = leaves;
    out->nodes          = nodes;
    out->node_visits    = c.nodeVisits;
    out->triangle_tests = c.triangleTests;
    out->hits           = c.hits;
    out->invalid_rays   = c.invalidRays;
    out->bvh_rebuilt    = rebuilt;
    out->build_ms       = buildMs;
    HIPCHK(hipEventElapsedTime(&out->trace_ms, ms.ev[kMevTraceBegin], ms.ev[kMevTraceEnd]));
    if(qp.reorder)
      HIPCHK(hipEventElapsedTime(&out->reorder_ms, ms.ev[kMevReorderBegin], ms.ev[kMevReorderEnd]));
  }
  return MGS_OK;
}

int traceMeshRaysImpl(MgsScene s, const void* rays, uint64_t count, const MgsMeshRayParams* qp, void* hits, MgsMeshRayOut* out, bool host)
{
  const char*            what = host ? "mgs_trace_mesh_rays" : "mgs_trace_mesh_rays_device";
  const MgsMeshRayParams q    = paramsOr(qp, mgs_mesh_ray_params_default);
  // (before the handle is looked at; host arrays need no alignment: they are staged)
  if(int rc = validateMeshRays(q, rays, hits, count, !host, what))
    return rc;
  MeshRayBatch b;
  b.count = count;
  if(!host)
  {
    b.rays = static_cast<const MgsRay*>(rays);
    b.hits = static_cast<MgsMeshHit*>(hits);
    return meshRaysOnDevice(s, b, q, out, what);
  }
  if(!s)
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_trace_mesh_rays: null scene");
  if(count == 0)
  {
    if(out)
      std::memset(out, 0, sizeof(*out));
    return MGS_OK;
  }
  HIPCHK(hipSetDevice(s->device));
  MeshRayState& ms = s->meshRays;
  int           rc;
  if((rc = ms.rayStage.ensure(2 * (size_t)count))) return rc;
  if((rc = ms.hitStage.ensure(4 * (size_t)count))) return rc;
  HIPCHK(hipMemcpyAsync(ms.rayStage.p, rays, (size_t)count * sizeof(MgsRay), hipMemcpyHostToDevice, s->stream));
  b.rays = reinterpret_cast<const MgsRay*>(ms.rayStage.p);
  b.hits = reinterpret_cast<MgsMeshHit*>(ms.hitStage.p);
  if((rc = meshRaysOnDevice(s, b, q, out, what)))
  {
    (void)hipStreamSynchronize(s->stream);  // the upload reads the caller's array
    return rc;
  }
  HIPCHK(hipMemcpyAsync(hits, ms.hitStage.p, (size_t)count * sizeof(MgsMeshHit), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return MGS_OK;
}
}  // namespace

int ensureMeshHierarchyLocked(MgsScene s, float* buildMs, uint32_t* rebuilt)
{
  if(int rc = ensureMeshRayEvents(s->meshRays))
    return rc;
  return ensureMeshHierarchy(s, buildMs, rebuilt);
}

int downloadMeshHierarchy(MgsScene s, MgsHierarchyInfo* info, float* nodes8, size_t nodeCapacity, float* tris12, size_t triCapacity)
{
  SceneData& d = *s->d;
  std::lock_guard<std::mutex> hierarchy(d.meshBvh.mtx);  // no rebuild on another context while this reads
  const MeshBvhState& B = d.meshBvh;
  if(!B.built)
    return failTrace(MGS_ERR_STATE, "mgs_debug_download_hierarchy: no triangle hierarchy has been built yet (a mesh query or a traced frame with meshes builds it)");
  if((nodes8 && nodeCapacity < B.totalNodes) || (tris12 && triCapacity < B.leaves))
    return failTrace(MGS_ERR_INVALID_ARG, "mgs_debug_download_hierarchy: node_capacity is below total_nodes or tri_capacity below leaves");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  std::memset(info, 0, sizeof(*info));
  info->levels      = (uint32_t)B.nLevels;
  info->total_nodes = B.totalNodes;
  info->leaves      = B.leaves;
  info->primitives  = B.triangles;
  static_assert(sizeof(info->level_offset) == sizeof(B.levelOffset) && sizeof(info->level_count) == sizeof(B.levelCount), "MgsHierarchyInfo: kBvhMaxLevels levels");
  std::memcpy(info->level_offset, B.levelOffset, sizeof(info->level_offset));
  std::memcpy(info->level_count, B.levelCount, sizeof(info->level_count));
  std::memcpy(info->box_lo, B.boxLo, sizeof(info->box_lo));
  std::memcpy(info->box_inv_ext, B.boxInvExt, sizeof(info->box_inv_ext));
  if(nodes8 && B.totalNodes)
    HIPCHK(hipMemcpy(nodes8, B.nodes.p, (size_t)B.totalNodes * 32, hipMemcpyDeviceToHost));
  if(tris12 && B.leaves)
    HIPCHK(hipMemcpy(tris12, B.tris.p, (size_t)B.leaves * 48, hipMemcpyDeviceToHost));
  return MGS_OK;
}

int mgs_trace_mesh_rays(MgsScene s, const MgsRay* rays, uint64_t count, const MgsMeshRayParams* qp, MgsMeshHit* hits, MgsMeshRayOut* out)
{
  return guarded("mgs_trace_mesh_rays", [&] { return traceMeshRaysImpl(s, rays, count, qp, hits, out, true); });
}
int mgs_trace_mesh_rays_device(MgsScene s, const MgsRay* rays, uint64_t count, const MgsMeshRayParams* qp, MgsMeshHit* hits, MgsMeshRayOut* out)
{
  return guarded("mgs_trace_mesh_rays_device", [&] { return traceMeshRaysImpl(s, rays, count, qp, hits, out, false); });
}
