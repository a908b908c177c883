// launchers.h — every host-callable kernel launcher, declared once: the k_*.hip file that defines one includes this header, and
// so does every caller, so a mismatch between the two is a compile error.  The sorts' and the compare kernels' launchers are
// declared next to their argument structs in the two headers included below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "compare_types.h"
#include "device_types.h"
#include "frame_state.h"
#include "sort_plan.h"

namespace mgs {

// splats per workgroup of the project kernels, sorted splats per workgroup of the binning: k_project.hip, k_project_gut.hip and k_bin.hip
// assert that their own constants equal it
constexpr uint32_t kPart = 2048;

// the project kernels (k_project.hip, k_project_gut.hip): cull, project, hand (key, id) pairs to the key sort (slot_emit.h)
struct ProjectLaunch
{
  const FrameArgs* dArgs;            // the frame's constants on the device
  uint32_t         totalPartitions;  // the grid: FrameConst::totalPartitions
  bool             full;             // false: keys only (mgs_sort_keys); the 3DGUT kernel always runs in full
  bool             sensor;           // launchProjectGut: FrameConst::sensor is bound (k_project_gut<true>)
  FrameCounters*   ctr;
  uint2*           slotPairs;
  uint32_t*        slotCount;
  SplatRec*        rec;     // launchProject
  GutRec*          recGut;  // launchProjectGut
  uint32_t*        rect;
  uint32_t*        slotHist2;
  uint32_t*        top16Rec;
  uint32_t*        top16Count;  // null: nobody consumes the counts (CPU sort)
  OsPlan*          osPlan;
  const uint32_t*  order;
};
void launchProject(hipStream_t stream, const ProjectLaunch& L);
void launchProjectGut(hipStream_t stream, const ProjectLaunch& L);

// the record + pair-sort path's binning (k_bin.hip)
struct BinLaunch
{
  const uint32_t* idsX;  // the sorted ids: planKeys->finalSel selects X or Y; the frame's key sort always ends in one buffer,
  const uint32_t* idsY;  // so the frame passes it as both
  const SortPlan* planKeys;
  const uint32_t* rect;
  uint32_t*       blockCount;
  uint32_t        maxBlocks;
  FrameCounters*  ctr;
  uint32_t*       sortedRect;
  uint32_t*       splatOffset;
  uint32_t*       chunkStart;
  uint32_t*       pairKey;
  uint32_t*       pairVal;
  uint32_t        capacity;
  int             binsX;
  bool            gatherRects;
};
void launchBinning(hipStream_t stream, const BinLaunch& L);

// the direct binning of frames with at most 256 bins (k_dbin.hip)
struct DirectBinLaunch
{
  const uint32_t* idsX;  // as in BinLaunch
  const uint32_t* idsY;
  const SortPlan* planKeys;
  const uint32_t* rect;
  const uint16_t* sortedCode16;
  uint64_t*       maskBuf;
  uint32_t        maxSplats;
  uint32_t*       binHist;
  uint32_t        pStride;
  DirectBinTables* tables;  // of the pairs plan (frame_state.h)
  uint32_t*       binList;
  uint2*          ranges;
  FrameCounters*  ctr;
  uint32_t        capacity;
  int             binsX, binsY;
  uint32_t*       binCost;
};
bool directBinningSupported(int binsX, int binsY);
void launchDirectBinning(hipStream_t stream, const DirectBinLaunch& L);

// the compositors (k_composite.hip, k_composite_gut.hip)
struct CompositeLaunch
{
  const FrameArgs* A;      // host copy of the frame's constants: selects the kernel variant and the grid
  const FrameArgs* dArgs;  // the same on the device
  const uint2*     ranges;
  const uint32_t*  valX;  // the per-bin lists: planPairs->finalSel selects X or Y
  const uint32_t*  valY;
  const SortPlan*  planPairs;
  const SplatRec*  rec;     // launchComposite
  const GutRec*    recGut;  // launchCompositeGut
  void*            image;
  int              fmt;  // kTargetF32 / kTargetF16 / kTargetU8
  int              shFormat;
  FrameCounters*   ctr;
  float*           outDepth;  // the three side outputs: null unless the frame has surface outputs
  uint32_t*        outSplatId;
  float4*          outNormal;
  const void*      instTable;  // launchComposite: the scene's SH table of all instances
  uint32_t*        binCost;    // launchComposite
  Occluder         occ;
};
void launchComposite(hipStream_t stream, const CompositeLaunch& L);
void launchCompositeGut(hipStream_t stream, const CompositeLaunch& L);

void launchFrameInit(hipStream_t stream, uint2* ranges, uint32_t nTiles);
void launchTileRanges(hipStream_t stream, const uint32_t* keyX, const uint32_t* keyY, const SortPlan* planPairs, uint2* ranges);
void launchLight(hipStream_t stream, const LightArgs& a, int fmt);
// the mesh pass (k_mesh.hip): clear, set-up + small triangles, large triangles, resolve + shade
// (totalTris: the grid of the set-up stage; largeBlocks: the fixed grid that strides over the device-side work list)
void launchMeshPass(hipStream_t stream, const MeshPassArgs& a, uint32_t totalTris, uint32_t largeBlocks);
// the frame's small kernels (k_frame.hip): the key plan's count of a frame sorted on the CPU, fill and iota of n words,
// and the temporal accumulation of the handle's strip
void launchSetPlanN(hipStream_t stream, SortPlan* plan, FrameCounters* ctr, uint32_t n);
void launchFillU32(hipStream_t stream, uint32_t* p, uint32_t v, uint32_t n);
void launchIotaU32(hipStream_t stream, uint32_t* p, uint32_t n);
void launchPostAccumulate(hipStream_t stream, const FrameArgs* dArgs, float4* accum, void* image, int fmt);
// the hierarchy of the traced pipeline (k_bvh.hip): leaf bounds + Morton codes; the count of valid leaves behind the sort; the
// gather of the sorted leaves into level 0; one plain kernel per upper level
void launchBvhLeaves(hipStream_t stream, const BvhBuildArgs& a);
void launchBvhCount(hipStream_t stream, const uint32_t* sortedKeys, uint32_t n, uint32_t* countOut);
void launchBvhGather(hipStream_t stream, const uint32_t* sortedVals, const float4* leafBox, float4* level0, uint32_t nLeaves);
void launchBvhLevel(hipStream_t stream, const float4* below, uint32_t nBelow, float4* level, uint32_t nLevel);
// the traversal (k_trace.hip): one ray per lane, a wave64 = an 8 x 8 pixel tile
void launchTrace(hipStream_t stream, const TraceArgs& a, const FrameConst& F, int shFormat);
void launchTraceWithMeshes(hipStream_t stream, const TraceWalkMeshArgs& a, const FrameConst& F, int shFormat);  // k_trace<., ., true>
// the stochastic trace strategies (k_trace_stochastic.hip): strategy 1 = pass-stochastic, 2 = stochastic any-hit
void launchTraceStochastic(hipStream_t stream, const TraceArgs& a, const FrameConst& F, int shFormat, int strategy);
void launchTraceLight(hipStream_t stream, const TraceLightArgs& L, const FrameConst& F);  // k_trace_light.hip
void launchTraceLightWithMeshes(hipStream_t stream, const TraceLightMeshArgs& L, const FrameConst& F);  // k_trace_light<., true>
// mesh hits of a traced frame (k_trace_mesh.hip), in k_trace's tiling: every pixel's closest mesh hit in front of k_trace; the unlit
// composite or the lit mesh shading behind k_trace and the light pass
void launchTraceMeshPrimary(hipStream_t stream, const TraceMeshArgs& m, const FrameArgs* frame, const FrameConst& F);
void launchTraceMeshComposite(hipStream_t stream, const TraceLightMeshArgs& L, const FrameConst& F, bool lit);
// bounces of an indirect frame (k_trace_bounce.hip): bounce 0's mesh shading in place of the lit composite; one bounce b >= 1
void launchTraceBouncePrimary(hipStream_t stream, const TraceBounceArgs& B, const FrameConst& F);
void launchTraceBounce(hipStream_t stream, const TraceBounceArgs& B, const FrameConst& F, int shFormat);
// ray queries (k_trace_rays.hip): the frame's primary rays written out row-major; a batch's coherence keys; one ray per lane
void launchRaysGenerate(hipStream_t stream, const FrameArgs* dArgs, float4* rays, uint32_t pixels);
void launchRaysKey(hipStream_t stream, const RayKeyArgs& a);
void launchTraceRays(hipStream_t stream, const TraceRaysArgs& a, int shFormat);
void launchPointsKey(hipStream_t stream, const PointKeyArgs& a);  // a batch of surface points: the position's Morton cell
// shadow and light queries (k_shadow_query.hip): one shadow ray, or one surface point under the scene's lights, per lane
void launchShadowRays(hipStream_t stream, const ShadowQueryArgs& a);
void launchShadePoints(hipStream_t stream, const ShadowQueryArgs& a);
// mesh ray queries: the triangle hierarchy's leaves and records (k_mesh_bvh.hip; count, gather and levels are k_bvh.hip's), and the
// ray/triangle kernel (k_mesh_rays.hip; mode 0 = closest hit, 1 = occlusion)
void launchMeshBvhLeaves(hipStream_t stream, const MeshBvhBuildArgs& a);
void launchMeshBvhRecords(hipStream_t stream, const MeshBvhRecordArgs& a);
void launchMeshRays(hipStream_t stream, const MeshRayArgs& a, int mode);
// the hand-over of a hybrid frame (k_hybrid.hip): the raster surface becomes the light pass's per-pixel inputs, in k_trace's tiling
void launchHybridSurface(hipStream_t stream, const HybridSurfaceArgs& a, const FrameConst& F, int fmt);
// a hybrid frame with meshes (mgs_frame_set_hybrid_meshes): the depth plane of the mesh pre-pass from its hit records, the hand-over
// that also leaves the pixel's transmittance, and the mesh shading behind the light pass (k_trace_mesh.hip) over that hand-over
void launchHybridMeshDepth(hipStream_t stream, const FrameArgs* frame, const float4* hits, float* plane, const FrameConst& F);
void launchHybridSurfaceWithMeshes(hipStream_t stream, const HybridSurfaceMeshArgs& a, const FrameConst& F, int fmt);
void launchHybridMeshComposite(hipStream_t stream, const TraceLightMeshArgs& L, const FrameConst& F);
void launchDepthConsolidate(hipStream_t stream, const float* picked, const float* occDepth, float* out, uint32_t n);

}  // namespace mgs
