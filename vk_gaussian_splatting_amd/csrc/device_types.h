// device_types.h — structs shared between the host orchestration and the gfx950 kernels.
#pragma once
#include <cstdint>

namespace mgs {

constexpr int kMaxInstances       = 256;  // instances per scene: FrameArgs lives in device memory, only the used part is uploaded
constexpr int kMaxInlineInstances = 16;   // SH-table entries the compositor carries by value; larger scenes read a device table
constexpr int kMaxLights          = 64;   // == MGS_MAX_LIGHTS: entries of the scene's light table (LightTable)
constexpr int kTilePx             = 16;  // compositing tile edge in pixels (one workgroup; 8x8 pixels per wave)

// the frame image's pixel format as the kernels and their launch structs carry it (`fmt`; scene_state.h: targetLayout() maps
// MgsFrameParams::target_format to it; CmpImage::fmt has the same numbering); target_pixel.h loads and stores a pixel in it
constexpr int kTargetF32 = 0;  // RGBA32F
constexpr int kTargetF16 = 1;  // RGBA16F
constexpr int kTargetU8  = 2;  // RGBA8 UNORM, linear

// error bits reported through MgsFrameOut.error_flags
enum : uint32_t {
  kErrPairOverflow  = 1u << 0,  // tile-pair capacity exceeded
  kErrSpinTimeout   = 1u << 1,  // a bounded look-back spin gave up (never hangs the GPU)
  kErrSortOverflow  = 1u << 2,
};

// per-instance constants (SplatSetDesc, shaders/shaderio.h:439-479, reduced to what the path reads)
struct InstanceConst
{
  const float* centers;  // [count*3]
  const float* cov6;     // planar: float4 covA[count] = (S00,S01,S02,S11) then float2 covB[count] = (S12,S22)
  const void*  rgba;     // [count*4] fp32 | fp16 | u8 as stored
  const float* rgbaF32;  // [count*4] the same, dequantised the way fetchColor does (== rgba for fp32 storage): what the
                         // compositor's shading phase reads for the records it stages
  const float* alpha;    // [count] opacity as the shaders read it back from `rgba` (dequantised), planar: all the
                         // projection needs of the colour
  const float* maxScale; // [count] max(exp(scale)) per splat, host-computed (only read by size culling)
  const float* partBox;  // per 2048-splat partition: min xyz, max xyz (model space), rmax (sqrt(8*trace(Sigma))), pad
  const void*  sh;       // [count] records of 48 elements, [coef][rgb] + padding (192 B fp32 / 96 B fp16 / 48 B uint8)
  const float* scales;    // [count*3] log-space, as stored (scalesAddress)     } read only by the integrated-normal
  const float* rotations; // [count*4] (w,x,y,z), as stored (rotationsAddress)  } side output (mesh.slang:209-235)
  float        model[16];      // M   (glm column-major)
  float        modelInv[16];   // M^-1 (3DGUT: model-space ray of a fragment, frag.slang:113-118)
  float        modelView[16];  // V*M (host-computed with the same unfused fp32 products the shader does per thread)
  float        camModel[3];    // M^-1 * cameraPosition
  float        modelAxisMax;   // max length of the model matrix columns (size culling, dist.comp.slang:110-115)
  float        modelScale;     // largest singular value of the model 3x3 (upper bound of any length stretch)
  uint32_t     count;
  uint32_t     modelIsIdentity; // M is bitwise the identity: M*p == p + 0.0f for finite p (k_project skips the product)
  uint32_t     modelIsAffine;   // M's last row is bitwise (+0, +0, +0, 1) and its entries are < 2^24 in magnitude (kernels_common.h: mulMat4ExactAffineW1)
  uint32_t     globalOffset;   // first global splat id of this instance
  uint32_t     blockBegin;     // first project-kernel partition of this instance
  int32_t      shDegree;       // of the splat set
  int32_t      shStride;       // stored elements per splat (logical 0/9/24/45 padded to a 16-byte multiple)
};

// the handle's sensor model (mgs_frame_set_sensor; CameraModelParameters, threedgut_camera_models.h.slang:25-50, global shutter) as the
// 3DGUT kernels read it: gutProjectSensor / gutSensorRay (gut_common.h).  bound == 0: none, the frame's cameraModel / fovRad hold.
struct SensorConst
{
  int32_t bound;
  int32_t model;          // MGS_SENSOR_OPENCV_PINHOLE 0 / MGS_SENSOR_OPENCV_FISHEYE 1
  float   focal[2];       // pixels, the sign convention of gutFocal
  float   principal[2];
  float   radial[6];      // pinhole: numerator k1..k3, denominator k4..k6
  float   tangential[2];
  float   thinPrism[4];
  float   fisheye[4];     // forward polynomial in theta^2
  float   maxAngle;       // fisheye; the caller's, or computeMaxAngle of the viewport, the principal point and the focal length
  float   clipRadius;     // length(resolution): the out-of-limits fallback of projectPointPinhole (:131-132)
  float   rcpFocal[2];    // 1 / focal (host double, rounded once): the inverse's normalised image point
  float   tolNorm;        // the inverse's convergence bound, kSensorTolPx pixels in normalised units: kSensorTolPx / max |focal|
  float   pad[5];
};
static_assert(sizeof(SensorConst) == 128, "32 words");
constexpr int   kSensorNewtonIters = 8;      // fixed iteration count of gutSensorRay
constexpr float kSensorTolPx       = 1e-2f;  // a pixel whose inverse misses its image point by more has no ray

// frame constants (shaderio::FrameInfo, shaders/shaderio.h:238-317, reduced)
struct FrameConst
{
  float    view[16];
  float    proj[16];
  float    focal[2];      // (P00*W/2, P11*H/2), src/gaussian_splatting.cpp:1248-1250
  int32_t  width, height;
  int32_t  tilesX, tilesY;
  int32_t  binShiftX, binShiftY;  // a bin = (1<<shift) x (1<<shift) tiles; lists are built per bin
  int32_t  binsX, binsY;
  int32_t  stripRow0, stripRow1;  // tile rows rendered by this device
  float    splatScale, frustumDilation, alphaCull;
  int32_t  shDegree;
  int32_t  frontToBack;   // key sign
  int32_t  cullMode;
  int32_t  msAA;
  int32_t  alphaMode;
  int32_t  targetFormat;
  int32_t  nInstances;
  uint32_t totalSplats;
  uint32_t totalPartitions;  // project-kernel partitions
  int32_t  partitionCull;    // 1: the project kernels test their partition as a whole first (partition_cull.h)
  int32_t  debugFlags;       // MGS_DEBUG_* bits
  int32_t  sizeCulling;      // dist.comp.slang:93-134
  float    sizeCullingMinPixels;
  float    maxFocal;         // max(|focal.x|, |focal.y|)
  int32_t  surfaceOutputs;   // picked depth + splat id side outputs (frag.slang:320-349)
  float    depthIsoThreshold;
  float    thinParticleThreshold;  // shaderio.h:316: scale below which a particle axis counts as degenerate
  int32_t  quantizeNormals;        // QUANTIZE_NORMALS (parameters.h:195): octahedral 2x16-bit round trip of the splat normal
  // 3DGUT pipeline
  int32_t  pipeline;               // 0 3DGS, 1 3DGUT
  int32_t  cameraModel;            // 0 pinhole, 1 fisheye
  int32_t  extentMethod;           // 0 eigen, 1 conic
  float    fovRad;
  float    alphaClamp, kernelMinResponse;
  float    gutFocal[2];            // pinhole: == focal; fisheye: (1,-1) * viewport / fovRad (gaussian_splatting.cpp:1243)
  float    gutMaxAngle;            // computeMaxAngle (threedgut_camera_models.h.slang:87-118)
  float    viewInv[16], projInv[16];  // glm::inverse (gaussian_splatting.cpp:1166,1200)
  // stochastic splats (SORTING_STOCHASTIC_SPLAT, frag.slang:265-290) / depth of field (3DGUT, frag.slang:104-109) /
  // temporal accumulation (post.comp.slang)
  int32_t  stochastic;             // 1: binary accept/reject per fragment, the nearest accepted fragment is the pixel
  int32_t  dofMode;                // 0 DOF_DISABLED, 1 DOF_FIXED_FOCUS (shaderio.h:136-138)
  int32_t  frameSampleId;          // frameInfo.frameSampleId: seeds the per-pixel random numbers
  int32_t  temporalSampling;       // 1: the frame is folded into the running mean of the samples 0..frameSampleId
  float    focusDist, aperture;    // shaderio.h:278-279
  int32_t  kernelDegree;           // KERNEL_DEGREE (3DGUT particle response), 2 = quadratic
  int32_t  normalMethod;           // NORMAL_METHOD (shaderio.h:126-128): 0 max-density plane, 1 iso-surface (3DGUT fragment normal)
  // the bin rectangles ride through the key sort in the id word's spare bits (kernels_common.h: rideEncode)
  int32_t  rideShift;              // bits the ids need; 0 = no ride
  int32_t  rideShapes;             // how many of the shapes 1x1, 2x1, 1x2, 2x2 have codes
  uint32_t rideEscape;             // the code of every other rectangle: (1 << code bits) - 1
  int32_t  perspAffine;            // 1: view's last row is bitwise (+0,+0,+0,1), proj has the perspective zero pattern with P[14] != 0, all
                                   // entries < 2^24 in magnitude: the project kernels may take the exact shortcuts of kernels_common.h
  int32_t  rideSplit;              // 1: the id word's spare bits do not hold the whole code (> 8 M splats): its low 8 bits travel in the
                                   // key's low byte — dead weight once the slot is grouped by it (slot_emit.h) —, the rest above the id
  // deferred lighting (k_light.hip; read by no other kernel)
  int32_t  lightingMode;           // MGS_LIGHTING_*: != 0 runs the pass
  float    cameraPos[3];           // frameInfo.cameraPosition
  float    lightViewInv[16], lightProjInv[16];  // viewInverse / projInverse computed in double and rounded once (viewInv / projInv
                                                // above are the fp32 closed form the 3DGUT rays are pinned to)
  // the handle's sensor model (read by k_project_gut<true>, the 3DGUT compositors' prologue and k_rays_generate; last, so that a
  // frame without one uploads zeros behind everything the other kernels read)
  SensorConst sensor;
};

struct FrameArgs
{
  FrameConst    f;
  InstanceConst inst[kMaxInstances];
};

// What the compositor needs besides the lists: screen geometry, mode knobs and the SH table of the instances.  All of
// it is constant for a captured frame graph (it is part of the graph's key, or scene state that a commit
// invalidates), so it travels BY VALUE: kernel arguments are preloaded into SGPRs, while reading the same fields through
// the per-frame FrameArgs pointer cost the compositor 10 us (an extra dependent scalar load at every workgroup start).
struct CompositeArgs
{
  int32_t width, height;
  int32_t tilesX;
  int32_t binShiftX, binShiftY;
  int32_t binsX, binsY;
  int32_t stripRow0, stripRow1;
  int32_t nInstances;
  int32_t shDegree;
#ifdef MGS_CMP_TRACE
  uint64_t* trace;            // debug build only (tools/cmp_trace.py): per-workgroup time stamps and counts
#endif
  float   depthIsoThreshold;
  int32_t shOnly;             // SHOW_SH_ONLY (mesh.slang:205-207): base colour 0.5
  uint32_t* binCost;          // [256] per bin: the longest region of this frame (100 MHz ticks) -> the NEXT frame's bin order
  struct Inst
  {
    const void*   sh;
    const float4* rgba;     // colours as fetchColor returns them (dequantised fp32; the fp32 storage buffer itself when
                            // the set is stored as fp32)
    const float*  centers;
    uint32_t     globalOffset;
    int32_t      shDegree;
  } inst[kMaxInlineInstances];
  const Inst* instTable;      // all instances (device memory, rebuilt at commit); used when nInstances > kMaxInlineInstances
};

// ... and what the occluder instantiations (MODE bit 4, mgs_frame_set_occluder) receive: the same, plus the caller's images.  A type
// of its own so that the other instantiations keep their argument block — and with it their code — byte for byte.  By value like
// the rest: the pointers are part of the captured graph's key (binding other images takes another graph), the images' CONTENTS
// are read every frame.
struct CompositeArgsOcc : CompositeArgs
{
  const float*  occDepth;     // [height][width] window depth of the caller's geometry
  const float4* occColor;     // [height][width] linear RGBA of that geometry, nullptr = transparent black
  int32_t       occStop;      // 1: the lists are sorted by the depth key (GPU sort): a record behind every pixel ends the walk
};

// ---- deferred lighting (k_light.hip) ----
// One light as the pass reads it: MgsLight with what is the same for every pixel done once on the host (the normalised direction,
// the cosines of the cone angles).  64 B.
struct LightDev
{
  int32_t type, attMode;
  float   color[3], intensity;
  float   pos[3], range;
  float   dirN[3];             // normalize(direction)
  float   innerCos, outerCos;  // cos(radians(angle))
  float   radius;              // LightSource::radius (mgs_scene_set_light_radii): read by soft shadows only
};
// one instance's material (shaderio::ObjMaterial reduced) + needShading as updateMaterialNeedsShading derives it.  64 B.
struct alignas(16) MaterialDev
{
  float   ambient[3], diffuse[3], specular[3], emission[3];
  float   shininess;
  int32_t needShading;
  float   pad[2];
};
// The scene's lights and materials: ONE device block per scene, read by the lighting pass of every context through its pointer,
// so that changing a light or a material re-captures nothing.
struct LightTable
{
  int32_t     count;  // 0: the headlight
  int32_t     pad[15];
  LightDev    lights[kMaxLights];
  MaterialDev mats[kMaxInstances];
};
static_assert(sizeof(LightDev) == 64 && sizeof(MaterialDev) == 64, "16 words each");
// what the lighting pass receives by value (all of it constant for a captured frame graph: part of its key, or buffers whose
// move drops the captured frames)
struct LightArgs
{
  void*             image;    // the frame, in the target format
  const float*      depth;    // picked depth
  const uint32_t*   id;       // picked splat (storage id space: instances are concatenated in creation order as in the caller's)
  const float4*     normal;   // integrated normal
  const LightTable* table;
  const FrameArgs*  frame;    // camera, inverses, instance prefix: this frame's upload
  int32_t           width;
  int32_t           row0, row1;  // pixel rows [row0, row1) of the handle's strip
};

// ---- mesh pass (k_mesh.hip, api_mesh.hip) ----
constexpr int      kMaxMeshInstances = 256;          // build-defined cap of mesh instances per scene
constexpr uint32_t kMeshMaxPrims     = 1u << 29;     // a visibility word holds (primitive << 3 | sub-triangle) in its low half
constexpr uint32_t kMeshNone         = 0xFFFFFFFFu;  // primitive id of a pixel no mesh covers
constexpr uint32_t kMeshWorkItems    = 1u << 20;     // default capacity of the large-triangle work list (MGS_MESH_WORK_ITEMS; a lane whose
                                                     // chunks do not fit walks its triangle itself)
constexpr int      kMeshSmallBox     = 8;            // bounding boxes up to this many pixels on each side are walked by their own lane
constexpr int      kMeshChunkTiles   = 16;           // 8 x 8-pixel tiles per work item
// one mesh instance as the kernels read it (MeshDesc, shaders/shaderio.h, reduced)
struct alignas(16) MeshInstDev
{
  const float*       pos;      // [3 * vertices]
  const float*       nrm;      // [3 * vertices]
  const uint32_t*    idx;      // [3 * triangles]
  const uint32_t*    matId;    // [triangles], already clamped to the material count
  const MaterialDev* mats;
  float              M[16];     // transform
  float              rsInv[9];  // transformRotScaleInverse = inverse(mat3(transform)), glm column-major; the shader transposes it
  uint32_t           triBegin;  // first global primitive index of this instance
  uint32_t           triCount;
  uint32_t           visible;
  uint32_t           pad[2];
};
struct MeshTable
{
  uint32_t    count, totalTris;
  uint32_t    pad[2];
  MeshInstDev inst[kMaxMeshInstances];
};
// set-up record of one rasterised triangle: window coordinates snapped to 1/256 pixel, window depth and 1 / w per vertex.  64 B,
// fetched by the resolve pass with four 16-byte loads.  A primitive that was clipped keeps its sub-triangles in MeshClipRec.
struct alignas(16) MeshTriRec
{
  int32_t  x[3], y[3];
  float    z[3], invw[3];
  uint32_t clipBase;  // kMeshNone: the primitive's own three vertices; otherwise the first of nSub MeshClipRec
  uint32_t nSub;
  uint32_t pad[2];
};
// a sub-triangle of a clipped primitive: the same, plus each vertex as weights of the primitive's three vertices.  96 B.
struct alignas(16) MeshClipRec
{
  int32_t x[3], y[3];
  float   z[3], invw[3];
  float   bary[9];  // [vertex][weight]
  uint32_t pad[3];
};
static_assert(sizeof(MeshTriRec) == 64 && sizeof(MeshClipRec) == 96, "whole 16-byte vectors");
struct MeshCounters
{
  unsigned long long workCount;  // work-list slots claimed (never decremented; may exceed the capacity)
  unsigned long long fragments;
  uint32_t clipCount;            // MeshClipRec allocated
  uint32_t trisRasterised;
  uint32_t flags;                // bit 0: the clip records overflowed (geometry was dropped); bit 1: the work list was full (slow, exact)
  uint32_t pad;
};
// what the mesh kernels receive by value
struct MeshPassArgs
{
  float              view[16], proj[16];
  float              origin[3];   // translation of viewInverse (host double, rounded once)
  float              cameraPos[3];
  int32_t            width, height;
  int32_t            row0, row1;  // pixel rows [row0, row1) of the handle's strip
  int32_t            lightingMode;
  const MeshTable*   table;
  const LightTable*  lights;
  unsigned long long* vis;        // [height][width] depth bits << 32 | primitive << 3 | sub-triangle
  MeshTriRec*        recs;        // [totalTris]
  MeshClipRec*       clips;
  uint32_t           clipCapacity;
  uint2*             work;        // (primitive << 3 | sub-triangle, chunk of tiles); x == kMeshNone: a void slot
  uint32_t           workCapacity;
  MeshCounters*      ctr;
  float*             outDepth;
  float4*            outColor;
  uint32_t*          outPrim;
};

// ---- ray-traced splats (k_bvh.hip, k_trace.hip, api_trace.hip) ----
// The hierarchy is an implicit complete 8-ary tree: level 0 holds the leaves (one per traceable particle, sorted by the 30-bit Morton
// code of the leaf centre), node i of level L + 1 bounds the children [8i, 8i + 8) of level L.  A node is two float4: (lo.xyz, w) and
// (hi.xyz, 0); a leaf's lo.w holds the particle's global STORAGE id as bits.  All levels live in one array.
constexpr int      kBvhMaxLevels = 11;           // 8^10 = 2^30 leaves, the library's limit of global splats
constexpr uint32_t kTraceInvalid = 0xFFFFFFFFu;  // PAYLOAD_INVALID_ID
struct TraceInst
{
  float rsInv[9];  // transformRotScaleInverse = inverse(mat3(transform)), host double rounded once, glm column-major
  float pad[3];
};
struct TraceInstTable
{
  TraceInst inst[kMaxInstances];
};
// what the leaf kernel and the traversal need to agree on: the proxy ellipsoid's threshold (particle_as_build.comp.slang:74-87)
struct TraceProxy
{
  float   kernelMinResponse;
  int32_t adaptiveClamping;
  int32_t kernelDegree;
  float   alphaCull;
};
struct BvhBuildArgs
{
  const FrameArgs* frame;       // instances (transforms, set buffers) of this frame's upload
  TraceProxy       proxy;
  float            sceneLo[3], sceneInvExt[3];  // Morton quantisation frame (host: the instances' transformed set boxes)
  uint32_t         totalSplats;
  uint32_t*        keys;        // [totalSplats] Morton code, kTraceInvalid = no leaf
  uint32_t*        vals;        // [totalSplats] global storage id
  float4*          leafBox;     // [2 * totalSplats]
};
struct TraceCounters
{
  unsigned long long nodeVisits, candidateTests, acceptedHits;
  uint32_t           maxPassesUsed, pad;
};
// what the traversal kernel receives by value
struct TraceArgs
{
  const FrameArgs*      frame;
  const float4*         nodes;
  const uint32_t*       callerId;   // [totalSplats] storage id -> caller's id (tie order)
  const TraceInstTable* inst;
  TraceCounters*        ctr;
  uint32_t              levelOffset[kBvhMaxLevels], levelCount[kBvhMaxLevels];
  int32_t               nLevels;    // 0: no leaf at all
  uint32_t              totalNodes;
  TraceProxy            proxy;
  int32_t               samplesPerPass, maxPasses;
  float                 minTransmittance, depthIsoThreshold;
  void*                 image;
  int32_t               fmt;
  uint32_t*             hitCount;   // [height][width]
  float*                outDepth;   // side outputs, null unless surface_outputs
  uint32_t*             outId;
  float4*               outNormal;
  float*                outIsoDist;   // a lit frame's inputs of the light pass (mgs_render_traced_lit), null otherwise: the ray
  float4*               outRadiance;  // parameter of the iso-surface hit (0 = none) and the pixel in fp32 (rgb, 1 - T)
};
// what k_trace<., ., true> receives by value, the traversal of a frame with mesh hits (mgs_frame_set_trace_meshes): TraceArgs, which
// every other kernel keeps as it is, plus the upper end of the pixel's particle walk and what the mesh composite weights the mesh with
struct TraceWalkMeshArgs
{
  TraceArgs    t;
  const float* meshT;     // [height][width] t of the pixel's closest mesh hit, +inf = none
  float*       outWalkT;  // [height][width] float(T) of the walk; -1 when T > meshMinT fails in double
  float        meshMinT;  // min_mesh_composite_transmittance
};
// the triangle hierarchy and the per-pixel mesh buffers of a traced frame with mesh hits (k_trace_mesh.hip, k_trace_light.hip)
struct MeshRayCounters;  // (below, with the mesh ray queries)
struct TraceMeshArgs
{
  TraceArgs        h;        // the triangle hierarchy for the traversal (nodes, levels, node count; nothing else of it is read)
  const float4*    tris;
  const MeshTable* table;
  float4*          hits;     // [height][width][4] the pixel's hit record, as a mesh ray query writes it
  float*           meshT;    // [height][width] its t, +inf = none
  const float*     walkT;    // [height][width] what k_trace left in TraceArgs::outWalkT
  MeshRayCounters* ctr;      // [2] the primary mesh rays' sums, the mesh occlusion rays' sums
  float            minT;     // min_mesh_composite_transmittance
};
// what a ray query (k_trace_rays.hip, mgs_trace_rays) receives by value: the traversal's arguments (image, hit counts and side outputs
// stay null) and the caller's batch.  A ray is two float4, (origin, t_min) and (direction, t_max); a result three, (radiance,
// float(T)), (t_iso, id, hit count, passes as bits) and the integrated normal with its weight.
struct TraceRaysArgs
{
  TraceArgs       t;
  const float4*   rays;     // [2 * count]
  float4*         results;  // [3 * count], at the ray's index in the caller's order
  const uint32_t* perm;     // [count] lane -> ray index (a reordered batch), or null: the caller's order
  uint32_t        count;
  uint32_t*       invalid;  // [1] rays that were refused (non-finite, zero direction, t_min > t_max)
  int32_t         surf;     // 1: integrate the normals (surface_outputs)
};
// the coherence keys of a reordered batch (k_rays_key): the scene box of the hierarchy's Morton frame (api_trace.hip: sceneBox)
struct RayKeyArgs
{
  const float4* rays;
  uint32_t*     keys;  // [count]
  uint32_t*     idx;   // [count] iota, the sort's values
  uint32_t      count;
  float         sceneLo[3], sceneInvExt[3];
};
// the shadow rays' statistics (MgsTraceLightOut)
struct TraceLightCounters
{
  unsigned long long shadowRays, nodeVisits, candidateTests, acceptedHits;
};
// what the light pass of a lit traced frame (k_trace_light.hip) receives by value.  Its per-pixel inputs are plain buffers: the
// primary surface may come from another producer than k_trace.
struct TraceLightArgs
{
  TraceArgs           t;            // hierarchy, frame, proxy, samplesPerPass, image, fmt as the primary rays had them
  const float*        isoDist;      // [height][width] ray parameter of the surface, 0 = none (discarded), < 0 = settled by the producer (left alone)
  const uint32_t*     pickId;       // [height][width] global storage id of the picked particle
  const float4*       normal;       // [height][width] integrated normal (unnormalised) and weight
  const float4*       radiance;     // [height][width] fp32 radiance and alpha of the primary walk
  const LightTable*   table;
  uint32_t*           shadowHits;   // [height][width] accepted shadow hits, summed over the lights
  TraceLightCounters* lctr;
  int32_t             shadowsMode;  // MGS_SHADOWS_*
  int32_t             shFormat;     // storage format of the SH records (read when shadowColorStrength != 0)
  float               shadowOffset, shadowThreshold, shadowColorStrength;
};

// what a shadow or light query (k_shadow_query.hip; mgs_trace_shadow_rays, mgs_shade_points) receives by value: the traversal's
// arguments (image, hit counts and side outputs stay null) and the caller's batch.  A shadow ray is a ray query's two float4; a
// surface point four, (position, material index as bits), (normal, -), (view direction, -), (radiance, -).  A result is one float4:
// (transmittance, hits as bits) of a shadow ray, (colour, shadow hits as bits) of a point.
struct ShadowQueryArgs
{
  TraceArgs           t;
  const float4*       items;     // [2 * count] rays or [4 * count] points
  float4*             results;   // [count], at the item's index in the caller's order
  const uint32_t*     perm;      // [count] lane -> item index (a reordered batch), or null: the caller's order
  uint32_t            count;
  uint32_t*           invalid;   // [1] items that were refused
  TraceLightCounters* lctr;      // points: the shadow rays' sums (the rays' own go to t.ctr)
  const LightTable*   table;     // points: the scene's lights
  const MaterialDev*  mats;      // points: the call's materials
  uint32_t            matCount;
  int32_t             shadowsMode;  // points: MGS_SHADOWS_*
  int32_t             shFormat;     // storage format of the SH records (read when shadowColorStrength != 0)
  float               shadowOffset, shadowThreshold, shadowColorStrength;
  float               cameraPos[3];  // points: the headlight's position
};
// the coherence keys of a reordered batch of points (k_points_key): the Morton cell of the position alone
struct PointKeyArgs
{
  const float4* points;  // [4 * count]
  uint32_t*     keys;
  uint32_t*     idx;
  uint32_t      count;
  float         sceneLo[3], sceneInvExt[3];
};

// what the hand-over of a hybrid frame (k_hybrid.hip, mgs_render_hybrid) receives by value: the raster pass's pixel and side outputs
// in, the light pass's per-pixel inputs (TraceLightArgs) out
struct HybridSurfaceArgs
{
  const FrameArgs* frame;
  void*            image;        // the frame as the compositor left it, in the target format (read; never written)
  const float*     depth;        // picked ndc depth                       } the raster side outputs,
  const uint32_t*  id;           // picked splat (global storage id)       } left as they are
  const float4*    normal;       // integrated normal and weight           }
  float*           outIsoDist;   // ray parameter of the surface; 0: discarded; < 0: the pixel is settled, the light pass leaves it alone
                                 // (the light pass reads the raster pass's picked ids as they are: the ray parameter alone filters)
  float4*          outNormal;    // the normalised normal (the handle's own scratch)
  float4*          outRadiance;  // the stored pixel in fp32: rgb and alpha
};
// the hand-over of a hybrid frame with meshes (mgs_frame_set_hybrid_meshes): besides the above, the pixel's transmittance for the mesh
// composite, and a surface that is not in front of the pixel's mesh hit is handed on settled
struct HybridSurfaceMeshArgs
{
  HybridSurfaceArgs a;
  const float*      meshT;  // [height][width] t of the pixel's closest mesh hit (the depth pre-pass), +inf = none
  float*            outT;   // [height][width] 1 - stored alpha; 1 for a discarded pixel; -1 when T > minT fails in double
  float             minT;   // min_mesh_composite_transmittance
};

// ---- mesh ray queries (k_mesh_bvh.hip, k_mesh_rays.hip, api_mesh_rays.hip) ----
// The triangle hierarchy has the splat hierarchy's layout (above): level 0 holds one leaf per valid triangle of every mesh instance,
// sorted by the 30-bit Morton code of the leaf centroid, and a leaf's lo.w holds the LEAF's own index as bits, which is also the index
// of its triangle record.  A record is three float4 in leaf order: (world v0, global primitive id), (world v1, instance id),
// (world v2, material id), the ids as bits.
struct MeshBvhBuildArgs
{
  const MeshTable* table;
  float            boxLo[3], boxInvExt[3];  // Morton quantisation frame (host: the instances' transformed local boxes)
  uint32_t         totalTris;
  uint32_t*        keys;     // [totalTris] Morton code, kTraceInvalid = no leaf
  uint32_t*        vals;     // [totalTris] global primitive id
  float4*          leafBox;  // [2 * totalTris]
};
struct MeshBvhRecordArgs
{
  const MeshTable* table;
  const uint32_t*  sortedVals;  // [leaves] global primitive id of leaf i
  float4*          level0;      // [2 * leaves] the gathered leaves: lo.w becomes i
  float4*          tris;        // [3 * leaves]
  uint32_t         leaves;
};
// what k_trace_light<., true> and k_trace_mesh_composite receive by value in a frame with mesh hits: the light pass's arguments as
// every other launch has them, the triangle hierarchy with the per-pixel mesh buffers, and the lit splat surface in fp32
struct TraceLightMeshArgs
{
  TraceLightArgs l;
  TraceMeshArgs  m;
  float4*        litOut;  // [height][width] for the mesh composite behind the light pass
};
struct MeshRayCounters
{
  unsigned long long nodeVisits, triangleTests, hits;
  uint32_t           invalidRays, pad;
};
// what the ray/triangle kernel receives by value.  `t` carries the hierarchy for the traversal of trace_traverse.h (nodes, levels,
// node count); nothing else of it is read and its frame pointer stays null.  A hit is four float4: (t, instance, primitive,
// material), (world position, b1), (world normal, b2), (hit flag, 0, 0, 0).
struct MeshRayArgs
{
  TraceArgs        t;
  const float4*    tris;
  const MeshTable* table;
  const float4*    rays;  // [2 * count]
  float4*          hits;  // [4 * count], at the ray's index in the caller's order
  const uint32_t*  perm;  // [count] lane -> ray index (a reordered batch), or null: the caller's order
  uint32_t         count;
  MeshRayCounters* ctr;
};

// ---- reflection and refraction bounces (k_trace_bounce.hip, api_trace.hip: mgs_render_traced_indirect) ----
constexpr int kMaxBounces = 16;  // the range of MgsTraceBounceParams::max_bounces
// MgsBounceMaterial as the kernels read it (two 16-byte loads)
struct alignas(16) BounceMatDev
{
  float    transmittance[3];
  float    ior;
  int32_t  illum;
  uint32_t pad[3];
};
// per mesh instance its slice of the scene's flat bounce-material array; count 0 = never set (every material id is illum 0)
struct BounceTable
{
  uint32_t offset[kMaxMeshInstances], count[kMaxMeshInstances];
};
struct BounceCounters
{
  unsigned long long rays[kMaxBounces], meshHits[kMaxBounces], particleHits;
};
// What the kernels of an indirect frame receive by value: the lit mesh frame's arguments as its composite has them, the bounce
// materials, and the per-pixel bounce state (64 B a pixel): a live word, nine fp32 planes (ray origin, ray direction, radiance) and
// three fp64 planes (the transmittance, carried between the kernels in double)
struct TraceBounceArgs
{
  TraceLightMeshArgs  g;
  const BounceTable*  btab;
  const BounceMatDev* bmats;
  uint32_t*           live;    // [pixels] 1: the pixel traces the next bounce
  float*              ray;     // [9][pixels]
  double*             T;       // [3][pixels]
  BounceCounters*     bctr;
  size_t              pixels;  // the planes' stride
  int32_t             bounce;  // 1 .. max_bounces: the bounce this launch traces (k_trace_bounce)
};

// the caller's geometry as the compositors' launchers receive it
struct Occluder
{
  const float* depth = nullptr;
  const float* color = nullptr;
  bool         sortedByKey = false;
};

// projected splat record consumed by the compositor: 32 B = half a 64-byte sector, 16-B aligned.  It holds only what
// the per-fragment arithmetic and the region cull need; base colour, view direction and fragCoord.z are rebuilt by the
// compositor for the records it stages (a quarter of them), from the splat's own buffers.
struct alignas(16) SplatRec
{
  float    cx, cy;    // centre in pixels
  float    p1x, p1y;  // 2*b1/|b1|^2 : (d.p1)^2 + (d.p2)^2 == A/2 of threedgs_raster.frag.slang:236
  float    p2x, p2y;
  float    a;         // opacity (after MS_ANTIALIASING)
  uint32_t exey;      // half2: tight half extents of the visible footprint in pixels, rounded UP (cull tests only)
};

// 3DGUT projected record: 96 B, indexed by global id.  The per-fragment evaluator needs the particle itself, not a 2D
// conic: with A = S^-1 R^T (canonical frame), N = 3x3 of M^-1, o = camera origin, the canonical ray of a fragment with
// world direction d is  origin ro = A (M^-1 o - p) (per splat)  and  direction ~ B d, B = A N (per splat), so
// dist^2 = |B d x ro|^2 / |B d|^2 (threedgrt.h.slang:57-81) costs 9 FMAs + a cross product per fragment.
struct alignas(16) GutRec
{
  float cx, cy;        // UT mean in pixels (quad centre)
  float q1x, q1y;      // half1 / |half1|^2 : |d.q1| <= 1 and |d.q2| <= 1  <=>  the pixel centre is inside the quad
  float q2x, q2y;
  float bex, bey;      // half extents of the quad's bounding box in pixels (culling only)
  float B[9];
  float ro[3];
  float r, g, b, a;    // colour incl. SH; opacity after MS antialiasing
};
static_assert(sizeof(GutRec) == 96, "six 16-byte vectors");

}  // namespace mgs
