/*
 * mgs.h — C ABI of the MI355X-native VK3DGSR hot path ("mgs" = MI355X gaussian splatting).
 *
 * This header is the drop-in boundary.  The reference
 * (nvpro-samples/vk_gaussian_splatting @ 2026.1.6) has no plugin/FFI API; the seam below is the
 * narrowest set of C++ member calls through which its renderer is reached.  Every entry point
 * cites the reference interface it replaces.  Plain pointers and sizes only; no exceptions
 * cross this boundary; every function returns an MgsStatus (0 = ok, <0 = error) and the
 * message is available from mgs_last_error() (thread-local).
 *
 * Matrix convention: float[16] in glm column-major memory order (m[col*4+row]), right-handed,
 * clip z in [0,1]; proj[5] may be negative (Vulkan Y flip) — exactly what
 * nvutils::CameraManipulator hands to GaussianSplatting::updateAndUploadFrameInfoUBO
 * (src/gaussian_splatting.cpp:1162-1173).
 *
 * Threading: handle-level thread compatibility — one thread per MgsScene at a time
 * (the reference has a single Vulkan submitter thread, src/gaussian_splatting.cpp:335).
 */
#ifndef MGS_H
#define MGS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_ABI_VERSION 5 /* 2: MgsFrameParams grew the 3DGUT fields; loader, strip-exchange and debug entry points added;
                            3: stochastic splats, depth of field, temporal accumulation (MgsFrameParams 256 -> 288 bytes);
                            4: MgsFrameOut 80 -> 88 bytes (escape_count);
                            5: occluder entry points (mgs_frame_set_occluder, mgs_frame_upload_occluder); no struct changed */
#define MGS_ABI_MINOR 1   /* backward-compatible additions within MGS_ABI_VERSION (same struct sizes, same defaults):
                            5.1: deferred lighting — MgsFrameParams::reserved_[0] is named lighting_mode (0 = what it was), MgsLight / MgsMaterial,
                                 mgs_light_default, mgs_material_default, mgs_scene_set_lights, mgs_instance_set_material,
                                 mgs_frame_download_surface(which = 3), MGS_STAGE_LIGHT;
                            image compare (MGS_HAS_IMAGE_COMPARE below): entry points only, both numbers stay — mgs_compare_capture,
                                 mgs_compare_capture_upload, mgs_compare_release, mgs_compare_params_default, mgs_compare_metrics,
                                 mgs_compare_view_default, mgs_compare_composite, mgs_compare_download_composite;
                            meshes (MGS_HAS_MESHES below): entry points only, both numbers stay — mgs_mesh_from_arrays, mgs_mesh_load_obj, mgs_mesh_view,
                                 mgs_mesh_destroy, mgs_mesh_instance_add, mgs_mesh_instance_set_transform, mgs_mesh_instance_set_visible,
                                 mgs_meshes_render, mgs_meshes_download;
                            ray-traced splats (MGS_HAS_TRACE below): entry points only, both numbers stay — mgs_trace_params_default,
                                 mgs_render_traced, mgs_trace_download_hit_counts;
                            lit traced frames (MGS_HAS_TRACE_LIGHTING below): entry points only, both numbers stay —
                                 mgs_trace_light_params_default, mgs_render_traced_lit, mgs_trace_download_shadow_hits;
                            hybrid frames (MGS_HAS_HYBRID below): one entry point, both numbers stay — mgs_render_hybrid;
                            3DGUT record hook (MGS_HAS_PROJECTED_GUT below): one entry point, both numbers stay —
                                 mgs_frame_download_projected_gut;
                            trace strategies (MGS_HAS_TRACE_STRATEGIES below): no entry point, both numbers stay — MgsTraceParams::reserved[0] is
                                 named trace_strategy (0 = what it was), MGS_TRACE_STRATEGY_*;
                            ray queries (MGS_HAS_RAY_QUERY below): entry points only, both numbers stay — mgs_ray_query_params_default,
                                 mgs_trace_rays, mgs_trace_rays_device, mgs_trace_generate_rays;
                            sensor models (MGS_HAS_SENSOR_MODEL below): entry points and one new struct, both numbers stay —
                                 mgs_sensor_model_from_frame, mgs_frame_set_sensor;
                            shadow and light queries (MGS_HAS_SHADOW_QUERY below): entry points and new structs, both numbers stay —
                                 mgs_trace_shadow_rays, mgs_trace_shadow_rays_device, mgs_shade_points, mgs_shade_points_device;
                            mesh ray queries (MGS_HAS_MESH_RAY_QUERY below): entry points and new structs, both numbers stay —
                                 mgs_mesh_ray_params_default, mgs_trace_mesh_rays, mgs_trace_mesh_rays_device;
                            hierarchy hook (MGS_HAS_DEBUG_HIERARCHY below): one entry point and one new struct, both numbers stay —
                                 mgs_debug_download_hierarchy;
                            meshes in the hybrid frames (MGS_HAS_HYBRID_MESHES below): two entry points, both numbers stay —
                                 mgs_frame_set_hybrid_meshes, mgs_debug_download_hybrid_depth */
#define MGS_HAS_IMAGE_COMPARE 1 /* feature macro: the mgs_compare_* entry points exist (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_TRACE 1         /* feature macro: mgs_render_traced and its companions exist (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_TRACE_LIGHTING 1 /* feature macro: mgs_render_traced_lit and its companions exist (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_TRACE_STRATEGIES 1 /* feature macro: MgsTraceParams::trace_strategy and MGS_TRACE_STRATEGY_* exist (within ABI 5.1: the first reserved word
                                     of MgsTraceParams is named, 0 = what it was; no struct size or default changed) */
#define MGS_HAS_RAY_QUERY 1     /* feature macro: mgs_trace_rays and its companions exist (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_SHADOW_QUERY 1  /* feature macro: mgs_trace_shadow_rays, mgs_shade_points and their _device variants exist (added within ABI 5.1, no
                                  existing struct or default changed) */
#define MGS_HAS_MESH_RAY_QUERY 1 /* feature macro: mgs_trace_mesh_rays and its companions exist (added within ABI 5.1, no existing struct or default
                                   changed) */
#define MGS_HAS_HYBRID 1        /* feature macro: mgs_render_hybrid exists (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_SOFT_SHADOWS 1  /* feature macro: mgs_scene_set_light_radii exists, and mgs_render_traced_lit and mgs_render_hybrid accept MGS_SHADOWS_SOFT
                                   in a process started with MGS_SOFT_SHADOWS=1 (added within ABI 5.1, no struct, default or outcome of an
                                   existing call changed: without the switch MGS_SHADOWS_SOFT stays MGS_ERR_UNSUPPORTED) */
#define MGS_HAS_MESHES 1        /* feature macro: the mgs_mesh_* / mgs_meshes_* entry points exist (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_PROJECTED_GUT 1 /* feature macro: mgs_frame_download_projected_gut exists (added within ABI 5.1, no struct or default changed) */
#define MGS_HAS_DEBUG_HIERARCHY 1 /* feature macro: MgsHierarchyInfo and mgs_debug_download_hierarchy exist (added within ABI 5.1, no existing struct
                                   or default changed) */
#define MGS_HAS_SENSOR_MODEL 1  /* feature macro: MgsSensorModel, mgs_sensor_model_from_frame and mgs_frame_set_sensor exist (added within ABI 5.1, no
                                  existing struct or default changed) */

typedef enum MgsStatus {
  MGS_OK              = 0,
  MGS_ERR_INVALID_ARG = -1,
  MGS_ERR_IO          = -2,  /* file missing / unreadable            (PlyLoaderAsync E_FAILURE, ply_loader_async.h:37-44) */
  MGS_ERR_FORMAT      = -3,  /* not a valid 3DGS .ply/.spz/.splat    ("invalid 3DGS PLY file", ply_loader_async.cpp:449)  */
  MGS_ERR_DEVICE      = -4,  /* HIP error                            (NVVK_CHECK, never aborts here)                     */
  MGS_ERR_OOM         = -5,
  MGS_ERR_STATE       = -6,  /* call order violated (e.g. render before commit)                                          */
  MGS_ERR_OVERFLOW    = -7,  /* tile-pair capacity exceeded; frame is incomplete                                         */
  MGS_ERR_UNSUPPORTED = -8
} MgsStatus;

/* storage formats — shaders/shaderio.h:60-62 (FORMAT_FLOAT32/16/UINT8), chosen at
 * SplatSetVk::initDataStorage(shFormat, rgbaFormat) (src/splat_set_vk.h:112) */
enum { MGS_FORMAT_FLOAT32 = 0, MGS_FORMAT_FLOAT16 = 1, MGS_FORMAT_UINT8 = 2 };
/* sorting methods — shaders/shaderio.h SORTING_* / parameters.h:182 */
enum { MGS_SORT_GPU_RADIX = 0, MGS_SORT_CPU_ASYNC = 1,
       /* SORTING_STOCHASTIC_SPLAT (shaderio.h:27; threedgs_raster.frag.slang:265-290, threedgut_raster.frag.slang:150-172):
        * every fragment is accepted with probability alpha and written opaque, the depth test keeps the nearest accepted
        * one.  The reference skips the sort and lets the depth buffer resolve; here the sorted per-bin lists are walked
        * nearest first and the first accepted fragment ends the pixel (same winner, ties aside). */
       MGS_SORT_STOCHASTIC = 3 };
enum { MGS_DOF_DISABLED = 0, MGS_DOF_FIXED_FOCUS = 1 }; /* shaderio.h:136-138; DOF_AUTO_FOCUS picks the distance under the UI's
                                                           cursor and then behaves as FIXED_FOCUS: pass that distance */
/* frustum culling — shaders/shaderio.h:84-86 / parameters.h:184 */
enum { MGS_CULL_NONE = 0, MGS_CULL_AT_DIST = 1, MGS_CULL_AT_RASTER = 2 };
/* colour target — src/gaussian_splatting.h:338-340 (RGBA16F default, RGBA32F optional) */
/* colour target (gaussian_splatting.h:338-340, doc/overview: RGBA8 / RGBA16F (default) / RGBA32F); RGBA8 is linear UNORM */
enum { MGS_TARGET_RGBA16F = 0, MGS_TARGET_RGBA32F = 1, MGS_TARGET_RGBA8 = 2 };
/* visualisation modes: POINT_CLOUD_MODE (threedgs.h.slang:108-110), SHOW_SH_ONLY (mesh.slang:205-207),
 * DISABLE_OPACITY_GAUSSIAN (frag.slang:248-255) */
enum { MGS_DEBUG_POINT_CLOUD = 1, MGS_DEBUG_SH_ONLY = 2, MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED = 4 };
/* alpha channel meaning: the reference's default back-to-front pipeline accumulates
 * A = sum(alpha) (src/gaussian_splatting.cpp:2083-2084); its FTB pipeline yields 1-T (:2071-2076). */
enum { MGS_ALPHA_COVERAGE = 0 /* 1-T */, MGS_ALPHA_SUM = 1 /* sum(alpha); disables early termination */ };
enum { MGS_NORMAL_MAX_DENSITY_PLANE = 0, MGS_NORMAL_ISO_SURFACE = 1 };
/* raster pipelines (parameters.h PIPELINE_MESH / PIPELINE_MESH_3DGUT), 3DGUT camera models and quad extents */
enum { MGS_PIPELINE_3DGS = 0, MGS_PIPELINE_3DGUT = 1 };
/* lighting of the splat surface — shaderio.h:131-133 (LIGHTING_*), parameters.h:128-132.  The raster-only pipelines only test
 * "!= disabled" (deferred_shading.comp.slang has no branch on direct / indirect): DIRECT and INDIRECT render the same frame. */
enum { MGS_LIGHTING_DISABLED = 0, MGS_LIGHTING_DIRECT = 1, MGS_LIGHTING_INDIRECT = 2 };
/* LightType, shaders/wavefront.h:73-78 */
enum { MGS_LIGHT_DIRECTIONAL = 0, MGS_LIGHT_POINT = 1, MGS_LIGHT_SPOT = 2 };
#define MGS_MAX_LIGHTS 64 /* build-defined cap of mgs_scene_set_lights (the reference's light table is a device buffer without one) */
enum { MGS_CAMERA_PINHOLE = 0, MGS_CAMERA_FISHEYE = 1 };
enum { MGS_EXTENT_EIGEN = 0, MGS_EXTENT_CONIC = 1 };

typedef struct MgsSplatSet_t* MgsSplatSet; /* RAM model == struct SplatSet, src/splat_set.h:33-48 */
typedef struct MgsScene_t*    MgsScene;    /* device scene == SplatSetManagerVk + renderer buffers  */

/* The six SoA arrays of SplatSet (src/splat_set.h:36-42), INRIA semantics, ALREADY in the
 * renderer's RUB frame (i.e. after SplatSet::convertCoordinates(RDF,RUB), splat_set.h:78-114):
 * positions[3n], f_dc[3n], f_rest[f_rest_per_splat*n] channel-major (all R, all G, all B),
 * opacity[n] (logit), scale[3n] (log), rotation[4n] (w,x,y,z). */
typedef struct MgsSplatSetView {
  const float* positions;
  const float* f_dc;
  const float* f_rest;
  const float* opacity;
  const float* scale;
  const float* rotation;
  uint64_t     splat_count;
  uint32_t     f_rest_per_splat; /* 0, 9, 24 or 45 */
  int32_t      sh_degree;        /* out only: SplatSet::maxShDegree(), splat_set.h:52-74 */
} MgsSplatSetView;

/* ---- errors ---- */
const char* mgs_last_error(void);
const char* mgs_version(void);

/* ---- ingest: replaces PlyLoaderAsync::loadScene / innerLoad (src/ply_loader_async.h:62,
 * src/ply_loader_async.cpp:291-453).  Synchronous; dispatches on the lower-cased extension
 * (.ply via the INRIA property names, .spz = Niantic gzip "NGSP" v1-3, .splat = 32-byte records)
 * and leaves the set in RUB coordinates exactly like the reference. */
int  mgs_splatset_load(const char* path, MgsSplatSet* out);
/* copies the arrays; caller keeps ownership of the host pointers (valid only during the call) */
int  mgs_splatset_from_arrays(const MgsSplatSetView* view, MgsSplatSet* out);
/* borrow the set's arrays (valid until mgs_splatset_destroy) */
int  mgs_splatset_view(MgsSplatSet set, MgsSplatSetView* out);
void mgs_splatset_destroy(MgsSplatSet set);

/* ---- asynchronous ingest with a request queue: PlyLoaderAsync (src/ply_loader_async.h:35-106: one loader thread,
 * states E_READY / E_LOADING / E_LOADED / E_FAILURE, reset before the next load) plus the scene-load queue the UI drains
 * one file at a time (prmScene.sceneLoadQueue, src/gaussian_splatting_ui.cpp:1149-1152,1235-1436: files are queued, the
 * loader takes the next one when idle, a failure does not stop the queue).  Host only: no device is touched. */
typedef struct MgsLoader_t* MgsLoader;
enum { MGS_LOADER_READY = 1, MGS_LOADER_LOADING = 2, MGS_LOADER_LOADED = 3, MGS_LOADER_FAILURE = 4 };  /* ply_loader_async.h:37-44 */
int  mgs_loader_create(MgsLoader* out);                 /* PlyLoaderAsync::initialize: starts the loader thread */
void mgs_loader_destroy(MgsLoader loader);              /* shutdown: joins the thread, drops what is queued */
int  mgs_loader_push(MgsLoader loader, const char* path); /* pushLoadRequest: append to the queue (any state) */
/* getStatus: the state of the request at the head (READY when nothing is queued or loading); *queued = requests waiting
 * behind it, *path_out (optional, >= path_capacity bytes) = its file name */
int  mgs_loader_status(MgsLoader loader, int* state, uint32_t* queued, char* path_out, size_t path_capacity);
/* LOADED: hands over the splat set (caller owns it) and resets — the next queued file starts loading.
 * FAILURE: returns the load's error code (message in mgs_last_error) and resets likewise.  Other states: MGS_ERR_STATE. */
int  mgs_loader_take(MgsLoader loader, MgsSplatSet* out);

/* ---- scene: replaces SplatSetManagerVk::createSplatSet/createInstance/updateInstanceTransform/
 * processVramUpdates (src/splat_set_manager_vk.h:202,222-249,261).  `device` is the HIP ordinal. */
int  mgs_scene_create(int device, MgsScene* out);
void mgs_scene_destroy(MgsScene scene);
/* run on a caller-owned hipStream_t (NULL = the scene's own stream) */
int  mgs_scene_set_stream(MgsScene scene, void* hip_stream);
/* instances are concatenated in creation order into the global splat id space
 * (rebuildGlobalIndexTables, src/splat_set_manager_vk.cpp:2304-2360) */
int  mgs_instance_add(MgsScene scene, MgsSplatSet set, const float transform[16], int* instance_id);
int  mgs_instance_set_transform(MgsScene scene, int instance_id, const float transform[16]);
/* SplatSetVk::initDataStorage + initDataBuffers (src/splat_set_vk.cpp:117-170,188-480): builds the
 * device buffers (centres, 3D covariances, RGBA, interleaved SH) in the requested formats.
 * Idempotent; call again after changing formats (the reference's --updateData). */
int  mgs_scene_commit(MgsScene scene, int sh_format, int rgba_format);
/* ---- lights and materials of the deferred lighting pass (MgsFrameParams::lighting_mode).
 * MgsLight: the fields of shaderio::LightSource (shaders/wavefront.h:81-93) minus `radius`, which only the ray-traced soft shadows
 * read and which has its own setter (mgs_scene_set_light_radii, below).  direction is the direction the light shines in (the reference derives it from the light instance's rotation applied
 * to (0,0,-1), light_manager_vk.cpp:470-471); cone angles in degrees; attenuation_mode 0 none, 1 linear, 2 quadratic, 3 physical. */
typedef struct MgsLight {
  int32_t type;             /* MGS_LIGHT_*, default MGS_LIGHT_POINT */
  float   color[3];         /* default 1 1 1 */
  float   intensity;        /* default 1 */
  float   position[3];      /* default 0 0 0 */
  float   range;            /* default 10: point / spot lights shade nothing farther away */
  float   direction[3];     /* default 0 0 -1 */
  float   inner_cone_deg, outer_cone_deg; /* default 30, 45 */
  int32_t attenuation_mode; /* default 2 */
} MgsLight;
void mgs_light_default(MgsLight* light); /* fills the defaults above (wavefront.h:81-93) */
/* The scene's light table, shared by all its frame contexts like the instance transforms (MGS_ERR_STATE on a context handle).
 * Copies `count` lights; count = 0 restores "no lights", which the lighting pass renders with a headlight at the camera
 * (createHeadlight, wavefront.h.slang:104-119).  More than MGS_MAX_LIGHTS lights, a type or an attenuation mode out of range:
 * MGS_ERR_INVALID_ARG.  Takes effect on every context's next frame without a re-commit: the call waits for the frames in
 * flight on all contexts, then rewrites the device table the lighting pass reads (captured frames are not re-captured). */
int  mgs_scene_set_lights(MgsScene scene, const MgsLight* lights, int count);
/* The radius of each entry of the light table (MGS_HAS_SOFT_SHADOWS): LightSource::radius (wavefront.h:92), which the reference
 * fills from the light's proxyScale (light_manager_vk.cpp:480, :533; default 1.0, :104).  Read by MGS_SHADOWS_SOFT only: a point or
 * spot light is sampled on a disk of HALF this radius (wavefront.h.slang:54), 0 makes the light a hard one.  `count` must equal the
 * current light count; anything else, or a radius that is negative or not finite: MGS_ERR_INVALID_ARG.  NULL with count 0 restores
 * the default 1.0 for every light, and so does every mgs_scene_set_lights.  A context handle: MGS_ERR_STATE.  Ordering as
 * mgs_scene_set_lights: waits for the frames in flight on all contexts, rewrites the device table, rebuilds no hierarchy. */
int  mgs_scene_set_light_radii(MgsScene scene, const float* radii, int count);
/* An instance's material: splatMaterial of the splat set instance (shaderio::ObjMaterial, wavefront.h:37-50, reduced to what the
 * deferred pass reads).  needShading is derived inside as updateMaterialNeedsShading does (wavefront.h:55-59: the length of
 * diffuse, ambient or specular above 0.001). */
typedef struct MgsMaterial {
  float ambient[3], diffuse[3], specular[3], emission[3];
  float shininess;
} MgsMaterial;
/* the splat sets' default (src/splat_set_vk.cpp:128-135): all zero except emission = 1 — fully emissive, the lit frame shows the
 * splats' own colours */
void mgs_material_default(MgsMaterial* material);
/* same ordering rule as mgs_scene_set_lights; valid before and after mgs_scene_commit */
int  mgs_instance_set_material(MgsScene scene, int instance_id, const MgsMaterial* material);
uint64_t mgs_scene_splat_count(MgsScene scene); /* getTotalGlobalSplatCount, gaussian_splatting.cpp:369 */
/* ---- frame contexts: frames in flight over ONE resident scene.
 * The reference keeps a single copy of the splat buffers however many frames its application loop has in flight; that is why
 * processUpdateRequests waits for the device before it touches them (src/gaussian_splatting.cpp:1092-1111).  A frame context
 * is the per-frame-in-flight state of that loop: its own HIP stream, working buffers (slots, sort ping-pong, projected records,
 * bin lists, frame image, counters) and captured frame graphs, reading the scene's committed buffers.  The returned handle is
 * accepted by every frame-level entry point below (mgs_render, mgs_sort_keys, mgs_frame_*, mgs_timings_query, mgs_sync,
 * mgs_scene_set_stream, the multi-GPU exchange); the scene-editing entry points (mgs_instance_add, mgs_instance_set_transform,
 * mgs_scene_commit) return MGS_ERR_STATE on it — edit the scene.  Transforms set on the scene reach every context's next
 * frame; mgs_scene_commit waits for the frames in flight on all contexts, and each context re-sizes its working set on its
 * next frame.  Threading: one thread per handle at a time; do not edit or commit the scene while another thread renders one
 * of its contexts.  Contexts may outlive the scene handle (the data is freed with the last handle). */
int  mgs_frame_context_create(MgsScene scene, MgsScene* context_out);
void mgs_frame_context_destroy(MgsScene context);
/* capacity of this handle's per-bin splat lists in entries (4 B each); 0 restores the default of 32 per global splat.  Takes
 * effect before the next frame.  A frame whose lists do not fit is incomplete: mgs_frame_stats returns MGS_ERR_OVERFLOW and
 * sets bit 0 of error_flags (the analogue of the reference's fixed-size sorting buffers, splat_set_manager_vk.cpp:2304-2360,
 * which are sized for the splat count and cannot overflow because a quad is not a list entry). */
int  mgs_scene_set_list_capacity(MgsScene scene_or_context, uint64_t entries);
/* ---- occluder: splats composited with the caller's opaque geometry.  Replaces the mesh passes of renderHybridPipeline
 * (src/gaussian_splatting.cpp:697-805): the depth pre-pass the splats are tested against (test on, write off, :1377-1395) and the
 * composition final = meshColor * (1 - dstAlpha) + splatColor (:2343-2356); in back-to-front mode the meshes are drawn first and the
 * splats blend over them (:836-843, :2066-2087).  The caller rasterises its own geometry and binds the two images that yields, or
 * lets mgs_meshes_render (below) make them from the scene's mesh instances.
 *
 * Bind the images for the following frames of this handle (scene or frame context; per handle, like
 * mgs_scene_set_list_capacity).  depth_device: [height][width] float32, row 0 = NDC y -1 (the frame's own layout), window depth
 * in [0,1] made with the SAME proj as the frame (clip z in [0,1]); 1.0 = no geometry (the reference's depth clear).
 * color_device: [height][width][4] float32 linear, or NULL (= transparent black).  Caller-owned device memory, read on the handle's
 * stream by every later frame until re-bound; the caller may rewrite the contents between frames, ordered on that stream, without
 * re-binding.  NULL depth unbinds both.  A frame whose params width/height differ from the bound size: MGS_ERR_INVALID_ARG.
 *
 * Per pixel, with D the bound depth and z_i the ndc depth of splat i's centre (every quad of the reference is emitted at that one
 * depth, threedgs_raster.mesh.slang:286):
 *   - a fragment of splat i exists only if z_i <= D.  LESS_OR_EQUAL is what the reference states wherever it names the operator
 *     for blended geometry over a depth pre-pass (:1489-1493); the splat pipelines inherit the default of a pipeline-state class
 *     that is not part of the reference tree, so PARITY OF THE OPERATOR IS UNPINNED (LESS would differ only where z_i == D
 *     bit for bit).  A NaN depth passes nothing.
 *   - z_i is computed by the operations of the depth key (dist.comp.slang:55-62), not by those of the quad's vertex
 *     (mesh.slang:175-178): the same quantity with another product order, a last-bit difference of the kind documented for the
 *     front end.  It makes the per-bin lists exactly monotone in the tested value, so that a region whose remaining list lies
 *     behind the geometry stops early without ever changing a pixel (MGS_SORT_GPU_RADIX; MGS_SORT_CPU_ASYNC orders by plane
 *     distance and only tests per fragment).
 *   - MGS_ALPHA_COVERAGE: rgb = C + T * color.rgb, a = 1 - T (the geometry's alpha is ignored);
 *     MGS_ALPHA_SUM:      rgb = C + T * color.rgb, a = sum(alpha of the fragments that passed) + color.a.
 *     C, T are the fp32 accumulators; the target conversion happens after the background term.
 *   - surface_outputs: fragments that fail the test take no part in picked depth, picked id or integrated normal.
 * Works with mgs_render, strips (the images are full-frame; a strip indexes its own rows), mgs_render_gathered, frame contexts,
 * both sort modes, graph replay on and off.  MGS_SORT_STOCHASTIC with an occluder bound: MGS_ERR_UNSUPPORTED.  Temporal
 * accumulation needs nothing special.  With nothing bound a frame is what it was before ABI 5. */
int  mgs_frame_set_occluder(MgsScene scene_or_context, const float* depth_device, const float* color_device, int width, int height);
/* host convenience: copies into device buffers the handle owns (waits for the handle's frames in flight first), then binds them;
 * NULL depth_host unbinds */
int  mgs_frame_upload_occluder(MgsScene scene_or_context, const float* depth_host, const float* color_host, int width, int height);
/* device bytes held by the committed scene data (shared by all its contexts) and by this handle's working set */
int  mgs_scene_memory_usage(MgsScene scene_or_context, uint64_t* scene_bytes, uint64_t* working_bytes);
/* The device keeps every splat set in a spatially coherent STORAGE ORDER (Morton order of the centres;
 * build-defined, the reference keeps file order).  Every id that crosses this ABI is in the caller's
 * order; this returns the permutation storage index -> caller's index of an instance's splat set.
 * Equal depth keys are drawn in storage order (the reference's tie order is nondeterministic). */
int  mgs_scene_storage_order(MgsScene scene, int instance_id, uint32_t* new_to_old, size_t count);
/* test/debug hook: copy a committed device buffer of a splat set to the host, dequantised to
 * fp32 exactly as the shaders would read it, in the caller's splat order.  which: 0 centres[3n] 1 cov[6n] 2 rgba[4n] 3 sh[stride*n] */
int  mgs_scene_download_set(MgsScene scene, int instance_id, int which, float* dst, size_t count);

/* ---- per-frame parameters: shaderio::FrameInfo (shaders/shaderio.h:238-317) as filled by
 * updateAndUploadFrameInfoUBO (src/gaussian_splatting.cpp:1150-1295) plus the raster knobs of
 * parameters.h:86-201.  focal and basisViewport are derived inside, exactly as :1218-1250. */
typedef struct MgsFrameParams {
  float   view[16];
  float   proj[16];
  float   camera_pos[3];
  int32_t width, height;
  float   splat_scale;          /* default 1.0    shaderio.h:261 */
  float   frustum_dilation;     /* default 0.2    shaderio.h:264 */
  float   alpha_cull_threshold; /* default 1/255  shaderio.h:265 */
  int32_t sh_degree;            /* default 3      shaderio.h:262 */
  int32_t sort_mode;            /* MGS_SORT_*      */
  int32_t frustum_culling;      /* MGS_CULL_*      (forced to AT_RASTER with CPU sort, gaussian_splatting_ui.cpp:1469-1479) */
  int32_t target_format;        /* MGS_TARGET_*    */
  int32_t alpha_mode;           /* MGS_ALPHA_*     */
  int32_t ms_antialiasing;      /* 0/1            threedgs.h.slang:63-76 */
  /* multi-GPU strip partition (no reference counterpart): this device renders
   * 16-pixel tile rows [strip_row_begin, strip_row_end); 0,0 = whole frame */
  int32_t strip_row_begin, strip_row_end;
  int32_t collect_timings;      /* 1: bracket each stage with hipEvents on the render stream and wait for them;
                                   2: record the events but do not wait (query later with mgs_timings_query) */
  int32_t cpu_sort_blocking;    /* CPU_ASYNC only: 1 = wait for the sorter (deterministic tests) */
  int32_t debug_flags;          /* MGS_DEBUG_* bits: the reference's visualisation modes (parameters.h:86-201) */
  int32_t size_culling;         /* 0/1, default 0 (parameters.h:185): drop splats whose projected extent is below ...  */
  float   size_culling_min_pixels; /* ... this many pixels, default 1.0 (shaderio.h:266, dist.comp.slang:93-134)      */
  int32_t surface_outputs;      /* 0/1, default 0: also produce the FTB side outputs of NEED_SURFACE_INFO
                                   (threedgs_raster.frag.slang:320-349; 3DGUT pipeline: threedgut_raster.frag.slang:195-228):
                                   picked depth + the splat that set it + the integrated normal */
  float   depth_iso_threshold;  /* default 0.7 (parameters.h:200): depth = ndc z of the first fragment after which
                                   the pixel's transmittance is below this */
  int32_t cpu_lazy_sort;        /* CPU_ASYNC only, default 1 (parameters.h:183): start a new sort only if the viewpoint changed */
  float   thin_particle_threshold; /* surface_outputs only, default 1e-6 (parameters.h:163): exp(scale) below this makes
                                   an axis degenerate for the splat normal (threedgrt.h.slang:358-419) */
  int32_t quantize_normals;     /* surface_outputs only, default 1 (parameters.h:195): the splat normal passes through
                                   the 2x16-bit octahedral code (octahedral_normal.h.slang) before it is integrated */
  /* ---- 3DGUT raster pipeline (PIPELINE_MESH_3DGUT): unscented-transform projection
   * (threedgut_raster.mesh.slang:111-254, threedgut.h.slang:26-163) + per-pixel particle response
   * (threedgut_raster.frag.slang:87-183, threedgrt.h.slang:57-135,238-278).  Keys, cull, sort and binning are shared. */
  int32_t pipeline;             /* MGS_PIPELINE_3DGS (default) | MGS_PIPELINE_3DGUT */
  int32_t camera_model;         /* 3DGUT: MGS_CAMERA_PINHOLE (default) | MGS_CAMERA_FISHEYE (perfect equidistant fisheye,
                                   threedgut_camera_models.h.slang:120-136; rays cameras.h.slang:46-82) */
  int32_t extent_method;        /* 3DGUT: MGS_EXTENT_CONIC (default, parameters.h:190) | MGS_EXTENT_EIGEN (shaderio.h:96-97) */
  float   fov_rad;              /* 3DGUT fisheye: frameInfo.fovRad (gaussian_splatting.cpp:1168,1243); 0 = derive the vertical
                                   field of view from proj[5] */
  float   alpha_clamp;          /* 3DGUT: default 0.99 (shaderio.h:271) */
  float   kernel_min_response;  /* 3DGUT: default 0.0113 (parameters.h:216) */
  /* ---- stochastic paths (ABI 3).  Random numbers: nvshaders/random.h.slang (xxhash32, pcg, rand) of nvpro_core2, which is
   * not part of the reference tree; restated from the published file (csrc/kernels_common.h). */
  int32_t dof_mode;             /* 3DGUT only: MGS_DOF_* — thin-lens perturbation of each pixel's ray, one sample per frame
                                   (threedgut_raster.frag.slang:104-109, cameras.h.slang:85-108) */
  float   focus_dist;           /* default 1.3   (shaderio.h:278) */
  float   aperture;             /* default 0.001 (shaderio.h:279) */
  int32_t frame_sample_id;      /* frameInfo.frameSampleId (shaderio.h:275): seeds the per-pixel random numbers of DoF and of
                                   MGS_SORT_STOCHASTIC; the caller counts it up while the view stands still
                                   (gaussian_splatting.cpp:3040-3075) */
  int32_t temporal_sampling;    /* 0/1 (post.comp.slang:29-43): the frame handed back is the running mean of the samples
                                   0..frame_sample_id of this scene (sample 0 restarts it: pass 0 whenever the view, the size
                                   or the scene changed, as updateFrameSampleId does); kept in fp32 */
  int32_t kernel_degree;        /* 3DGUT: KERNEL_DEGREE (shaderio.h:112-119, default 2 = quadratic, parameters.h:215): the generalised
                                   Gaussian of particleRayMaxKernelResponse (threedgrt.h.slang:83-127); 0,1,2,3,4,5,8 */
  int32_t normal_method;        /* 3DGUT + surface_outputs: NORMAL_METHOD (shaderio.h:126-128, parameters.h:121-125) — MGS_NORMAL_MAX_DENSITY_PLANE
                                   (default) | MGS_NORMAL_ISO_SURFACE: the fragment's normal is the normal of the kernel ellipsoid
                                   (3 sigma) where the pixel's ray enters it (threedgrt.h.slang:423-497).  The 3DGS pipeline's
                                   mesh shader always uses the max-density plane (threedgs_raster.mesh.slang:219). */
  /* ---- deferred lighting of the splat surface (ABI 5.1; the struct's last word, reserved until then): MGS_LIGHTING_*.  deferred_shading.comp.slang, dispatched
   * by the raster-only pipelines whenever lightingMode != eLightingDisabled (src/gaussian_splatting.cpp:888-908).  A frame with
   * lighting on
   *  - is rendered as if surface_outputs = 1 (needSurfaceInfo, gaussian_splatting.h:169-179) with the caller's depth_iso_threshold,
   *    thin_particle_threshold, quantize_normals and normal_method; the side outputs are downloadable afterwards;
   *  - after the compositor (hence after the occluder's background term) and BEFORE temporal accumulation (the reference shades the
   *    fresh sample and post.comp averages shaded samples) has every pixel of the handle's strip rewritten in place
   *    (deferred_shading.comp.slang:52-167): integrated normal .w < 0.001 -> pixel untouched; else n = normalize(normal.xyz), world
   *    position from (pixel + 0.5) / viewport * 2 - 1, the picked depth (0 where none: followed as written), projInverse and
   *    viewInverse; base colour = the frame's pixel AS STORED in the target format; material = the material of the instance that owns
   *    the picked splat, each colour times the base colour (id 0xFFFFFFFF: diffuse = base colour, ambient 0.1, specular 0, shininess
   *    32, no emission); colour = emission + for each light of the scene's table (the headlight when it is empty)
   *    wavefrontComputeShadingDirectOnly (wavefront.h.slang:104-280,388-403: ambient once PER LIGHT, diffuse by type with range cull,
   *    attenuation mode and spot cone, specular with max(shininess, 4)) if the material needs shading; the pixel becomes
   *    (colour, 1.0) in the target format.
   *  - projInverse / viewInverse: glm::inverse is not part of the reference tree, so the rounding of the inverses is PARITY UNPINNED.
   *    Here both are computed on the host in double and rounded once to fp32.
   *  - the normal attachment is RGBA16F in the reference and fp32 here (see mgs_frame_download_surface, which = 2); the lighting
   *    reads the fp32 one.
   * MGS_SORT_STOCHASTIC with lighting on: MGS_ERR_UNSUPPORTED.  MGS_ALPHA_SUM with lighting: lit pixels get alpha 1.0 as written.
   * Works with strips (a strip lights its own rows; the pass is per pixel), mgs_render_gathered, frame contexts, both pipelines, all
   * targets, both sort modes, graph replay.  Values other than MGS_LIGHTING_*: MGS_ERR_INVALID_ARG.  0 (the default): the frame is
   * what it was before ABI 5.1. */
  int32_t lighting_mode;
} MgsFrameParams;

void mgs_frame_params_default(MgsFrameParams* p); /* fills the defaults cited above */

enum { MGS_STAGE_PROJECT = 0, MGS_STAGE_SORT = 1, MGS_STAGE_BIN = 2, MGS_STAGE_PAIRSORT = 3,
       MGS_STAGE_COMPOSITE = 4, MGS_STAGE_TOTAL = 5,
       MGS_STAGE_CULL = 6, /* the head of MGS_STAGE_PROJECT (included in it): from the frame's upload to the first kernel; the partition
                              cull ran here as a kernel of its own until round 3, it is part of the project kernels now */
       MGS_STAGE_LIGHT = 7, /* the deferred lighting pass (lighting_mode != 0), 0 otherwise; not part of MGS_STAGE_COMPOSITE, part of
                               MGS_STAGE_TOTAL */
       MGS_STAGE_COUNT = 8 };

typedef struct MgsFrameOut {
  void*    rgba_device;     /* device pointer: [height][width][4] fp16 (or fp32), row 0 = NDC y -1, linear */
  uint64_t rgba_bytes;
  uint32_t frustum_count;   /* survivors of the dist-stage cull == IndirectParams.instanceCount (shaderio.h:343-356) */
  uint32_t sorted_count;    /* elements actually sorted (after alpha/extent/off-screen rejection) */
  uint64_t tile_pairs;      /* (tile, splat) records built by the binning stage */
  uint32_t error_flags;     /* device-side diagnostics, 0 = clean.  bit 0: a per-bin list overflowed (mgs_frame_stats returns
                               MGS_ERR_OVERFLOW); bit 1: a bounded look-back wait of the key sort gave up — the sorted order,
                               hence the frame, is invalid (mgs_frame_stats / mgs_sort_keys / mgs_radix_sort_u32 return
                               MGS_ERR_DEVICE; nothing hangs) */
  uint32_t shaded_count;    /* (splat, screen region) pairs staged and shaded by the compositor (deferred SH evaluation) */
  uint64_t scanned_entries; /* bin-list entries the compositor looked at before its regions saturated */
  float    stage_ms[MGS_STAGE_COUNT]; /* valid when collect_timings; HIP-event times on the render stream */
  uint32_t escape_count;    /* sorted splats whose bin rectangle did not fit a code that rides through the key sort (more than 2 x 2
                               bins): the only ones whose rectangle is stored and gathered by id (build-only diagnostic) */
  uint32_t reserved0;
} MgsFrameOut;

/* GaussianSplatting::onRender -> renderHybridPipeline (src/gaussian_splatting.cpp:335,414,494):
 * processSortingOnGPU (:1298-1367) + drawSplatPrimitives (:1369-1465) + blending (:2066-2087).
 * Asynchronous on the scene's stream; counters in `out` are read back when the call returns
 * only if collect_timings or MGS_SYNC_STATS were requested via mgs_frame_stats(). */
int mgs_render(MgsScene scene, const MgsFrameParams* params, MgsFrameOut* out);
/* waits for the last mgs_render and fills counters / timings (readBackIndirectParametersIfNeeded, :1536) */
int mgs_frame_stats(MgsScene scene, MgsFrameOut* out);
/* per-stage HIP-event times of the timed frame rendered `frames_back` frames ago (0 = latest;
 * a ring of 128 timed frames is kept).  Waits only for that frame's last event. */
int mgs_timings_query(MgsScene scene, uint32_t frames_back, float stage_ms[MGS_STAGE_COUNT]);
/* side outputs of the last frame rendered with surface_outputs = 1, [height][width], row 0 = NDC y -1:
 * which 0: picked depth, float32 (0 where the transmittance never fell below the threshold);
 * which 1: global id (caller's order) of the splat that set it, uint32 (0xFFFFFFFF where none);
 * which 2: integrated normal, float32 x 4 per pixel = sum over the fragments (front to back) of
 *          (world normal * opacity, opacity) * transmittance — the RASTER_NORMAL attachment
 *          (gaussian_splatting.cpp:2090-2107, RGBA16F in the reference, fp32 here);
 * which 3: consolidated depth, float32 (depth_consolidate.frag.slang, gaussian_splatting.cpp:807-834,2374-2404): one depth image
 *          for whatever follows the splats — picked > 0.0001 && picked < D ? picked : D, with D the occluder depth bound when the
 *          frame was rendered (1.0, the depth clear, where nothing was bound; compare op LESS, :2383).  Computed when asked for,
 *          from that image's contents at the time of the call (caller-owned images must still be alive).
 * Available after a frame with surface_outputs = 1 or lighting_mode != 0; MGS_ERR_STATE after any other frame. */
int mgs_frame_download_surface(MgsScene scene, int which, void* host_dst, size_t bytes);
/* copy the last frame to the host (screenshot path, gaussian_splatting_ui.cpp:508-540, no tonemap) */
int mgs_frame_download(MgsScene scene, void* host_dst, size_t bytes);
/* copy this device's strip of the last frame into a caller-owned device buffer (all-gather staging) */
int mgs_frame_copy_strip(MgsScene scene, void* device_dst, size_t bytes);
/* ---- multi-GPU strip partition (no reference counterpart: the reference is single-GPU).  One process
 * per GPU, replicated splat buffers; every rank renders its tile rows of the SAME frame with the whole path, and the
 * strips are exchanged with RCCL (one grouped collective per frame on the scene's stream, in place in the frame buffer:
 * no staging copy).  Afterwards every rank's frame buffer holds the complete frame, bit-identical to a single-GPU
 * frame.  librccl is loaded on first use (dlopen); MGS_ERR_UNSUPPORTED when it is absent. */
#define MGS_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank, hand the 128 bytes to every rank out of band (MPI, torch.distributed, a file) */
int mgs_comm_unique_id(void* id_out);
/* ncclCommInitRank on the scene's device (collective: every rank calls it with the same id).  world_size 1 is valid. */
int mgs_scene_comm_init(MgsScene scene, int rank, int world_size, const void* id);
int mgs_scene_comm_destroy(MgsScene scene);
/* tile-row boundaries of all ranks, row_bounds[world_size + 1], ascending, [0] = 0, [world_size] >= tile rows of the
 * frame (16-pixel rows).  NULL restores the default: equal strips of ceil(rows / world_size).  Cost-balanced tables
 * come from mgs_frame_row_costs of earlier frames ("optionally cost-balanced from last frame's D"). */
int mgs_scene_set_strip_rows(MgsScene scene, const int32_t* row_bounds, int count);
/* mgs_render of this rank's strip + the exchange.  params->strip_row_* are ignored (the table decides).  A rank whose strip is
 * empty (equal consecutive bounds, more ranks than tile rows) renders nothing and only receives.  A rank whose own render fails
 * still joins the exchange (its rows are stale) and returns the render's error afterwards, so the peers never block; if it
 * cannot even hold a frame buffer it aborts its communicator, which fails the peers' collective instead of hanging it. */
int mgs_render_gathered(MgsScene scene, const MgsFrameParams* params, MgsFrameOut* out);
/* per 16-pixel tile row of the last full frame: bin-list entries attributed to that row (a bin's entries spread
 * evenly over its tile rows) — the cost proxy the strip balancing uses.  Waits for the frame.  Calibrate on full-frame
 * mgs_render calls: after mgs_render_gathered the lists cover this rank's rows only, every rank would derive a different
 * table and the exchange sizes would disagree — MGS_ERR_STATE. */
int mgs_frame_row_costs(MgsScene scene, uint32_t* cost_per_tile_row, size_t rows);

/* ---- triangle meshes and the mesh pass (MGS_HAS_MESHES): the producer of the occluder images.  Replaces ObjLoader
 * (src/obj_loader.cpp:26-205), the instances of MeshManagerVk (src/mesh_manager_vk.cpp, transformRotScaleInverse at :187), the
 * shaders threedmesh_raster.{vert,frag}.slang and GaussianSplatting::drawMeshPrimitives (src/gaussian_splatting.cpp:1467-1525).
 * Out of scope: textures (the reference's fragment shader samples none), light proxies, wireframe, the hybrid / ray-traced variants
 * (HYBRID_ENABLED), MSAA. */
typedef struct MgsMesh_t* MgsMesh;
typedef struct MgsMeshView {           /* indexed triangles, RUB frame like the splats */
  const float*       positions;        /* [3 * vertex_count] */
  const float*       normals;          /* [3 * vertex_count] or NULL: generated as obj_loader.cpp:95-152 does (faces in index order: the
                                          first face at a vertex sets its normal, each later one replaces it by mix(old, face normal, 0.5)) */
  const uint32_t*    indices;          /* [index_count], index_count % 3 == 0, each < vertex_count */
  const uint32_t*    material_ids;     /* [index_count / 3] or NULL (= 0); ids >= material_count become 0 (obj_loader.cpp:190-196) */
  const MgsMaterial* materials;        /* material_count == 0: the loader's default (ambient .1, diffuse .7, specular 1, shininess 32, :72-81) */
  uint64_t vertex_count, index_count;
  uint32_t material_count;
} MgsMeshView;
/* copies the arrays.  NULL positions / indices, no vertices, index_count % 3 != 0, an index >= vertex_count: MGS_ERR_INVALID_ARG
 * (checked on the host; no device is touched).  2^29 or more triangles: MGS_ERR_UNSUPPORTED. */
int  mgs_mesh_from_arrays(const MgsMeshView* view, MgsMesh* out);
/* Host only.  Reads this SUBSET of Wavefront OBJ: "v x y z", "vn x y z", "f" with corners v, v/t, v//n or v/t/n (1-based; negative
 * indices count back from the last element read so far), triangles and polygons (fan-triangulated from their first corner), "o" and
 * "g" (a new shape, if the current one has faces), "usemtl name", "mtllib file..." (relative to the OBJ; statements newmtl, Ka, Kd,
 * Ks, Ke, Ns; a material starts as all zero with shininess 1; a missing library is ignored and leaves the default material).
 * Every other statement is skipped.  Output as ObjLoader::load emits it: vertices de-indexed, one per face corner, indices 0, 1,
 * 2, ...; a corner without a normal takes the generated normal of its position (as written, :98-151: per shape, faces in order,
 * running mix(., n, 0.5); the arrays persist across shapes); a triangle without usemtl, or with an unknown name, gets material 0.
 * The reference parses with tinyobj, which is not restated here: the subset is build-defined and files outside it (other polygon
 * triangulation, smoothing groups, vertex colours, ...) are PARITY UNPINNED.
 * A file that cannot be opened: MGS_ERR_IO.  A malformed v / vn / f statement, an index out of range, a face with fewer than three
 * corners, no face at all: MGS_ERR_FORMAT. */
int  mgs_mesh_load_obj(const char* path, MgsMesh* out);
int  mgs_mesh_view(MgsMesh mesh, MgsMeshView* out);   /* borrow the arrays (valid until mgs_mesh_destroy); normals and material ids are always set */
void mgs_mesh_destroy(MgsMesh mesh);                  /* instances keep their own reference to the data */
/* Mesh instances belong to the SCENE and are shared by its frame contexts, like the light table: the calls below return
 * MGS_ERR_STATE on a context handle, wait for the frames in flight on all contexts and then rewrite the device table (the rule of
 * mgs_scene_set_lights).  Device copies of vertices, indices and materials are made when a mesh's first instance is added;
 * mgs_scene_commit is not involved and a scene without splats may hold meshes.  At most 256 instances and 2^29 - 1 triangles per
 * scene (build-defined).  The bytes are part of scene_bytes of mgs_scene_memory_usage.
 * transformRotScaleInverse = inverse(mat3(transform)) is computed on the host in double and rounded once to fp32; glm::inverse is
 * not part of the reference tree: PARITY UNPINNED (as for projInverse of the lighting pass). */
int  mgs_mesh_instance_add(MgsScene scene, MgsMesh mesh, const float transform[16], int* mesh_instance_id);
int  mgs_mesh_instance_set_transform(MgsScene scene, int mesh_instance_id, const float transform[16]);
int  mgs_mesh_instance_set_visible(MgsScene scene, int mesh_instance_id, int visible);
typedef struct MgsMeshOut {
  uint64_t triangles_in;          /* triangles of the visible instances */
  uint64_t triangles_rasterised;  /* ... that reached coverage with a non-empty bounding box in the handle's rows and a non-zero area */
  uint64_t fragments;             /* samples covered with depth in [0, 1), summed over all (sub-)triangles: covered pixels plus overdraw */
  float    elapsed_ms;            /* HIP events around the four launches */
  uint32_t flags;                 /* MGS_MESH_WORK_LIST_FULL: the images are exact, the pass was slow (see below) */
} MgsMeshOut;
#define MGS_MESH_WORK_LIST_FULL 1u
/* The mesh pass.  Rasterises all visible mesh instances of the scene for `params` (read: view, proj, camera_pos, width, height,
 * strip_row_begin, strip_row_end, lighting_mode; everything else is ignored) into a depth image [height][width] float32 and a colour
 * image [height][width][4] float32 that the handle owns — the same buffers mgs_frame_upload_occluder fills — and binds them as the
 * handle's occluder exactly as that call does.  Ordered on the handle's stream; does not wait unless `out` is given.  The next
 * mgs_render / mgs_render_gathered on the handle composites the splats over the meshes through the occluder path; the frame graph
 * is not changed.  No mesh instance, or none visible: the cleared images (depth 1.0, colour 0 0 0 0).  With strip rows only those
 * pixel rows are written, bit-identical to the same rows of the full pass.
 *
 * Vertex stage (threedmesh_raster.vert.slang:53-62, fp32, products in the written order): worldPos = M p; clip = P (V worldPos);
 * worldNrm = normalize(transpose(transformRotScaleInverse) n); viewDir = worldPos - origin, origin = the translation of
 * viewInverse (host double, rounded once).
 * Clipping: the depth range is the frame's, clip z in [0, w].  A triangle with a non-finite clip coordinate is dropped.  Triangles
 * are clipped geometrically (Sutherland-Hodgman on the weights of the three vertices, planes in this order) at the near plane
 * z >= 0 and at a guard band |x| <= 256 w, |y| <= 256 w, which keeps window coordinates below 2^21 pixels at the 8192-pixel limit
 * (2^29 in fixed point); the resulting polygon is fan-triangulated from its first vertex and every sub-triangle is snapped and
 * rasterised on its own.  A primitive with a clipped vertex whose w is not positive is dropped (a projection whose z >= 0 half
 * space does not imply w > 0 is not supported).  Fragments with depth outside [0, 1] are dropped (depth clip).  At most two
 * sub-triangles per triangle are held on average (every triangle may cross the near plane); beyond that geometry is dropped and a
 * pass that was asked for `out` returns MGS_ERR_OVERFLOW.
 * Triangles whose bounding box exceeds 8 x 8 pixels are cut into chunks of 16 tiles of 8 x 8 pixels on a device-side work list of
 * 2^20 chunks (environment MGS_MESH_WORK_ITEMS, 1 .. 2^26).  A triangle whose chunks no longer fit is rasterised by a single lane
 * instead: the images are the same bit for bit, the pass is slower, and MgsMeshOut.flags carries MGS_MESH_WORK_LIST_FULL.
 * Coverage: window = (ndc * 0.5 + 0.5) * size in fp32, row 0 = NDC y -1; snapped to 1/256 pixel, round to nearest even; edge
 * functions in 64-bit integers; sample = the pixel centre; top-left rule in the frame's row order: with the triangle oriented so
 * that its interior has positive edge functions, a LEFT edge is one whose interior lies toward larger x, a TOP edge is a horizontal
 * edge whose interior lies toward larger row index; samples exactly on such an edge are covered, on any other edge not.  Both
 * windings are drawn (VK_CULL_MODE_NONE, gaussian_splatting.cpp:2057); zero-area triangles produce nothing.  A shared edge is
 * covered exactly once whatever the order of execution.  Vulkan asks for at least 4 sub-pixel bits and the reference names no
 * device: the sub-pixel precision is PARITY UNPINNED.
 * Depth: fp32 z / w per vertex, interpolated linearly in window space as fma(b2, z2 - z0, fma(b1, z1 - z0, z0)) with b_i =
 * float(edge function i) / float(2 area), each operation rounded once, so that a triangle of constant depth keeps exactly that depth;
 * compare LESS against a clear of 1.0 (:1493) in primitive order (instances in creation order, triangles in index order,
 * sub-triangles in fan order): equal depths keep the earlier primitive.  A fragment at exactly 1.0 fails.  Implemented as a 64-bit
 * unsigned atomic minimum on (depth bits << 32 | primitive << 3 | sub-triangle): the frame is bit-reproducible.
 * Fragment stage (threedmesh_raster.frag.slang:67-103, non-hybrid colour branch), evaluated for the winning fragment only:
 * worldPos, worldNrm (not renormalised), viewDir interpolated with perspective correction from the snapped triangle; the
 * primitive's material; lighting_mode 0: colour = emission + ambient + diffuse; otherwise emission, plus, if the material needs
 * shading, wavefrontComputeShadingDirectOnly for each light of the scene's table (mgs_scene_set_lights), or for the headlight
 * when it is empty — the function the lighting pass calls.  Colour alpha is 1 on mesh pixels, 0 elsewhere; fp32 (the occluder
 * path converts after the background term).
 * With the splats: the reference's back-to-front order (meshes first, splats blended over them, :836-843) and its front-to-back
 * order (depth pre-pass, splats, mesh colour times the remaining transmittance, :697-805) both reduce to the composition
 * documented at mgs_frame_set_occluder.  mgs_frame_download_surface(which = 3) then consolidates against the mesh depth. */
int  mgs_meshes_render(MgsScene scene_or_context, const MgsFrameParams* params, MgsMeshOut* out /* may be NULL */);
/* the last pass's images, [height][width] of that pass; waits.  which 0: depth float32; 1: colour float32 x 4; 2: primitive id
 * uint32 (global: instances concatenated in creation order, visible or not; 0xFFFFFFFF = none).  MGS_ERR_STATE before any pass.
 * (The depth and colour images are the handle's owned occluder buffers: a later mgs_frame_upload_occluder overwrites them.) */
int  mgs_meshes_download(MgsScene scene_or_context, int which, void* host_dst, size_t bytes);

/* ---- ray-traced splats (MGS_HAS_TRACE): primary rays of the reference's PIPELINE_RTX, the 3DGRT ray tracer, without fixed-function
 * hardware.  Replaces GaussianSplatting::raytrace with shaders/threedgrt_raytrace.{rgen,rahit,rint}.slang (primary rays), the
 * particle proxies of particle_as_build.comp.slang and the acceleration-structure managers: a hierarchy over the particles built on
 * the device, and a per-ray traversal that collects the samples_per_pass nearest hits per pass as the any-hit shader does.
 * Direct lighting with hard or soft shadow rays through the particles is mgs_render_traced_lit (MGS_HAS_TRACE_LIGHTING, below).
 * A rasterised primary surface under the same light pass is mgs_render_hybrid (MGS_HAS_HYBRID, below).
 * Rays of the caller's own (other sensors, probes, picking, secondary rays shot from the caller's geometry) are mgs_trace_rays
 * (MGS_HAS_RAY_QUERY, below): the caller cuts a ray at its own surfaces with the ray's window, as the occluder does for the raster pipelines.
 * Out of scope: meshes in the traced scene, soft shadows, indirect lighting and bounces, wireframe, visualisation modes other than final, DLSS, mgs_render_gathered for traced frames (strip rows are honoured, the exchange
 * is not wired), trace profile feedback.
 *
 * Ray (threedgrt_raytrace.rgen.slang:159-196): pinhole = generatePinholeRay at the pixel centre (subPixelOffset 0.5,
 * cameras.h.slang:27-44); fisheye = generateFisheyeRay of the pixel's integer coordinate, as written (:46-82), a pixel outside the
 * field of view is written as (0,0,0,1); depth of field as depthOfField (:85-105) seeded with xxhash32(pixel, frame_sample_id)
 * (rgen:193).  viewInverse and projInverse are computed on the host in double and rounded once (the lighting pass's rule; glm::inverse
 * is not part of the reference tree: PARITY UNPINNED).  tMin = 0.001, tMax = 10000, epsT = 1e-9 (rgen:157,247-248).
 * A hit of particle i on a ray: t_i = -dot(o,d)/dot(d,d) in the particle's canonical frame with the UNNORMALISED direction
 * (particleDensityHitInstance, rint.slang:166-168; the reference's default is instances on), i.e. the world ray's parameter of the
 * point of maximum response.  It exists for a pass when TMin < t_i < TMax and the response along the ray exceeds the response the
 * reference circumscribes its proxy around (kernelScale, particle_as_build.comp.slang:74-87): min(kernel_min_response / density,
 * 0.97) with kernel_adaptive_clamping, min(kernel_min_response, 0.97) without.  How far the reference's icosahedron or hardware box
 * reaches beyond that ellipsoid, the entry-point t it reports in icosahedron mode and its traversal's tie order are PARITY UNPINNED;
 * here ties in t resolve by ascending global id (caller's order).  It is ACCEPTED when particleProcessHit accepts it
 * (threedgrt.h.slang:166-185: density > alpha_cull_threshold, alpha = min(alpha_clamp, response * density) > alpha_cull_threshold,
 * response > kernel_min_response).  Model-space ray of a hit: origin through transformInverse, direction through
 * transformRotScaleInverse (normalised; the host-double inverse of the mesh instances) (rgen:697-698); the SH direction is
 * normalize(position - modelRayOrigin) (threedgrt.h.slang:193).
 * Passes, as written (traceRayParticlesInsertionSort, rgen:615-819; insertion rahit.slang:152-167): each pass collects the
 * samples_per_pass nearest hits with t in (tMin + epsT, tMax + epsT), walks them in order while the transmittance exceeds
 * min_transmittance, sets tMin = max(tMin, t) after every walked slot, accepted or not, and the loop ends when a pass finds nothing,
 * after max_passes, or when the transmittance test fails.  A hit that ties with the last slot, or lies within epsT of the last walked
 * one, is therefore lost, here as there.  Integration as particleIntegrate (threedgrt.h.slang:226-235) with the transmittance in double.
 * The frame's alpha is 1 - T, this library's MGS_ALPHA_COVERAGE meaning; the reference writes 1.0.
 * kernel_min_response must be > 0 (at 0 the proxy is unbounded): MGS_ERR_INVALID_ARG.
 *
 * Trace strategies (MGS_HAS_TRACE_STRATEGIES; RTX_TRACE_STRATEGY_*, shaderio.h:122-124, parameters.h:219).  The above is
 * MGS_TRACE_STRATEGY_FULL_ANYHIT, the default.  The other two trade noise for speed and converge under temporal accumulation
 * (frame_sample_id = 0, 1, ... with temporal_sampling = 1; the reference switches its automatic temporal sampling on for them,
 * gaussian_splatting.cpp:311-316).  They share with strategy 0: the ray and its lens (whose draws come from their own seed, rgen:193,
 * and do not advance the strategies' seedRayPass = xxhash32(pixel, frame_sample_id), rgen:228), tMin / tMax / epsT, what a hit is and
 * when it is accepted, radiance and normals, debug flags, strips, contexts, target formats, the surface outputs, the hit counts and the
 * hierarchy (a change of trace_strategy does not rebuild it).  A particle's id that enters a hash is its global id in the CALLER's order.
 *   MGS_TRACE_STRATEGY_PASS_STOCHASTIC (rgen:615-819 with kStochasticPass): the passes of strategy 0, unchanged; the pixel state
 *     (radiance, transmittance, hit count, normal, pick) is snapshot before a pass's walk (:669-673).  After the walk of a pass that found
 *     a hit: opacity = float(1 - T); if rand(seedRayPass) < opacity the radiance is divided by opacity, a pixel without an iso-surface
 *     pick takes the last payload slot that was valid and walked while the transmittance test held, accepted or not (lastValidHitIdx,
 *     :684-687, :772-790), T = 0 (the frame's alpha is 1) and tracing ends; otherwise the pixel returns to the snapshot (tMin does
 *     not) and the next pass follows (:765-801).  A ray whose passes are all rejected is an untouched pixel: (0,0,0,0), hit count 0,
 *     nothing picked.  max_passes_used and accepted_hits keep their meaning (the sum of the hit counts as written to the pixels).
 *   MGS_TRACE_STRATEGY_STOCHASTIC_ANYHIT (rahit.slang:94-150, rgen:823-961, PARTICLES_SPP forced to 1, gaussian_splatting.cpp:1693):
 *     ONE traversal of (tMin + epsT, tMax + epsT) and one payload slot, initially (inf, none).  Every hit with t < slot.t is evaluated
 *     by particleProcessHit; an accepted one draws u = rand(xxhash32(rngSeed, id ^ floatBits(t), 0)) with rngSeed = xxhash32(pixel,
 *     frame_sample_id) (rand consumes the hashed value as its state, rahit:131-133) and becomes the slot when u < alpha.  With one
 *     slot the IgnoreHit rule of rahit:147-150 cannot lose a hit that would have won, and a hit's draw depends on nothing but the
 *     pixel, the sample, the particle and t: the result is the NEAREST KEPT HIT, whatever the order of traversal (which may therefore
 *     cut subtrees beyond slot.t).  Two kept hits with bit-identical t resolve to the lower id in the caller's order; the reference
 *     keeps whichever its traversal met first: PARITY UNPINNED.  The t whose bits are hashed is this library's t of the point of
 *     maximum response; the reference hashes RayTCurrent() of its hardware intersection: PARITY UNPINNED (another random stream of the
 *     same distribution).  Pixel (rgen:951-960): with a kept hit rgb = its radiance, alpha = 1, hit count 1, the pick is that hit
 *     (id; ndc z of origin + t * direction), the normal is the normalised sample normal (0 if its length is 0) with w = 1; without
 *     one (0,0,0,0), hit count 0, nothing picked, normal 0.  samples_per_pass, max_passes, min_transmittance and depth_iso_threshold
 *     are range-checked but NOT READ; max_passes_used is 1 wherever a ray was traced.
 * As in every unlit traced frame surfaceFinalFiltering is not applied (it belongs to the lit path).  Any other value of trace_strategy is
 * MGS_ERR_INVALID_ARG.  mgs_render_traced_lit and mgs_render_hybrid take trace_strategy 0 only and return MGS_ERR_UNSUPPORTED
 * otherwise (before the handle is looked at): the reference also randomises the shadow rays under the any-hit strategy
 * (rgen:1364-1400), which is later work. */
typedef enum MgsTraceStrategy {
  MGS_TRACE_STRATEGY_FULL_ANYHIT       = 0, /* RTX_TRACE_STRATEGY_FULL_ANYHIT: sorted passes until the transmittance is used up (default) */
  MGS_TRACE_STRATEGY_PASS_STOCHASTIC   = 1, /* RTX_TRACE_STRATEGY_PASS_STOCHASTIC: Russian roulette on every pass's opacity */
  MGS_TRACE_STRATEGY_STOCHASTIC_ANYHIT = 2  /* RTX_TRACE_STRATEGY_STOCHASTIC_ANYHIT: one traversal, the nearest hit kept with probability alpha */
} MgsTraceStrategy;
typedef struct MgsTraceParams {
  int32_t samples_per_pass;          /* PARTICLES_SPP, default 18 (parameters.h:218); 1..32 */
  int32_t max_passes;                /* frameInfo.maxPasses, default 200 (shaderio.h:269); >= 1 */
  float   min_transmittance;         /* default 0.01 (shaderio.h:272); [0, 1) */
  int32_t kernel_adaptive_clamping;  /* default 1 (parameters.h:217); 0 / 1 */
  float   depth_iso_threshold;       /* depthIsoThresholdRTX, default 0.7 (parameters.h:226); replaces MgsFrameParams::depth_iso_threshold */
  int32_t trace_strategy;            /* MGS_TRACE_STRATEGY_*, default MGS_TRACE_STRATEGY_FULL_ANYHIT (parameters.h:219) */
  uint32_t reserved[2];
} MgsTraceParams;
void mgs_trace_params_default(MgsTraceParams* p);
typedef struct MgsTraceOut {
  uint64_t leaves, nodes;            /* of the scene's hierarchy: particles with a leaf, nodes of all levels (leaves included) */
  uint64_t node_visits;              /* nodes whose box was tested when taken from a ray's stack, summed over rays and passes */
  uint64_t candidate_tests;          /* particles evaluated against a ray */
  uint64_t accepted_hits;            /* sum of pixel.hitCount */
  uint32_t max_passes_used;          /* the most passes any ray started */
  uint32_t bvh_rebuilt;              /* 1: this call rebuilt the hierarchy */
  float    build_ms, trace_ms;       /* HIP events around the build's launches (0 when not rebuilt) and around the traversal */
} MgsTraceOut;
/* One traced frame into the handle's frame buffer.  Reads of MgsFrameParams: view, proj, camera_pos, width, height, strip_row_begin,
 * strip_row_end, sh_degree, alpha_cull_threshold, target_format, camera_model, fov_rad, kernel_degree, kernel_min_response,
 * alpha_clamp, dof_mode, focus_dist, aperture, frame_sample_id, temporal_sampling, surface_outputs, normal_method,
 * thin_particle_threshold, debug_flags (MGS_DEBUG_SH_ONLY and MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED only); the rest is ignored, except:
 * lighting_mode != 0, sort_mode == MGS_SORT_STOCHASTIC and a bound occluder each return MGS_ERR_UNSUPPORTED.  The ranges of both
 * structs are checked before the handle is looked at.  `trace` NULL = the defaults; `out` non-NULL waits for the frame.
 * Afterwards mgs_frame_download, mgs_frame_copy_strip, the image-compare entry points and temporal accumulation work as after
 * mgs_render.  With surface_outputs = 1, mgs_frame_download_surface returns
 *   which 0: ndc z of primaryHitPos = origin + t * direction of the first accepted hit after which the transmittance is below
 *            depth_iso_threshold, as writeToGBuffers writes the depth buffer (rgen:1490-1502); 0 where nothing was picked — this
 *            library's "none" value, NOT the reference's 1.0;
 *   which 1: that particle's global id in the caller's order (0xFFFFFFFF where none);
 *   which 2: integratedNormal in xyz (sum of normalWorld * weight, rgen:725; normal_method as computeEllipsoidNormalMaxDensityPlane /
 *            computeEllipsoidNormal, threedgrt.h.slang:358-496, to world space by the inverse transpose, :218) and the sum of weight.x in w.
 * The hierarchy (an implicit complete 8-ary tree over leaves in Morton order) covers all instances' particles in world
 * space, belongs to the scene and is shared by its frame contexts.  It is rebuilt lazily by the next traced frame after
 * mgs_scene_commit, mgs_instance_add, mgs_instance_set_transform, or a change of kernel_degree, kernel_min_response,
 * kernel_adaptive_clamping or alpha_cull_threshold; a rebuild first waits for the frames in flight on all contexts (the rule of
 * mgs_scene_set_lights).  Its bytes are part of scene_bytes of mgs_scene_memory_usage.  A leaf bound contains the exact box of the affine
 * image of the proxy ellipsoid and exceeds it by no more than 2^-19 of (half extent + the sum of the absolute terms of the centre's
 * transform) per face (mgs_debug_download_hierarchy shows it); particles with density <=
 * alpha_cull_threshold or a non-finite bound get no leaf and are never hit.  A scene without instances (committed or not) yields the
 * frame (0,0,0) with alpha 0. */
int mgs_render_traced(MgsScene scene_or_context, const MgsFrameParams* params, const MgsTraceParams* trace /* NULL = defaults */,
                      MgsTraceOut* out /* may be NULL */);
/* pixel.hitCount of the last traced frame of this handle, [height][width] uint32 (rows outside a strip frame's rows are stale); waits */
int mgs_trace_download_hit_counts(MgsScene scene_or_context, uint32_t* host_dst, size_t count);

/* ---- lit traced frames (MGS_HAS_TRACE_LIGHTING): the traced frame's splat surface under the scene's lights and the instances'
 * materials (mgs_scene_set_lights, mgs_instance_set_material), each light shadowed by one more ray through the same particle
 * hierarchy.  Replaces surfaceFinalFiltering, evaluateLightingAndShadingParticles, traceShadowRayForLight and
 * traceShadowRayParticle of shaders/threedgrt_raytrace.rgen.slang (:991-1009, :1082-1144, :1262-1292, :1344-1464) with
 * computeLightToSurfaceVector and wavefrontComputeShadingDirectOnly (shaders/wavefront.h.slang:33-70, :233-280).  No mesh is in the
 * traced scene, so every mesh branch of those functions is its meshCount == 0 branch.
 * Primary rays: exactly mgs_render_traced with surface outputs on (NEED_SURFACE_INFO is 1 whenever lighting is on).
 * surfaceFinalFiltering (:991-1009): an integrated normal of length <= 0.2 is replaced by -rayDirection; a pixel without an
 * iso-surface hit is discarded (discardSplatContribution :468-491: radiance 0, transmittance 1), here rgb 0 and alpha 0; otherwise
 * the normal is normalised.  A fisheye pixel outside the field of view stays (0,0,0,1).
 * Shading (:1082-1144): the material is the picked hit's instance's.  radiance restarts at radiance * emission, and that alone is the
 * pixel when the material's needShading is 0 (the default material).  ambient, diffuse and specular are the pixel's fp32 radiance
 * (the accumulator of the primary walk, not the pixel as stored in an RGBA16F / RGBA8 target) times the material's.  Position =
 * origin + t_iso * direction, the view direction is the ray's.  Per light computeLightToSurfaceVector: directional lightDist = 1e10;
 * a point or spot light farther away than its range is SKIPPED ENTIRELY and adds no ambient term — unlike the deferred raster pass
 * (lighting_mode of mgs_render), whose shading adds the ambient term once per light, in range or not.  With no lights: a headlight
 * at camera_pos, never shadowed.  A surface point that coincides with a point or spot light has no light direction (0 / 0): the
 * pixel is NaN, there as here.
 * Shadow ray (hard shadows, :1344-1464): origin = position + lightDir * particle_shadow_offset, TMin 0.0, TMax lightDist - 0.001, no
 * epsT.  ONE collection of the samples_per_pass nearest hits through the same proxies with the tie rule of the primary rays; there
 * is no second pass, so occluders beyond the samples_per_pass-th are not seen, there as here.  The slots are walked in order, slots
 * with t >= lightDist skipped, particleProcessHit / particleIntegrate with the transmittance in double; after each slot a
 * transmittance below particle_shadow_transmittance_threshold becomes 0 and ends the walk.  Then (:1453-1460) T = saturate(T),
 * scaledT = saturate((T - threshold) / (1 - threshold)), normalizedColor = shadowRadiance / max component (1 when that is <= 0.001),
 * transmittance = saturate(scaledT * lerp(1, normalizedColor, particle_shadow_color_strength * (1 - scaledT))).  light.color is
 * multiplied by it; inShadow = its max component < 0.001 (:1126-1127) returns from the shading after the ambient term.
 * Alpha stays 1 - T of the primary walk (the reference writes 1.0).
 * Soft shadows (MGS_SHADOWS_SOFT, MGS_HAS_SOFT_SHADOWS; SHADOWS_MODE == SHADOWS_SOFT, shaderio.h:141-143) are opt-in per process: the
 * environment switch MGS_SOFT_SHADOWS=1, read once when the library first looks at its switches.  The switch is TEMPORARY: it exists because callers of ABI 5.1 were promised
 * MGS_ERR_UNSUPPORTED for this mode; the next ABI minor drops it and accepts the mode unconditionally.  Without it MGS_SHADOWS_SOFT is
 * MGS_ERR_UNSUPPORTED at the range checks, the answer every earlier build of ABI 5.1 gave.  With it: computeLightToSurfaceVector
 * with buildOrthonormalBasis and sampleDisk (shaders/wavefront.h.slang:33-102).  ONE sample per light and frame; a soft frame
 * converges over frame_sample_ids by temporal accumulation, as depth of field does (the reference turns it on for soft shadows,
 * gaussian_splatting.cpp:313).
 *   Seed: one uint32 state per pixel, seedRayPass = xxhash32(px, py, frame_sample_id) (rgen.slang:228) with the ABSOLUTE pixel
 *   coordinates, so a strip frame draws what the full frame draws.  The depth-of-field lens seeds its own copy (:193) and does not
 *   advance this state; trace strategy 0 draws nothing from it before the lighting.  xxhash32 / pcg / rand are the restated ones
 *   of the stochastic strategies (PARITY UNPINNED as they are: nvshaders/random.h.slang is not in the reference tree).
 *   Per light, in table order, BEFORE the range test: a point or spot light with radius > 0 (mgs_scene_set_light_radii) draws two
 *   numbers.  n = normalize(light.position - position); tangent, bitangent = Frisvad's basis of n (:78-92: for n.z < -0.9999999
 *   (0,-1,0) and (-1,0,0), else a = 1 / (1 + n.z), b = -n.x n.y a, (1 - n.x n.x a, b, -n.x), (b, 1 - n.y n.y a, -n.y));
 *   r = (radius * 0.5) * sqrt(rand(seed)) FIRST, then theta = 2 * 3.14159265 * rand(seed) (:97-101);
 *   samplePos = light.position + r * (cos(theta) * tangent + sin(theta) * bitangent); lightDist = |samplePos - position|; the
 *   light is SKIPPED when lightDist > range (the sample's distance decides, not the centre's; the two numbers are consumed anyway);
 *   lightDir = normalize(samplePos - position).  A directional light, or a radius <= 0, draws nothing and is exactly the hard path.
 *   Shadow rays: both take the sample's lightDir and lightDist — the mesh occlusion ray of a frame with trace meshes from the
 *   un-offset position over (0.001, lightDist - 0.001), the particle ray from position + lightDir * particle_shadow_offset with
 *   TMax = lightDist - 0.001.  Shading is unchanged: computePointLight and computeSpotLight read light.position, not the sample;
 *   the light's colour is multiplied by the sample's transmittance.  The headlight is never shadowed and draws nothing.
 *   A lit frame with trace meshes can run the loop over the lights twice on one pixel, for the splat surface and then for the mesh
 *   hit (:1054, :1061, the same inout seed): the mesh shading's draws continue where the splat surface's ended, and start from the
 *   fresh seed where that loop did not run (no pick, the splat surface behind the mesh, or the picked instance's needShading 0:
 *   :1091-1095 returns before the loop).  No per-pixel word is carried for this: the first loop draws two numbers per light with a
 *   disk whether the light is culled or not, so the mesh composite recomputes its end state from the light table and the light
 *   pass's own conditions.  A hybrid frame has the same seed (:228) and one loop per pixel.
 *   MgsTraceLightOut keeps its meaning: shadow_rays counts the rays traced.  Hard shadows, shadows off and every other entry point
 *   keep their frames bit for bit.  Not built: several samples per light in one frame; soft shadows in mgs_render_traced_indirect
 *   (the state would have to be carried across the bounce launches) and in mgs_trace_shadow_rays / mgs_shade_points (a query point
 *   has no pixel to seed from), which return MGS_ERR_UNSUPPORTED. */
#define MGS_SHADOWS_DISABLED 0 /* default (parameters.h:167) */
#define MGS_SHADOWS_HARD 1
#define MGS_SHADOWS_SOFT 2     /* mgs_render_traced_lit and mgs_render_hybrid under MGS_SOFT_SHADOWS=1; otherwise and elsewhere MGS_ERR_UNSUPPORTED */
typedef struct MgsTraceLightParams {
  int32_t  shadows_mode;                            /* MGS_SHADOWS_*, default MGS_SHADOWS_DISABLED */
  float    particle_shadow_offset;                  /* default 0.2 (parameters.h:222); finite, >= 0 */
  float    particle_shadow_transmittance_threshold; /* default 0.8 (parameters.h:223); [0, 1): at 1 the ramp divides by zero */
  float    particle_shadow_color_strength;          /* default 0.0 (parameters.h:224); [0, 1] */
  uint32_t reserved[4];
} MgsTraceLightParams;
void mgs_trace_light_params_default(MgsTraceLightParams* p);
typedef struct MgsTraceLightOut {
  uint64_t shadow_rays;            /* shadow rays traced: pixels with a surface and a shaded material x lights in range (0 with shadows off) */
  uint64_t shadow_node_visits;     /* as MgsTraceOut::node_visits, of the shadow rays */
  uint64_t shadow_candidate_tests; /* particles evaluated against a shadow ray's window */
  uint64_t shadow_accepted_hits;   /* hits the shadow walks accepted */
  float    light_ms;               /* HIP events around the light pass */
  uint32_t reserved;
} MgsTraceLightOut;
/* One lit traced frame into the handle's frame buffer.  Reads everything mgs_render_traced reads, plus lighting_mode, which must be
 * MGS_LIGHTING_DIRECT: MGS_LIGHTING_INDIRECT needs bounces (mgs_render_traced_indirect) and returns MGS_ERR_UNSUPPORTED here, MGS_LIGHTING_DISABLED or any other value
 * MGS_ERR_INVALID_ARG.  The ranges of the three structs are checked before the handle is looked at.  `trace` / `light` NULL = the
 * defaults; `out` or `light_out` non-NULL waits for the frame.  Afterwards mgs_frame_download, mgs_frame_copy_strip,
 * mgs_frame_download_surface (always: lighting turns the surface outputs on), mgs_trace_download_hit_counts, the image-compare entry
 * points, temporal accumulation, strip rows and frame contexts work as after mgs_render_traced.  Lights and materials keep their
 * rules: one table per scene, rewritten after waiting for the frames in flight; neither rebuilds the hierarchy.  The light pass's
 * per-pixel scratch (ray parameter, fp32 radiance, shadow hits) belongs to the handle and counts into working_bytes. */
int mgs_render_traced_lit(MgsScene scene_or_context, const MgsFrameParams* params, const MgsTraceParams* trace /* NULL = defaults */,
                          const MgsTraceLightParams* light /* NULL = defaults */, MgsTraceOut* out /* may be NULL */,
                          MgsTraceLightOut* light_out /* may be NULL */);
/* shadow hits accepted for the pixel, summed over the lights, of the last lit traced frame of this handle: [height][width] uint32
 * (rows outside a strip frame's rows are stale); waits.  MGS_ERR_STATE unless the handle's last traced frame was a lit one. */
int mgs_trace_download_shadow_hits(MgsScene scene_or_context, uint32_t* host_dst, size_t count);

/* ---- hybrid frames (MGS_HAS_HYBRID): the rasterised splat surface lit with traced shadow rays — the reference's PIPELINE_HYBRID
 * (params->pipeline = MGS_PIPELINE_3DGS) and PIPELINE_HYBRID_3DGUT (MGS_PIPELINE_3DGUT) without meshes
 * (doc/hybrid_rendering_3d_gaussians.md, doc/lighting_and_shadows.md section 5).  The raster pass supplies radiance, picked depth, picked
 * id and integrated normal "in place of first-bounce ray tracing"; everything after that is the ray tracer's.  Three steps:
 * 1. Primary surface: exactly the frame mgs_render makes from *params with lighting_mode = 0 and surface_outputs = 1 (the deferred
 *    shading pass is off in hybrid mode, NEED_SURFACE_INFO is on).  depth_iso_threshold is MgsFrameParams'; `out` is filled as
 *    mgs_render fills it.  MgsTraceParams::depth_iso_threshold and max_passes are NOT READ (there is no primary walk), not even
 *    range-checked.
 * 2. Hand-over (initRtxStateFromRasterPass, shaders/threedgrt_raytrace.rgen.slang:346-460), per pixel of the handle's strip rows:
 *    radiance = the frame's pixel as stored in its target format (what the reference and the deferred pass read), alpha = that
 *    pixel's alpha, kept in the output (1 - T, this library's convention; the reference writes 1.0).  validDepth = picked ndc depth
 *    > 0.0001.  Pinhole: position = the unprojection of (pixel centre, picked depth) through the host-double inverses of proj and
 *    view, rounded once (the deferred pass's reconstructWorldPos, operation for operation), ray parameter = length(position - ray
 *    origin).  Fisheye (3DGUT only, :402-419): view z of the picked depth through the inverse projection, ray parameter = view z /
 *    (view-space ray direction).z.  The ray is the traced pipeline's (mgs_render_traced, "Ray"), depth of field included for 3DGUT;
 *    the reference's 3DGS hybrid skips the lens (rgen:191), so MGS_PIPELINE_3DGS with dof_mode != 0 is MGS_ERR_UNSUPPORTED
 *    (mgs_render's code) and with a fisheye camera MGS_ERR_INVALID_ARG.  normal = normalize(normal.xyz) when normal.w > 0.001,
 *    else 0; the pixel is DISCARDED when !validDepth or length(normal) < 0.001: rgb 0 and alpha 0 (this library's convention for a
 *    discarded lit pixel; the reference writes (0,0,0,1)).  The traced path's "length <= 0.2 -> -rayDirection" fallback is NOT part
 *    of hybrid: surfaceFinalFiltering is only called from the particle trace, which hybrid skips at bounce 0.  A pixel with a valid
 *    depth and normal whose picked id is 0xFFFFFFFF keeps its raster colour unlit (splatIsClosest && isoSurfSplatSetId != INVALID
 *    fails, :1047-1049), as does a fisheye pixel outside the field of view.  A ray parameter that is not > 0 discards the pixel.
 * 3. Shading and shadows: exactly what mgs_render_traced_lit documents for one pixel — material of the picked id's instance,
 *    emission, the range rule without the ambient term, headlight with no lights, one samples_per_pass collection per light through
 *    the scene's hierarchy, the transmittance ramp and the tint — at position = ray origin + ray parameter * ray direction, which
 *    is also where the shadow ray starts (the reference shades at the unprojected position, :1110).
 * Temporal accumulation runs after the light pass.  The hierarchy is the scene's, built lazily under mgs_render_traced's rules and
 * shared with traced frames; its proxy is kernel_degree, kernel_min_response, alpha_cull_threshold of `params` and
 * kernel_adaptive_clamping of `trace`, whichever raster pipeline runs (kernel_min_response must be > 0).  Afterwards
 * mgs_frame_download, mgs_frame_copy_strip, the image-compare entry points and mgs_trace_download_shadow_hits work as after a lit
 * traced frame (mgs_trace_download_hit_counts: MGS_ERR_STATE, there is no primary walk); mgs_frame_download_surface returns the
 * raster pass's outputs untouched.  Strip rows and frame contexts work; mgs_render_gathered is not wired.  The normalised normal is
 * a 16 B / pixel scratch of the handle and counts into working_bytes.
 * The ranges of the three structs are checked before the handle is looked at.  lighting_mode == MGS_LIGHTING_INDIRECT:
 * MGS_ERR_UNSUPPORTED; 0 or any other value: MGS_ERR_INVALID_ARG (a hybrid frame without lighting is mgs_render's);
 * MGS_SORT_STOCHASTIC and a bound occluder (shadowing mesh pixels needs meshes in the traced scene): MGS_ERR_UNSUPPORTED.
 * MGS_SHADOWS_SOFT is the lit traced frame's, with the same seed (rgen.slang:228 runs in hybrid too) and one loop per pixel at the
 * handed-over position.
 * `trace` / `light` NULL = the defaults; `light_out` non-NULL waits for the frame. */
int mgs_render_hybrid(MgsScene scene_or_context, const MgsFrameParams* params, const MgsTraceParams* trace /* NULL = defaults */,
                      const MgsTraceLightParams* light /* NULL = defaults */, MgsFrameOut* out /* may be NULL */,
                      MgsTraceLightOut* light_out /* may be NULL */);

/* ---- sensor models (MGS_HAS_SENSOR_MODEL): the 3DGUT raster pipeline through a calibrated camera.  The unscented transform pushes a
 * particle's sigma points through a non-linear camera; the reference carries the OpenCV pinhole model (radial, tangential and
 * thin-prism distortion) and the OpenCV fisheye polynomial in full (CameraModelParameters, shaders/threedgut_camera_models.h.slang:25-61;
 * projectPointPinhole, projectPointFisheye, shaders/threedgut_camera_projections.h.slang:85-186) but its application only ever fills in
 * the perfect models (initPerfectPinholeCamera / initPerfectFisheyeCamera, threedgut_camera_models.h.slang:66-138).  A bound
 * MgsSensorModel fills in the rest.
 *
 * Projection of a sigma point: projectPointWithShutter with the global shutter (threedgut_camera_projections.h.slang:189-205) and
 *   pinhole (:85-136): uv = xy / z; icD = (1 + r2 (k1 + r2 (k2 + r2 k3))) / (1 + r2 (k4 + r2 (k5 + r2 k6))); delta from tangential[2] and
 *     thin_prism[4] (:109-112); p = (icD uv + delta) * focal_length + principal_point where icD lies in (0.8, 1.2) (:118-124), else the
 *     point is invalid and clipped to length(resolution) / sqrt(r2) * uv + principal_point (:125-133); z <= 0: invalid, (0, 0) (:88-92);
 *   fisheye (:149-171): theta = min(atan2(|xy|, z), max_angle) (:152-160), p = focal_length * xy * theta (1 + poly(theta^2) theta^2) / |xy|
 *     + principal_point with evalPolyHorner4 (:51-59, :163-165); theta >= max_angle: invalid;
 *   both: valid only withinResolution with the 0.1 margin (:78-83, GUT_IN_IMAGE_MARGIN_FACTOR).
 * Everything downstream of the seven projected points is the frame's as before: centroid, covariance, extents, the quad's depth from
 * `proj`, bin rectangle, canonical frame.  max_angle = 0 asks for computeMaxAngle of the viewport, the principal point and the focal
 * length (threedgut_camera_models.h.slang:87-119).  shutter: 0 = global; any rolling type is MGS_ERR_UNSUPPORTED (the reference marks
 * that code untested, threedgut_camera_projections.h.slang:207-210).  applyRenderingResolution (:138-147) is not applied, as in the
 * reference (:167-168).
 *
 * Ray of pixel (x, y).  PARITY UNPINNED: the reference has no inverse of these models (its fragment shader generates the perfect
 * pinhole / equidistant ray, threedgut_raster.frag.slang:101-111), so the inverse is defined by this library.  The ray is the
 * camera-space direction whose projection is the image point (x + 0.5, y + 0.5) — the pixel centre the front end's quad placement
 * assumes —, rotated to world space by viewInverse and normalised.  This convention is self-consistent: projecting a pixel's ray
 * lands on the pixel's centre.  (Without a sensor the pinhole ray keeps the reference's second 0.5, and the fisheye ray its
 * resolution - 1.)  Pinhole: Newton on the 2x2 Jacobian of the forward map uv -> icD uv + delta from (p - c) / f; fisheye: Newton on
 * theta (1 + poly(theta^2) theta^2) = |(p - c) / f| from that radius.  Both run 8 iterations in fp32.  A pixel has NO ray where the
 * iteration ends outside the model's validity (icD outside (0.8, 1.2); theta >= max_angle), where it misses the image point by more
 * than 0.01 pixel (no convergence), or where the forward map is not monotone at the result (Jacobian determinant / derivative <= 0).
 * Such a pixel is what a fisheye pixel outside the field of view is without a sensor: no fragment, transparent black (opaque black
 * under MGS_SORT_STOCHASTIC), no side output.
 *
 * mgs_sensor_model_from_frame fills *out with the perfect model the frame *p uses without a sensor: `model` from camera_model, the
 * focal length of the 3DGUT front end ((proj[0] width / 2, proj[5] height / 2); fisheye: (width, -height) / fov_rad,
 * src/gaussian_splatting.cpp:1239-1251 — focal_length[1] follows the sign of proj[5]), the principal point at the viewport's centre,
 * zero coefficients and max_angle = computeMaxAngle.  Callers start from it and perturb.
 *
 * mgs_frame_set_sensor binds a copy of *sensor to the handle (a scene or a frame context; each has its own, as the occluder), NULL
 * unbinds.  Ranges are checked before the handle is looked at: model and shutter in range, every value finite, focal_length non-zero,
 * max_angle >= 0, reserved words 0 (MGS_ERR_INVALID_ARG); a rolling shutter: MGS_ERR_UNSUPPORTED.  While a sensor is bound it
 * replaces camera_model and fov_rad for the projection and the rays of
 *   mgs_render / mgs_render_gathered with MGS_PIPELINE_3DGUT — both extent methods, every kernel degree, depth of field, surface_outputs,
 *     occluder, MGS_SORT_STOCHASTIC, strips, frame contexts, temporal accumulation, every target format, graph replay on and off;
 *   mgs_frame_download_projected_gut (the records of such a frame);
 *   mgs_trace_generate_rays, which then writes the sensor's rays (origin viewInverse's translation, or the lens sample under depth of
 *     field; a pixel without a ray gets the invalid window t_min = 1, t_max = 0): trace them with mgs_trace_rays_device.
 * The depth key, the frustum cull and the sort keep using view / proj: a caller whose sensor sees beyond proj's dilated frustum sets
 * frustum_culling to MGS_CULL_NONE.  The workgroup-level pre-cull of the front end is off for such a frame.
 * MGS_ERR_UNSUPPORTED while a sensor is bound (unbind it with mgs_frame_set_sensor(handle, NULL)): mgs_render with MGS_PIPELINE_3DGS
 * (EWA splatting has no model of distortion), lighting_mode != 0 (the deferred pass unprojects through projInverse), mgs_meshes_render,
 * mgs_render_traced, mgs_render_traced_lit and mgs_render_hybrid.  mgs_trace_rays / mgs_trace_rays_device take the caller's rays and
 * do not look at the binding.  With no sensor bound every entry point behaves exactly as before. */
#define MGS_SENSOR_OPENCV_PINHOLE 0
#define MGS_SENSOR_OPENCV_FISHEYE 1
typedef struct MgsSensorModel {
  int32_t  model;              /* MGS_SENSOR_* */
  int32_t  shutter;            /* 0 = global; anything else: MGS_ERR_UNSUPPORTED */
  float    focal_length[2];    /* pixels, in the sign convention of the frame's own focal length (y follows proj[5]) */
  float    principal_point[2]; /* pixels */
  float    radial[6];          /* pinhole: k1..k6 (numerator 0..2, denominator 3..5) */
  float    tangential[2];      /* pinhole */
  float    thin_prism[4];      /* pinhole */
  float    fisheye_radial[4];  /* fisheye: forward polynomial in theta^2 */
  float    max_angle;          /* fisheye; 0 = computeMaxAngle of the viewport, principal point and focal length */
  uint32_t reserved[9];        /* must be 0 */
} MgsSensorModel; /* 128 B */
int mgs_sensor_model_from_frame(const MgsFrameParams* params, MgsSensorModel* out);
int mgs_frame_set_sensor(MgsScene scene_or_context, const MgsSensorModel* sensor /* NULL unbinds */);

/* ---- ray queries (MGS_HAS_RAY_QUERY): the caller's rays through the scene's particle hierarchy, with the walk of mgs_render_traced's
 * MGS_TRACE_STRATEGY_FULL_ANYHIT (traceRayParticlesInsertionSort, shaders/threedgrt_raytrace.rgen.slang:615-819; insertion
 * rahit.slang:152-167; hit parameter rint.slang:159-172; particleProcessHit and particleIntegrate, threedgrt.h.slang:166-235).  For
 * sensors the library has no model of (rolling shutter: every ray its own origin; the OpenCV pinhole and fisheye models with
 * distortion are mgs_frame_set_sensor's, whose rays mgs_trace_generate_rays writes), lidar and depth probes, picking, and
 * the reflection, refraction and shadow rays an integrator shoots from its OWN geometry into the splats: the library knows no
 * geometry but the particles, the caller ends a ray at its own surface with t_max and starts the secondary ray itself.
 *
 * The ray and its window.  A ray is used AS GIVEN: the direction is not renormalised, and t is the parameter along the given
 * direction (world units for a unit direction).  Nothing in the walk assumes unit length: the hit parameter is -dot(o,d)/dot(d,d)
 * with the unnormalised canonical direction (rint.slang:166-168), the distance to the ray divides by dot(d,d), the node test runs
 * on 1 / direction, and the two places that need a unit vector (the response's model-space direction, rgen:697-698, and the normal
 * fallback -rayDirection) normalise it themselves.  The window of the first pass is (t_min + epsT, t_max + epsT) with the primary
 * walk's epsT = 1e-9; a negative t_min is taken as 0 (a ray has no hits behind its origin).  From there everything is strategy 0 of
 * mgs_render_traced: passes of samples_per_pass nearest hits, max_passes, min_transmittance, what a hit is and when it is accepted,
 * radiance with SH, the transmittance in double, ties in t by ascending global id in the caller's order, depth_iso_threshold,
 * normal_method / thin_particle_threshold, MGS_DEBUG_SH_ONLY and MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED.
 *
 * Results, at the ray's index: radiance and transmittance = float(T) of the walk (the frame's alpha is 1 - this); t_iso = the ray
 * parameter of the first accepted hit after which T is below depth_iso_threshold (0 when nothing was picked) and id = that
 * particle's global id in the caller's order (0xFFFFFFFF when none); hit_count = accepted hits; passes = passes started; normal =
 * the integrated normal in xyz and the sum of the weights in w.  t_iso, id and normal are filled when params->surface_outputs is 1
 * (as the side outputs of a traced frame are: set it for picking and depth probes), else 0 / 0xFFFFFFFF / zeros.
 *
 * Invalid rays.  A ray with a non-finite component (t_min and t_max included), a zero-length direction or t_min > t_max never reaches
 * the traversal: its result is radiance 0, transmittance 1, nothing picked, hit_count 0, passes 0, and it is counted in invalid_rays.
 * Device arrays cannot be checked on the host, so this is a per-ray outcome and not an error code.
 *
 * Reads of MgsFrameParams: sh_degree, alpha_cull_threshold, kernel_degree, kernel_min_response (> 0), alpha_clamp, normal_method,
 * thin_particle_threshold, surface_outputs and debug_flags (the two bits the traced frames honour).  view, proj, camera_pos, width,
 * height, the strip rows, the lens, target_format and temporal_sampling are neither read nor range-checked.  trace_strategy != 0 (the
 * stochastic strategies' seeds are per pixel), lighting_mode != 0 and sort_mode == MGS_SORT_STOCHASTIC: MGS_ERR_UNSUPPORTED; reorder
 * other than 0 / 1, NULL rays or results with count > 0, misaligned device pointers: MGS_ERR_INVALID_ARG; more than 2^31 - 1 rays:
 * MGS_ERR_UNSUPPORTED.  All of this is checked before the handle is looked at.  `trace` / `query` NULL = the defaults.
 *
 * count == 0 is MGS_OK without a launch.  A scene without instances (committed or not) yields transmittance 1 and nothing else for
 * every valid ray.  The hierarchy is the scene's, built lazily under mgs_render_traced's rules and shared with the traced frames.  A
 * bound occluder is not looked at.  A ray query writes its results only: the handle's frame, side outputs and hit counts stay as
 * they are; it does rewrite the handle's per-frame device constants and counters, so mgs_frame_stats, mgs_frame_row_costs and
 * mgs_frame_download_projected of an earlier frame are not meaningful afterwards (a frame context keeps the two apart).
 * mgs_trace_rays copies the batch through staging buffers of the handle and waits; mgs_trace_rays_device takes device pointers
 * (16-byte aligned), is ordered on the handle's stream and, with reorder = 0, waits only when `out` is non-NULL.  With reorder = 1
 * it always blocks the host: mgs_radix_sort_u32 waits for the stream two or three times (and for the device when its scratch grows).
 *
 * Reorder (query->reorder = 1): the lanes of a wave walk nearly the same nodes only when their rays are alike.  A 32-bit coherence
 * key per ray — 21 bits of Morton code of the origin's cell in the scene's box (origins outside are clamped), the direction's
 * octant, 4 + 4 bits of |d.x| and |d.y| over the direction's 1-norm; the largest key for an invalid ray; nothing but the ray and
 * the box enters — is sorted with the ray's index by the library's stable radix sort (mgs_radix_sort_u32), and lane i of workgroup b
 * traces the ray at position b * 256 + i of that order.  Results are written at the ray's own index and do not depend on the
 * order, bit for bit; the integer statistics are equal as well.  Keys and indices (8 B / ray) and the staging buffers of the host
 * variant belong to the handle and count into working_bytes.  reorder_ms is the time between HIP events before the key kernel and
 * behind the sort: it includes the stream standing idle during the sort's host round trips, not only the kernels.  Default 0:
 * DESIGN.md section 3.14 has what was measured (tools/trace_probe.py --rays measures it). */
typedef struct MgsRay {
  float origin[3];
  float t_min;
  float direction[3];
  float t_max;
} MgsRay; /* 32 B */
typedef struct MgsRayResult {
  float    radiance[3];
  float    transmittance; /* float(T) of the walk; 1 for an invalid ray */
  float    t_iso;
  uint32_t id;
  uint32_t hit_count;
  uint32_t passes;
  float    normal[4];
} MgsRayResult; /* 48 B */
typedef struct MgsRayQueryParams {
  int32_t  reorder; /* 0 / 1, default 0 */
  uint32_t reserved[3];
} MgsRayQueryParams;
typedef struct MgsRayQueryOut {
  MgsTraceOut trace;        /* as of a traced frame: the hierarchy, the batch's integer sums, the most passes any ray started, trace_ms
                               from HIP events around the traversal */
  float       reorder_ms;   /* HIP events around the key and sort launches, the sort's host waits included (0 without reorder) */
  uint32_t    invalid_rays;
  uint32_t    reserved[2];
} MgsRayQueryOut;
void mgs_ray_query_params_default(MgsRayQueryParams* q);
int  mgs_trace_rays(MgsScene scene_or_context, const MgsRay* rays_host, uint64_t count, const MgsFrameParams* params,
                    const MgsTraceParams* trace /* NULL = defaults */, const MgsRayQueryParams* query /* NULL = defaults */,
                    MgsRayResult* results_host, MgsRayQueryOut* out /* may be NULL */);
int  mgs_trace_rays_device(MgsScene scene_or_context, const MgsRay* rays_device, uint64_t count, const MgsFrameParams* params,
                           const MgsTraceParams* trace /* NULL = defaults */, const MgsRayQueryParams* query /* NULL = defaults */,
                           MgsRayResult* results_device, MgsRayQueryOut* out /* may be NULL */);
/* The primary rays mgs_render_traced would trace for *params, written to rays_device[height][width] (device memory, 16-byte
 * aligned, row-major; the strip rows are not looked at): pinhole, fisheye and depth of field as "Ray" above (rgen:159-196), exactly
 * the ray the kernel of mgs_render_traced's strategy 0 traces, rounding for rounding (the light pass and the stochastic strategies
 * compute the same ray with roundings of their own in the last bit),
 * t_min = 0.001, t_max = 10000.  A fisheye pixel outside the image circle gets t_min = 1, t_max = 0, an invalid ray.  Reads and
 * checks *params as mgs_render_traced does; ordered on the handle's stream, does not wait.  The seam for a caller who starts
 * from the library's camera and perturbs it: tracing these rays gives the traced frame's radiance, 1 - alpha, hit counts, picked
 * ids and normals bit for bit. */
int  mgs_trace_generate_rays(MgsScene scene_or_context, const MgsFrameParams* params, MgsRay* rays_device);

/* ---- shadow and light queries (MGS_HAS_SHADOW_QUERY): the splats' shadows on the caller's own surfaces.  A caller who rasterises
 * meshes with mgs_meshes_render, or brings a G-buffer of its own, hands over shadow rays, or whole surface points, and gets back what
 * the light pass of mgs_render_traced_lit computes for a splat-surface pixel: traceShadowRayParticle
 * (shaders/threedgrt_raytrace.rgen.slang:1344-1464) per ray, evaluateLightingAndShadingParticles (:1082-1144) per point.  The library
 * still knows no geometry but the particles, and no existing entry point changes: a bound occluder or sensor is refused by the traced
 * and hybrid frames as before.  The ray queries above return the PRIMARY walk's radiance and transmittance, which is not a light
 * pass's shadow: that is one collection, a window that ends 0.001 before the light, the threshold cut, the ramp and the tint.
 *
 * Shadow rays (mgs_trace_shadow_rays, mgs_trace_shadow_rays_device).  The ray is an MgsRay, used AS GIVEN: the direction is not
 * renormalised, and t is the parameter along the given direction (world units for a unit direction).  Nothing in the walk assumes
 * unit length: the hit parameter is -dot(o,d)/dot(d,d) with the unnormalised canonical direction (rint.slang:166-168), the distance
 * to the ray divides by dot(d,d), the node test runs on 1 / direction, and the response's model-space direction (rgen:697-698)
 * normalises itself.  t_max plays lightDist: the collection window is (max(t_min, 0), t_max - 0.001) with the subtraction in fp32
 * and no epsT; ONE collection of the samples_per_pass nearest hits, no second pass (occluders beyond the samples_per_pass-th are not
 * seen); the slots are walked in order, a slot with t >= t_max is skipped; particleProcessHit / particleIntegrate with the
 * transmittance in double; after each slot a transmittance below particle_shadow_transmittance_threshold becomes 0 and ends the
 * walk; then T = saturate(T), scaledT = saturate((T - threshold) / (1 - threshold)), normalizedColor = shadowRadiance / max
 * component (1 where that is <= 0.001), transmittance = saturate(scaledT * lerp(1, normalizedColor,
 * particle_shadow_color_strength * (1 - scaledT))).  With t_min = 0 and t_max = lightDist this is the light pass's shadow ray,
 * operation for operation (one device function serves both).  MGS_DEBUG_SH_ONLY and MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED are honoured
 * as they are there.  Of MgsTraceLightParams the call reads particle_shadow_transmittance_threshold and
 * particle_shadow_color_strength; particle_shadow_offset is NOT READ (the caller has placed the origin), not even range-checked.
 * shadows_mode must be MGS_SHADOWS_HARD: MGS_SHADOWS_SOFT is MGS_ERR_UNSUPPORTED (a query point has no pixel to seed a light's disk sample from), any other value MGS_ERR_INVALID_ARG; `light` NULL =
 * the defaults with shadows_mode MGS_SHADOWS_HARD.  Of MgsTraceParams it reads samples_per_pass and kernel_adaptive_clamping.
 * An invalid ray (a non-finite component, a zero-length direction or t_min > t_max) never reaches the traversal: transmittance
 * (1,1,1), 0 hits, counted in invalid_rays; a per-ray outcome, not an error code.  Reads of MgsFrameParams, the range checks before
 * the handle is looked at, count == 0, the lazily built shared hierarchy, the staging of the host variant, the alignment and stream
 * order of the device variant and `query->reorder` (the ray queries' coherence key and sort) are those of the ray queries, above;
 * trace_strategy must be 0.  A scene without instances yields (1,1,1) and 0 hits.  MgsRayQueryOut is filled as for a ray query:
 * accepted_hits is the sum of `hits`, max_passes_used is 1 where any valid ray was traced.
 *
 * Light queries (mgs_shade_points, mgs_shade_points_device).  A surface point is position, normal, view direction (the direction the
 * viewer's ray TRAVELS, rayDirection, as given), the surface's own colour `radiance` (what the light pass multiplies the material
 * by) and an index into the call's material array (host memory, 1 to 256 entries; uploaded to a table of the handle's).  Per point
 * the result is step 3 of the hybrid frames' documentation at the caller's position: needShading as updateMaterialNeedsShading
 * derives it; radiance * emission alone when it is 0; each light of the scene's table (mgs_scene_set_lights) through
 * computeLightToSurfaceVector, a point or spot light out of range SKIPPED without an ambient term; with shadows_mode =
 * MGS_SHADOWS_HARD one shadow ray per light as above, from position + lightDir * particle_shadow_offset (read here) with t_min 0
 * and t_max lightDist; shading with the shadowed light colour, inShadow (max component < 0.001) returning after the ambient term;
 * with no lights a headlight at params->camera_pos (the one camera field that is read; it must be finite), never shadowed.  The
 * normal is normalised; a normal of length <= 0.2 is replaced by -view_dir, the light pass's fallback.  With shadows_mode =
 * MGS_SHADOWS_DISABLED the call is pure shading and builds no hierarchy.  lighting_mode is not read.
 * An invalid point (a non-finite position, normal, view direction or radiance, or a material index at or above the count) gets colour
 * 0 and 0 hits and is counted in *invalid_points.  The host variant checks the indices itself: one out of range is
 * MGS_ERR_INVALID_ARG, as is a material count outside [1, 256].  Statistics go out through MgsTraceLightOut (shadow_rays = points
 * with a shaded material x lights in range, 0 with shadows off; light_ms = HIP events around the kernel).  Reorder sorts on the
 * position's Morton cell alone (the key kernel's second entry).  Everything else as for shadow rays: the materials are converted into a
 * host table of the handle's and uploaded on its stream, so the device variant does not wait for them (the caller's array may be
 * reused when the call returns).
 *
 * Both write their results and the handle's per-frame device constants and counters only: the handle's frame, side outputs, hit
 * counts and shadow hits stay as they are, but mgs_frame_stats, mgs_frame_row_costs and mgs_frame_download_projected of an earlier
 * frame are not meaningful afterwards (a frame context keeps the two apart).  A bound occluder or sensor is not looked at.  Staging
 * buffers, keys and the material table belong to the handle and count into working_bytes.
 * PARITY UNPINNED: the reference shades a MESH hit with its own mesh function (barycentric normals, the mesh's material, mesh
 * shadow rays through both acceleration structures); this shades a caller's point with the PARTICLES' function and shadows it by
 * particles only, so a hybrid picture made this way agrees with the reference's in the splats' shadows on the mesh, not in the mesh's
 * own shading model or in mesh-on-mesh shadows.  The window's lower bound t_min and non-unit directions have no counterpart in the
 * reference (its shadow rays start at TMin 0 with a unit direction).  The headlight sits at camera_pos, which for a caller's point
 * need not be where view_dir starts. */
typedef struct MgsShadowResult {
  float    transmittance[3]; /* what the light's colour is multiplied by; (1,1,1) for an invalid ray */
  uint32_t hits;             /* hits the walk accepted */
} MgsShadowResult; /* 16 B */
typedef struct MgsSurfacePoint {
  float    position[3];
  uint32_t material; /* index into the call's material array */
  float    normal[3];
  float    _pad0;
  float    view_dir[3]; /* the direction the viewer's ray travels (rayDirection), as given */
  float    _pad1;
  float    radiance[3]; /* the surface's own colour: what the light pass multiplies the material by */
  float    _pad2;
} MgsSurfacePoint; /* 64 B */
typedef struct MgsShadeResult {
  float    color[3];
  uint32_t shadow_hits; /* accepted shadow hits, summed over the lights */
} MgsShadeResult; /* 16 B */
int mgs_trace_shadow_rays(MgsScene scene_or_context, const MgsRay* rays_host, uint64_t count, const MgsFrameParams* params,
                          const MgsTraceParams* trace /* NULL = defaults */, const MgsTraceLightParams* light /* NULL = defaults, hard shadows */,
                          const MgsRayQueryParams* query /* NULL = defaults */, MgsShadowResult* results_host, MgsRayQueryOut* out /* may be NULL */);
int mgs_trace_shadow_rays_device(MgsScene scene_or_context, const MgsRay* rays_device, uint64_t count, const MgsFrameParams* params,
                                 const MgsTraceParams* trace /* NULL = defaults */, const MgsTraceLightParams* light /* NULL = defaults, hard shadows */,
                                 const MgsRayQueryParams* query /* NULL = defaults */, MgsShadowResult* results_device,
                                 MgsRayQueryOut* out /* may be NULL */);
int mgs_shade_points(MgsScene scene_or_context, const MgsSurfacePoint* points_host, uint64_t count, const MgsMaterial* materials_host,
                     uint32_t material_count, const MgsFrameParams* params, const MgsTraceParams* trace /* NULL = defaults */,
                     const MgsTraceLightParams* light /* NULL = defaults */, const MgsRayQueryParams* query /* NULL = defaults */,
                     MgsShadeResult* results_host, MgsTraceLightOut* light_out /* may be NULL */, uint32_t* invalid_points /* may be NULL */);
int mgs_shade_points_device(MgsScene scene_or_context, const MgsSurfacePoint* points_device, uint64_t count, const MgsMaterial* materials_host,
                            uint32_t material_count, const MgsFrameParams* params, const MgsTraceParams* trace /* NULL = defaults */,
                            const MgsTraceLightParams* light /* NULL = defaults */, const MgsRayQueryParams* query /* NULL = defaults */,
                            MgsShadeResult* results_device, MgsTraceLightOut* light_out /* may be NULL */,
                            uint32_t* invalid_points /* may be NULL */);

/* ---- mesh ray queries (MGS_HAS_MESH_RAY_QUERY): the caller's rays against the scene's triangle meshes.  Replaces, for rays the
 * caller supplies, the mesh TLAS with traceBounceRayMeshes (shaders/threedgrt_raytrace.rgen.slang:495-553), the closest-hit shader
 * (shaders/threedgrt_raytrace.rchit.slang:31-67) and traceShadowRayMesh (rgen:1295-1341).  For picking on meshes, reflection and
 * refraction rays shot from or at meshes, mesh-on-mesh shadow rays (multiply the result with mgs_trace_shadow_rays' splat shadow), and
 * as a second, independent implementation next to the mesh rasteriser.  Everything here is additive: no frame kernel and no other
 * entry point looks at the triangle hierarchy yet.
 *
 * The hierarchy.  One leaf per triangle of every mesh instance, in world space: world vertices are M p in fp32, the products in the
 * order of the mesh pass's vertex stage (mgs_meshes_render: ((x m0 + y m4) + z m8) + m12), here with each operation rounded once.
 * The rasteriser's kernel writes the same expression but leaves the compiler free to fuse a product into the following sum, so
 * the two triangles are the same up to that contraction: a vertex may differ in its last bit.  A triangle with a non-finite world vertex or with zero area in float (the cross
 * product of its edge vectors is exactly 0) gets no leaf.  The leaf's box is the min / max of the three vertices inflated by 4 ulps
 * of its extent plus 2 ulps of its magnitude plus 1e-37 per axis: it strictly contains the triangle.  The tree is the splat hierarchy's implicit complete 8-ary tree: leaves sorted
 * (the library's stable radix sort) by the 30-bit Morton code of the leaf centroid in the meshes' world box, which the host computes
 * in double from the meshes' local boxes and the instances' transforms; a node bounds eight consecutive nodes of the level below.  No
 * pointers, no atomics: the build is bit-reproducible.  Triangle records (world vertices, global primitive id, instance id, material
 * id; 48 B) are stored in leaf order.  The hierarchy belongs to the SCENE and is shared by its frame contexts; it is rebuilt lazily
 * by the next mesh query after mgs_mesh_instance_add or mgs_mesh_instance_set_transform, and a rebuild first waits for the work in
 * flight on all contexts (the rule of the splat hierarchy).  Mesh queries on different contexts of one scene may run from different
 * threads: the check, a rebuild and the query's launches are serialised by a mutex of the hierarchy.  The editing calls
 * (mgs_mesh_instance_*) are not part of that: do not edit the scene while another thread queries it.  Its bytes count into scene_bytes of mgs_scene_memory_usage; staging,
 * keys and counters belong to the handle and count into working_bytes.  mgs_mesh_instance_set_visible does NOT rebuild: visibility
 * is read per candidate triangle at query time from the device mesh table.  No mesh instance, or no valid triangle: every ray
 * misses and nothing is launched for the build.
 *
 * The ray and its window.  The ray is an MgsRay, used AS GIVEN: the direction is not renormalised and t is the parameter along the
 * given direction, as in mgs_trace_rays.  A hit needs t_min' < t < t_max with t_min' = max(t_min, 0): both ends are OPEN and there is
 * no epsT; the caller adds 0.001 where it wants the reference's TMin.  What the reference's hardware does with a hit exactly at an
 * end of the window is PARITY UNPINNED.  An invalid ray (a non-finite component, t_min and t_max included, a zero-length direction or
 * t_min > t_max) never reaches the traversal: it is a miss and is counted in invalid_rays (a per-ray outcome, not an error code).
 *
 * Intersection.  Watertight, both facings: the reference sets VK_GEOMETRY_INSTANCE_TRIANGLE_FACING_CULL_DISABLE_BIT_KHR on every
 * mesh instance (src/mesh_manager_vk.cpp:446), so the RAY_FLAG_CULL_BACK_FACING_TRIANGLES of its mesh rays has no effect and back
 * faces are hit.  The test is the shear-to-ray-space formulation of Woop, Benthin and Wald (JCGT 2013): the vertices are moved to
 * the ray's origin and sheared so that the ray runs along the axis of its largest direction component; the three edge functions are
 * taken from the sheared x and y, each product and difference rounded once (never contracted into a fused multiply-add), so an edge
 * shared by two triangles gives both the same magnitude with the opposite sign; edges are inclusive (all three >= 0 or all three
 * <= 0); when any edge function is exactly 0 the three are recomputed in double; t = (U z0 + V z1 + W z2) / (U + V + W) with the
 * sheared z.  The fixed-function test of the reference's device is not specified beyond watertightness: which of two triangles a ray
 * exactly on their shared edge reports, and the last bits of t and of the barycentrics, are PARITY UNPINNED.
 * Ties.  Two hits with bit-identical t resolve to the LOWER global primitive id, whatever the order of traversal.
 *
 * MGS_MESH_RAYS_CLOSEST reports the nearest hit: t; instance_id (creation order); primitive_id, the GLOBAL primitive id, exactly the
 * id mgs_meshes_download(which = 2) reports (instances concatenated in creation order, visible or not); material_id (the
 * triangle's index into its mesh's materials); the barycentrics b1, b2 of vertices 1 and 2 (rchit.slang:50-51; vertex 0 has
 * 1 - b1 - b2); position = the instance transform of the interpolated LOCAL positions (rchit.slang:54-55); normal =
 * normalize(transpose(transformRotScaleInverse) n) of the interpolated vertex normals (rchit.slang:58-59), with the
 * transformRotScaleInverse the mesh pass uses, NOT flipped towards the ray; hit = 1.  A miss is t = +inf, all three ids 0xFFFFFFFF,
 * position, normal and barycentrics 0, hit = 0.
 * MGS_MESH_RAYS_OCCLUSION reports only whether ANYTHING is hit in the window (traceShadowRayMesh with
 * RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH): hit = 1 or 0, every other field as for a miss; the traversal stops at the first hit it
 * finds.  Meshes carry no transmittance here (MgsMaterial has no such field and the OBJ subset reads no Tf), so every mesh is
 * opaque and the shadow is transmittance 1 - hit; a boolean keeps "first hit" deterministic.  Coloured mesh shadows are later work.
 *
 * Independence from the splats.  A scene without splats may be queried (mesh instances do not need mgs_scene_commit); the splat
 * hierarchy is neither built nor read; a bound occluder or sensor is not looked at; the handle's frame, side outputs, hit counts and
 * mesh-pass images stay untouched.  A hierarchy build and a reorder run mgs_radix_sort_u32 on the handle, which rewrites the handle's
 * per-frame device counters: mgs_frame_stats and mgs_frame_row_costs of an earlier frame are not meaningful afterwards (a frame
 * context keeps the two apart).
 * Reorder (params->reorder = 1): the ray queries' coherence key and sort (see there) with the meshes' world box in place of the
 * scene's.  Hits and integer statistics are identical with and without it, bit for bit.
 *
 * Arguments, checked before the handle is looked at: mode not one of the two, reorder not 0 / 1, a non-zero reserved word, NULL rays
 * or hits with count > 0, misaligned device pointers: MGS_ERR_INVALID_ARG; more than 2^31 - 1 rays: MGS_ERR_UNSUPPORTED.  `params`
 * NULL = the defaults (closest, no reorder).  count == 0 is MGS_OK without a launch.  mgs_trace_mesh_rays copies the batch through
 * staging buffers of the handle and waits; mgs_trace_mesh_rays_device takes device pointers (16-byte aligned), is ordered on the
 * handle's stream and, with reorder = 0 and no rebuild due, waits only when `out` is non-NULL.
 *
 * Mesh hits inside mgs_render_traced and mgs_render_traced_lit are the next section's (MGS_HAS_TRACE_MESHES: the same traversal and
 * triangle test called from the frame kernels).  Out of scope here, and what the hierarchy is meant to serve next: mesh hits inside
 * mgs_render_hybrid, and mesh occlusion inside mgs_trace_shadow_rays and mgs_shade_points (the occlusion mode's walk).  Not planned on it: mesh material transmittance,
 * ior, reflection and refraction bounces, light proxies, ray masks, refitting instead of rebuilding, mgs_render_gathered. */
typedef enum MgsMeshRayMode {
  MGS_MESH_RAYS_CLOSEST   = 0,
  MGS_MESH_RAYS_OCCLUSION = 1
} MgsMeshRayMode;
typedef struct MgsMeshHit {     /* 64 B = four 16-byte vectors; arrays of it on the device must be 16-byte aligned */
  float    t;                   /* offset  0: ray parameter of the hit; +inf = miss (and always in occlusion mode) */
  uint32_t instance_id;         /*         4: mesh instance, creation order; 0xFFFFFFFF = none */
  uint32_t primitive_id;        /*         8: global primitive id as mgs_meshes_download(which = 2); 0xFFFFFFFF = none */
  uint32_t material_id;         /*        12: index into the mesh's materials; 0xFFFFFFFF = none */
  float    position[3];         /*        16: world position */
  float    b1;                  /*        28: barycentric weight of vertex 1 */
  float    normal[3];           /*        32: world normal, unit length, not flipped towards the ray */
  float    b2;                  /*        44: barycentric weight of vertex 2 */
  uint32_t hit;                 /*        48: 1 = something is hit in the window, 0 = nothing */
  uint32_t reserved[3];         /*        52: written as 0 */
} MgsMeshHit;
typedef struct MgsMeshRayParams {
  int32_t  mode;    /* MgsMeshRayMode, default MGS_MESH_RAYS_CLOSEST */
  int32_t  reorder; /* 0 / 1, default 0 */
  uint32_t reserved[2]; /* must be 0 */
} MgsMeshRayParams;
typedef struct MgsMeshRayOut {
  uint64_t triangles;      /* triangles of all mesh instances, visible or not */
  uint64_t leaves;         /* ... that got a leaf */
  uint64_t nodes;          /* nodes of all levels, the leaves included */
  uint64_t node_visits;    /* integer sums over the valid rays of the batch */
  uint64_t triangle_tests; /* ray/triangle tests (triangles of invisible instances are skipped before the test) */
  uint64_t hits;           /* rays with hit = 1 */
  uint32_t invalid_rays;
  uint32_t bvh_rebuilt;    /* 1: this call rebuilt the hierarchy */
  float    build_ms;       /* HIP events around the build's launches (0 when nothing was built) */
  float    trace_ms;       /* HIP events around the ray/triangle kernel */
  float    reorder_ms;     /* HIP events around the key and sort launches, the sort's host waits included (0 without reorder) */
  uint32_t reserved;
} MgsMeshRayOut;
void mgs_mesh_ray_params_default(MgsMeshRayParams* params);
int  mgs_trace_mesh_rays(MgsScene scene_or_context, const MgsRay* rays_host, uint64_t count, const MgsMeshRayParams* params /* NULL = defaults */,
                         MgsMeshHit* hits_host, MgsMeshRayOut* out /* may be NULL */);
int  mgs_trace_mesh_rays_device(MgsScene scene_or_context, const MgsRay* rays_device, uint64_t count,
                                const MgsMeshRayParams* params /* NULL = defaults */, MgsMeshHit* hits_device, MgsMeshRayOut* out /* may be NULL */);

/* ---- mesh hits in the traced frames (MGS_HAS_TRACE_MESHES): the scene's triangle meshes take part in mgs_render_traced (unlit) and
 * mgs_render_traced_lit, at bounce 0.  Restates, of shaders/threedgrt_raytrace.rgen.slang, traceBounceRayMeshes at bounce 0
 * (:495-553), the mesh parts of evaluateLightingAndShadingForBounce (:1037-1077), evaluateLightingAndShadingMeshes in its direct
 * mode (:1222-1255), traceShadowRayForLight with traceShadowRayMesh (:1262-1341) and the depth rule of writeToGBuffers (:1490-1502).
 * Added within ABI 5.1: entry points and one new struct; MgsTraceParams (32 B) and MgsTraceOut (56 B) do not change.
 *
 * The setting.  mgs_frame_set_trace_meshes belongs to the handle, scene or frame context, as mgs_frame_set_occluder and
 * mgs_frame_set_sensor do.  Off is the default (NULL = off), and with it off every entry point does exactly what it did before,
 * bit for bit, whether or not the scene holds mesh instances.  enabled not 0 / 1, a threshold outside [0, 1] (NaN included) or a
 * non-zero reserved word: MGS_ERR_INVALID_ARG, checked before the handle is looked at.  With the setting on, mgs_render_traced with
 * trace_strategy 0 and mgs_render_traced_lit include the scene's visible mesh instances; mgs_render_traced with strategy 1 or 2 and
 * mgs_render_hybrid (whose meshes are mgs_frame_set_hybrid_meshes', MGS_HAS_HYBRID_MESHES) return MGS_ERR_UNSUPPORTED; mgs_render, mgs_meshes_render and the ray,
 * shadow and mesh-ray queries do not read it.  A scene without splats but with meshes renders the meshes alone.  A scene with no
 * visible mesh instance renders the frame it renders with the setting off, bit for bit (the frame's kernels are then the same ones;
 * only the all-miss hit records are written besides).  mgs_render_gathered is not wired.
 *
 * Primary mesh ray (:495-553).  The hit of a pixel with a valid ray is exactly what mgs_trace_mesh_rays in closest mode reports for
 * the ray mgs_trace_generate_rays makes for that pixel, depth of field and fisheye included, with the window t_min = 0.001,
 * t_max = 10000 (in fp32 the reference's epsT = 1e-9 vanishes), byte for byte; a fisheye pixel outside the image circle is a miss
 * counted in invalid_rays.  The query's rules apply unchanged: open window, both facings, the watertight test, ties to the lower
 * primitive id, invisible instances skipped.  A hit sets the upper end of the pixel's particle walk: its passes collect in
 * (tMin + epsT, t_mesh + epsT).
 * Unlit composite (:1064-1075).  Where a mesh is hit and T > min_mesh_composite_transmittance (compared in double against the walk's
 * transmittance), rgb += float(T) * (emission + ambient + diffuse) of the hit triangle's material.
 * Lit frame.  The primary walk and surfaceFinalFiltering are as in a frame without meshes; a discarded splat surface leaves radiance 0
 * and T = 1.  The splat surface is shaded when t_iso > 0 && t_iso < t_mesh and the pick is valid (:1047-1049): the shading of
 * mgs_render_traced_lit with one change, every shadow ray first asks the meshes.  The mesh occlusion ray (:1295-1341) starts at the
 * UN-offset shadow origin and runs along lightDir with the window (0.001, lightDist - 0.001); meshes are opaque, so an occluded
 * light has shadow transmittance 0 and the particle shadow ray is not traced for it (:1285); otherwise the particle shadow ray runs
 * as before and the two transmittances multiply.  Mesh shading (:1148-1165, :1222-1255) has the condition of the unlit composite:
 * rgb += emission, unweighted, as written at :1159; that is all when the material's needShading is 0 (MgsMaterial's rule); otherwise
 * every light in range at meshHitWorldPos, or the never-shadowed headlight when the scene has no lights, is shaded with
 * wavefrontComputeShadingDirectOnly(light x shadow, meshHitWorldPos, meshHitWorldNrm, material, rayDirection, inShadow, T, rgb),
 * where meshHitWorldPos and meshHitWorldNrm are the closest hit's position and normal as MgsMeshHit reports them (the normal is not
 * flipped towards the ray), and the shadow comes from traceShadowRayForLight at meshHitWorldPos: the meshes first, then the
 * particles with particle_shadow_offset.  This is what puts the splats' shadow on a mesh floor.  With shadows_mode
 * MGS_SHADOWS_DISABLED neither ray is traced.
 * Outputs.  Alpha is 1 where a mesh was composited (the mesh is opaque); elsewhere it stays this library's 1 - T (the reference
 * writes 1.0 everywhere).  Surface output 0 is the ndc z of the iso pick where there is one, else of origin + t_mesh * direction
 * where a mesh is hit (:547-551), else 0; id and normal stay the splats'.  The shadow hit counts of a pixel include the particle
 * shadow rays of its mesh point, and MgsTraceLightOut's sums include them.  Temporal accumulation, target formats, strip rows and
 * frame contexts work as after any traced frame.
 *
 * mgs_trace_download_mesh_hits copies the last traced frame's per-pixel hit records ([height][width] MgsMeshHit; a miss as the
 * query writes it); MGS_ERR_STATE unless the handle's last traced frame ran with the setting on; rows outside a strip frame's
 * rows are stale.  mgs_trace_mesh_stats waits and reports the integer sums of that frame's primary mesh rays in `primary`
 * (triangles, leaves, nodes, node_visits, triangle_tests, hits, invalid_rays, bvh_rebuilt, build_ms, trace_ms: HIP events around
 * the primary mesh kernel) and of the mesh occlusion rays of a lit frame in `shadow` (hits = rays occluded; trace_ms: HIP events
 * around the mesh composite kernel, which traces those of the mesh points; those of the splat surface run inside the light pass and
 * are in light_ms); `shadow` is all zero after an unlit frame.  Either may be NULL.
 *
 * The frame's set-up runs the lazy build of the mesh ray queries' triangle hierarchy as it stands and holds the hierarchy's mutex
 * from the signature check to the frame's last launch; a rebuild waits for all contexts' streams.  Per-pixel buffers belong to the
 * handle and count into working_bytes: the hit record (64 B), its t (4 B) and the walk's transmittance rounded once to fp32 (4 B);
 * an unlit frame with a visible mesh also keeps the lit frames' fp32 pixel and ray parameter (16 B + 4 B).
 * PARITY UNPINNED: what the mesh ray queries list, and the reference's RAY_FLAG_CULL_BACK_FACING_TRIANGLES, which has no effect there.
 * Out of scope: mesh occlusion inside mgs_trace_shadow_rays / mgs_shade_points, the stochastic
 * strategies with meshes, light proxies, ray masks, mgs_render_gathered.  Mesh transmittance / ior / reflection /
 * refraction bounces and indirect lighting are mgs_render_traced_indirect's (MGS_HAS_TRACE_BOUNCES, below). */
#define MGS_HAS_TRACE_MESHES 1
typedef struct MgsTraceMeshParams {
  int32_t  enabled;                          /* 0 / 1, default 0 */
  float    min_mesh_composite_transmittance; /* frameInfo.minMeshCompositeTransmittance, default 0.0 (shaderio.h:285); [0, 1] */
  uint32_t reserved[2];                      /* must be 0 */
} MgsTraceMeshParams;
void mgs_trace_mesh_params_default(MgsTraceMeshParams* params);
int  mgs_frame_set_trace_meshes(MgsScene scene_or_context, const MgsTraceMeshParams* params /* NULL = off */);
int  mgs_trace_download_mesh_hits(MgsScene scene_or_context, MgsMeshHit* host_dst, size_t count); /* [height][width] */
int  mgs_trace_mesh_stats(MgsScene scene_or_context, MgsMeshRayOut* primary, MgsMeshRayOut* shadow); /* either may be NULL; waits */

/* ---- meshes in the hybrid frames (MGS_HAS_HYBRID_MESHES): the scene's triangle meshes take part in mgs_render_hybrid, the reference's
 * PIPELINE_HYBRID and PIPELINE_HYBRID_3DGUT for composed scenes (doc/hybrid_rendering_3d_gaussians.md;
 * shaders/threedgrt_raytrace.rgen.slang:252-281, :346-460, :1037-1077): the splats are rasterised against a traced mesh depth pre-pass,
 * then splats and meshes are shaded together, each shadowing the other.  Added within ABI 5.1: entry points only, no struct or default
 * changes.
 *
 * The setting belongs to the handle, scene or frame context, and is off by default (NULL = off).  It reuses MgsTraceMeshParams with
 * mgs_frame_set_trace_meshes' checks (enabled 0 / 1, the threshold in [0, 1] with NaN refused, reserved words 0: MGS_ERR_INVALID_ARG
 * before the handle is looked at).  It is deliberately a setting of its own: with it off, mgs_render_hybrid does exactly what it did
 * before, bit for bit, including MGS_ERR_UNSUPPORTED while mgs_frame_set_trace_meshes is on or an occluder is bound.  With it on,
 * mgs_render_hybrid does not read the trace-mesh setting; a caller-bound occluder is still MGS_ERR_UNSUPPORTED (the frame binds its own
 * depth plane), and so is MGS_SHADOWS_SOFT (the mesh composite continues the light pass's random state, whose conditions differ in a
 * hybrid frame: later work).  MGS_SORT_STOCHASTIC, a bound sensor, MGS_LIGHTING_INDIRECT and mgs_render_gathered behave as without
 * the setting.  With the setting on but no visible mesh instance that has a leaf, the frame is the setting-off frame, bit for bit
 * (only the all-miss hit records are written besides).  No other entry point reads the setting.
 *
 * The frame, on the handle's stream:
 * 1. Mesh depth pre-pass (meshDepthOnly, :252-281).  The primary mesh ray of "mesh hits in the traced frames" on the pixel's ray (the
 *    hand-over's ray; lens and fisheye included for 3DGUT) leaves the pixel's MgsMeshHit.  The handle's own depth plane gets
 *    clip.z / clip.w of clip = (meshHitWorldPos * view) * proj in fp32 on a hit, and 1.0 on a miss or outside the fisheye circle.
 * 2. Raster frame: mgs_render's unlit frame with surface_outputs = 1, as in a hybrid frame without meshes, with that plane bound as
 *    the occluder depth and no occluder colour.
 * 3. Hand-over, as documented for mgs_render_hybrid, and besides: T = 1 - stored alpha in fp32, from the pixel as stored in its target
 *    format (:357-358); a discarded pixel has radiance 0 and T = 1 (:468-478); a surface with a valid pick whose ray parameter is not
 *    < t_mesh is not discarded: splatIsClosest fails (:1047), it keeps its raster colour unlit and its own T.
 * 4. Light pass: the splat surface in front of the mesh is shaded as in mgs_render_traced_lit with mesh hits: every shadow ray asks
 *    the meshes first, from the un-offset origin, then the particles.
 * 5. Mesh shading, where a mesh is hit and T > min_mesh_composite_transmittance (compared in double): exactly the lit frame's of
 *    "mesh hits in the traced frames" (emission unweighted, needShading, the lights in range at meshHitWorldPos with the un-flipped
 *    normal, the mesh occlusion ray then the particle shadow ray, the headlight without lights), on the base colour and T of step 3.
 * 6. Temporal accumulation runs after step 5.  MgsTraceLightOut::light_ms brackets steps 3 and 4.
 * Deliberate differences from the reference: alpha is 1 where a mesh was composited, elsewhere the stored alpha, and 0 where the pixel
 * is discarded (the reference writes 1.0 everywhere); the splat surface is shaded and its shadow rays start at ONE position, ray
 * origin + ray parameter * ray direction, as in every hybrid frame.
 * Afterwards mgs_trace_download_mesh_hits and mgs_trace_mesh_stats work as after a lit traced frame with mesh hits (`primary`: the
 * pre-pass, both kernels; `shadow`: the occlusion rays, trace_ms around the mesh shading); mgs_frame_download_surface returns the
 * raster pass's outputs untouched; mgs_trace_download_shadow_hits includes the mesh points' particle shadow hits; strip rows and frame
 * contexts work.  The two downloads and the statistics answer for the handle's last HYBRID frame: a frame that fails clears them, a
 * later mgs_render does not (as the traced frames' downloads outlive one).  The depth plane (4 B / pixel) belongs to the handle and counts into working_bytes with the per-pixel mesh buffers.
 * Out of scope: bounces and soft shadows in hybrid frames with meshes. */
#define MGS_HAS_HYBRID_MESHES 1
int mgs_frame_set_hybrid_meshes(MgsScene scene_or_context, const MgsTraceMeshParams* params /* NULL = off */);
/* test/debug hook: the depth plane of the handle's last hybrid frame's pre-pass, [height][width] floats (rows outside a strip frame's
 * rows are stale); MGS_ERR_STATE unless that frame ran the pre-pass (setting on, a visible mesh instance with a leaf); waits */
int mgs_debug_download_hybrid_depth(MgsScene scene_or_context, float* host_dst, size_t count);

/* ---- reflection and refraction bounces (MGS_HAS_TRACE_BOUNCES): the indirect traced frame, the reference's LIGHTING_INDIRECT
 * (shaderio.h:133) for trace strategy 0: the bounce loop of shaders/threedgrt_raytrace.rgen.slang:230-337 off mesh materials that
 * say "mirror" or "glass".  mgs_render_traced_lit, mgs_render_hybrid and mgs_render keep answering MGS_LIGHTING_INDIRECT as before.
 *
 * Bounce 0 is the frame mgs_render_traced_lit makes with the handle's trace-mesh setting on, except that the mesh is shaded in the
 * indirect mode of evaluateLightingAndShadingMeshes (:1169-1219) through wavefrontComputeShading (wavefront.h.slang:282-376), and the
 * transmittance is a double3 from the first material multiplication on.  The light term is the direct function's (:233-280).  After
 * it the material's illum selects: <= 0: T = 0; == 1: T *= specular, new ray = (meshHitWorldPos, reflect(rayDir, worldNrm));
 * >= 2: T *= transmittance, new ray from meshHitWorldPos along refract(rayDir, N, eta) with eta = 1 / ior, and N = -worldNrm,
 * eta = ior when dot(rayDir, worldNrm) > 0; the result is normalised; when length(refracted) > 0 fails, reflect(rayDir, N) (total
 * internal reflection).  Both set done = 0.  The light loop's state rule (:1186-1197): a light out of range is skipped before
 * anything happens; T, ray and done are restored before every light but the first; what survives is what the last light shaded
 * left; radiance accumulates over all lights with the restored T; with every light out of range nothing is called, done stays 1
 * and the pixel ends; with no lights the never-shadowed headlight at camera_pos applies.  A material whose needShading is 0 adds its
 * emission and never bounces (:1159-1165).
 *
 * Bounce b >= 1, for pixels with done == 0, b up to max_bounces inclusive (:328-330): tMin = 0.001, tMax = 10000; the closest mesh
 * hit of the bounce ray under the rules of mgs_trace_mesh_rays (:505-552); isoSurfDepth and integratedNormal reset (:568-573); the
 * pass walk of strategy 0 in (tMin + epsT, t_mesh + epsT) with the CARRIED radiance, double3 transmittance and hit count
 * (:615-763): loop and slot conditions are maxComponent(T) > min_transmittance, the iso pick is taken when isoSurfDepth == 0 and
 * T.x < depth_iso_threshold (the x channel, as written).  surfaceFinalFiltering does not run (:581): the integrated normal is the
 * raw weighted sum and a walk without a pick keeps its unshaded radiance.  Then evaluateLightingAndShadingForBounce (:1037-1062):
 * the splat surface is shaded when t_iso > 0, t_iso < t_mesh and there is a pick, on radiance - radianceBeforeParticles (added back
 * afterwards), at origin + t_iso * dir, with the lit frame's shadow origin and both shadow walks; then the mesh as at bounce 0 when
 * hit and maxComponent(T) > min_mesh_composite_transmittance (in double).
 *
 * Outputs.  The image is the final radiance; alpha, surface depth, picked id and normal are bounce 0's, as the lit mesh frame
 * defines them.  mgs_trace_download_hit_counts and mgs_trace_download_shadow_hits sum over all bounces; MgsTraceOut::accepted_hits
 * and MgsTraceLightOut's sums include the bounces' rays; mgs_trace_download_mesh_hits stays the primary hit.  Temporal accumulation,
 * target formats, strip rows and frame contexts work as after any traced frame.
 *
 * Bounce materials are the three fields of ObjMaterial (wavefront.h:37-50) MgsMaterial leaves out; illum is the reference's DERIVED
 * model (0, 1, >= 2), not the MTL statement's number.  mgs_bounce_material_from_mtl restates src/obj_loader.cpp:50-59 as written: it
 * tests transmittance.x twice and never .z, so Tf = (0, 0, 1) is not refractive.  mgs_mesh_instance_set_bounce_materials is indexed by
 * the triangle's material id; ids >= count and an instance never set are illum 0; count = 0 clears.  It belongs to the scene and
 * follows the ordering rule of mgs_scene_set_lights (waits for all contexts, rewrites the device table, MGS_ERR_STATE on a context
 * handle); it does not invalidate the triangle hierarchy.  A non-finite field, illum >= 2 with ior not finite or <= 0, or a non-zero
 * reserved word is MGS_ERR_INVALID_ARG.
 *
 * mgs_render_traced_indirect follows mgs_render_traced_lit's conventions (NULL = defaults, a non-NULL out waits, ranges are checked
 * before the handle is looked at).  lighting_mode must be MGS_LIGHTING_INDIRECT (anything else: MGS_ERR_INVALID_ARG);
 * trace_strategy != 0 and MGS_SHADOWS_SOFT (its random state would have to be carried across the bounce launches: later work) are MGS_ERR_UNSUPPORTED; max_bounces outside [1, 16] is MGS_ERR_INVALID_ARG; the
 * handle's trace-mesh setting off is MGS_ERR_STATE (nothing to bounce off; min_mesh_composite_transmittance is read from that
 * setting).  A bound sensor model and a bound occluder are refused as the lit frame refuses them.  MgsTraceBounceOut: index b - 1
 * holds the live pixels and the mesh hits of bounce b, particle_hits the hits accepted at b >= 1, bounce_ms HIP events around
 * everything after bounce 0.  The host enqueues max_bounces rounds unconditionally; counts never leave the device in between.
 *
 * Bounce 0 runs the lit mesh frame's launches as they are; a hand-over kernel behind them shades the pixels whose material bounces a
 * second time, in fp32 for the carried radiance (their shadow rays are traced twice and counted once).  With every bounce material
 * illum 0, or every mesh instance invisible, the frame is mgs_render_traced_lit's byte for byte.
 * Per-pixel bounce state belongs to the handle and counts into working_bytes: 64 B a pixel — a live word (4 B), ray origin and
 * direction (24 B), the fp32 radiance (12 B) and the double3 transmittance (24 B) — plus a 264-byte counter block, besides the lit
 * mesh frame's 92 B.  The closest mesh walks of the bounce rays are not part of mgs_trace_mesh_stats' `primary`; the bounces' mesh
 * occlusion rays are in `shadow`.
 * Out of scope: the stochastic strategies' bounces, soft shadows, hybrid frames, light proxies, ray masks, textures, multi-GPU
 * (mgs_render_gathered).
 * mgs_mesh_load_obj additionally reads Tf / Kt, Ni and illum from the material library (initial values 0, 1, 0; tinyobj is not in
 * the reference tree, so these defaults are build-defined, PARITY UNPINNED as the loader's subset is); MgsMeshView and everything
 * the loader returned before are unchanged.  mgs_mesh_bounce_materials returns them through mgs_bounce_material_from_mtl, one per
 * material of the mesh (`count` receives that number; capacity 0 only asks for it; a smaller capacity is MGS_ERR_INVALID_ARG); a
 * mesh from arrays returns defaults. */
#define MGS_HAS_TRACE_BOUNCES 1
typedef struct MgsBounceMaterial {
  float    transmittance[3]; /* ObjMaterial::transmittance (Tf), default 0 */
  float    ior;              /* ObjMaterial::ior (Ni), default 1 */
  int32_t  illum;            /* the derived model: <= 0 none, 1 reflective, >= 2 refractive; default 0 */
  uint32_t reserved[3];      /* must be 0 */
} MgsBounceMaterial;
typedef struct MgsTraceBounceParams {
  int32_t  max_bounces;      /* frameInfo.rtxMaxBounces, default 3 (shaderio.h:273); [1, 16] */
  uint32_t reserved[3];      /* must be 0 */
} MgsTraceBounceParams;
typedef struct MgsTraceBounceOut {
  uint64_t rays[16];         /* [b - 1]: pixels live at bounce b */
  uint64_t mesh_hits[16];    /* [b - 1]: of them, bounce rays that hit a mesh */
  uint64_t particle_hits;    /* particle hits accepted at b >= 1 */
  float    bounce_ms;        /* HIP events around everything after bounce 0 */
  uint32_t reserved;
} MgsTraceBounceOut;
void mgs_bounce_material_default(MgsBounceMaterial* m);
void mgs_bounce_material_from_mtl(const float tf[3], float ni, int mtl_illum, MgsBounceMaterial* out);
int  mgs_mesh_bounce_materials(MgsMesh mesh, MgsBounceMaterial* out, uint32_t capacity, uint32_t* count);
int  mgs_mesh_instance_set_bounce_materials(MgsScene scene, int mesh_instance_id, const MgsBounceMaterial* m, uint32_t count);
void mgs_trace_bounce_params_default(MgsTraceBounceParams* params);
int  mgs_render_traced_indirect(MgsScene scene_or_context, const MgsFrameParams* params, const MgsTraceParams* trace,
                                const MgsTraceLightParams* light, const MgsTraceBounceParams* bounce, MgsTraceOut* out,
                                MgsTraceLightOut* light_out, MgsTraceBounceOut* bounce_out);

/* ---- runtime image comparison: replaces ImageCompare (src/image_compare.{h,cpp}) with its two compute shaders
 * (shaders/image_compare_metric.comp.slang, shaders/image_compare_composite.comp.slang, colour helpers shaders/color.h.slang).
 * Capture a frame, then compute MSE / PSNR / FLIP of every later frame against it on the device and build the split view.  Valid
 * per handle (scene or frame context, like mgs_frame_set_occluder): a capture belongs to the handle it was made on.  With no
 * capture held, and as long as these entry points are not called, the library does what it did before they existed.
 *
 * The "current image" is the handle's last complete frame as mgs_frame_download would return it (after lighting and temporal
 * accumulation), read AS STORED in its target format (fp16 / fp32 / UNORM8 -> float).  A frame is complete after mgs_render of the
 * whole frame or after mgs_render_gathered; after a strip-only mgs_render the buffer holds only some rows: MGS_ERR_STATE. */
enum { MGS_FLIP_DISABLED = 0, MGS_FLIP_APPROX = 1, MGS_FLIP_REFERENCE = 2 };   /* FLIPMode, image_compare_shaderio.h:52-57 */
enum { MGS_COMPARE_SHOW_CAPTURE = 0, MGS_COMPARE_SHOW_CURRENT = 1, MGS_COMPARE_SHOW_DIFF_RAW = 2, MGS_COMPARE_SHOW_DIFF_RED_GRAY = 3,
       MGS_COMPARE_SHOW_DIFF_RED_ONLY = 4, MGS_COMPARE_SHOW_FLIP = 5 };          /* DisplayMode, image_compare_shaderio.h:37-45 */
/* ImageCompare::capture (image_compare.cpp:145-223): device-to-device copy of the last complete frame into an image the handle
 * owns, ordered on the handle's stream; the copy keeps the frame's size and target format.  MGS_ERR_STATE before any frame and
 * after a strip-only frame. */
int  mgs_compare_capture(MgsScene scene_or_context);
/* a capture made elsewhere (a reference screenshot, another build's frame): [height][width][4] float32, kept as RGBA32F */
int  mgs_compare_capture_upload(MgsScene scene_or_context, const float* rgba_host, int width, int height);
int  mgs_compare_release(MgsScene scene_or_context); /* releaseCaptureImage; valid without a capture */
typedef struct MgsCompareParams {
  int32_t flip_mode;          /* MGS_FLIP_*, default MGS_FLIP_REFERENCE (PushConstantMetrics, image_compare_shaderio.h:105-112) */
  float   pixels_per_degree;  /* default 67: the reference's hard-coded value with its TODO (image_compare.cpp:785-788) */
} MgsCompareParams;
void mgs_compare_params_default(MgsCompareParams* p);
typedef struct MgsCompareMetrics {
  /* as written: the shader's two uint32 sums (each pixel adds uint(contribution / N * 1e9), truncated), and what
   * collectMetricsResult derives from them (image_compare.cpp:869-906): float(sum) / 1e9f; PSNR 99.99 below 1e-10, else
   * min(10 log10(1 / mse), 99.99) in float; FLIP = float(pow(double(sum) / 1e9, 1/3)).  The truncation drops most of the signal at
   * real sizes (at 1920 x 1080 a pixel's contribution is below 1 for errors below about 0.05): compare with the exact fields.
   * Defined for images in [0,1]; outside that range the reference's sum can wrap and its float-to-uint conversion is undefined,
   * here a pixel's contribution saturates (negative or NaN: 0; too large: 0xFFFFFFFF) and the sum wraps. */
  uint32_t mse_fixed, flip_fixed;
  float    mse, psnr, flip;
  /* exact: the same per-pixel fp32 values without the truncation, summed in double — per-workgroup partials combined in a fixed
   * order, no floating-point atomics: two calls on the same images return the same bits.  mse_exact = sum / (W H 3), psnr_exact =
   * 10 log10(1 / mse_exact) (+inf for identical images), flip_exact = (sum of powered errors / (W H))^(1/3).  Defined for all
   * finite inputs. */
  double   mse_exact, psnr_exact, flip_exact;
  float    elapsed_ms;        /* HIP events around the metric launches */
  uint32_t reserved0;
} MgsCompareMetrics;
/* computeMetrics + readBackMetricsResult + collectMetricsResult (image_compare.cpp:735-924).  Runs on the handle's stream after its
 * last frame and waits.  Semantics, as written (image_compare_metric.comp.slang):
 *  - one value per pixel of the CAPTURE.  The current image is read by Load when the sizes are equal and sampled bilinearly at
 *    (p + 0.5) / captureSize otherwise (:96-110).  The sampler is nvvk's pool default and nvpro_core2 is not part of the reference
 *    tree: clamp-to-edge with fp32 weights is chosen here, PARITY UNPINNED.  Loads outside an image (approx mode on a smaller
 *    current image) return 0, the robust-access rule; likewise unpinned.
 *  - MSE over RGB only, divider float(W * H * 3) (:117-130, image_compare.cpp:783).
 *  - MGS_FLIP_APPROX (:371-477): YCxCz colour error with the CSF at 1 cycle per degree (both images loaded at the capture's
 *    coordinate), 3 x 3 Sobel on Rec.709 luminance with zero feature on the one-pixel border of each image's own size, CSF at 4 cpd,
 *    weight 3.83, pow(saturate(e), 3).
 *  - MGS_FLIP_REFERENCE (:198-304, :486-541): sigma = max(ppd / (f * 6.28), 0.5) for f = 0.5, 1, 2, 4, 8; r = ceil(3 sigma); a pixel
 *    within r of any border takes its centre luminance as the blurred value (feature 0), otherwise the normalised Gaussian mean of
 *    the luminance; feature = |centre - blurred| * csfLuminance(f); on a current image of another size the feature is taken at
 *    int(uv * currentSize); error = colour error + sum |feature difference|, saturated and cubed.  The shader's (2r+1)^2 loop is
 *    evaluated as a row pass and a column pass (the weights are a product of two 1-D Gaussians and interior pixels never clamp),
 *    normalised by the square of the 1-D weight sum: the same value up to fp32 rounding.  Radii above 96 (pixels_per_degree above
 *    100) are not held by this build: MGS_ERR_UNSUPPORTED.
 * MGS_ERR_STATE without a capture, before a frame, after a strip-only frame. */
int  mgs_compare_metrics(MgsScene scene_or_context, const MgsCompareParams* params, MgsCompareMetrics* out);
typedef struct MgsCompareView {
  float   split_position;     /* default 0.5 (PushConstantComparison, image_compare_shaderio.h:93-102) */
  int32_t left, right;        /* MGS_COMPARE_SHOW_*, default capture | current */
  float   difference_amplify; /* default 5.0 */
  int32_t width, height;      /* output size; 0 = the current frame's */
} MgsCompareView;
void mgs_compare_view_default(MgsCompareView* v);
/* ImageCompare::render's composite dispatch (image_compare.cpp:690-733, image_compare_composite.comp.slang:44-267): splitPos =
 * int(split * width), a 5-pixel divider with a 1-pixel white centre, the side's display mode elsewhere; sampleImage loads when that
 * image's size equals the output's and samples bilinearly (the sampler above) otherwise; the heat map is the composite shader's own
 * computeFLIP (:186-254: sRGB -> opponent colour, three-scale contrast at the output pixel's coordinate, pow(., 0.75), Turbo colour
 * map) — a different formula from the metric's.  The output is [height][width][4] float32 in a buffer the handle owns, valid until
 * the next call; *device_out / *bytes (either may be NULL) receive it.  Ordered on the handle's stream, does not wait. */
int  mgs_compare_composite(MgsScene scene_or_context, const MgsCompareView* view, void** device_out, uint64_t* bytes);
/* copies the last composite to the host and waits */
int  mgs_compare_download_composite(MgsScene scene_or_context, void* host_dst, size_t bytes);

/* test/debug hook (no reference counterpart: these are the mesh shader's per-quad outputs,
 * threedgs_raster.mesh.slang:243-289, which the reference never stores): the projected records the last full frame
 * built for the given global splat ids (caller's id space; meaningful only for ids that frame sorted, see
 * mgs_sort_download).  out10[i] = { centre_px.x, centre_px.y, basisVector1.xy, basisVector2.xy (pixels),
 * opacity (after MS antialiasing), conservative half extents x/y of the visible footprint (pixels), 0 };
 * rect_out[i] (may be NULL) = the footprint's bin rectangle x0 | y0<<8 | x1<<16 | y1<<24. */
int mgs_frame_download_projected(MgsScene scene, const uint32_t* global_ids, size_t count, float* out10, uint32_t* rect_out);
/* the same hook for a 3DGUT frame (MGS_HAS_PROJECTED_GUT; threedgut_raster.mesh.slang:111-254, whose per-quad outputs the
 * reference never stores either): out24[i] = the record the 3DGUT front end built for the id, as the compositors read it:
 * { centre_px.x, centre_px.y (the unscented mean), q1.xy, q2.xy (quad half axis h / |h|^2, 1 / pixels: the pixel centre c + d is
 * inside the quad where |d.q1| <= 1 and |d.q2| <= 1), half extents x/y of the quad's bounding box (pixels, culling only),
 * B[9] (row-major 3x3: canonical ray direction ~ B * world direction, B = S^-1 R^T * (M^-1)3x3), ro[3] (canonical ray origin of
 * the camera), r, g, b (0: the compositors shade), opacity (after MS antialiasing) }; rect_out as above.  Valid after a full
 * 3DGUT frame only (MGS_ERR_STATE otherwise); meaningful only for ids that frame sorted. */
int mgs_frame_download_projected_gut(MgsScene scene, const uint32_t* global_ids, size_t count, float* out24, uint32_t* rect_out);
/* test/debug hook (MGS_HAS_DEBUG_HIERARCHY; no reference counterpart: the reference's acceleration structures are opaque): the
 * scene's device-built hierarchy as the last build left it.  which 0: the splat hierarchy of the traced entry points (k_bvh.hip),
 * which 1: the triangle hierarchy of the mesh ray queries and of traced frames with meshes (k_mesh_bvh.hip).  An implicit complete
 * 8-ary tree: level 0 holds the leaves in Morton order, level l + 1 has ceil(level_count[l] / 8) nodes, node i of it is the union of
 * the nodes [8i, 8i + 8) below; the levels lie one after the other from level_offset[l], the last one is the root.
 * nodes8[i] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w } as raw bits.  lo.w of a leaf (read as uint32): which 0 the splat's
 * global storage id (instances concatenated in creation order, the index inside a set in storage order: mgs_scene_storage_order),
 * which 1 the leaf's own index; every other .w is 0.  tris12[i] (which 1 only) = the record of leaf i: vertex 0 xyz, global primitive
 * id, vertex 1 xyz, mesh instance, vertex 2 xyz, material id (the ids read as uint32).  primitives = the splats / triangles the
 * build looked at; box_lo, box_inv_ext = the frame in which the leaves' Morton codes were quantised.
 * Waits for the handle's stream; starts no build, changes nothing the next frame or query sees and allocates no device memory.
 * MGS_ERR_STATE when no such hierarchy has been built yet; which outside 0 / 1, NULL info: MGS_ERR_INVALID_ARG.  nodes8 / tris12
 * NULL: not copied (info alone, to size the buffers); not NULL with node_capacity < total_nodes / tri_capacity < leaves (counted in
 * nodes and records): MGS_ERR_INVALID_ARG, nothing written. */
typedef struct MgsHierarchyInfo {
  uint32_t levels, total_nodes, leaves, primitives;
  uint32_t level_offset[11], level_count[11];
  float    box_lo[3], box_inv_ext[3];
} MgsHierarchyInfo;
int mgs_debug_download_hierarchy(MgsScene scene_or_context, int which, MgsHierarchyInfo* info, float* nodes8, size_t node_capacity,
                                 float* tris12, size_t tri_capacity);
int mgs_sync(MgsScene scene);

/* ---- sort only (metric hook): vrdxCmdSortKeyValueIndirect (3rdparty/vrdx/include/vk_radix_sort.h:73-78)
 * fed by dist.comp.slang, or SplatSorterAsync::sortAsync/consume (src/splat_sorter_async.h:84-128)
 * when params->sort_mode == MGS_SORT_CPU_ASYNC. */
typedef struct MgsSortOut {
  uint32_t count;      /* number of sorted elements (visible count) */
  float    key_ms;     /* dist stage */
  float    sort_ms;    /* radix sort (GPU) / std::sort (CPU) */
  float    hist_ms;    /* GPU: the up-front histogram kernel, included in sort_ms */
  uint32_t passes;     /* GPU: radix passes executed */
  uint32_t reserved[3]; /* [0] 1: pass 2 sorted on the rank of key >> 16 and pass 3 did not run; [1] occurring values of key >> 16 */
} MgsSortOut;
int mgs_sort_keys(MgsScene scene, const MgsFrameParams* params, MgsSortOut* out);
/* download the sorted keys (GPU mode: u32 encodeMinMaxFp32 keys; CPU mode: fp32 distances) and global ids.  `keys` may be
 * NULL.  In GPU mode the sorted keys exist after mgs_sort_keys only (a frame's last sort pass writes the ids alone, as the
 * raster stage reads nothing else): asking for them after mgs_render returns MGS_ERR_STATE. */
int mgs_sort_download(MgsScene scene, uint32_t* keys, uint32_t* ids, uint32_t capacity);

/* sort an arbitrary device-resident (key,value) u32 array (LSD radix): the full key width on the frame's single-kernel pass
 * sort (k_osort_pass.hip), partial bit ranges on the generic sort (k_sort.hip)
 * (keys_device/values_device are overwritten with the result) — used by the sort parity tests
 * and the sorted-Gsplats/s microbenchmark. */
int mgs_radix_sort_u32(MgsScene scene, void* keys_device, void* values_device, uint32_t count,
                       int begin_bit, int end_bit, float* elapsed_ms);
/* host convenience for the above: uploads, sorts, downloads */
int mgs_radix_sort_host(MgsScene scene, uint32_t* keys, uint32_t* values, uint32_t count,
                        int begin_bit, int end_bit, float* elapsed_ms);

/* ---- camera helper (BUILD-DEFINED: nvutils::CameraManipulator lives in the absent nvpro_core2;
 * SURVEY.md §8c "parity unpinned").  Right-handed lookAt + perspective with clip z in [0,1];
 * flip_y != 0 negates proj[5] (Vulkan convention).  Defaults mirror src/camera_set.h:48-53. */
void mgs_camera_lookat_perspective(const float eye[3], const float center[3], const float up[3],
                                   float fov_y_degrees, float z_near, float z_far,
                                   int width, int height, int flip_y,
                                   float view_out[16], float proj_out[16]);
/* T*R*S instance transform, computeTransform (src/utilities.h:170-199); rotation = Euler degrees */
void mgs_compute_transform(const float scale[3], const float rotation_deg[3], const float translation[3],
                           float transform_out[16], float inverse_out[16]);

#ifdef __cplusplus
}
#endif
#endif /* MGS_H */
