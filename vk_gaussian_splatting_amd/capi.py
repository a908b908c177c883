"""ctypes mirror of include/mgs.h (the C ABI of csrc/libmgs.so).

Names, argument meaning and error behaviour follow the header one to one; see the header for
the reference interface (file:line) each entry point replaces.
"""
import ctypes as C
import os
import numpy as np

FORMAT_FLOAT32, FORMAT_FLOAT16, FORMAT_UINT8 = 0, 1, 2
SORT_GPU_RADIX, SORT_CPU_ASYNC, SORT_STOCHASTIC = 0, 1, 3
DOF_DISABLED, DOF_FIXED_FOCUS = 0, 1
CULL_NONE, CULL_AT_DIST, CULL_AT_RASTER = 0, 1, 2
TARGET_RGBA16F, TARGET_RGBA32F, TARGET_RGBA8 = 0, 1, 2
ALPHA_COVERAGE, ALPHA_SUM = 0, 1
DEBUG_POINT_CLOUD, DEBUG_SH_ONLY, DEBUG_OPACITY_GAUSSIAN_DISABLED = 1, 2, 4
PIPELINE_3DGS, PIPELINE_3DGUT = 0, 1
NORMAL_MAX_DENSITY_PLANE, NORMAL_ISO_SURFACE = 0, 1
CAMERA_PINHOLE, CAMERA_FISHEYE = 0, 1
EXTENT_EIGEN, EXTENT_CONIC = 0, 1
LIGHTING_DISABLED, LIGHTING_DIRECT, LIGHTING_INDIRECT = 0, 1, 2
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2
MAX_LIGHTS = 64
STAGE_LIGHT = 7  # index into timings_all(): the deferred lighting pass
FLIP_DISABLED, FLIP_APPROX, FLIP_REFERENCE = 0, 1, 2  # FLIPMode
# DisplayMode of the split view, by value and by the names tools/mgs_render.py accepts
SHOW_CAPTURE, SHOW_CURRENT, SHOW_DIFF_RAW, SHOW_DIFF_RED_GRAY, SHOW_DIFF_RED_ONLY, SHOW_FLIP = 0, 1, 2, 3, 4, 5
SHOW_NAMES = {"capture": 0, "current": 1, "diff-raw": 2, "diff-red-gray": 3, "diff-red-only": 4, "flip": 5}
STAGE_NAMES = ["project", "sort", "bin", "pairsort", "composite", "total"]


# status codes of include/mgs.h
OK, ERR_INVALID_ARG, ERR_IO, ERR_FORMAT, ERR_DEVICE, ERR_OOM, ERR_STATE, ERR_OVERFLOW, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7, -8


class MgsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mgs error {code}: {msg}")
        self.code = code


class SplatSetView(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("f_dc", C.POINTER(C.c_float)),
                ("f_rest", C.POINTER(C.c_float)), ("opacity", C.POINTER(C.c_float)),
                ("scale", C.POINTER(C.c_float)), ("rotation", C.POINTER(C.c_float)),
                ("splat_count", C.c_uint64), ("f_rest_per_splat", C.c_uint32), ("sh_degree", C.c_int32)]


class FrameParams(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("camera_pos", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32),
                ("splat_scale", C.c_float), ("frustum_dilation", C.c_float), ("alpha_cull_threshold", C.c_float),
                ("sh_degree", C.c_int32), ("sort_mode", C.c_int32), ("frustum_culling", C.c_int32),
                ("target_format", C.c_int32), ("alpha_mode", C.c_int32), ("ms_antialiasing", C.c_int32),
                ("strip_row_begin", C.c_int32), ("strip_row_end", C.c_int32),
                ("collect_timings", C.c_int32), ("cpu_sort_blocking", C.c_int32), ("debug_flags", C.c_int32),
                ("size_culling", C.c_int32), ("size_culling_min_pixels", C.c_float),
                ("surface_outputs", C.c_int32), ("depth_iso_threshold", C.c_float), ("cpu_lazy_sort", C.c_int32),
                ("thin_particle_threshold", C.c_float), ("quantize_normals", C.c_int32),
                ("pipeline", C.c_int32), ("camera_model", C.c_int32), ("extent_method", C.c_int32), ("fov_rad", C.c_float),
                ("alpha_clamp", C.c_float), ("kernel_min_response", C.c_float),
                ("dof_mode", C.c_int32), ("focus_dist", C.c_float), ("aperture", C.c_float),
                ("frame_sample_id", C.c_int32), ("temporal_sampling", C.c_int32), ("kernel_degree", C.c_int32),
                ("normal_method", C.c_int32), ("lighting_mode", C.c_int32)]


class Light(C.Structure):
    """MgsLight: shaderio::LightSource; angles in degrees.  The soft-shadow radius is not a field of the C struct: make_light(radius=R)
    keeps it as a Python attribute, which Scene.set_lights hands to mgs_scene_set_light_radii"""
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("intensity", C.c_float), ("position", C.c_float * 3),
                ("range", C.c_float), ("direction", C.c_float * 3), ("inner_cone_deg", C.c_float), ("outer_cone_deg", C.c_float),
                ("attenuation_mode", C.c_int32)]


class Material(C.Structure):
    """MgsMaterial: an instance's splatMaterial as the deferred pass reads it"""
    _fields_ = [("ambient", C.c_float * 3), ("diffuse", C.c_float * 3), ("specular", C.c_float * 3), ("emission", C.c_float * 3),
                ("shininess", C.c_float)]


def make_light(**kw):
    """an MgsLight with the reference's defaults (mgs_light_default), fields overridden by keyword; radius = the soft-shadow radius
    (LightSource::radius, default 1.0), carried beside the struct for Scene.set_lights"""
    l = Light()
    load_library().mgs_light_default(C.byref(l))
    for k, v in kw.items():
        if k == "radius":
            l.radius = float(v)
            continue
        if k not in dict(Light._fields_):
            raise TypeError(f"make_light: unknown field {k}")
        if k in ("color", "position", "direction"):
            setattr(l, k, (C.c_float * 3)(*[float(x) for x in v]))
        else:
            setattr(l, k, v)
    return l


def make_material(**kw):
    """an MgsMaterial with the splat sets' default (mgs_material_default: emission 1, everything else 0), fields overridden"""
    m = Material()
    load_library().mgs_material_default(C.byref(m))
    for k, v in kw.items():
        if k not in dict(Material._fields_):
            raise TypeError(f"make_material: unknown field {k}")
        if k == "shininess":
            m.shininess = float(v)
        else:
            setattr(m, k, (C.c_float * 3)(*[float(x) for x in v]))
    return m


class MeshView(C.Structure):
    """MgsMeshView: indexed triangles in the RUB frame"""
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_uint32)),
                ("material_ids", C.POINTER(C.c_uint32)), ("materials", C.POINTER(Material)),
                ("vertex_count", C.c_uint64), ("index_count", C.c_uint64), ("material_count", C.c_uint32)]


MESH_WORK_LIST_FULL = 1


class MeshOut(C.Structure):
    """MgsMeshOut: counters and device time of one mesh pass; flags & MESH_WORK_LIST_FULL: exact images, slow pass"""
    _fields_ = [("triangles_in", C.c_uint64), ("triangles_rasterised", C.c_uint64), ("fragments", C.c_uint64),
                ("elapsed_ms", C.c_float), ("flags", C.c_uint32)]


class TraceParams(C.Structure):
    """MgsTraceParams: the knobs of the traced pipeline that MgsFrameParams has no room for"""
    _fields_ = [("samples_per_pass", C.c_int32), ("max_passes", C.c_int32), ("min_transmittance", C.c_float),
                ("kernel_adaptive_clamping", C.c_int32), ("depth_iso_threshold", C.c_float), ("trace_strategy", C.c_int32),
                ("reserved", C.c_uint32 * 2)]


# MgsTraceStrategy (MgsTraceParams::trace_strategy)
TRACE_STRATEGY_FULL_ANYHIT, TRACE_STRATEGY_PASS_STOCHASTIC, TRACE_STRATEGY_STOCHASTIC_ANYHIT = 0, 1, 2


class TraceLightParams(C.Structure):
    """MgsTraceLightParams: the shadow rays of a lit traced frame (mgs_render_traced_lit)"""
    _fields_ = [("shadows_mode", C.c_int32), ("particle_shadow_offset", C.c_float), ("particle_shadow_transmittance_threshold", C.c_float),
                ("particle_shadow_color_strength", C.c_float), ("reserved", C.c_uint32 * 4)]


class TraceLightOut(C.Structure):
    """MgsTraceLightOut: the shadow rays' counters and the light pass's device time of one lit traced frame"""
    _fields_ = [("shadow_rays", C.c_uint64), ("shadow_node_visits", C.c_uint64), ("shadow_candidate_tests", C.c_uint64),
                ("shadow_accepted_hits", C.c_uint64), ("light_ms", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class TraceOut(C.Structure):
    """MgsTraceOut: the hierarchy's size, the traversal's counters and the device times of one traced frame"""
    _fields_ = [("leaves", C.c_uint64), ("nodes", C.c_uint64), ("node_visits", C.c_uint64), ("candidate_tests", C.c_uint64),
                ("accepted_hits", C.c_uint64), ("max_passes_used", C.c_uint32), ("bvh_rebuilt", C.c_uint32),
                ("build_ms", C.c_float), ("trace_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Ray(C.Structure):
    """MgsRay: origin, t_min, direction, t_max (32 bytes; RAY_DTYPE is the same layout for numpy)"""
    _fields_ = [("origin", C.c_float * 3), ("t_min", C.c_float), ("direction", C.c_float * 3), ("t_max", C.c_float)]


class RayResult(C.Structure):
    """MgsRayResult (48 bytes; RAY_RESULT_DTYPE is the same layout for numpy)"""
    _fields_ = [("radiance", C.c_float * 3), ("transmittance", C.c_float), ("t_iso", C.c_float), ("id", C.c_uint32),
                ("hit_count", C.c_uint32), ("passes", C.c_uint32), ("normal", C.c_float * 4)]


class RayQueryParams(C.Structure):
    """MgsRayQueryParams"""
    _fields_ = [("reorder", C.c_int32), ("reserved", C.c_uint32 * 3)]


class RayQueryOut(C.Structure):
    """MgsRayQueryOut: MgsTraceOut of the batch, the device time of the reorder and the number of refused rays"""
    _fields_ = [("trace", TraceOut), ("reorder_ms", C.c_float), ("invalid_rays", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return dict(self.trace.as_dict(), reorder_ms=self.reorder_ms, invalid_rays=self.invalid_rays)


class ShadowResult(C.Structure):
    """MgsShadowResult (16 bytes; SHADOW_RESULT_DTYPE is the same layout for numpy)"""
    _fields_ = [("transmittance", C.c_float * 3), ("hits", C.c_uint32)]


class SurfacePoint(C.Structure):
    """MgsSurfacePoint (64 bytes; SURFACE_POINT_DTYPE is the same layout for numpy)"""
    _fields_ = [("position", C.c_float * 3), ("material", C.c_uint32), ("normal", C.c_float * 3), ("_pad0", C.c_float),
                ("view_dir", C.c_float * 3), ("_pad1", C.c_float), ("radiance", C.c_float * 3), ("_pad2", C.c_float)]


class ShadeResult(C.Structure):
    """MgsShadeResult (16 bytes; SHADE_RESULT_DTYPE is the same layout for numpy)"""
    _fields_ = [("color", C.c_float * 3), ("shadow_hits", C.c_uint32)]


# MgsMeshRayMode (MgsMeshRayParams::mode)
MESH_RAYS_CLOSEST, MESH_RAYS_OCCLUSION = 0, 1


class MeshHit(C.Structure):
    """MgsMeshHit (64 bytes; MESH_HIT_DTYPE is the same layout for numpy)"""
    _fields_ = [("t", C.c_float), ("instance_id", C.c_uint32), ("primitive_id", C.c_uint32), ("material_id", C.c_uint32),
                ("position", C.c_float * 3), ("b1", C.c_float), ("normal", C.c_float * 3), ("b2", C.c_float),
                ("hit", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class MeshRayParams(C.Structure):
    """MgsMeshRayParams"""
    _fields_ = [("mode", C.c_int32), ("reorder", C.c_int32), ("reserved", C.c_uint32 * 2)]


class MeshRayOut(C.Structure):
    """MgsMeshRayOut: the triangle hierarchy's size, the batch's integer sums and the device times of one mesh ray query"""
    _fields_ = [("triangles", C.c_uint64), ("leaves", C.c_uint64), ("nodes", C.c_uint64), ("node_visits", C.c_uint64),
                ("triangle_tests", C.c_uint64), ("hits", C.c_uint64), ("invalid_rays", C.c_uint32), ("bvh_rebuilt", C.c_uint32),
                ("build_ms", C.c_float), ("trace_ms", C.c_float), ("reorder_ms", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


MESH_HIT_DTYPE = np.dtype([("t", np.float32), ("instance_id", np.uint32), ("primitive_id", np.uint32), ("material_id", np.uint32),
                           ("position", np.float32, 3), ("b1", np.float32), ("normal", np.float32, 3), ("b2", np.float32),
                           ("hit", np.uint32), ("reserved", np.uint32, 3)])


class HierarchyInfo(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("total_nodes", C.c_uint32), ("leaves", C.c_uint32), ("primitives", C.c_uint32),
                ("level_offset", C.c_uint32 * 11), ("level_count", C.c_uint32 * 11), ("box_lo", C.c_float * 3), ("box_inv_ext", C.c_float * 3)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("levels", "total_nodes", "leaves", "primitives")}
        d.update(level_offset=np.array(self.level_offset, np.uint32), level_count=np.array(self.level_count, np.uint32),
                 box_lo=np.array(self.box_lo, np.float32), box_inv_ext=np.array(self.box_inv_ext, np.float32))
        return d


class TraceMeshParams(C.Structure):
    """MgsTraceMeshParams (16 bytes): mesh hits in the traced frames (mgs_frame_set_trace_meshes)"""
    _fields_ = [("enabled", C.c_int32), ("min_mesh_composite_transmittance", C.c_float), ("reserved", C.c_uint32 * 2)]


class BounceMaterial(C.Structure):
    """MgsBounceMaterial (32 bytes): what a mesh material says about bounces (mgs_mesh_instance_set_bounce_materials)"""
    _fields_ = [("transmittance", C.c_float * 3), ("ior", C.c_float), ("illum", C.c_int32), ("reserved", C.c_uint32 * 3)]


class TraceBounceParams(C.Structure):
    """MgsTraceBounceParams (16 bytes): the bounces of an indirect traced frame (mgs_render_traced_indirect)"""
    _fields_ = [("max_bounces", C.c_int32), ("reserved", C.c_uint32 * 3)]


class TraceBounceOut(C.Structure):
    """MgsTraceBounceOut: per bounce the live pixels and their mesh hits, the particle hits of all bounces, the bounces' device time"""
    _fields_ = [("rays", C.c_uint64 * 16), ("mesh_hits", C.c_uint64 * 16), ("particle_hits", C.c_uint64), ("bounce_ms", C.c_float),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return dict(rays=list(self.rays), mesh_hits=list(self.mesh_hits), particle_hits=self.particle_hits, bounce_ms=self.bounce_ms)


def bounce_material(transmittance=(0.0, 0.0, 0.0), ior=1.0, illum=0):
    """a BounceMaterial from its three fields (illum: the derived model 0 / 1 / >= 2)"""
    m = BounceMaterial()
    load_library().mgs_bounce_material_default(C.byref(m))
    m.transmittance[:] = [float(v) for v in transmittance]
    m.ior, m.illum = float(ior), int(illum)
    return m


def bounce_material_from_mtl(tf, ni, mtl_illum):
    """mgs_bounce_material_from_mtl: the loader's rule (src/obj_loader.cpp:50-59) for a material's Tf, Ni and illum statements"""
    m = BounceMaterial()
    load_library().mgs_bounce_material_from_mtl((C.c_float * 3)(*[float(v) for v in tf]), float(ni), int(mtl_illum), C.byref(m))
    return m


SENSOR_OPENCV_PINHOLE, SENSOR_OPENCV_FISHEYE = 0, 1


class SensorModel(C.Structure):
    """MgsSensorModel (128 bytes): the OpenCV pinhole / fisheye camera of the 3DGUT pipeline with its distortion coefficients"""
    _fields_ = [("model", C.c_int32), ("shutter", C.c_int32), ("focal_length", C.c_float * 2), ("principal_point", C.c_float * 2),
                ("radial", C.c_float * 6), ("tangential", C.c_float * 2), ("thin_prism", C.c_float * 4), ("fisheye_radial", C.c_float * 4),
                ("max_angle", C.c_float), ("reserved", C.c_uint32 * 9)]

    FIELDS = ("model", "shutter", "focal_length", "principal_point", "radial", "tangential", "thin_prism", "fisheye_radial", "max_angle")

    def as_dict(self):
        return {k: (getattr(self, k) if k in ("model", "shutter", "max_angle") else list(getattr(self, k))) for k in self.FIELDS}

    def update(self, **fields):
        """set fields by name (scalars, or sequences of the field's length); returns self"""
        for k, v in fields.items():
            if k not in self.FIELDS:
                raise KeyError(k)
            if k in ("model", "shutter"):
                setattr(self, k, int(v))
            elif k == "max_angle":
                self.max_angle = float(v)
            else:
                arr = getattr(self, k)
                v = [float(x) for x in v]
                if len(v) != len(arr):
                    raise ValueError(f"{k}: {len(arr)} values expected")
                for i, x in enumerate(v):
                    arr[i] = x
        return self


def sensor_model_from_frame(params):
    """mgs_sensor_model_from_frame: the perfect model the frame uses without a sensor; start from it and perturb"""
    m = SensorModel()
    _check(load_library().mgs_sensor_model_from_frame(C.byref(params), C.byref(m)))
    return m


RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("direction", np.float32, 3), ("t_max", np.float32)])
RAY_RESULT_DTYPE = np.dtype([("radiance", np.float32, 3), ("transmittance", np.float32), ("t_iso", np.float32), ("id", np.uint32),
                             ("hit_count", np.uint32), ("passes", np.uint32), ("normal", np.float32, 4)])


SHADOW_RESULT_DTYPE = np.dtype([("transmittance", np.float32, 3), ("hits", np.uint32)])
SURFACE_POINT_DTYPE = np.dtype([("position", np.float32, 3), ("material", np.uint32), ("normal", np.float32, 3), ("_pad0", np.float32),
                                ("view_dir", np.float32, 3), ("_pad1", np.float32), ("radiance", np.float32, 3), ("_pad2", np.float32)])
SHADE_RESULT_DTYPE = np.dtype([("color", np.float32, 3), ("shadow_hits", np.uint32)])


def make_surface_points(position, normal, view_dir, radiance, material=0):
    """a SURFACE_POINT_DTYPE array from positions, normals, view directions and radiances [n,3] and material indices (scalar or [n])"""
    o = np.asarray(position, np.float32).reshape(-1, 3)
    r = np.zeros(o.shape[0], SURFACE_POINT_DTYPE)
    r["position"], r["normal"] = o, np.asarray(normal, np.float32).reshape(-1, 3)
    r["view_dir"], r["radiance"] = np.asarray(view_dir, np.float32).reshape(-1, 3), np.asarray(radiance, np.float32).reshape(-1, 3)
    r["material"] = material
    return r


def make_rays(origin, direction, t_min=0.001, t_max=10000.0):
    """a RAY_DTYPE array from origins [n,3], directions [n,3] and windows (scalars or [n])"""
    o = np.asarray(origin, np.float32).reshape(-1, 3)
    r = np.zeros(o.shape[0], RAY_DTYPE)
    r["origin"], r["direction"] = o, np.asarray(direction, np.float32).reshape(-1, 3)
    r["t_min"], r["t_max"] = t_min, t_max
    return r


class CompareParams(C.Structure):
    """MgsCompareParams"""
    _fields_ = [("flip_mode", C.c_int32), ("pixels_per_degree", C.c_float)]


class CompareMetrics(C.Structure):
    """MgsCompareMetrics: the reference's fixed-point sums and what it derives from them, the exact values, the device time"""
    _fields_ = [("mse_fixed", C.c_uint32), ("flip_fixed", C.c_uint32), ("mse", C.c_float), ("psnr", C.c_float), ("flip", C.c_float),
                ("mse_exact", C.c_double), ("psnr_exact", C.c_double), ("flip_exact", C.c_double),
                ("elapsed_ms", C.c_float), ("reserved0", C.c_uint32)]

    def __repr__(self):
        return (f"CompareMetrics(mse={self.mse:.6g}, psnr={self.psnr:.2f}, flip={self.flip:.5f}, mse_exact={self.mse_exact:.6g}, "
                f"psnr_exact={self.psnr_exact:.2f}, flip_exact={self.flip_exact:.5f}, elapsed_ms={self.elapsed_ms:.3f})")


class CompareView(C.Structure):
    """MgsCompareView"""
    _fields_ = [("split_position", C.c_float), ("left", C.c_int32), ("right", C.c_int32), ("difference_amplify", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32)]


class FrameOut(C.Structure):
    _fields_ = [("rgba_device", C.c_void_p), ("rgba_bytes", C.c_uint64),
                ("frustum_count", C.c_uint32), ("sorted_count", C.c_uint32), ("tile_pairs", C.c_uint64),
                ("error_flags", C.c_uint32), ("shaded_count", C.c_uint32), ("scanned_entries", C.c_uint64),
                ("stage_ms", C.c_float * 8), ("escape_count", C.c_uint32), ("reserved0", C.c_uint32)]


class SortOut(C.Structure):
    _fields_ = [("count", C.c_uint32), ("key_ms", C.c_float), ("sort_ms", C.c_float), ("hist_ms", C.c_float),
                ("passes", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def lib_path():
    if os.environ.get("MGS_LIB"):  # experiments: a variant build of the same library (tools/build_variant.sh); never a fallback
        return os.path.abspath(os.environ["MGS_LIB"])
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmgs.so")


_lib = None


def load_library():
    """Load csrc/libmgs.so.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MgsError(-4, f"{path} is missing — run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback for the MI355X path")
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Load torch first so that this
    # process ends up with exactly ONE HIP runtime, whichever library asks for it later.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    F, P = C.c_float, C.POINTER
    vp = C.c_void_p
    sig = {
        "mgs_last_error": (C.c_char_p, []),
        "mgs_version": (C.c_char_p, []),
        "mgs_splatset_load": (C.c_int, [C.c_char_p, P(vp)]),
        "mgs_splatset_from_arrays": (C.c_int, [P(SplatSetView), P(vp)]),
        "mgs_splatset_view": (C.c_int, [vp, P(SplatSetView)]),
        "mgs_splatset_destroy": (None, [vp]),
        "mgs_scene_create": (C.c_int, [C.c_int, P(vp)]),
        "mgs_scene_destroy": (None, [vp]),
        "mgs_scene_set_stream": (C.c_int, [vp, vp]),
        "mgs_instance_add": (C.c_int, [vp, vp, P(F), P(C.c_int)]),
        "mgs_instance_set_transform": (C.c_int, [vp, C.c_int, P(F)]),
        "mgs_scene_commit": (C.c_int, [vp, C.c_int, C.c_int]),
        "mgs_light_default": (None, [P(Light)]),
        "mgs_material_default": (None, [P(Material)]),
        "mgs_scene_set_lights": (C.c_int, [vp, P(Light), C.c_int]),
        "mgs_scene_set_light_radii": (C.c_int, [vp, P(C.c_float), C.c_int]),
        "mgs_instance_set_material": (C.c_int, [vp, C.c_int, P(Material)]),
        "mgs_scene_splat_count": (C.c_uint64, [vp]),
        "mgs_compare_capture": (C.c_int, [vp]),
        "mgs_compare_capture_upload": (C.c_int, [vp, P(F), C.c_int, C.c_int]),
        "mgs_compare_release": (C.c_int, [vp]),
        "mgs_compare_params_default": (None, [P(CompareParams)]),
        "mgs_compare_metrics": (C.c_int, [vp, P(CompareParams), P(CompareMetrics)]),
        "mgs_compare_view_default": (None, [P(CompareView)]),
        "mgs_compare_composite": (C.c_int, [vp, P(CompareView), P(vp), P(C.c_uint64)]),
        "mgs_compare_download_composite": (C.c_int, [vp, vp, C.c_size_t]),
        "mgs_mesh_from_arrays": (C.c_int, [P(MeshView), P(vp)]),
        "mgs_mesh_load_obj": (C.c_int, [C.c_char_p, P(vp)]),
        "mgs_mesh_view": (C.c_int, [vp, P(MeshView)]),
        "mgs_mesh_destroy": (None, [vp]),
        "mgs_mesh_instance_add": (C.c_int, [vp, vp, P(F), P(C.c_int)]),
        "mgs_mesh_instance_set_transform": (C.c_int, [vp, C.c_int, P(F)]),
        "mgs_mesh_instance_set_visible": (C.c_int, [vp, C.c_int, C.c_int]),
        "mgs_meshes_render": (C.c_int, [vp, P(FrameParams), P(MeshOut)]),
        "mgs_meshes_download": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
        "mgs_trace_params_default": (None, [P(TraceParams)]),
        "mgs_render_traced": (C.c_int, [vp, P(FrameParams), P(TraceParams), P(TraceOut)]),
        "mgs_trace_download_hit_counts": (C.c_int, [vp, P(C.c_uint32), C.c_size_t]),
        "mgs_trace_light_params_default": (None, [P(TraceLightParams)]),
        "mgs_render_traced_lit": (C.c_int, [vp, P(FrameParams), P(TraceParams), P(TraceLightParams), P(TraceOut), P(TraceLightOut)]),
        "mgs_trace_download_shadow_hits": (C.c_int, [vp, P(C.c_uint32), C.c_size_t]),
        "mgs_ray_query_params_default": (None, [P(RayQueryParams)]),
        "mgs_trace_rays": (C.c_int, [vp, vp, C.c_uint64, P(FrameParams), P(TraceParams), P(RayQueryParams), vp, P(RayQueryOut)]),
        "mgs_trace_rays_device": (C.c_int, [vp, vp, C.c_uint64, P(FrameParams), P(TraceParams), P(RayQueryParams), vp, P(RayQueryOut)]),
        "mgs_trace_generate_rays": (C.c_int, [vp, P(FrameParams), vp]),
        "mgs_trace_shadow_rays": (C.c_int, [vp, vp, C.c_uint64, P(FrameParams), P(TraceParams), P(TraceLightParams), P(RayQueryParams), vp, P(RayQueryOut)]),
        "mgs_trace_shadow_rays_device": (C.c_int, [vp, vp, C.c_uint64, P(FrameParams), P(TraceParams), P(TraceLightParams), P(RayQueryParams), vp,
                                                   P(RayQueryOut)]),
        "mgs_shade_points": (C.c_int, [vp, vp, C.c_uint64, P(Material), C.c_uint32, P(FrameParams), P(TraceParams), P(TraceLightParams),
                                       P(RayQueryParams), vp, P(TraceLightOut), P(C.c_uint32)]),
        "mgs_shade_points_device": (C.c_int, [vp, vp, C.c_uint64, P(Material), C.c_uint32, P(FrameParams), P(TraceParams), P(TraceLightParams),
                                              P(RayQueryParams), vp, P(TraceLightOut), P(C.c_uint32)]),
        "mgs_mesh_ray_params_default": (None, [P(MeshRayParams)]),
        "mgs_trace_mesh_rays": (C.c_int, [vp, vp, C.c_uint64, P(MeshRayParams), vp, P(MeshRayOut)]),
        "mgs_trace_mesh_rays_device": (C.c_int, [vp, vp, C.c_uint64, P(MeshRayParams), vp, P(MeshRayOut)]),
        "mgs_trace_mesh_params_default": (None, [P(TraceMeshParams)]),
        "mgs_frame_set_trace_meshes": (C.c_int, [vp, P(TraceMeshParams)]),
        "mgs_frame_set_hybrid_meshes": (C.c_int, [vp, P(TraceMeshParams)]),
        "mgs_debug_download_hybrid_depth": (C.c_int, [vp, C.POINTER(C.c_float), C.c_size_t]),
        "mgs_trace_download_mesh_hits": (C.c_int, [vp, vp, C.c_size_t]),
        "mgs_trace_mesh_stats": (C.c_int, [vp, P(MeshRayOut), P(MeshRayOut)]),
        "mgs_bounce_material_default": (None, [P(BounceMaterial)]),
        "mgs_bounce_material_from_mtl": (None, [P(F), F, C.c_int, P(BounceMaterial)]),
        "mgs_mesh_bounce_materials": (C.c_int, [vp, P(BounceMaterial), C.c_uint32, P(C.c_uint32)]),
        "mgs_mesh_instance_set_bounce_materials": (C.c_int, [vp, C.c_int, P(BounceMaterial), C.c_uint32]),
        "mgs_trace_bounce_params_default": (None, [P(TraceBounceParams)]),
        "mgs_render_traced_indirect": (C.c_int, [vp, P(FrameParams), P(TraceParams), P(TraceLightParams), P(TraceBounceParams), P(TraceOut),
                                                 P(TraceLightOut), P(TraceBounceOut)]),
        "mgs_frame_context_create": (C.c_int, [vp, P(vp)]),
        "mgs_frame_context_destroy": (None, [vp]),
        "mgs_scene_memory_usage": (C.c_int, [vp, P(C.c_uint64), P(C.c_uint64)]),
        "mgs_scene_set_list_capacity": (C.c_int, [vp, C.c_uint64]),
        "mgs_frame_set_occluder": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
        "mgs_frame_upload_occluder": (C.c_int, [vp, P(F), P(F), C.c_int, C.c_int]),
        "mgs_sensor_model_from_frame": (C.c_int, [P(FrameParams), P(SensorModel)]),
        "mgs_frame_set_sensor": (C.c_int, [vp, P(SensorModel)]),
        "mgs_scene_download_set": (C.c_int, [vp, C.c_int, C.c_int, P(F), C.c_size_t]),
        "mgs_scene_storage_order": (C.c_int, [vp, C.c_int, P(C.c_uint32), C.c_size_t]),
        "mgs_frame_params_default": (None, [P(FrameParams)]),
        "mgs_render": (C.c_int, [vp, P(FrameParams), P(FrameOut)]),
        "mgs_render_hybrid": (C.c_int, [vp, P(FrameParams), P(TraceParams), P(TraceLightParams), P(FrameOut), P(TraceLightOut)]),
        "mgs_frame_stats": (C.c_int, [vp, P(FrameOut)]),
        "mgs_timings_query": (C.c_int, [vp, C.c_uint32, P(F)]),
        "mgs_frame_download": (C.c_int, [vp, vp, C.c_size_t]),
        "mgs_frame_download_surface": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
        "mgs_frame_copy_strip": (C.c_int, [vp, vp, C.c_size_t]),
        "mgs_sync": (C.c_int, [vp]),
        "mgs_frame_download_projected": (C.c_int, [vp, P(C.c_uint32), C.c_size_t, P(F), P(C.c_uint32)]),
        "mgs_frame_download_projected_gut": (C.c_int, [vp, P(C.c_uint32), C.c_size_t, P(F), P(C.c_uint32)]),
        "mgs_debug_download_hierarchy": (C.c_int, [vp, C.c_int, P(HierarchyInfo), P(F), C.c_size_t, P(F), C.c_size_t]),
        "mgs_loader_create": (C.c_int, [P(vp)]),
        "mgs_loader_destroy": (None, [vp]),
        "mgs_loader_push": (C.c_int, [vp, C.c_char_p]),
        "mgs_loader_status": (C.c_int, [vp, P(C.c_int), P(C.c_uint32), C.c_char_p, C.c_size_t]),
        "mgs_loader_take": (C.c_int, [vp, P(vp)]),
        "mgs_comm_unique_id": (C.c_int, [vp]),
        "mgs_scene_comm_init": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "mgs_scene_comm_destroy": (C.c_int, [vp]),
        "mgs_scene_set_strip_rows": (C.c_int, [vp, P(C.c_int32), C.c_int]),
        "mgs_render_gathered": (C.c_int, [vp, P(FrameParams), P(FrameOut)]),
        "mgs_frame_row_costs": (C.c_int, [vp, P(C.c_uint32), C.c_size_t]),
        "mgs_sort_keys": (C.c_int, [vp, P(FrameParams), P(SortOut)]),
        "mgs_sort_download": (C.c_int, [vp, P(C.c_uint32), P(C.c_uint32), C.c_uint32]),
        "mgs_radix_sort_u32": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, P(F)]),
        "mgs_radix_sort_host": (C.c_int, [vp, P(C.c_uint32), P(C.c_uint32), C.c_uint32, C.c_int, C.c_int, P(F)]),
        "mgs_camera_lookat_perspective": (None, [P(F), P(F), P(F), F, F, F, C.c_int, C.c_int, C.c_int, P(F), P(F)]),
        "mgs_compute_transform": (None, [P(F), P(F), P(F), P(F), P(F)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here == the library does not export what mgs.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "mgs_last_error", "mgs_version", "mgs_splatset_load", "mgs_splatset_from_arrays", "mgs_splatset_view",
    "mgs_splatset_destroy", "mgs_scene_create", "mgs_scene_destroy", "mgs_scene_set_stream", "mgs_instance_add",
    "mgs_instance_set_transform", "mgs_scene_commit", "mgs_scene_splat_count", "mgs_scene_storage_order", "mgs_scene_download_set",
    "mgs_frame_context_create", "mgs_frame_context_destroy", "mgs_scene_memory_usage", "mgs_scene_set_list_capacity",
    "mgs_frame_set_occluder", "mgs_frame_upload_occluder", "mgs_sensor_model_from_frame", "mgs_frame_set_sensor",
    "mgs_light_default", "mgs_material_default", "mgs_scene_set_lights", "mgs_scene_set_light_radii", "mgs_instance_set_material",
    "mgs_compare_capture", "mgs_compare_capture_upload", "mgs_compare_release", "mgs_compare_params_default", "mgs_compare_metrics",
    "mgs_compare_view_default", "mgs_compare_composite", "mgs_compare_download_composite",
    "mgs_mesh_from_arrays", "mgs_mesh_load_obj", "mgs_mesh_view", "mgs_mesh_destroy", "mgs_mesh_instance_add",
    "mgs_mesh_instance_set_transform", "mgs_mesh_instance_set_visible", "mgs_meshes_render", "mgs_meshes_download",
    "mgs_trace_params_default", "mgs_render_traced", "mgs_trace_download_hit_counts",
    "mgs_trace_light_params_default", "mgs_render_traced_lit", "mgs_trace_download_shadow_hits", "mgs_render_hybrid",
    "mgs_ray_query_params_default", "mgs_trace_rays", "mgs_trace_rays_device", "mgs_trace_generate_rays",
    "mgs_trace_shadow_rays", "mgs_trace_shadow_rays_device", "mgs_shade_points", "mgs_shade_points_device",
    "mgs_mesh_ray_params_default", "mgs_trace_mesh_rays", "mgs_trace_mesh_rays_device",
    "mgs_trace_mesh_params_default", "mgs_frame_set_trace_meshes", "mgs_trace_download_mesh_hits", "mgs_trace_mesh_stats",
    "mgs_frame_set_hybrid_meshes", "mgs_debug_download_hybrid_depth",
    "mgs_bounce_material_default", "mgs_bounce_material_from_mtl", "mgs_mesh_bounce_materials", "mgs_mesh_instance_set_bounce_materials",
    "mgs_trace_bounce_params_default", "mgs_render_traced_indirect",
    "mgs_frame_params_default", "mgs_render", "mgs_frame_stats", "mgs_timings_query", "mgs_frame_download", "mgs_frame_download_surface", "mgs_frame_copy_strip",
    "mgs_frame_download_projected", "mgs_frame_download_projected_gut", "mgs_debug_download_hierarchy", "mgs_sync", "mgs_comm_unique_id", "mgs_scene_comm_init", "mgs_scene_comm_destroy",
    "mgs_scene_set_strip_rows", "mgs_render_gathered", "mgs_frame_row_costs",
    "mgs_loader_create", "mgs_loader_destroy", "mgs_loader_push", "mgs_loader_status", "mgs_loader_take", "mgs_sort_keys", "mgs_sort_download", "mgs_radix_sort_u32", "mgs_radix_sort_host",
    "mgs_camera_lookat_perspective", "mgs_compute_transform"]


def _check(rc):
    if rc != 0:
        raise MgsError(rc, load_library().mgs_last_error().decode(errors="replace"))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


IDENTITY = np.eye(4, dtype=np.float32)


class SplatSet:
    """RAM splat model (struct SplatSet, src/splat_set.h:33-48)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.mgs_splatset_load(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, positions, f_dc, f_rest, opacity, scale, rotation):
        lib = load_library()
        keep = [_f32(positions).reshape(-1), _f32(f_dc).reshape(-1),
                None if f_rest is None else _f32(f_rest).reshape(-1),
                _f32(opacity).reshape(-1), _f32(scale).reshape(-1), _f32(rotation).reshape(-1)]
        n = keep[0].size // 3
        v = SplatSetView()
        v.positions, v.f_dc = _fp(keep[0]), _fp(keep[1])
        v.f_rest = _fp(keep[2]) if keep[2] is not None and keep[2].size else None
        v.opacity, v.scale, v.rotation = _fp(keep[3]), _fp(keep[4]), _fp(keep[5])
        v.splat_count = n
        v.f_rest_per_splat = 0 if keep[2] is None or n == 0 else keep[2].size // n
        h = C.c_void_p()
        _check(lib.mgs_splatset_from_arrays(C.byref(v), C.byref(h)))
        return cls(h)

    def arrays(self):
        """dict of numpy copies of the six SoA arrays + sh_degree."""
        lib = load_library()
        v = SplatSetView()
        _check(lib.mgs_splatset_view(self._h, C.byref(v)))
        n = v.splat_count

        def cp(ptr, cnt):
            return np.ctypeslib.as_array(ptr, shape=(cnt,)).copy() if cnt and ptr else np.zeros(0, np.float32)
        return dict(positions=cp(v.positions, 3 * n), f_dc=cp(v.f_dc, 3 * n),
                    f_rest=cp(v.f_rest, v.f_rest_per_splat * n), opacity=cp(v.opacity, n), scale=cp(v.scale, 3 * n),
                    rotation=cp(v.rotation, 4 * n), count=n, f_rest_per_splat=v.f_rest_per_splat,
                    sh_degree=v.sh_degree)

    def close(self):
        if self._h:
            load_library().mgs_splatset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MESH_NONE = 0xFFFFFFFF  # primitive id of a pixel no mesh covers


class Mesh:
    """RAM triangle mesh (ObjLoader's output, src/obj_loader.h): mgs_mesh_*"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_arrays(cls, positions, indices, normals=None, material_ids=None, materials=None):
        """positions [V,3], indices [T,3] (or flat), normals [V,3] or None (generated), material_ids [T] or None, materials: a
        sequence of Material (make_material) or None (the loader's default)"""
        pos = _f32(positions).reshape(-1)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        nrm = None if normals is None else _f32(normals).reshape(-1)
        mid = None if material_ids is None else np.ascontiguousarray(material_ids, np.uint32).reshape(-1)
        mats = list(materials or [])
        if nrm is not None and nrm.size != pos.size:
            raise ValueError("Mesh.from_arrays: normals must match positions")
        if mid is not None and mid.size * 3 != idx.size:
            raise ValueError("Mesh.from_arrays: one material id per triangle")
        v = MeshView()
        v.positions = _fp(pos) if pos.size else None
        v.normals = None if nrm is None else _fp(nrm)
        v.indices = idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx.size else None
        v.material_ids = None if mid is None else mid.ctypes.data_as(C.POINTER(C.c_uint32))
        arr = (Material * max(len(mats), 1))(*mats)
        v.materials = arr if mats else None
        v.vertex_count, v.index_count, v.material_count = pos.size // 3, idx.size, len(mats)
        h = C.c_void_p()
        _check(load_library().mgs_mesh_from_arrays(C.byref(v), C.byref(h)))
        return cls(h)

    @classmethod
    def load_obj(cls, path):
        h = C.c_void_p()
        _check(load_library().mgs_mesh_load_obj(os.fsencode(path), C.byref(h)))
        return cls(h)

    def view(self):
        """dict of numpy copies: positions [V,3], normals [V,3], indices [T,3], material_ids [T], materials (list of dicts)"""
        v = MeshView()
        _check(load_library().mgs_mesh_view(self._h, C.byref(v)))
        nv, ni = int(v.vertex_count), int(v.index_count)
        cp = lambda ptr, cnt: np.ctypeslib.as_array(ptr, shape=(cnt,)).copy()
        mats = [{k: (float(getattr(v.materials[i], k)) if k == "shininess" else tuple(getattr(v.materials[i], k))) for k, _ in Material._fields_}
                for i in range(v.material_count)]
        return dict(positions=cp(v.positions, 3 * nv).reshape(-1, 3), normals=cp(v.normals, 3 * nv).reshape(-1, 3),
                    indices=cp(v.indices, ni).reshape(-1, 3), material_ids=cp(v.material_ids, ni // 3), materials=mats)

    def bounce_materials(self):
        """mgs_mesh_bounce_materials: one BounceMaterial per material of the mesh, from the MTL's Tf / Ni / illum through the loader's
        rule (a mesh from arrays: defaults); pass the list to Scene.set_mesh_bounce_materials"""
        n = C.c_uint32()
        _check(load_library().mgs_mesh_bounce_materials(self._h, None, 0, C.byref(n)))
        arr = (BounceMaterial * max(n.value, 1))()
        _check(load_library().mgs_mesh_bounce_materials(self._h, arr, n.value, C.byref(n)))
        out = []
        for i in range(n.value):   # copies: the array's elements would keep it alive and alias it
            m = BounceMaterial()
            C.memmove(C.byref(m), C.byref(arr[i]), C.sizeof(BounceMaterial))
            out.append(m)
        return out

    def close(self):
        if self._h:
            load_library().mgs_mesh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LOADER_READY, LOADER_LOADING, LOADER_LOADED, LOADER_FAILURE = 1, 2, 3, 4


class Loader:
    """PlyLoaderAsync + the scene-load queue: push files, poll, take the loaded SplatSets in order"""

    def __init__(self):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.mgs_loader_create(C.byref(h)))
        self._h = h

    def push(self, path):
        _check(self._lib.mgs_loader_push(self._h, os.fsencode(path)))

    def status(self):
        """(state, requests queued behind the head, head's path)"""
        st, q = C.c_int(), C.c_uint32()
        buf = C.create_string_buffer(1024)
        _check(self._lib.mgs_loader_status(self._h, C.byref(st), C.byref(q), buf, 1024))
        return st.value, q.value, buf.value.decode(errors="replace")

    def take(self):
        h = C.c_void_p()
        _check(self._lib.mgs_loader_take(self._h, C.byref(h)))
        return SplatSet(h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mgs_loader_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_params(width=1920, height=1080):
    p = FrameParams()
    load_library().mgs_frame_params_default(C.byref(p))
    p.width, p.height = width, height
    return p


def default_trace_params(**overrides):
    """MgsTraceParams with the reference's defaults (mgs_trace_params_default); keyword arguments override fields"""
    t = TraceParams()
    load_library().mgs_trace_params_default(C.byref(t))
    for k, v in overrides.items():
        if k not in dict(TraceParams._fields_):
            raise TypeError(f"default_trace_params: unknown field {k}")
        setattr(t, k, v)
    return t


def default_trace_light_params(**overrides):
    """MgsTraceLightParams with the reference's defaults (mgs_trace_light_params_default); keyword arguments override fields"""
    t = TraceLightParams()
    load_library().mgs_trace_light_params_default(C.byref(t))
    for k, v in overrides.items():
        if k not in dict(TraceLightParams._fields_):
            raise TypeError(f"default_trace_light_params: unknown field {k}")
        setattr(t, k, v)
    return t


def set_camera(p, view, proj, camera_pos):
    """view/proj: 4x4 numpy in math (row, col) convention; stored glm column-major."""
    v = _f32(view).T.reshape(-1)
    pr = _f32(proj).T.reshape(-1)
    for i in range(16):
        p.view[i] = float(v[i])
        p.proj[i] = float(pr[i])
    for i in range(3):
        p.camera_pos[i] = float(camera_pos[i])


def camera_lookat_perspective(eye, center, up, fov_deg, z_near, z_far, width, height, flip_y=False):
    """returns (view, proj) as 4x4 numpy arrays in math convention (row, col)."""
    lib = load_library()
    e, c, u = _f32(eye), _f32(center), _f32(up)
    v = np.zeros(16, np.float32)
    p = np.zeros(16, np.float32)
    lib.mgs_camera_lookat_perspective(_fp(e), _fp(c), _fp(u), fov_deg, z_near, z_far, width, height, int(flip_y),
                                      _fp(v), _fp(p))
    return v.reshape(4, 4).T.copy(), p.reshape(4, 4).T.copy()


def comm_unique_id():
    """ncclGetUniqueId through libmgs: 128 bytes; call on one rank and distribute"""
    buf = C.create_string_buffer(128)
    _check(load_library().mgs_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf.raw)


def compute_transform(scale, rotation_deg, translation):
    lib = load_library()
    m = np.zeros(16, np.float32)
    mi = np.zeros(16, np.float32)
    lib.mgs_compute_transform(_fp(_f32(scale)), _fp(_f32(rotation_deg)), _fp(_f32(translation)), _fp(m), _fp(mi))
    return m.reshape(4, 4).T.copy(), mi.reshape(4, 4).T.copy()


class Scene:
    """Device scene (SplatSetManagerVk + renderer buffers) on one MI355X."""

    def __init__(self, device=0, _context_of=None):
        lib = load_library()
        self._lib = lib
        h = C.c_void_p()
        if _context_of is None:
            _check(lib.mgs_scene_create(device, C.byref(h)))
        else:
            _check(lib.mgs_frame_context_create(_context_of._h, C.byref(h)))
        self._h = h
        self._sets = [] if _context_of is None else _context_of._sets
        self._frame_wh = None  # size of the last frame rendered through this object (compare_composite's default output size)

    def frame_context(self):
        """a frame in flight over this scene's committed data: own stream, working buffers and graphs (mgs_frame_context_create)"""
        return Scene(_context_of=self)

    def set_list_capacity(self, entries):
        _check(self._lib.mgs_scene_set_list_capacity(self._h, int(entries)))

    # ---- the caller's opaque geometry: splats are depth-tested against it, its colour shows through them ----
    def set_occluder(self, depth_ptr, color_ptr, width, height):
        """bind device images for the following frames of this handle (mgs_frame_set_occluder): depth_ptr float32[H,W] window
        depth in [0,1] made with the frame's proj (1.0 = no geometry), color_ptr float32[H,W,4] linear or 0/None.  The memory stays
        the caller's; its contents are read by every frame until re-bound.  The test is z_splat <= depth (LESS_OR_EQUAL; the
        reference does not pin the operator for the splat pipelines)."""
        _check(self._lib.mgs_frame_set_occluder(self._h, C.c_void_p(depth_ptr or None), C.c_void_p(color_ptr or None),
                                                int(width), int(height)))

    def upload_occluder(self, depth, color=None):
        """host convenience (mgs_frame_upload_occluder): depth float32[H,W], color float32[H,W,4] or None, copied into buffers
        the handle owns"""
        d = _f32(depth)
        if d.ndim != 2:
            raise ValueError("upload_occluder: depth must be [height, width]")
        c = None
        if color is not None:
            c = _f32(color)
            if c.shape != d.shape + (4,):
                raise ValueError("upload_occluder: color must be [height, width, 4]")
        _check(self._lib.mgs_frame_upload_occluder(self._h, _fp(d), None if c is None else _fp(c), d.shape[1], d.shape[0]))

    def clear_occluder(self):
        _check(self._lib.mgs_frame_set_occluder(self._h, None, None, 0, 0))

    def set_sensor(self, model):
        """bind a SensorModel to this handle (mgs_frame_set_sensor; copied at the call), None unbinds.  While bound it replaces
        camera_model / fov_rad for the projection and the rays of this handle's 3DGUT frames and of generate_rays."""
        _check(self._lib.mgs_frame_set_sensor(self._h, None if model is None else C.byref(model)))

    def memory_usage(self):
        """(scene_bytes, working_bytes): the committed data shared by all contexts, and this handle's working set"""
        a, b = C.c_uint64(), C.c_uint64()
        _check(self._lib.mgs_scene_memory_usage(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_stream(self, stream_ptr):
        _check(self._lib.mgs_scene_set_stream(self._h, C.c_void_p(stream_ptr)))

    def add_instance(self, splat_set, transform=None):
        m = _f32(IDENTITY if transform is None else transform).T.reshape(-1).copy()  # -> glm column-major
        idx = C.c_int()
        _check(self._lib.mgs_instance_add(self._h, splat_set._h, _fp(m), C.byref(idx)))
        self._sets.append(splat_set)
        return idx.value

    def set_transform(self, instance, transform):
        m = _f32(transform).T.reshape(-1).copy()
        _check(self._lib.mgs_instance_set_transform(self._h, instance, _fp(m)))

    # ---- deferred lighting (FrameParams.lighting_mode): the scene's light table and the instances' materials ----
    def set_lights(self, lights):
        """replace the scene's lights (mgs_scene_set_lights): a sequence of Light (make_light); empty = the headlight.  Every radius
        restarts at 1.0; where a light carries one (make_light(radius=R)) the radii are set too (mgs_scene_set_light_radii)"""
        lights = list(lights)
        arr = (Light * max(len(lights), 1))(*lights)
        _check(self._lib.mgs_scene_set_lights(self._h, arr if lights else None, len(lights)))
        if any(hasattr(l, "radius") for l in lights):
            self.set_light_radii([getattr(l, "radius", 1.0) for l in lights])

    def set_light_radii(self, radii=None):
        """the soft-shadow radius of each light of the table, in its order (mgs_scene_set_light_radii); None = the default 1.0 for all"""
        if radii is None:
            _check(self._lib.mgs_scene_set_light_radii(self._h, None, 0))
            return
        r = [float(x) for x in radii]
        arr = (C.c_float * max(len(r), 1))(*r)
        _check(self._lib.mgs_scene_set_light_radii(self._h, arr, len(r)))

    def set_material(self, instance, material):
        _check(self._lib.mgs_instance_set_material(self._h, int(instance), C.byref(material)))

    # ---- triangle meshes: instances of the scene, the mesh pass that makes this handle's occluder images ----
    def add_mesh_instance(self, mesh, transform=None):
        m = _f32(IDENTITY if transform is None else transform).T.reshape(-1).copy()
        idx = C.c_int()
        _check(self._lib.mgs_mesh_instance_add(self._h, mesh._h, _fp(m), C.byref(idx)))
        return idx.value

    def set_mesh_transform(self, mesh_instance, transform):
        m = _f32(transform).T.reshape(-1).copy()
        _check(self._lib.mgs_mesh_instance_set_transform(self._h, int(mesh_instance), _fp(m)))

    def set_mesh_visible(self, mesh_instance, visible):
        _check(self._lib.mgs_mesh_instance_set_visible(self._h, int(mesh_instance), int(bool(visible))))

    def render_meshes(self, params, want_stats=False):
        """mgs_meshes_render: rasterise the visible mesh instances for params and bind the result as this handle's occluder;
        want_stats waits and returns a MeshOut"""
        out = MeshOut()
        self._mesh_wh = (params.width, params.height)
        _check(self._lib.mgs_meshes_render(self._h, C.byref(params), C.byref(out) if want_stats else None))
        return out if want_stats else None

    def download_meshes(self):
        """(depth float32[H,W], colour float32[H,W,4], primitive id uint32[H,W], MESH_NONE = none) of the last mesh pass"""
        w, h = self._mesh_wh
        depth, color, prim = np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.uint32)
        for which, a in enumerate((depth, color, prim)):
            _check(self._lib.mgs_meshes_download(self._h, which, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return depth, color, prim

    def commit(self, sh_format=FORMAT_FLOAT32, rgba_format=FORMAT_FLOAT32):
        _check(self._lib.mgs_scene_commit(self._h, sh_format, rgba_format))

    @property
    def splat_count(self):
        return int(self._lib.mgs_scene_splat_count(self._h))

    def storage_order(self, instance, count):
        """permutation storage index -> caller's index of the instance's splat set"""
        out = np.zeros(count, np.uint32)
        _check(self._lib.mgs_scene_storage_order(self._h, instance, out.ctypes.data_as(C.POINTER(C.c_uint32)), count))
        return out

    def download_set(self, instance, which, count):
        out = np.zeros(count, np.float32)
        _check(self._lib.mgs_scene_download_set(self._h, instance, which, _fp(out), out.size))
        return out

    def render(self, params, want_stats=False):
        out = FrameOut()
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render(self._h, C.byref(params), C.byref(out)))
        if want_stats and not params.collect_timings:
            _check(self._lib.mgs_frame_stats(self._h, C.byref(out)))
        return out

    def render_traced(self, params, trace=None, want_stats=False):
        """mgs_render_traced: one ray-traced (3DGRT primary rays) frame into this handle's frame buffer; trace = a TraceParams or
        None for the defaults; want_stats waits and returns a TraceOut"""
        out = TraceOut()
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render_traced(self._h, C.byref(params), C.byref(trace) if trace is not None else None,
                                           C.byref(out) if want_stats else None))
        return out if want_stats else None

    def render_traced_lit(self, params, trace=None, light=None, want_stats=False):
        """mgs_render_traced_lit: one traced frame under the scene's lights with shadow rays through the splats (params.lighting_mode
        must be MGS_LIGHTING_DIRECT); trace / light = a TraceParams / TraceLightParams or None for the defaults; want_stats waits
        and returns (TraceOut, TraceLightOut)"""
        out, lout = TraceOut(), TraceLightOut()
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render_traced_lit(self._h, C.byref(params), C.byref(trace) if trace is not None else None,
                                               C.byref(light) if light is not None else None,
                                               C.byref(out) if want_stats else None, C.byref(lout) if want_stats else None))
        return (out, lout) if want_stats else None

    def render_traced_indirect(self, params, trace=None, light=None, bounce=None, want_stats=False):
        """mgs_render_traced_indirect: the lit traced frame with mesh hits (set_trace_meshes on) whose mirror and glass materials
        (set_mesh_bounce_materials) send bounce rays (params.lighting_mode must be MGS_LIGHTING_INDIRECT); trace / light / bounce = a
        TraceParams / TraceLightParams / TraceBounceParams, or an int max_bounces, or None for the defaults; want_stats waits and
        returns (TraceOut, TraceLightOut, TraceBounceOut)"""
        out, lout, bout = TraceOut(), TraceLightOut(), TraceBounceOut()
        if isinstance(bounce, int):
            b = TraceBounceParams()
            self._lib.mgs_trace_bounce_params_default(C.byref(b))
            b.max_bounces = bounce
            bounce = b
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render_traced_indirect(self._h, C.byref(params), C.byref(trace) if trace is not None else None,
                                                    C.byref(light) if light is not None else None,
                                                    C.byref(bounce) if bounce is not None else None,
                                                    C.byref(out) if want_stats else None, C.byref(lout) if want_stats else None,
                                                    C.byref(bout) if want_stats else None))
        return (out, lout, bout) if want_stats else None

    def set_mesh_bounce_materials(self, mesh_instance, materials):
        """mgs_mesh_instance_set_bounce_materials: materials = BounceMaterial objects (bounce_material(...)) indexed by the triangles'
        material id; an empty list clears"""
        arr = (BounceMaterial * max(len(materials), 1))(*materials)
        _check(self._lib.mgs_mesh_instance_set_bounce_materials(self._h, int(mesh_instance), arr if materials else None, len(materials)))

    def render_hybrid(self, params, trace=None, light=None, want_stats=False):
        """mgs_render_hybrid: the rasterised frame of params.pipeline (3DGS or 3DGUT) as the primary surface, lit by the scene's
        lights with shadow rays through the splats (params.lighting_mode must be MGS_LIGHTING_DIRECT); trace / light = a TraceParams /
        TraceLightParams or None for the defaults; want_stats waits and returns (FrameOut with the raster frame's statistics,
        TraceLightOut)"""
        out, lout = FrameOut(), TraceLightOut()
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render_hybrid(self._h, C.byref(params), C.byref(trace) if trace is not None else None,
                                           C.byref(light) if light is not None else None,
                                           C.byref(out) if want_stats else None, C.byref(lout) if want_stats else None))
        if not want_stats:
            return None
        if not params.collect_timings:
            _check(self._lib.mgs_frame_stats(self._h, C.byref(out)))
        return out, lout

    def trace_rays(self, rays, params, trace=None, reorder=False, want_stats=False, results=None):
        """mgs_trace_rays / mgs_trace_rays_device: the caller's rays through the scene's hierarchy with the walk of render_traced's
        strategy 0.  rays = a RAY_DTYPE array (make_rays) -> returns a RAY_RESULT_DTYPE array (waits); or rays = (device pointer,
        count) with results = a device pointer to count * 48 bytes, both 16-byte aligned -> ordered on the handle's stream, returns
        None.  want_stats waits and returns (results, RayQueryOut)."""
        out, q = RayQueryOut(), RayQueryParams()
        self._lib.mgs_ray_query_params_default(C.byref(q))
        q.reorder = int(bool(reorder))
        tr = C.byref(trace) if trace is not None else None
        if isinstance(rays, tuple):
            ptr, count = rays
            _check(self._lib.mgs_trace_rays_device(self._h, C.c_void_p(ptr or None), int(count), C.byref(params), tr, C.byref(q),
                                                   C.c_void_p(results or None), C.byref(out) if want_stats else None))
            res = None
        else:
            r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
            res = np.zeros(r.shape[0], RAY_RESULT_DTYPE)
            _check(self._lib.mgs_trace_rays(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], C.byref(params), tr, C.byref(q),
                                            res.ctypes.data_as(C.c_void_p), C.byref(out) if want_stats else None))
        return (res, out) if want_stats else res

    def _query_params(self, reorder):
        q = RayQueryParams()
        self._lib.mgs_ray_query_params_default(C.byref(q))
        q.reorder = int(bool(reorder))
        return q

    def trace_shadow_rays(self, rays, params, trace=None, light=None, reorder=False, want_stats=False):
        """mgs_trace_shadow_rays: the caller's shadow rays (a RAY_DTYPE array; t_max is the light's ray parameter) as the light pass of a
        lit frame traces its own -> a SHADOW_RESULT_DTYPE array (waits).  light = a TraceLightParams (shadows_mode must be
        MGS_SHADOWS_HARD = 1) or None for the defaults with hard shadows.  want_stats returns (results, RayQueryOut)."""
        out, q = RayQueryOut(), self._query_params(reorder)
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        res = np.zeros(r.shape[0], SHADOW_RESULT_DTYPE)
        _check(self._lib.mgs_trace_shadow_rays(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], C.byref(params),
                                               C.byref(trace) if trace is not None else None, C.byref(light) if light is not None else None,
                                               C.byref(q), res.ctypes.data_as(C.c_void_p), C.byref(out) if want_stats else None))
        return (res, out) if want_stats else res

    def trace_shadow_rays_device(self, rays_device, count, params, results_device, trace=None, light=None, reorder=False, want_stats=False):
        """mgs_trace_shadow_rays_device: count rays at the device pointer rays_device, results (count * 16 bytes) to results_device, both
        16-byte aligned; ordered on the handle's stream.  want_stats waits and returns a RayQueryOut."""
        out, q = RayQueryOut(), self._query_params(reorder)
        _check(self._lib.mgs_trace_shadow_rays_device(self._h, C.c_void_p(rays_device or None), int(count), C.byref(params),
                                                      C.byref(trace) if trace is not None else None, C.byref(light) if light is not None else None,
                                                      C.byref(q), C.c_void_p(results_device or None), C.byref(out) if want_stats else None))
        return out if want_stats else None

    @staticmethod
    def _material_array(materials):
        mats = [m if isinstance(m, Material) else make_material(**m) for m in materials]
        return (Material * max(len(mats), 1))(*mats), len(mats)

    def shade_points(self, points, materials, params, trace=None, light=None, reorder=False, want_stats=False):
        """mgs_shade_points: the caller's surface points (a SURFACE_POINT_DTYPE array, make_surface_points) under the scene's lights,
        each light shadowed by one ray through the splats when light.shadows_mode is MGS_SHADOWS_HARD = 1; materials = a list of Material or
        of make_material keyword dicts (1 to 256) -> a SHADE_RESULT_DTYPE array (waits).  want_stats returns (results, TraceLightOut,
        invalid points)."""
        lout, bad, q = TraceLightOut(), C.c_uint32(0), self._query_params(reorder)
        pts = np.ascontiguousarray(points, dtype=SURFACE_POINT_DTYPE).reshape(-1)
        res = np.zeros(pts.shape[0], SHADE_RESULT_DTYPE)
        arr, n = self._material_array(materials)
        _check(self._lib.mgs_shade_points(self._h, pts.ctypes.data_as(C.c_void_p), pts.shape[0], arr, n, C.byref(params),
                                          C.byref(trace) if trace is not None else None, C.byref(light) if light is not None else None,
                                          C.byref(q), res.ctypes.data_as(C.c_void_p), C.byref(lout) if want_stats else None,
                                          C.byref(bad) if want_stats else None))
        return (res, lout, int(bad.value)) if want_stats else res

    def shade_points_device(self, points_device, count, materials, params, results_device, trace=None, light=None, reorder=False,
                            want_stats=False):
        """mgs_shade_points_device: count points at the device pointer points_device, results (count * 16 bytes) to results_device, both
        16-byte aligned; ordered on the handle's stream.  want_stats waits and returns (TraceLightOut, invalid points)."""
        lout, bad, q = TraceLightOut(), C.c_uint32(0), self._query_params(reorder)
        arr, n = self._material_array(materials)
        _check(self._lib.mgs_shade_points_device(self._h, C.c_void_p(points_device or None), int(count), arr, n, C.byref(params),
                                                 C.byref(trace) if trace is not None else None, C.byref(light) if light is not None else None,
                                                 C.byref(q), C.c_void_p(results_device or None), C.byref(lout) if want_stats else None,
                                                 C.byref(bad) if want_stats else None))
        return (lout, int(bad.value)) if want_stats else None

    def mesh_ray_params(self, mode=MESH_RAYS_CLOSEST, reorder=False):
        q = MeshRayParams()
        self._lib.mgs_mesh_ray_params_default(C.byref(q))
        q.mode, q.reorder = int(mode), int(bool(reorder))
        return q

    def trace_mesh_rays(self, rays, mode=MESH_RAYS_CLOSEST, reorder=False, want_stats=False, params=None):
        """mgs_trace_mesh_rays: the caller's rays (a RAY_DTYPE array, make_rays) against the scene's triangle meshes -> a MESH_HIT_DTYPE
        array (waits).  mode = MESH_RAYS_CLOSEST (nearest hit with ids, barycentrics, position, normal) or MESH_RAYS_OCCLUSION (the hit
        flag alone).  params = a MeshRayParams replaces mode / reorder.  want_stats returns (hits, MeshRayOut)."""
        out, q = MeshRayOut(), (params if params is not None else self.mesh_ray_params(mode, reorder))
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        res = np.zeros(r.shape[0], MESH_HIT_DTYPE)
        _check(self._lib.mgs_trace_mesh_rays(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], C.byref(q), res.ctypes.data_as(C.c_void_p),
                                             C.byref(out) if want_stats else None))
        return (res, out) if want_stats else res

    def trace_mesh_rays_device(self, rays_device, count, hits_device, mode=MESH_RAYS_CLOSEST, reorder=False, want_stats=False, params=None):
        """mgs_trace_mesh_rays_device: count rays at the device pointer rays_device, hits (count * 64 bytes) to hits_device, both 16-byte
        aligned (torch allocations are); ordered on the handle's stream.  want_stats waits and returns a MeshRayOut."""
        out, q = MeshRayOut(), (params if params is not None else self.mesh_ray_params(mode, reorder))
        _check(self._lib.mgs_trace_mesh_rays_device(self._h, C.c_void_p(rays_device or None), int(count), C.byref(q),
                                                    C.c_void_p(hits_device or None), C.byref(out) if want_stats else None))
        return out if want_stats else None

    def set_trace_meshes(self, enabled=True, min_transmittance=0.0, params=None):
        """mgs_frame_set_trace_meshes: the scene's triangle meshes take part in this handle's render_traced (strategy 0) and
        render_traced_lit frames; min_transmittance = min_mesh_composite_transmittance.  params = a TraceMeshParams replaces both;
        enabled=False turns the setting off."""
        if params is None:
            params = TraceMeshParams()
            self._lib.mgs_trace_mesh_params_default(C.byref(params))
            params.enabled, params.min_mesh_composite_transmittance = int(bool(enabled)), float(min_transmittance)
        _check(self._lib.mgs_frame_set_trace_meshes(self._h, C.byref(params)))

    def set_hybrid_meshes(self, enabled=True, min_mesh_composite_transmittance=0.0, params=None):
        """mgs_frame_set_hybrid_meshes: the scene's triangle meshes take part in this handle's render_hybrid frames through a traced
        mesh depth pre-pass (a setting of its own: render_hybrid does not read set_trace_meshes while it is on).  params = a
        TraceMeshParams replaces both; enabled=False turns the setting off."""
        if params is None:
            params = TraceMeshParams()
            self._lib.mgs_trace_mesh_params_default(C.byref(params))
            params.enabled, params.min_mesh_composite_transmittance = int(bool(enabled)), float(min_mesh_composite_transmittance)
        _check(self._lib.mgs_frame_set_hybrid_meshes(self._h, C.byref(params)))

    def hybrid_mesh_depth(self, params):
        """mgs_debug_download_hybrid_depth: the depth plane of the last hybrid frame's mesh pre-pass, float32[H,W]"""
        out = np.zeros((params.height, params.width), np.float32)
        _check(self._lib.mgs_debug_download_hybrid_depth(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def trace_mesh_hits(self, params):
        """the per-pixel closest mesh hits of the last traced frame (setting on), a MESH_HIT_DTYPE array [H,W]"""
        out = np.zeros((params.height, params.width), MESH_HIT_DTYPE)
        _check(self._lib.mgs_trace_download_mesh_hits(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def trace_mesh_stats(self):
        """mgs_trace_mesh_stats of the last traced frame (setting on): (primary, shadow), two MeshRayOut; waits"""
        primary, shadow = MeshRayOut(), MeshRayOut()
        _check(self._lib.mgs_trace_mesh_stats(self._h, C.byref(primary), C.byref(shadow)))
        return primary, shadow

    def generate_rays(self, params, rays_device):
        """mgs_trace_generate_rays: the primary rays render_traced would trace for params, written row-major to the device pointer
        rays_device (height * width * 32 bytes, 16-byte aligned); ordered on the handle's stream"""
        _check(self._lib.mgs_trace_generate_rays(self._h, C.byref(params), C.c_void_p(rays_device or None)))

    def trace_shadow_hits(self, params):
        """shadow hits accepted per pixel of the last lit traced frame, summed over the lights, uint32[H,W]"""
        out = np.zeros((params.height, params.width), np.uint32)
        _check(self._lib.mgs_trace_download_shadow_hits(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def trace_hit_counts(self, params):
        """pixel.hitCount of the last traced frame, uint32[H,W]"""
        out = np.zeros((params.height, params.width), np.uint32)
        _check(self._lib.mgs_trace_download_hit_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def frame_stats(self):
        out = FrameOut()
        _check(self._lib.mgs_frame_stats(self._h, C.byref(out)))
        return out

    def timings(self, frames_back=0):
        ms = (C.c_float * 8)()
        _check(self._lib.mgs_timings_query(self._h, frames_back, ms))
        return [float(x) for x in ms[:6]]

    def timings_all(self, frames_back=0):
        """all MGS_STAGE_COUNT slots: the six of timings() + [6] = MGS_STAGE_CULL (the head of the project stage)"""
        ms = (C.c_float * 8)()
        _check(self._lib.mgs_timings_query(self._h, frames_back, ms))
        return [float(x) for x in ms]

    def download_frame(self, params):
        if params.target_format == TARGET_RGBA8:
            img = np.zeros((params.height, params.width, 4), np.uint8)
        elif params.target_format == TARGET_RGBA16F:
            img = np.zeros((params.height, params.width, 4), np.float16)
        else:
            img = np.zeros((params.height, params.width, 4), np.float32)
        _check(self._lib.mgs_frame_download(self._h, img.ctypes.data_as(C.c_void_p), img.nbytes))
        return img

    def download_surface(self, params, normals=False):
        """FTB side outputs of a frame rendered with params.surface_outputs = 1: (picked depth float32[H,W],
        splat id uint32[H,W] in the caller's id space, 0xFFFFFFFF = none[, integrated normal float32[H,W,4]])"""
        depth = np.zeros((params.height, params.width), np.float32)
        ids = np.zeros((params.height, params.width), np.uint32)
        _check(self._lib.mgs_frame_download_surface(self._h, 0, depth.ctypes.data_as(C.c_void_p), depth.nbytes))
        _check(self._lib.mgs_frame_download_surface(self._h, 1, ids.ctypes.data_as(C.c_void_p), ids.nbytes))
        if not normals:
            return depth, ids
        nrm = np.zeros((params.height, params.width, 4), np.float32)
        _check(self._lib.mgs_frame_download_surface(self._h, 2, nrm.ctypes.data_as(C.c_void_p), nrm.nbytes))
        return depth, ids, nrm

    def download_consolidated_depth(self, params):
        """mgs_frame_download_surface(which = 3): float32[H,W], the picked depth where it is valid and in front of the occluder
        the frame was rendered against, that occluder's depth (1.0 where none was bound) elsewhere"""
        depth = np.zeros((params.height, params.width), np.float32)
        _check(self._lib.mgs_frame_download_surface(self._h, 3, depth.ctypes.data_as(C.c_void_p), depth.nbytes))
        return depth

    # ---- image comparison (mgs_compare_*): a capture per handle, metrics and the split view against the last complete frame ----
    def compare_capture(self):
        """keep a device copy of the last complete frame as this handle's capture"""
        _check(self._lib.mgs_compare_capture(self._h))

    def compare_capture_upload(self, img):
        """take float32[H,W,4] (RGBA; a 3-channel image gets alpha 1) made elsewhere as the capture"""
        img = np.asarray(img)
        if img.ndim != 3 or img.shape[2] not in (3, 4):
            raise ValueError("compare_capture_upload: expected an [H,W,3|4] image")
        if img.shape[2] == 3:
            img = np.concatenate([img, np.ones(img.shape[:2] + (1,), img.dtype)], axis=2)
        a = _f32(img)
        _check(self._lib.mgs_compare_capture_upload(self._h, _fp(a), a.shape[1], a.shape[0]))

    def compare_release(self):
        _check(self._lib.mgs_compare_release(self._h))

    def compare_metrics(self, flip_mode=FLIP_REFERENCE, ppd=67.0):
        """MSE / PSNR / FLIP of the last complete frame against the capture: a CompareMetrics"""
        p = CompareParams(int(flip_mode), float(ppd))
        m = CompareMetrics()
        _check(self._lib.mgs_compare_metrics(self._h, C.byref(p), C.byref(m)))
        return m

    def compare_composite(self, split=0.5, left=SHOW_CAPTURE, right=SHOW_CURRENT, amplify=5.0, width=0, height=0):
        """the split view as float32[H,W,4]; left / right: SHOW_* values or their names (SHOW_NAMES)"""
        v = CompareView(float(split), int(SHOW_NAMES.get(left, left)), int(SHOW_NAMES.get(right, right)), float(amplify), int(width), int(height))
        nbytes = C.c_uint64(0)
        _check(self._lib.mgs_compare_composite(self._h, C.byref(v), None, C.byref(nbytes)))
        out = np.zeros(nbytes.value // 4, np.float32)
        _check(self._lib.mgs_compare_download_composite(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes))
        if not width and self._frame_wh is None:
            raise MgsError(-1, "compare_composite: pass width and height (this object has rendered no frame itself)")
        w = int(width) if width else self._frame_wh[0]  # 0 = the current frame's size
        return out.reshape(-1, w, 4)

    def copy_strip(self, device_ptr, nbytes):
        _check(self._lib.mgs_frame_copy_strip(self._h, C.c_void_p(device_ptr), nbytes))

    def sync(self):
        _check(self._lib.mgs_sync(self._h))

    # ---- multi-GPU strips (RCCL inside libmgs) ----
    def comm_init(self, rank, world_size, unique_id):
        """unique_id: 128 bytes from comm_unique_id() of ONE rank, distributed out of band"""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(self._lib.mgs_scene_comm_init(self._h, rank, world_size, C.cast(buf, C.c_void_p)))

    def comm_destroy(self):
        _check(self._lib.mgs_scene_comm_destroy(self._h))

    def set_strip_rows(self, bounds):
        if bounds is None:
            _check(self._lib.mgs_scene_set_strip_rows(self._h, None, 0))
            return
        b = np.ascontiguousarray(bounds, np.int32)
        _check(self._lib.mgs_scene_set_strip_rows(self._h, b.ctypes.data_as(C.POINTER(C.c_int32)), b.size))

    def render_gathered(self, params):
        out = FrameOut()
        self._sort_only = False
        self._frame_wh = (params.width, params.height)
        _check(self._lib.mgs_render_gathered(self._h, C.byref(params), C.byref(out)))
        return out

    def row_costs(self, height):
        rows = (height + 15) // 16
        out = np.zeros(rows, np.uint32)
        _check(self._lib.mgs_frame_row_costs(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), rows))
        return out

    def download_projected(self, global_ids):
        """debug hook: (records[n,10] float32, rect[n] uint32) of the last frame for the given global ids"""
        ids = np.ascontiguousarray(global_ids, np.uint32)
        out = np.zeros((ids.size, 10), np.float32)
        rect = np.zeros(ids.size, np.uint32)
        _check(self._lib.mgs_frame_download_projected(self._h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                                      _fp(out), rect.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out, rect

    def download_projected_gut(self, global_ids):
        """debug hook: (records[n,24] float32 — cx, cy, q1, q2, bex, bey, B[9], ro[3], r, g, b, a —, rect[n] uint32) of the last
        3DGUT frame for the given global ids"""
        ids = np.ascontiguousarray(global_ids, np.uint32)
        out = np.zeros((ids.size, 24), np.float32)
        rect = np.zeros(ids.size, np.uint32)
        _check(self._lib.mgs_frame_download_projected_gut(self._h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                                          _fp(out), rect.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out, rect

    def download_hierarchy(self, which, info_only=False, node_capacity=None, tri_capacity=None):
        """mgs_debug_download_hierarchy: (info dict, nodes uint32[total_nodes, 8] raw bits, tris uint32[leaves, 12] raw bits or None)
        of the splat (which 0) or triangle (which 1) hierarchy as the last build left it; the capacities override the buffers' sizes"""
        info = HierarchyInfo()
        _check(self._lib.mgs_debug_download_hierarchy(self._h, int(which), C.byref(info), None, 0, None, 0))
        d = info.as_dict()
        if info_only:
            return d, None, None
        nn = d["total_nodes"] if node_capacity is None else int(node_capacity)
        nt = d["leaves"] if tri_capacity is None else int(tri_capacity)
        nodes = np.zeros((max(nn, 1), 8), np.float32)
        tris = np.zeros((max(nt, 1), 12), np.float32) if which == 1 else None
        _check(self._lib.mgs_debug_download_hierarchy(self._h, int(which), C.byref(info), _fp(nodes), nn, None if tris is None else _fp(tris), nt))
        return d, nodes[:nn].view(np.uint32), None if tris is None else tris[:nt].view(np.uint32)

    def sort_keys(self, params):
        out = SortOut()
        _check(self._lib.mgs_sort_keys(self._h, C.byref(params), C.byref(out)))
        self._sort_only = True
        return out

    def sort_download(self, count):
        """(keys, ids) of the last sort.  The sorted keys exist after sort_keys() only: a frame's last sort pass writes the ids
        alone, and keys is None then."""
        ids = np.zeros(max(count, 1), np.uint32)
        keys = np.zeros(max(count, 1), np.uint32) if getattr(self, "_sort_only", False) else None
        kp = keys.ctypes.data_as(C.POINTER(C.c_uint32)) if keys is not None else None
        _check(self._lib.mgs_sort_download(self._h, kp, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size))
        return (keys[:count] if keys is not None else None), ids[:count]

    def radix_sort_host(self, keys, values, begin_bit=0, end_bit=32):
        k = np.ascontiguousarray(keys, np.uint32).copy()
        v = np.ascontiguousarray(values, np.uint32).copy()
        ms = C.c_float()
        _check(self._lib.mgs_radix_sort_host(self._h, k.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             v.ctypes.data_as(C.POINTER(C.c_uint32)), k.size, begin_bit, end_bit,
                                             C.byref(ms)))
        return k, v, ms.value

    def radix_sort_device(self, keys_ptr, vals_ptr, count, begin_bit=0, end_bit=32):
        ms = C.c_float()
        _check(self._lib.mgs_radix_sort_u32(self._h, C.c_void_p(keys_ptr), C.c_void_p(vals_ptr), count, begin_bit,
                                            end_bit, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mgs_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
