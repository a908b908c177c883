""".vkgs project files — the reference's own scene description.

Format = the JSON written by VkgsProjectWriter (src/vkgs_project_writer.cpp:75-330, PROJECT_FILE_VERSION 5) and
read by VkgsProjectReader (src/vkgs_project_reader.cpp:55-345).  Only the sections the VK3DGSR path consumes are
interpreted: "renderer" (raster knobs), "camera" / "cameras", "splatsGlobals" (storage formats), "splatSets"
(assets: id + path relative to the project file) and "splats" (instances: splatSetId + position / rotation in
degrees / scale, composed as T*R*S like computeTransform, src/utilities.h:170-199; "material" = the instance's splatMaterial,
:252-260), "renderer.lightingMode" (and the legacy "lightingEnabled", :143-153) and "lights" in the three layouts the reader accepts
(:616-770: assets / instances of version 3+, with the version 3 names "radius" / "position"; the flat list of versions 0-2).  The raw
"lights" section is also kept in `extra` and written back unchanged.  Meshes (:353-558) are read in both layouts, "meshAssets" +
"meshInstances" of version 2+ and the "meshes" list of versions 0 / 1, and written back as read.  RTX and DLSS settings are carried
through untouched on save but otherwise ignored (out of scope).
"""
import json
import os
from dataclasses import dataclass, field

import numpy as np

from .cameras import Camera

PROJECT_FILE_VERSION = 5


@dataclass
class SplatInstance:
    splat_set_id: int
    name: str = ""
    position: tuple = (0.0, 0.0, 0.0)
    rotation: tuple = (0.0, 0.0, 0.0)   # Euler degrees
    scale: tuple = (1.0, 1.0, 1.0)
    material: dict = None               # {"ambient", "diffuse", "specular", "emission": [3], "shininess"}; None = the splat sets' default


@dataclass
class Project:
    version: int = PROJECT_FILE_VERSION
    renderer: dict = field(default_factory=dict)
    camera: Camera = field(default_factory=Camera)
    cameras: list = field(default_factory=list)
    sh_format: int = 0
    rgba_format: int = 0
    splat_sets: dict = field(default_factory=dict)      # id -> absolute path
    instances: list = field(default_factory=list)       # [SplatInstance]
    extra: dict = field(default_factory=dict)           # sections written back as read (meshes, ..., and the raw "lights")
    lights: list = field(default_factory=list)          # "lights" interpreted: dicts with the field names of MgsLight
    mesh_assets: dict = field(default_factory=dict)     # "meshAssets" interpreted: id -> absolute path of the .obj ("meshes": entry index)
    mesh_instances: list = field(default_factory=list)  # "meshInstances" interpreted: dicts(asset, position, rotation, scale, materials)

    @property
    def lighting_mode(self):
        """renderer.lightingMode; files from before it have "lightingEnabled", which maps to indirect (vkgs_project_reader.cpp:143-153)"""
        r = self.renderer
        if "lightingMode" in r:
            return int(r["lightingMode"])
        return 2 if r.get("lightingEnabled", False) else 0

    # ---- mapping onto the C ABI ------------------------------------------------------------------
    def frame_params(self, width, height, flip_y=False):
        """MgsFrameParams filled from "renderer" + "camera" (defaults where a key is absent, like the reader's LOAD1)"""
        from . import capi
        r = self.renderer
        p = capi.default_params(width, height)
        V, P = self.camera.matrices(width, height, flip_y)
        capi.set_camera(p, V, P, self.camera.eye)
        p.sh_degree = int(r.get("maxShDegree", 3))
        p.frustum_culling = int(r.get("frustumCulling", capi.CULL_AT_DIST))
        p.size_culling = int(r.get("sizeCulling", 0))
        p.size_culling_min_pixels = float(r.get("sizeCullingMinPixels", 1.0))
        # shaderio.h:24-27: 0 GPU radix, 1/2 CPU async (mono / multi), 3 stochastic splat
        sm = int(r.get("sortingMethod", 0))
        p.sort_mode = {0: capi.SORT_GPU_RADIX, 3: capi.SORT_STOCHASTIC}.get(sm, capi.SORT_CPU_ASYNC)
        # "pipeline" (shaderio.h:61-66): 4 / 5 = the 3DGUT mesh pipeline (5 = hybrid with ray-traced secondary rays: its raster part);
        # everything else renders through the 3DGS raster path here
        p.pipeline = capi.PIPELINE_3DGUT if int(r.get("pipeline", 1)) in (4, 5) else capi.PIPELINE_3DGS
        p.kernel_degree = int(r.get("kernelDegree", 2))
        p.kernel_min_response = float(r.get("kernelMinResponse", 0.0113))
        p.temporal_sampling = int(bool(r.get("temporalSampling", False)))
        self.camera.apply(p)
        if p.pipeline != capi.PIPELINE_3DGUT:
            p.dof_mode = capi.DOF_DISABLED   # the 3DGS raster pipeline has no per-pixel rays
        p.cpu_lazy_sort = int(bool(r.get("cpuLazySort", True)))
        p.thin_particle_threshold = float(r.get("thinParticleThreshold", 1e-6))
        p.debug_flags = ((capi.DEBUG_POINT_CLOUD if r.get("pointCloudModeEnabled", False) else 0)
                         | (capi.DEBUG_SH_ONLY if r.get("showShOnly", False) else 0)
                         | (capi.DEBUG_OPACITY_GAUSSIAN_DISABLED if r.get("opacityGaussianDisabled", False) else 0))
        p.lighting_mode = self.lighting_mode
        return p

    def build_scene(self, device=0):
        """load the assets, add the instances in file order and commit (needs an MI355X)"""
        from . import capi
        sets = {sid: capi.SplatSet.load(path) for sid, path in self.splat_sets.items()}
        scene = capi.Scene(device)
        for inst in self.instances:
            if inst.splat_set_id not in sets:
                continue  # "Invalid splatSetId reference" is skipped by the reader (vkgs_project_reader.cpp:268-270)
            M, _ = capi.compute_transform(inst.scale, inst.rotation, inst.position)
            idx = scene.add_instance(sets[inst.splat_set_id], M)
            if inst.material is not None:
                scene.set_material(idx, capi.make_material(**inst.material))
        scene.commit(self.sh_format, self.rgba_format)
        if self.lights:
            scene.set_lights([capi.make_light(**l) for l in self.lights])
        self.add_meshes(scene)
        return scene

    def resolve_meshes(self):
        """loadMeshAssets / loadMeshInstances (vkgs_project_reader.cpp:353-454) on the host: (views, placed).  views: asset id -> the
        arrays of Mesh.view(); a mesh file that cannot be loaded is skipped with a warning.  An instance's "materials" overwrite the
        MESH's materials in order (they are shared by its instances, as in the reference: the last instance that carries them wins).
        placed: (asset id, transform) of every instance whose asset was loaded, in file order; an instance of an unknown asset is skipped"""
        import warnings
        from . import capi
        views = {}
        for aid, path in self.mesh_assets.items():
            try:
                views[aid] = capi.Mesh.load_obj(path).view()
            except capi.MgsError as e:
                warnings.warn(f"mesh asset {aid} ({path}) skipped: {e}")
        placed = []
        for inst in self.mesh_instances:
            v = views.get(inst["asset"])
            if v is None:
                continue
            for k, item in enumerate(inst.get("materials") or []):
                if k >= len(v["materials"]):
                    break
                for f in ("ambient", "diffuse", "specular", "emission"):
                    if f in item:
                        v["materials"][k][f] = tuple(float(x) for x in item[f])
                if "shininess" in item:
                    v["materials"][k]["shininess"] = float(item["shininess"])
            M, _ = capi.compute_transform(inst["scale"], inst["rotation"], inst["position"])
            placed.append((inst["asset"], M))
        return views, placed

    def add_meshes(self, scene):
        """adds the mesh instances of resolve_meshes() to `scene`; returns their mesh instance ids"""
        from . import capi
        views, placed = self.resolve_meshes()
        meshes, ids = {}, []
        for aid, M in placed:
            if aid not in meshes:
                v = views[aid]
                meshes[aid] = capi.Mesh.from_arrays(v["positions"], v["indices"], v["normals"], v["material_ids"],
                                                    [capi.make_material(**m) for m in v["materials"]])
            ids.append(scene.add_mesh_instance(meshes[aid], M))
        return ids


def _cam_from(item):
    c = Camera()
    if "eye" in item: c.eye = np.asarray(item["eye"], np.float32)
    if "ctr" in item: c.ctr = np.asarray(item["ctr"], np.float32)
    if "up" in item: c.up = np.asarray(item["up"], np.float32)
    if "fov" in item: c.fov = float(item["fov"])
    if "clip" in item: c.clip = (float(item["clip"][0]), float(item["clip"][1]))
    if "model" in item: c.model = int(item["model"])
    # old files carry "dofEnabled" (bool), newer ones "dofMode", which wins (vkgs_project_reader.cpp:579-582)
    if "dofEnabled" in item: c.dof_mode = int(bool(item["dofEnabled"]))
    if "dofMode" in item: c.dof_mode = int(item["dofMode"])
    if "focusDist" in item: c.focus_dist = float(item["focusDist"])
    if "aperture" in item: c.aperture = float(item["aperture"])
    return c


def _cam_to(c):
    return {"model": int(c.model), "ctr": [float(x) for x in c.ctr], "eye": [float(x) for x in c.eye], "up": [float(x) for x in c.up],
            "fov": float(c.fov), "clip": [float(c.clip[0]), float(c.clip[1])], "dofMode": int(c.dof_mode),
            "focusDist": float(c.focus_dist), "aperture": float(c.aperture)}


def _material_from(item):
    """LOAD3 / LOAD1 keep the default where a key is absent; the default is the splat sets' (emission 1, splat_set_vk.cpp:128-135)"""
    m = {"ambient": [0.0, 0.0, 0.0], "diffuse": [0.0, 0.0, 0.0], "specular": [0.0, 0.0, 0.0], "emission": [1.0, 1.0, 1.0], "shininess": 0.0}
    for k in ("ambient", "diffuse", "specular", "emission"):
        if k in item:
            m[k] = [float(x) for x in item[k]]
    if "shininess" in item:
        m["shininess"] = float(item["shininess"])
    return m


def _light_direction(rotation_deg):
    """the instance rotation applied to (0, 0, -1) (light_manager_vk.cpp:470-471, rotateDirection in utilities.h: the rotation of
    computeTransform)"""
    if not any(float(x) != 0.0 for x in rotation_deg):
        return [0.0, 0.0, -1.0]
    from . import capi
    M, _ = capi.compute_transform((1.0, 1.0, 1.0), rotation_deg, (0.0, 0.0, 0.0))
    return [float(x) for x in (np.asarray(M, np.float64)[:3, :3] @ np.array([0.0, 0.0, -1.0]))]


def _lights_from(section, version):
    """loadLights (vkgs_project_reader.cpp:616-770) -> dicts with the field names of MgsLight"""
    def asset_fields(a, v4):
        L = {"type": int(a.get("type", 1)), "color": [float(x) for x in a.get("color", (1.0, 1.0, 1.0))], "intensity": float(a.get("intensity", 1.0)),
             "range": 10.0, "inner_cone_deg": 30.0, "outer_cone_deg": 45.0, "attenuation_mode": 2, "radius": 1.0}
        if v4:  # "radius" of the result is LightSource::radius = proxyScale (light_manager_vk.cpp:480), the soft shadows' disk
            for src, dst, conv in (("range", "range", float), ("innerConeAngle", "inner_cone_deg", float), ("outerConeAngle", "outer_cone_deg", float),
                                   ("attenuationMode", "attenuation_mode", int), ("proxyScale", "radius", float)):
                if src in a:
                    L[dst] = conv(a[src])
        elif "radius" in a:  # the old "radius" is the new "range"
            L["range"] = float(a["radius"])
        return L

    out = []
    if version >= 3 and isinstance(section, dict) and "assets" in section and "instances" in section:
        assets = {int(a["id"]): a for a in section["assets"]}
        for inst in section["instances"]:
            L = asset_fields(assets[int(inst["assetId"])], version >= 4)
            if version >= 4:
                L["position"] = [float(x) for x in inst.get("translation", (0.0, 2.0, 0.0))]
                L["direction"] = _light_direction(inst.get("rotation", (0.0, 0.0, 0.0)))
            else:
                L["position"] = [float(x) for x in inst.get("position", (0.0, 2.0, 0.0))]
                L["direction"] = [0.0, 0.0, -1.0]
                if "scale" in assets[int(inst["assetId"])]:  # the old "scale" is the new "proxyScale" (:675-679)
                    L["radius"] = float(assets[int(inst["assetId"])]["scale"])
            out.append(L)
        return out
    items = section["items"] if isinstance(section, dict) and "items" in section else section
    for item in (items if isinstance(items, list) else []):
        L = asset_fields(item, False)
        L["position"] = [float(x) for x in item.get("position", (0.0, 2.0, 0.0))]
        L["direction"] = [0.0, 0.0, -1.0]
        out.append(L)
    return out


def load_project(path):
    with open(path) as f:
        data = json.load(f)
    base = os.path.dirname(os.path.abspath(path))
    pr = Project(version=int(data.get("version", 0)))
    if pr.version > PROJECT_FILE_VERSION:
        raise ValueError(f".vkgs version {pr.version} is newer than the supported {PROJECT_FILE_VERSION}")
    pr.renderer = dict(data.get("renderer", {}))
    if "camera" in data:
        pr.camera = _cam_from(data["camera"])
    pr.cameras = [_cam_from(c) for c in data.get("cameras", [])]
    g = data.get("splatsGlobals", {})
    pr.sh_format, pr.rgba_format = int(g.get("shFormat", 0)), int(g.get("rgbaFormat", 0))
    if "splatSets" in data:
        for item in data["splatSets"]:
            pr.splat_sets[int(item["id"])] = os.path.normpath(os.path.join(base, item["path"]))
        for item in data.get("splats", []):
            inst = SplatInstance(int(item["splatSetId"]), item.get("name", ""))
            if all(k in item for k in ("position", "rotation", "scale")):
                inst.position, inst.rotation, inst.scale = tuple(item["position"]), tuple(item["rotation"]), tuple(item["scale"])
            if "material" in item:
                inst.material = _material_from(item["material"])
            pr.instances.append(inst)
    else:  # legacy (version 0): every splat entry carries its own path
        for i, item in enumerate(data.get("splats", [])):
            pr.splat_sets[i] = os.path.normpath(os.path.join(base, item["path"]))
            inst = SplatInstance(i, item.get("name", ""))
            if all(k in item for k in ("position", "rotation", "scale")):
                inst.position, inst.rotation, inst.scale = tuple(item["position"]), tuple(item["rotation"]), tuple(item["scale"])
            if "material" in item:
                inst.material = _material_from(item["material"])
            pr.instances.append(inst)
    pr.extra = {k: v for k, v in data.items()
                if k not in ("version", "renderer", "camera", "cameras", "splatsGlobals", "splatSets", "splats")}
    if "lights" in data:
        pr.lights = _lights_from(data["lights"], pr.version)
    # loadMeshes (vkgs_project_reader.cpp:459-558); the sections stay in `extra` and are written back as read
    def instance(it, asset):
        return dict(asset=asset, name=it.get("name", ""), position=tuple(it.get("position", (0.0, 0.0, 0.0))),
                    rotation=tuple(it.get("rotation", (0.0, 0.0, 0.0))), scale=tuple(it.get("scale", (1.0, 1.0, 1.0))),
                    materials=it.get("materials"))
    if pr.version >= 2 and "meshAssets" in data and "meshInstances" in data:  # separate assets and instances (:461-475)
        for a in data["meshAssets"] if isinstance(data["meshAssets"], list) else []:
            pr.mesh_assets[int(a["id"])] = os.path.normpath(os.path.join(base, a["path"]))
        mi = data["meshInstances"]
        items = mi["items"] if isinstance(mi, dict) and "items" in mi else mi if isinstance(mi, list) else []
        for it in items:
            pr.mesh_instances.append(instance(it, int(it["meshAssetId"])))
    elif "meshes" in data:  # version 0 (a list) and version 1 ({"items": [...]}): every entry loads its own mesh and is its one instance (:476-553)
        ms = data["meshes"]
        items = ms["items"] if isinstance(ms, dict) and "items" in ms else ms if isinstance(ms, list) else []
        for k, it in enumerate(items):
            if not it.get("path"):
                continue
            pr.mesh_assets[k] = os.path.normpath(os.path.join(base, it["path"]))  # the entry's index stands in for an asset id
            pr.mesh_instances.append(instance(it, k))
    return pr


def save_project(pr, path):
    base = os.path.dirname(os.path.abspath(path))
    data = {"version": PROJECT_FILE_VERSION, "renderer": dict(pr.renderer), "camera": _cam_to(pr.camera),
            "cameras": [_cam_to(c) for c in pr.cameras],
            "splatsGlobals": {"shFormat": pr.sh_format, "rgbaFormat": pr.rgba_format},
            "splatSets": [{"id": sid, "path": os.path.relpath(p, base), "storage": 0, "shFormat": pr.sh_format,
                           "rgbaFormat": pr.rgba_format} for sid, p in sorted(pr.splat_sets.items())],
            "splats": [dict({"splatSetId": i.splat_set_id, "name": i.name, "position": list(i.position),
                             "rotation": list(i.rotation), "scale": list(i.scale)},
                            **({"material": dict(i.material)} if i.material is not None else {})) for i in pr.instances]}
    data.update(pr.extra)  # the raw "lights" section among them, unchanged
    with open(path, "w") as f:
        json.dump(data, f, indent=4)
