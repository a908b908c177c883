"""The scenes of the soft-shadow tests (test_trace_soft_cpu.py, test_gpu_trace_soft.py), numpy only: trace_lit_cases' floor and blobs
in 48 x 40 frames, every case with shadows_mode = 2 and a `radii` list beside its lights (mgs_scene_set_light_radii) and a
`hybrid` flag (mgs_render_hybrid, restated from the device's own raster G-buffer as hybrid_cases does).  restate(name, sample_id)
runs the float64 restatement once per process and sample.
A case with `meshes` is a lit frame with trace meshes (mgs_frame_set_trace_meshes), restated by np_trace_soft.mesh_frame."""
import functools

import numpy as np

import hybrid_cases as hc
import np_lighting as nl
import np_trace_lit as ntl
import np_trace_soft as nts
import trace_cases as tc
import trace_lit_cases as lc
import trace_mesh_cases as tmc

FRAGILE_CAP = 0.05  # the lit suite's ok.mean() >= 0.95
SOFT = dict(shadows_mode=2)


def _case(sets, lights, radii, hybrid=None, **kw):
    kw["light"] = dict(SOFT, **(kw.get("light") or {}))
    c = hc._case(sets, lights, hybrid, **kw) if hybrid is not None else lc._case(sets, lights, **kw)
    c.update(radii=list(radii), hybrid=hybrid is not None)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    scene = lc.join(lc.floor(), lc.blob())
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), intensity=1.0)
    spot = nl.default_light(type=nl.LIGHT_SPOT, position=(-0.2, 1.4, 0.1), direction=(0.1, -1.0, 0.0), range=10.0, intensity=5.0,
                            inner_cone_deg=14.0, outer_cone_deg=24.0)
    c = {}
    # 1. a real penumbra: the disk (radius 0.3) is wider than the occluder's splats
    c["s01_penumbra"] = _case([(scene, tc.I4)], [point], [0.6])
    # 2. draw order and no-draw lights: the spot draws two numbers, the sun and the radius-0 point light none
    c["s02_order"] = _case([(scene, tc.I4)], [spot, dict(sun, intensity=0.5), dict(point, intensity=2.0)], [0.5, 0.7, 0.0])
    # 3. the range (1.4) cuts through the floor: within 0.25 of it the sample's distance decides, not the centre's
    c["s03_range"] = _case([(scene, tc.I4)], [nl.default_light(position=(0.9, 0.4, 0.0), range=1.4, intensity=2.0, attenuation_mode=1)], [0.5])
    # 4. the K-buffer's ends
    # (with 32 slots every neighbouring pair of up to 33 candidates is an order decision: the taller stack of trace_lit_cases is past
    # the fragile cap there, 0.059 of the frame; 45 splats of another seed leave up to 26 hits on a ray and 0.049)
    for k, n, seed in ((1, 60, 21), (32, 45, 22)):
        stack = lc.join(lc.floor(), lc.blob(n=n, centre=(0.0, 0.45, 0.0), radius=0.5, opacity=-2.2, seed=seed, log_scale=-1.8))
        c[f"s04_kcut_{k}"] = _case([(stack, tc.I4)], [point], [0.6], light=dict(particle_shadow_transmittance_threshold=0.05), trace=dict(samples_per_pass=k))
    # 5. the lens seeds its own copy of the state
    c["s05_fisheye_dof"] = _case([(scene, tc.I4)], [point], [0.6], frame=dict(camera_model=1, fov_rad=1.4, dof_mode=1, focus_dist=2.9, aperture=0.004))
    # 6. a lit mesh frame: the mesh floor and the OBJ fixture under a translucent veil with a shaded material (both loops over the
    # lights run where the veil is picked in front of a mesh) beside a blob with the default material (needShading 0: the mesh loop
    # starts from the fresh seed behind it, as it does where nothing is picked); two lights with a radius
    veil = lc.blob(centre=(-0.3, 0.15, 0.3), opacity=0.0, seed=5, n=30)  # (40 splats: 0.054 of the frame fragile, past the cap)
    glow = lc.blob(centre=(0.55, 0.1, 0.2), opacity=0.0, seed=6, n=30)
    c["s06_mesh"] = _case([(veil, tc.I4), (glow, tc.I4)], [point, dict(spot, range=10.0)], [0.6, 0.4], materials=[lc.SHADED, nl.default_material()])
    c["s06_mesh"].update(meshes=[tmc.placed(tmc.FLOOR, materials=[tmc.MAT_SHADED, tmc.MAT_SPEC]), tmc.fixture(tc.trs((0.3, 0.3, 0.3), (0, 1, 0), 25.0, (-0.8, -0.32, 0.3)))], mesh_min_T=0.0)
    # (the K-buffer's ends of the two lit mesh kernels' soft instantiations: the same frame at samples_per_pass 4 and 32)
    for k in (4, 32):
        c[f"s06_mesh_spp_{k}"] = dict(c["s06_mesh"], trace=dict(c["s06_mesh"]["trace"], samples_per_pass=k))
    # 7. hybrid frames, both raster pipelines
    c["s07_hybrid_3dgs"] = _case([(scene, tc.I4)], [point], [0.6], hybrid=hc.GS)
    c["s07_hybrid_3dgut"] = _case([(scene, tc.I4)], [point], [0.6], hybrid=hc.GUT)
    return c


def traced():
    return sorted(n for n, c in cases().items() if not c["hybrid"] and "meshes" not in c)


def meshed():
    return sorted(n for n, c in cases().items() if "meshes" in c)


def hybrids():
    return sorted(n for n, c in cases().items() if c["hybrid"])


def _light_kw(c):
    L = c["light"]
    return dict(shadows=L.get("shadows_mode", 0), offset=L.get("particle_shadow_offset", 0.2),
                threshold=L.get("particle_shadow_transmittance_threshold", 0.8), strength=L.get("particle_shadow_color_strength", 0.0))


@functools.lru_cache(maxsize=None)
def prepared(name):
    return [(ntl.prepare_set(a), M) for a, M in cases()[name]["sets"]]


@functools.lru_cache(maxsize=None)
def base(name):
    """np_trace.trace of a traced case without a lens (the primary walk does not depend on the sample id then); do not modify"""
    c = cases()[name]
    return nts.trace(prepared(name), c["V"], c["P"], c["W"], c["H"], **lc._trace_kw(c))


@functools.lru_cache(maxsize=None)
def restate(name, sample_id=0, radii=None):
    """the restatement of a traced case (radii: a tuple overriding the case's); computed once and shared: do not modify the result"""
    c = cases()[name]
    kw = lc._trace_kw(c)
    b = None
    if kw["dof"] is not None:
        kw["dof"] = kw["dof"][:2] + (sample_id,)
    else:
        b = base(name)
    return nts.lit(prepared(name), c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"], radii=c["radii"] if radii is None else list(radii),
                   sample_id=sample_id, base=b, **_light_kw(c), **kw)


@functools.lru_cache(maxsize=None)
def restate_mesh(name, sample_id=0, radii=None):
    """the restatement of a lit mesh frame; computed once and shared: do not modify the result"""
    c = cases()[name]
    return nts.mesh_frame(prepared(name), c["meshes"], [m["materials"] for m in c["meshes"]], c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"],
                          c["materials"], radii=c["radii"] if radii is None else list(radii), sample_id=sample_id, lit=True,
                          mesh_min_T=c["mesh_min_T"], **_light_kw(c), **lc._trace_kw(c))


def restate_hybrid(name, gbuffer, sample_id=0):
    """gbuffer = (image as stored, picked depth, ids in the caller's order, integrated normal) of the unlit raster frame"""
    c = cases()[name]
    kw = lc._trace_kw(c)
    image, depth, ids, normal = gbuffer
    return nts.hybrid_lit(image, depth, ids, normal, prepared(name), c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"],
                          radii=c["radii"], sample_id=sample_id, **_light_kw(c), **kw)
