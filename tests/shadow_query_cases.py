"""The batches of the shadow and light query tests (test_shadow_query_cpu.py, test_gpu_shadow_query.py), numpy only.  Scenes are
trace_lit_cases': MAIN = l11_materials (a floor and two blob instances under TRS transforms), STACK = the l08_kcut scene (a tall stack
of more faint occluders than slots).  Every batch is built from a fixed seed; restatements are computed once per process and shared:
do not modify what these functions return."""
import functools

import numpy as np

import np_lighting as nl
import np_shadow_query as nsq
import np_trace_lit as ntl
import trace_lit_cases as lc

MAIN, STACK = "l11_materials", "l08_kcut_18"
N = 2000
INVALID_AT = (7, 255, 256, 1023, 1999)
POINT = np.array((0.3, 1.6, 0.2))
SPOT = np.array((-0.2, 1.4, 0.1))
SUN = np.array((-0.3, -1.0, -0.2))
KMR, ACULL = 0.0113, 1.0 / 255.0

# ray configurations: MgsTraceLightParams knobs, debug bits, samples_per_pass; `rays` names the batch
RAY_CONFIGS = {
    "default": dict(rays="main", threshold=0.8, strength=0.0),
    "thr0_tint": dict(rays="main", threshold=0.0, strength=1.0),
    "sh_only": dict(rays="main", threshold=0.3, strength=1.0, debug=2),
    "no_gauss": dict(rays="main", threshold=0.3, strength=0.0, debug=4),
    **{f"stack_{k}": dict(rays="stack", threshold=0.05, strength=0.0, spp=k) for k in (1, 4, 18, 32)},
}
# The transmittance bar.  test_gpu_trace_lit.py holds the light pass to an image PSNR and has no separable bar for the shadow term,
# so the bar is gut_cases.BAR_FACTOR times the largest distance, over the non-fragile rays of a configuration, between the float32
# run of the restatement (np_shadow_query's dt) and the float64 one.  test_shadow_query_cpu.py::test_float32_run_of_the_restatement
# fails when a measurement exceeds its entry or falls below a third of it.
TWIN_DEV = {"default": 2.5e-6, "thr0_tint": 1.3e-6, "sh_only": 1.7e-6, "no_gauss": 0.0, "stack_1": 6.5e-8, "stack_4": 6.5e-8, "stack_18": 1.1e-7,
            "stack_32": 1.1e-7}

LIGHTS = [nl.default_light(position=tuple(POINT), range=2.3, intensity=4.0),  # out of range for the far part of the points
          nl.default_light(type=nl.LIGHT_SPOT, position=tuple(SPOT), direction=(0.1, -1.0, 0.0), range=10.0, intensity=5.0,
                           inner_cone_deg=14.0, outer_cone_deg=24.0),
          nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=tuple(SUN), intensity=0.5)]
MATERIALS = [nl.default_material(), dict(lc.SHADED, specular=(0.5, 0.5, 0.5), shininess=64.0),
             dict(lc.SHADED, diffuse=(0.0, 0.0, 0.0), ambient=(0.6, 0.6, 0.6))]
POINT_CONFIGS = {"three_lights": dict(lights=LIGHTS, shadows=1), "headlight": dict(lights=[], shadows=1), "no_shadows": dict(lights=LIGHTS, shadows=0),
                 # the K-buffer's ends (samples_per_pass; the others take the default 18): k_shade_points has an instantiation per size
                 "three_lights_spp_4": dict(lights=LIGHTS, shadows=1, spp=4), "three_lights_spp_32": dict(lights=LIGHTS, shadows=1, spp=32)}
CAMERA = (0.0, 1.3, 2.6)


def scene(name):
    return lc.cases()[name]["sets"]


@functools.lru_cache(maxsize=None)
def prepared(name):
    return nsq.per_inst([(ntl.prepare_set(a), M) for a, M in scene(name)], float(np.float32(KMR)), float(np.float32(ACULL)), True)


def _toward(o, target):
    d = target - o
    return d, np.linalg.norm(d, axis=1)


@functools.lru_cache(maxsize=None)
def ray_batch(which="main"):
    """(O [n,3], D [n,3], tmin [n], tmax [n]) float32"""
    rng = np.random.Generator(np.random.PCG64(3 if which == "main" else 4))
    n = N if which == "main" else 600
    O = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.34, -0.15, n), rng.uniform(-1.2, 1.2, n)], 1)
    if which == "stack":  # from just above the floor through the stack toward the point light, unit directions
        d, dist = _toward(O, POINT)
        return O.astype(np.float32), (d / dist[:, None]).astype(np.float32), np.zeros(n, np.float32), dist.astype(np.float32)
    kind = rng.integers(0, 100, n)
    outside = (kind >= 70) & (kind < 80)  # origins outside the scene box: below the floor and far to the side
    O[outside] = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-2.5, -1.0, n), rng.uniform(-3.0, 3.0, n)], 1)[outside]
    target = np.where((kind % 3 == 0)[:, None], SPOT[None], POINT[None])
    d, dist = _toward(O, target)
    D, tmin, tmax = d / dist[:, None], np.zeros(n), dist.copy()
    sun = (kind >= 40) & (kind < 55)      # "directional": t_max = 1e10
    D[sun], tmax[sun] = (-SUN / np.linalg.norm(SUN))[None], 1e10
    scale = np.where((kind >= 55) & (kind < 70), rng.uniform(0.3, 3.0, n), 1.0)  # non-unit directions: t runs along them
    D, tmax = D * scale[:, None], np.where(sun, tmax, tmax / scale)
    cut_lo = (kind >= 80) & (kind < 90)   # a window that starts behind the first occluders
    tmin[cut_lo] = (rng.uniform(0.1, 0.9, n) * tmax)[cut_lo]
    cut_hi = kind >= 90                   # a window that ends between the occluders
    tmax[cut_hi] = (rng.uniform(0.2, 0.9, n) * tmax)[cut_hi]
    O, D, tmin, tmax = O.astype(np.float32), D.astype(np.float32), tmin.astype(np.float32), tmax.astype(np.float32)
    bad = list(INVALID_AT)
    O[bad[0], 1] = np.nan
    D[bad[1], 0] = np.inf
    D[bad[2]] = 0.0
    tmin[bad[3]], tmax[bad[3]] = 2.0, 1.0
    tmax[bad[4]] = np.nan
    return O, D, tmin, tmax


def _ray_kw(cfg, dt=np.float64):
    dbg = cfg.get("debug", 0)
    return dict(K=cfg.get("spp", 18), threshold=cfg["threshold"], strength=cfg["strength"], sh_only=bool(dbg & 2), no_gauss=bool(dbg & 4), dt=dt)


@functools.lru_cache(maxsize=None)
def restate_rays(name, f32=False):
    cfg = RAY_CONFIGS[name]
    return nsq.shadow_rays(prepared(MAIN if cfg["rays"] == "main" else STACK), *ray_batch(cfg["rays"]), **_ray_kw(cfg, np.float32 if f32 else np.float64))


def restate_rays_with(name, pinst):
    cfg = RAY_CONFIGS[name]
    return nsq.shadow_rays(pinst, *ray_batch(cfg["rays"]), **_ray_kw(cfg))


@functools.lru_cache(maxsize=None)
def point_batch():
    """surface points on and around the floor of MAIN, looking down from CAMERA: a structured array (capi.SURFACE_POINT_DTYPE's fields)"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = N
    dt = np.dtype([("position", np.float32, 3), ("material", np.uint32), ("normal", np.float32, 3), ("_pad0", np.float32),
                   ("view_dir", np.float32, 3), ("_pad1", np.float32), ("radiance", np.float32, 3), ("_pad2", np.float32)])
    p = np.zeros(n, dt)
    pos = np.stack([rng.uniform(-1.3, 1.3, n), rng.uniform(-0.34, -0.2, n), rng.uniform(-1.3, 1.3, n)], 1)
    nrm = np.array((0.0, 1.0, 0.0))[None] + rng.uniform(-0.3, 0.3, (n, 3))
    nrm *= rng.uniform(0.5, 2.0, n)[:, None]          # the call normalises
    short = rng.integers(0, 10, n) == 0                # shorter than 0.2: replaced by -view_dir
    nrm[short] *= (0.1 / np.linalg.norm(nrm[short], axis=1))[:, None]
    view = pos - np.asarray(CAMERA)[None]
    view /= np.linalg.norm(view, axis=1, keepdims=True)
    p["position"], p["normal"], p["view_dir"], p["radiance"] = pos, nrm, view, rng.uniform(0.2, 1.0, (n, 3))
    p["material"] = rng.integers(0, 3, n)
    bad = list(INVALID_AT)
    p["position"][bad[0], 2] = np.inf
    p["normal"][bad[1], 0] = np.nan
    p["view_dir"][bad[2], 1] = np.nan
    p["radiance"][bad[3], 0] = np.inf
    p["material"][bad[4]] = 3                          # out of range (the device variant: an invalid point)
    return p


@functools.lru_cache(maxsize=None)
def restate_points(name):
    cfg = POINT_CONFIGS[name]
    return nsq.shade_points(prepared(MAIN), point_batch(), MATERIALS, cfg["lights"], CAMERA, shadows=cfg["shadows"], offset=0.2, threshold=0.8, strength=0.0,
                            K=cfg.get("spp", 18))
