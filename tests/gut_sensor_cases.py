"""The cases of the sensor-model tests (mgs_frame_set_sensor): small scenes of tests/gut_cases.py on frames of at most 152x104 pixels,
ragged against the 16-px tile and the 32x16-px region, each with one sensor model.  Shared by tests/test_gut_sensor_cpu.py (which
asserts each case's premise from the float64 restatement tests/np_gut_sensor.py alone) and tests/test_gpu_gut_sensor.py.

Sensors: `identity_*` is mgs_sensor_model_from_frame's perfect model; `mild` a calibrated pinhole with every coefficient non-zero and
the principal point 10 % off centre; `strong` a pinhole whose radial factor leaves (0.8, 1.2) inside the image, so that sigma points
of splats near the border take the clipped fallback while their mean does not and corner pixels have no ray; `ocv_fisheye` a fisheye
polynomial with four terms and a max_angle that cuts inside the image's corners."""
import functools

import numpy as np

import gut_cases as gc
import np_gut
import np_gut_sensor as ns

DELTA = gc.DELTA
W_PIN, H_PIN = 152, 104
W_FISH, H_FISH = 120, 120
CASES = ["identity_pinhole", "identity_fisheye", "mild", "strong", "ocv_fisheye"]
SEED = dict(pinhole=71, fisheye=14)

# The float32 run of the WHOLE restatement (np_gut_sensor._twin: the front end, the sensor's projection and Newton, the rays, the
# particle response and the blend in numpy float32) against its float64 run, MEASURED by
# test_gut_sensor_cpu.py::test_float32_run_of_the_restatement, which fails when a measurement exceeds its entry or falls below a
# quarter of it: GAUSS_DEV, the float32 frame's largest distance from the float64 interval on the pixels the float64 run does not set
# aside (the mask the GPU test uses); RAY_RESIDUAL, the largest distance of the float64 projection of a float32 ray (fixed-count Newton,
# rotation and normalisation in float32) from its pixel's centre, in pixels.  The kernels' bars are gc.BAR_FACTOR times these figures
# and nothing else.
GAUSS_DEV = {"identity_pinhole": 4.9e-06, "identity_fisheye": 4.8e-06, "mild": 6.5e-06, "strong": 4.6e-06, "ocv_fisheye": 3.7e-06}
RAY_RESIDUAL = {"identity_pinhole": 1.6e-05, "identity_fisheye": 1.2e-05, "mild": 2.3e-05, "strong": 1.3e-05, "ocv_fisheye": 1.3e-05}
# The records' bars are borrowed, as the issue allows: BAR_FACTOR times the oracle's measured deviations (gc.ORACLE_DEV) on the gut_cases
# frame with the same particle recipe, camera and settings.  Those frames are 200x136 / 136x136 and lack `strong`'s corner particles, so
# the kinship is the recipe, not the picture.
RECORD_BASE = {"identity_pinhole": "cloud+eigen+s05", "mild": "cloud+eigen+s05", "strong": "cloud+eigen+s05", "identity_fisheye": "fisheye150", "ocv_fisheye": "fisheye150"}


# icD = 1 - 0.22 r2 leaves (0.8, 1.2) where r2 > 0.909: the frame's corners (r2 up to 1.04 at tan(fov / 2) = 0.577, aspect 152 / 104)
STRONG_RADIAL = (-0.22, 0.0, 0.0, 0.0, 0.0, 0.0)


def _with_corner_particles(arrays, V, eye):
    """24 particles around the icD limit of `strong` (normalised radius^2 0.909), some three units from the camera, whose sigma points
    (sqrt(3) * 0.08 / 3 = 0.046 to either side in normalised coordinates) straddle it"""
    V = np.asarray(V, np.float64)
    right, up, fwd = V[0, :3], V[1, :3], -V[2, :3]
    rng = np.random.default_rng(7)   # chosen so that the case stays inside the caps
    pos = []
    for j in range(24):
        r = np.sqrt(0.909) + rng.uniform(-0.03, 0.03)
        phi = np.arctan2(0.577, 0.843) * (1 if j % 2 else -1) + (np.pi if j % 4 >= 2 else 0.0) + rng.uniform(-0.12, 0.12)
        pos.append(eye + (2.7 + 0.025 * j) * (fwd + r * np.cos(phi) * right + r * np.sin(phi) * up))   # (no two at the same depth)
    n = arrays["positions"].shape[0] + 24
    extra = dict(positions=np.asarray(pos, np.float32), scale=np.full((24, 3), np.log(0.08), np.float32),
                 rotation=np.tile(np.float32([1, 0, 0, 0]), (24, 1)), opacity=np.full(24, 2.0, np.float32))
    out = {k: np.concatenate([arrays[k], extra[k]]) for k in extra}
    out["f_dc"], out["f_rest"] = gc.id_colour(n), np.zeros((n, 9), np.float32)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """gc.case's dict plus `sensor` (np_gut_sensor.sensor); st carries it as st["sensor"]"""
    fish = name in ("identity_fisheye", "ocv_fisheye")
    params = {}
    if fish:
        W, H = W_FISH, H_FISH
        sets = [(gc.make_set(np.random.default_rng(SEED["fisheye"]), 400, (2.0, 2.0, 2.0), (-3.4, -1.6)), None)]
        cam = gc.camera((0.05, 0.1, 0.3), (0.2, 0.0, -1.0), 150.0, W, H)
        st = np_gut.settings(camera_model=1)
        params["camera_model"] = 1
    else:
        W, H = W_PIN, H_PIN
        cam = gc.camera((2.6, 1.0, 1.4), (0, 0, 0), 60.0, W, H)
        arrays = gc.make_set(np.random.default_rng(SEED["pinhole"]), 400, (1.2, 0.8, 1.2), (-4.2, -1.8))
        if name == "strong":
            arrays = _with_corner_particles(arrays, cam[0], np.asarray(cam[2], np.float64))
        sets = [(arrays, None)]
        st = np_gut.settings(extent_method=0, splat_scale=0.5)   # the frame of gc's "cloud+eigen+s05"
        params.update(extent_method=0, splat_scale=0.5)
    ident = ns.from_frame(cam[1], W, H, st)
    f, pp = ident["focal_length"], ident["principal_point"]
    if name.startswith("identity"):
        sn = ident
    elif name == "mild":
        sn = ns.sensor(ns.PINHOLE, f * (1.02, 0.99), pp + (0.1 * W, -0.1 * H), radial=(-0.12, 0.03, -0.004, 0.02, 0.006, 0.001),
                       tangential=(0.004, -0.003), thin_prism=(0.002, -0.001, -0.0015, 0.0008))
    elif name == "strong":
        sn = ns.sensor(ns.PINHOLE, f, pp, radial=STRONG_RADIAL)
    elif name == "ocv_fisheye":
        sn = ns.sensor(ns.FISHEYE, f, pp + (3.0, -2.0), fisheye_radial=(0.04, -0.012, 0.0025, -0.0003), max_angle=1.5)
    else:
        raise KeyError(name)
    st = dict(st, sensor=sn)
    return dict(name=name, sets=sets, cam=cam, W=W, H=H, st=st, params=params, sensor=sn)


def sensor_fields(name):
    """the sensor as keyword fields of capi.SensorModel.update"""
    sn = case(name)["sensor"]
    return {k: (sn[k] if k in ("model", "max_angle") else [float(x) for x in sn[k]]) for k in ns.FIELDS}


@functools.lru_cache(maxsize=None)
def projected(name, dtype="float64"):
    c = case(name)
    V, P, _ = c["cam"]
    log = []
    st = dict(c["st"], pipeline_dtype=np.dtype(dtype).type, sensor_log=log)
    prs = [ns.project(a, m, V, P, c["W"], c["H"], st, DELTA) for a, m in c["sets"]]
    for pr in prs:
        pr["sensor_log"] = log
    return prs


@functools.lru_cache(maxsize=None)
def reference_fragments(name, degree=2):
    c = case(name)
    V, P, _ = c["cam"]
    return ns.fragments(projected(name), V, P, c["W"], c["H"], dict(c["st"], kernel_degree=degree), False, DELTA, None)


def _blend(name, dtype):
    c = case(name)
    V, P, _ = c["cam"]
    st = dict(c["st"], pipeline_dtype=np.dtype(dtype).type)
    fr = ns.fragments(projected(name, dtype), V, P, c["W"], c["H"], st, True, DELTA, None)
    lo, hi = fr.blend(np.concatenate([gc.colour_table(a["positions"].shape[0]) for a, _ in c["sets"]]).astype(dtype))
    return lo, hi, ((hi - lo).max(-1) > gc.GAUSS_FRAGILE) | fr.order_open | (fr.rays[2] <= DELTA)


@functools.lru_cache(maxsize=None)
def reference_blend(name):
    """(lo, hi, fragile) as gc.reference_blend; a pixel whose ray is within the margin of not existing is fragile too"""
    return _blend(name, "float64")


@functools.lru_cache(maxsize=None)
def float32_blend(name):
    """the same restatement, all of it, in numpy float32 (np_gut_sensor._twin): the interval's lower edge serves as its frame"""
    return _blend(name, "float32")


@functools.lru_cache(maxsize=None)
def rays(name, dtype="float64"):
    """(view-space directions [H, W, 3], has_ray, edge, residual in pixels) of every pixel's centre"""
    c = case(name)
    yy, xx = np.mgrid[0:c["H"], 0:c["W"]]
    t = np.dtype(dtype).type
    return ns.unproject(c["sensor"], xx + 0.5, yy + 0.5, c["W"], c["H"], None if t == np.float64 else ns.NEWTON_ITERS, t)


def world_rays(name, dtype="float64"):
    """the rays as the library hands them out: rotated to world space by viewInverse and normalised, in the arithmetic of dtype"""
    c = case(name)
    t = np.dtype(dtype).type
    d = rays(name, dtype)[0]
    Vi = np.linalg.inv(np.asarray(c["cam"][0], np.float64))[:3, :3].astype(t)
    w = d @ Vi.T
    return w / np.sqrt((w * w).sum(-1, keepdims=True))


def ray_residual(name, world_dirs):
    """per pixel, the distance (pixels, larger of x and y) of the float64 projection of world_dirs [H, W, 3] from the pixel's centre"""
    c = case(name)
    V = np.asarray(c["cam"][0], np.float64)
    px, _ = ns.forward_pixels(c["sensor"], np.asarray(world_dirs, np.float64) @ V[:3, :3].T, c["W"], c["H"])
    yy, xx = np.mgrid[0:c["H"], 0:c["W"]]
    return np.maximum(np.abs(px[..., 0] - xx - 0.5), np.abs(px[..., 1] - yy - 0.5))
