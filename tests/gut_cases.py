"""The scenes of the 3DGUT record and fragment tests, shared by tests/test_gut_cpu.py (which holds the oracle to the float64
restatement of tests/np_gut.py, asserts each case's premise from the restatement alone and measures the oracle's own deviations) and
tests/test_gpu_gut_records.py (which holds the kernels to the same restatement).

A case = splat sets with instance matrices, a camera, a frame size ragged against the 16-px tile and the 32x16-px region, and the
frame's settings.  Seeded: the same particles every time."""
import functools

import numpy as np

import np_gut
from fragment_cases import _trs, lookat, persp

DELTA = 1e-4                       # relative distance from a threshold below which fp32 may decide either way (np_gut.py)
FRAGILE_CAP = 0.02                 # at most this share of a case's emitted particles may be fragile
BORDERLINE_CAP = {"default": 0.02, "shapes": 0.05, "fisheye150": 0.05, "fisheye175": 0.05}   # ... and of its pixels borderline
SH_C0 = 0.28209479177387814

# The oracle's largest deviation from the restatement per field, over the non-fragile emitted particles of every case: MEASURED by
# test_gut_cpu.py::test_oracle_records_match_the_restatement, which fails when a measurement exceeds its entry here.  The kernels'
# bar (test_gpu_gut_records.py) is BAR_FACTOR times the entry: they use the hardware's 1-ulp rcp / sqrt / exp / log where the oracle
# rounds correctly, and fold the affine map differently (mean once, axis offsets through the 3x3).  DESIGN.md has the table per case.
BAR_FACTOR = 4.0
ORACLE_DEV = {
    "cloud": dict(centre=3.5e-06, q=2.8e-06, box=2.8e-06, B=4.0e-07, ro=6.2e-07, opacity=9.1e-08),
    "cloud+eigen": dict(centre=3.1e-06, q=9.0e-06, box=8.3e-06, B=4.0e-07, ro=6.2e-07, opacity=9.1e-08),
    "cloud+msaa+flip": dict(centre=3.7e-06, q=2.8e-06, box=2.8e-06, B=4.0e-07, ro=6.2e-07, opacity=2.8e-06),
    "cloud+eigen+s05": dict(centre=6.2e-06, q=9.0e-06, box=8.3e-06, B=4.0e-07, ro=6.2e-07, opacity=9.1e-08),
    "trs": dict(centre=3.4e-06, q=1.9e-06, box=1.9e-06, B=5.5e-07, ro=6.6e-07, opacity=1.1e-07),
    "trs+eigen+msaa+s2": dict(centre=1.1e-06, q=1.6e-05, box=8.9e-06, B=5.5e-07, ro=6.6e-07, opacity=5.8e-06),
    "inside": dict(centre=3.2e-07, q=2.1e-06, box=2.1e-06, B=4.7e-07, ro=6.8e-07, opacity=8.5e-08),
    "inside+eigen": dict(centre=2.8e-07, q=3.4e-06, box=1.9e-06, B=4.7e-07, ro=6.8e-07, opacity=8.5e-08),
    "inside+flip": dict(centre=3.2e-07, q=2.1e-06, box=2.1e-06, B=4.7e-07, ro=6.8e-07, opacity=8.5e-08),
    "fisheye150": dict(centre=3.1e-06, q=2.1e-06, box=2.1e-06, B=3.6e-07, ro=5.0e-07, opacity=8.8e-08),
    "fisheye150+flip": dict(centre=3.1e-06, q=2.1e-06, box=2.1e-06, B=3.6e-07, ro=5.0e-07, opacity=8.8e-08),
    "fisheye175": dict(centre=3.5e-06, q=2.4e-06, box=2.4e-06, B=3.6e-07, ro=5.0e-07, opacity=8.8e-08),
    "shapes": dict(centre=8.2e-06, q=1.7e-06, box=1.7e-06, B=3.8e-07, ro=5.5e-06, opacity=9.5e-08),
    "shapes+eigen": dict(centre=3.1e-06, q=5.1e-05, box=3.1e-05, B=3.8e-07, ro=5.5e-06, opacity=8.2e-08),
    "opacity": dict(centre=9.8e-06, q=1.4e-06, box=1.4e-06, B=3.6e-07, ro=5.7e-07, opacity=9.2e-08),
    "opacity+msaa": dict(centre=1.1e-05, q=1.6e-06, box=1.6e-06, B=3.6e-07, ro=5.7e-07, opacity=2.3e-07),
    "strip": dict(centre=3.2e-06, q=2.7e-06, box=2.7e-06, B=4.0e-07, ro=6.2e-07, opacity=9.1e-08),
}


SEED = dict(cloud=71, trs=22, inside=73, fisheye=14, shapes=33, opacity=31)   # chosen so that every case stays inside the caps


def id_colour(n, offset=0):
    """f_dc such that the base colour 0.5 + SH_C0 f_dc of particle i is ((i & 31) + 1, ((i >> 5) & 31) + 1, 15) / 51: multiples of 5 / 255,
    which the uint8 colour storage keeps as they are (the fp16 storage rounds them by 2e-4 at most)"""
    return ((colour_table(n, offset) - 0.5) / SH_C0).astype(np.float32)


def colour_table(n, offset=0):
    i = np.arange(n) + offset
    return np.stack([(i & 31) + 1, ((i >> 5) & 31) + 1, np.full(n, 15)], 1) / 51.0


def decode_colour(rgb, tol=1e-3):
    """index of id_colour's colour in its set, -1 where the pixel is none of them.  tol (in steps of 1/51): 1e-3 for the fp32 storage;
    0.25 where the storage formats round (fp16 colours: 0.01 steps; uint8 SH of zeros dequantise to 1/255: 0.17 steps of radiance)"""
    v = np.asarray(rgb, np.float64) * 51.0
    k = np.rint(v).astype(np.int64)
    ok = (k[..., 2] == 15) & (np.abs(v - k).max(-1) < tol) & (k[..., 0] >= 1) & (k[..., 1] >= 1)
    return np.where(ok, (k[..., 0] - 1) + 32 * (k[..., 1] - 1), -1)


def make_set(rng, n, box, log_scale, opacity=(-1.0, 4.0), centre=(0, 0, 0)):
    q = rng.normal(size=(n, 4))
    lo, hi = log_scale
    return dict(positions=(np.asarray(centre) + rng.uniform(-1, 1, (n, 3)) * np.asarray(box)).astype(np.float32),
                scale=rng.uniform(lo, hi, (n, 3)).astype(np.float32), rotation=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                opacity=rng.uniform(*opacity, n).astype(np.float32), f_dc=id_colour(n), f_rest=np.zeros((n, 9), np.float32))   # SH degree 1, all zero


def camera(eye, at, fov, W, H, flip=False):
    P = persp(np.tan(np.radians(fov) / 2), W / H, 0.1, 2000.0)
    if flip:
        P[1, 1] = -P[1, 1]
    return lookat(eye, at), P, np.asarray(eye, np.float32)


def _cloud():
    return make_set(np.random.default_rng(SEED["cloud"]), 400, (1.2, 0.8, 1.2), (-4.2, -1.8))


def _shapes():
    rng = np.random.default_rng(SEED["shapes"])
    s = make_set(rng, 260, (1.0, 0.7, 0.6), (-4.0, -2.2))
    n = s["scale"].shape[0]
    s["scale"][0:30] = np.log(np.stack([rng.uniform(0.2, 0.5, 30), rng.uniform(2e-4, 5e-4, 30), rng.uniform(2e-4, 5e-4, 30)], 1))     # needles
    s["scale"][60:90] = np.log(np.stack([rng.uniform(0.1, 0.3, 30), rng.uniform(0.1, 0.3, 30), rng.uniform(1e-4, 3e-4, 30)], 1))    # discs
    s["scale"][120:170] = np.log(rng.uniform(2e-4, 9e-4, (50, 3)))                                                                  # sub-pixel
    # ... half of them so faint that the conic extent sqrt(2 ln(100 a) (0.3 + cov)) stays below a quarter of a pixel: most cover no
    # pixel centre.  (The eigen extent rejects every sub-pixel particle: its smaller eigenvalue falls under the 0.1 floor.)
    a = rng.uniform(0.0101, 0.0108, 25)
    s["opacity"][120:145] = np.log(a / (1.0 - a))
    s["scale"][170] = np.log([40.0, 8.0, 0.5])          # the 2048 clamp: sigma points 1880 px to either side of the centre
    s["positions"][170] = (0.0, 0.0, -1.0)
    s["rotation"][170] = (1.0, 0.0, 0.0, 0.0)
    # flat discs facing the camera (eye on +z, tan(fov / 2) = 1/2, H = 136: one unit at distance 4 is 34 px) whose conic box ends on
    # tile (16), region (32 x 16) and bin (128 x 64) edges: centre on the edge minus a half extent chosen below
    k = 0
    for ex in (32.0, 64.0, 128.0):
        for ey in (16.0, 64.0, 48.0):
            i = 171 + k
            s["positions"][i] = ((ex - 100.0 - 6.0) / 34.0, (ey - 68.0 - 6.0) / 34.0, 0.0)
            s["scale"][i] = np.log([0.05 + 0.004 * k, 0.05 + 0.003 * k, 1e-3])
            s["rotation"][i] = (1.0, 0.0, 0.0, 0.0)
            s["opacity"][i] = 3.0
            k += 1
    assert 171 + k <= n
    # move each so that its conic box ends on the edge (the projection of these discs is linear in the position: 34 px per unit)
    sub = {key: (v[171:180] if v is not None else None) for key, v in s.items()}
    V, P, _ = SHAPES_CAMERA
    pr = np_gut.project(sub, None, V, P, 200, 136, np_gut.settings())
    s["positions"][171:180, 0] += ((np.repeat(SHAPES_EDGES[0], 3) - (pr["cx"] + pr["box"][:, 0])) / 34.0).astype(np.float32)
    s["positions"][171:180, 1] += ((np.tile(SHAPES_EDGES[1], 3) - (pr["cy"] + pr["box"][:, 1])) / 34.0).astype(np.float32)
    return s


SHAPES_EDGES = (np.array([32.0, 64.0, 128.0]), np.array([16.0, 64.0, 48.0]))
SHAPES_CAMERA = (lookat((0, 0, 4.0), (0, 0, 0)), persp(0.5, 200 / 136, 0.1, 100.0), np.asarray((0, 0, 4.0), np.float32))


def _inside(V, eye, half_width):
    """400 particles around the camera, and sixteen small ones placed for two rejections that a random cloud does not reach: eight
    between the dist stage's near bound (ndc z -0.2) and the near plane, which the quad's clip takes; eight whose centres lie in
    the dist stage's 20 % side band, so that their quads miss the screen"""
    s = make_set(np.random.default_rng(SEED["inside"]), 400, (1.0, 1.0, 1.0), (-3.0, -0.6))
    right, up, fwd = (np.asarray(V, np.float64)[0, :3], np.asarray(V, np.float64)[1, :3], -np.asarray(V, np.float64)[2, :3])
    pos = [eye + 0.09 * fwd + 0.004 * (j - 3.5) * right for j in range(8)] + \
          [eye + 1.0 * fwd + 1.1 * half_width * right + 0.05 * (j - 3.5) * up for j in range(8)]
    n = 416
    extra = dict(positions=np.asarray(pos, np.float32), scale=np.concatenate([np.full((8, 3), -7.0), np.full((8, 3), -5.0)]).astype(np.float32),
                 rotation=np.tile(np.float32([1, 0, 0, 0]), (16, 1)), opacity=np.full(16, 2.0, np.float32))
    out = {k: np.concatenate([s[k], extra[k]]) for k in extra}
    out["f_dc"], out["f_rest"] = id_colour(n), np.zeros((n, 9), np.float32)
    return out


def _opacity():
    rng = np.random.default_rng(SEED["opacity"])
    s = make_set(rng, 300, (1.0, 0.7, 0.8), (-3.6, -2.0))
    a = np.concatenate([rng.uniform(0.5 / 255, 1.6 / 255, 100), rng.uniform(0.006, 0.016, 120), rng.uniform(0.02, 0.9, 80)])
    s["opacity"] = np.log(a / (1.0 - a)).astype(np.float32)
    return s


MIRROR = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(np.float32)
MIRROR[:3, 3] = (0.9, -0.2, 0.3)
TRS = _trs([0.6, 1.5, 0.9], [0.3, 1.0, 0.2], 0.8, [-0.7, 0.2, -0.4])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(sets = [(arrays, matrix or None)], cam = (V, P, eye), W, H, st = np_gut.settings, params = the frame's fields)"""
    W, H = 200, 136
    st, params, cam = {}, {}, None
    base = name.split("+")[0]
    if base in ("cloud", "strip"):
        sets = [(_cloud(), None)]
        cam = camera((2.6, 1.0, 1.4), (0, 0, 0), 60.0, W, H)
        if base == "strip":
            st["strip"] = (2, 5)
            params.update(strip_row_begin=2, strip_row_end=5)
    elif base == "trs":
        s = make_set(np.random.default_rng(SEED["trs"]), 250, (0.9, 0.6, 0.9), (-4.0, -2.0))
        sets = [(s, TRS), (s, MIRROR)]
        W, H = 97, 61
        cam = camera((2.4, 0.8, 1.8), (0, 0, 0), 60.0, W, H)
    elif base == "inside":
        cam = camera((0.1, 0.05, 0.2), (0.3, 0.0, -1.0), 70.0, W, H)
        sets = [(_inside(cam[0], np.asarray(cam[2], np.float64), np.tan(np.radians(35.0)) * W / H), None)]
    elif base in ("fisheye150", "fisheye175"):
        sets = [(make_set(np.random.default_rng(SEED["fisheye"]), 400, (2.0, 2.0, 2.0), (-3.4, -1.6)), None)]
        W, H = 136, 136
        cam = camera((0.05, 0.1, 0.3), (0.2, 0.0, -1.0), 150.0 if base == "fisheye150" else 175.0, W, H)
        st["camera_model"] = 1
        params["camera_model"] = 1
    elif base == "shapes":
        sets = [(_shapes(), None)]
        cam = SHAPES_CAMERA
    elif base == "opacity":
        sets = [(_opacity(), None)]
        cam = camera((2.0, 0.7, 1.5), (0, 0, 0), 60.0, W, H)
    else:
        raise KeyError(name)
    for opt in name.split("+")[1:]:
        if opt == "eigen":
            st["extent_method"] = 0
            params["extent_method"] = 0
        elif opt == "msaa":
            st["ms_antialiasing"] = 1
            params["ms_antialiasing"] = 1
        elif opt == "flip":
            V, P, eye = cam
            P = P.copy()
            P[1, 1] = -P[1, 1]
            cam = (V, P, eye)
        elif opt in ("s05", "s2"):
            st["splat_scale"] = 0.5 if opt == "s05" else 2.0
            params["splat_scale"] = st["splat_scale"]
        else:
            raise KeyError(opt)
    return dict(name=name, sets=sets, cam=cam, W=W, H=H, st=np_gut.settings(**st), params=params)


CASES = ["cloud", "cloud+eigen", "cloud+msaa+flip", "cloud+eigen+s05", "trs", "trs+eigen+msaa+s2", "inside", "inside+eigen", "inside+flip",
         "fisheye150", "fisheye150+flip", "fisheye175", "shapes", "shapes+eigen", "opacity", "opacity+msaa", "strip"]


@functools.lru_cache(maxsize=None)
def projected(name, bin_px=(16, 16)):
    """[np_gut.project(...)] per instance of the case"""
    c = case(name)
    st = dict(c["st"], bin_px=bin_px)
    V, P, _ = c["cam"]
    return [np_gut.project(a, m, V, P, c["W"], c["H"], st, DELTA) for a, m in c["sets"]]


def stack(prs, key):
    return np.concatenate([pr[key] for pr in prs])


@functools.lru_cache(maxsize=None)
def reference_fragments(name, degree=2, occluder=None):
    c = case(name)
    V, P, _ = c["cam"]
    st = dict(c["st"], kernel_degree=degree)
    return np_gut.fragments(projected(name), V, P, c["W"], c["H"], st, False, DELTA, None if occluder is None else occluder_depth(name, occluder))


# The gaussian-on blend (np_gut.GutFragments.blend): the oracle frame's largest distance from the float64 interval per case, MEASURED by
# test_gut_cpu.py::test_oracle_blend_lies_in_the_interval; the kernels' tolerance is BAR_FACTOR times it.  A pixel whose interval is wider
# than GAUSS_FRAGILE is left out; at most GAUSS_FRAGILE_CAP of a case's pixels may be.
GAUSS_CASES = ["cloud+eigen+s05", "trs", "inside", "fisheye175", "shapes+eigen", "opacity+msaa"]
GAUSS_FRAGILE, GAUSS_FRAGILE_CAP = 1e-2, 0.005
GAUSS_DEV = {"cloud+eigen+s05": 5.3e-05, "trs": 1.8e-05, "inside": 1.1e-04, "fisheye175": 4.4e-05, "shapes+eigen": 9.9e-04, "opacity+msaa": 4.6e-06}


@functools.lru_cache(maxsize=None)
def reference_blend(name):
    """(lo, hi) [H, W, 4] of the case with the opacity gaussian on, and the mask of the fragile pixels: interval wider than GAUSS_FRAGILE, or two fragments whose fp32 depths tie"""
    c = case(name)
    V, P, _ = c["cam"]
    fr = np_gut.fragments(projected(name), V, P, c["W"], c["H"], c["st"], True, DELTA, None)
    lo, hi = fr.blend(np.concatenate([colour_table(a["positions"].shape[0]) for a, _ in c["sets"]]))
    return lo, hi, ((hi - lo).max(-1) > GAUSS_FRAGILE) | fr.order_open


def interval_distance(img, lo, hi, fragile):
    """largest distance of a channel of a non-fragile pixel from its interval"""
    d = np.maximum(np.maximum(lo - img, img - hi), 0.0).max(-1)
    return float(np.where(fragile, 0.0, d).max())


def occluder_depth(name, kind):
    """a depth image that cuts through the cloud: "plane" is tilted across the particles' key depths, "step" jumps in the middle"""
    c = case(name)
    z = stack(projected(name), "ndc_z")[stack(projected(name), "emits")]
    lo, hi = np.quantile(z, 0.2), np.quantile(z, 0.8)
    yy, xx = np.mgrid[0:c["H"], 0:c["W"]]
    if kind == "plane":
        return (lo + (hi - lo) * (0.7 * xx / c["W"] + 0.3 * yy / c["H"])).astype(np.float32)
    return np.where(xx < c["W"] // 2 + 3, np.float32(np.quantile(z, 0.35)), np.float32(np.quantile(z, 0.75))).astype(np.float32)
