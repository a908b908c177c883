"""The scenes and ray batches of the mesh ray query tests, shared by tests/test_mesh_rays_cpu.py (which establishes the fragile cap and
the float32-vs-float64 errors on the numpy restatement alone) and tests/test_gpu_mesh_rays.py (which holds the kernels to them)."""
import numpy as np

import mesh_cases as mc
import np_mesh as nm
import np_mesh_rays as nr
import np_trace as nt
import trace_cases as tc

FRAGILE_CAP = 0.05          # at most this share of a case's rays may be fragile: a condition on the cases
RASTER_EXCLUDED_CAP = 0.15  # at most this share of the pick image's pixels may be left out of the comparison with the rasteriser

# Largest float32-vs-float64 differences of np_mesh_rays.trace_f32 against np_mesh_rays.trace over all cases below, on the non-fragile
# rays both hit: the MEASURED values themselves (test_mesh_rays_cpu.py::test_f32_restatement_agrees_and_sets_the_bars measures them
# afresh and fails if one moves by more than 2 %).  t and position relative to max(1, |value|), barycentrics and normal absolute.
T_F32_VS_F64 = 4.522e-7      # big_4000
BARY_F32_VS_F64 = 1.115e-5   # big_4000: a sliver of the soup
POS_F32_VS_F64 = 1.551e-6    # big_4000
NRM_F32_VS_F64 = 2.911e-6    # big_4000
# the kernel may differ from numpy in a few roundings (contraction in the interpolation, rsqrt): exactly 4 x the measured error
GPU_T_BAR, GPU_BARY_BAR, GPU_POS_BAR, GPU_NRM_BAR = 4 * T_F32_VS_F64, 4 * BARY_F32_VS_F64, 4 * POS_F32_VS_F64, 4 * NRM_F32_VS_F64

NONUNIFORM = tc.trs((1.4, 0.7, 1.1), (0.3, 1.0, 0.2), 35.0, (0.2, -0.1, 0.3))         # non-uniform scale and a rotation
MIRRORED = tc.trs((-1.0, 1.0, 1.0), (0.0, 1.0, 0.0), 20.0, (-0.3, 0.2, -0.2))         # negative determinant
SHIFTED = tc.trs((1.0, 1.0, 1.0), (0.0, 0.0, 1.0), 0.0, (0.5, 0.25, -0.5))   # dyadic: the collinear triangle stays exactly collinear


MATERIALS = 2   # every mesh of the cases is created with this many materials (the child makes them), ids drawn below it


def _mesh(pos, idx, seed, materials=MATERIALS, **kw):
    pos, idx = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(idx, np.uint32).reshape(-1, 3)
    r = np.random.default_rng(seed)
    nrm = nm.generate_normals(pos, idx)
    return dict(positions=pos, indices=idx, normals=np.asarray(nrm, np.float32).reshape(-1, 3),
                material_ids=r.integers(0, materials, idx.shape[0]).astype(np.uint32), transform=kw.get("transform"), visible=kw.get("visible", True))


def soup(n, seed, half=1.0, size=0.6, **kw):
    r = np.random.default_rng(seed)
    c = (r.random((n, 1, 3)) - 0.5) * 2 * half
    tri = c + (r.random((n, 3, 3)) - 0.5) * size
    return _mesh(tri.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3), seed, **kw)


def grid(nx, ny, seed, ext=1.5, bump=0.25, **kw):
    """a tessellated (nx x ny quads, 2 nx ny triangles) height field with shared vertices"""
    r = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-ext, ext, nx + 1), np.linspace(-ext, ext, ny + 1))
    z = (r.random(x.shape) - 0.5) * bump
    pos = np.stack([x, y, z], -1).reshape(-1, 3)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    idx = np.concatenate([np.stack([a, a + 1, a + nx + 2], 1), np.stack([a, a + nx + 2, a + nx + 1], 1)], 0)
    return _mesh(pos, idx, seed, **kw)


def box(half, seed, **kw):
    """a closed box (12 triangles) around the origin"""
    s = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * half
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return _mesh(s, idx, seed, **kw)


def degenerate(seed, **kw):
    """zero-area triangles (no leaf) and duplicated triangles (bit-identical t: the lower primitive id wins)"""
    base = soup(10, seed, half=0.8, size=0.9)
    p = base["positions"].reshape(-1, 3, 3)
    p[1, 2] = p[1, 1]                     # two equal vertices
    p[4] = np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]]) * np.float32(0.25)   # collinear with an exactly zero cross product
    p[6] = p[2]                           # duplicates of 2 and 3, same vertex order
    p[8] = p[3]
    p[9] = p[2]
    return _mesh(p.reshape(-1, 3), np.arange(30).reshape(-1, 3), seed, **kw)


def scenes():
    return {
        "tiny": [soup(1, 11, transform=NONUNIFORM), soup(7, 12, transform=MIRRORED), grid(2, 2, 13), soup(9, 14, visible=False)],
        "mid": [soup(64, 21, transform=NONUNIFORM), soup(65, 22, transform=MIRRORED), box(3.0, 23), grid(2, 2, 24, visible=False, transform=SHIFTED)],
        "big": [grid(16, 16, 31, transform=NONUNIFORM), soup(513, 32, half=1.3, size=0.35, transform=MIRRORED), degenerate(33, transform=SHIFTED),
                grid(8, 4, 34, visible=False)],
    }


EYE = (2.4, 1.3, 2.6)


def cameras():
    """name -> (V, P, W, H, fisheye, fov_rad): the frames whose primary rays mgs_trace_generate_rays writes"""
    V = tc.lookat(EYE, (0, 0, 0))
    return {"pinhole": (V, tc.persp(50.0, 48 / 36), 48, 36, False, 0.0), "fisheye": (V, tc.persp(50.0, 40 / 30), 40, 30, True, 2.2)}


def camera_rays(name):
    """the numpy stand-in for mgs_trace_generate_rays (np_trace.rays in float64, rounded): a RAY-shaped tuple (O, D, tmin, tmax)"""
    V, P, W, H, fish, fov = cameras()[name]
    o, d, ok = nt.rays(V, P, W, H, fisheye=fish, fov_rad=fov)
    ok = ok.reshape(-1)
    return (o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32), np.where(ok, 0.001, 1.0).astype(np.float32),
            np.where(ok, 10000.0, 0.0).astype(np.float32))


def extra_rays(n, seed, inside=False):
    """random rays towards the scene, a share with non-unit directions, windows that end in front of, between and behind the
    surfaces; `inside`: origins inside the closed box"""
    r = np.random.default_rng(seed)
    O = (r.random((n, 3)) - 0.5) * (3.0 if inside else 9.0)
    target = (r.random((n, 3)) - 0.5) * 2.4
    D = target - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    scale = np.where(r.random(n) < 0.3, r.random(n) * 3.9 + 0.1, 1.0)   # non-unit directions: t scales by 1 / scale
    D *= scale[:, None]
    tmin, tmax = np.zeros(n), np.full(n, 1000.0)
    dist = np.linalg.norm(target - O, axis=1) / scale
    kind = r.integers(0, 5, n)
    tmax = np.where(kind == 1, dist * 0.4, tmax)      # ends in front of most surfaces
    tmax = np.where(kind == 2, dist * 1.05, tmax)     # ends between
    tmin = np.where(kind == 3, dist * 0.9, tmin)      # starts between
    tmin = np.where(kind == 4, -5.0, tmin)            # negative: taken as 0
    return O.astype(np.float32), D.astype(np.float32), tmin.astype(np.float32), tmax.astype(np.float32)


def invalid_rays():
    O = np.zeros((6, 3), np.float32)
    D = np.tile(np.float32([0, 0, 1]), (6, 1))
    tmin, tmax = np.zeros(6, np.float32), np.full(6, 10.0, np.float32)
    O[0, 1] = np.nan
    D[1, 0] = np.inf
    D[2] = 0
    tmin[3], tmax[3] = 2.0, 1.0
    tmax[4] = np.inf
    tmin[5] = np.nan
    return O, D, tmin, tmax


def _cat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


# name -> (scene, the batch's parts); a part is a camera's name (replaced on the device by the generated rays) or (O, D, tmin, tmax)
def batches():
    return {
        "tiny_1": ("tiny", [extra_rays(1, 101)]),
        "tiny_255": ("tiny", [extra_rays(249, 102), invalid_rays()]),
        "mid_256": ("mid", [extra_rays(128, 103), extra_rays(128, 104, inside=True)]),
        "mid_257": ("mid", [extra_rays(200, 105, inside=True), extra_rays(57, 106)]),
        "big_4000": ("big", ["pinhole", "fisheye", extra_rays(1066, 107), invalid_rays()]),   # 1728 + 1200 + 1066 + 6
    }


def rays_of(name, generated=None):
    """the batch as (O, D, tmin, tmax); generated: camera name -> (O, D, tmin, tmax) from mgs_trace_generate_rays"""
    _, parts = batches()[name]
    return _cat([((generated or {}).get(p) or camera_rays(p)) if isinstance(p, str) else p for p in parts])


_REF = {}


def reference(name, rays=None):
    """np_mesh_rays.trace of the batch (computed once per batch and ray set)"""
    rays = rays_of(name) if rays is None else rays
    key = (name, hash(b"".join(np.ascontiguousarray(a).tobytes() for a in rays)))
    if key not in _REF:
        _REF[key] = nr.trace(scenes()[batches()[name][0]], *rays)
    return _REF[key]


# ---- the watertight case: an integer grid in the plane z = 0, quads split along the (0,0)-(1,1) diagonal ----
WT_N = 4
WT_SHIFT = np.float32([3, -2, 5])


def watertight_mesh(shift=None):
    n = WT_N
    x, y = np.meshgrid(np.arange(n + 1, dtype=np.float32), np.arange(n + 1, dtype=np.float32))
    pos = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    idx = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)], 0)
    M = np.eye(4, dtype=np.float32)
    if shift is not None:
        M[:3, 3] = shift
    return _mesh(pos, idx, 41, transform=M)


def watertight_rays(shift=None):
    """axis-parallel rays at every vertex, every edge midpoint (axis edges and diagonals) and quarter points of every edge, from
    above (direction -z, length 1 and 2) and from below (+z: the back face).  Returns (O, D, tmin, tmax, expected t, expected id)."""
    n = WT_N
    s = np.zeros(3, np.float32) if shift is None else np.asarray(shift, np.float32)
    pts = set()
    for i in range(n + 1):
        for j in range(n + 1):
            pts.add((i, j))
            for f in (0.25, 0.5, 0.75):
                if i < n:
                    pts.add((i + f, j))
                if j < n:
                    pts.add((i, j + f))
                if i < n and j < n:
                    pts.add((i + f, j + f))
    pts = np.array(sorted(pts), np.float64)
    m = watertight_mesh()
    tri = m["positions"][m["indices"]].astype(np.float64)[:, :, :2]              # [T,3,2], exact
    e = lambda a, b, p: (b[:, None, 0] - a[:, None, 0]) * (p[None, :, 1] - a[:, None, 1]) - (b[:, None, 1] - a[:, None, 1]) * (p[None, :, 0] - a[:, None, 0])
    w0, w1, w2 = e(tri[:, 0], tri[:, 1], pts), e(tri[:, 1], tri[:, 2], pts), e(tri[:, 2], tri[:, 0], pts)
    closed = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))  # [T,P]
    assert closed.any(0).all()
    expect = np.argmax(closed, axis=0).astype(np.uint32)                         # the lowest primitive id whose closed set holds the point
    O, D, T, E = [], [], [], []
    for dz, h, t in ((-1.0, 7.0, 7.0), (-2.0, 7.0, 3.5), (1.0, -3.0, 3.0)):
        o = np.concatenate([pts, np.full((pts.shape[0], 1), h)], 1) + s[None]
        O.append(o)
        D.append(np.tile([0.0, 0.0, dz], (pts.shape[0], 1)))
        T.append(np.full(pts.shape[0], t))
        E.append(expect)
    O, D = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
    return O, D, np.zeros(O.shape[0], np.float32), np.full(O.shape[0], 100.0, np.float32), np.concatenate(T).astype(np.float32), np.concatenate(E)


# ---- against the mesh rasteriser: the committed fixture, instanced as the mesh pass's tests do, 160 x 120 pinhole ----
RW, RH = 160, 120


def raster_camera():
    return mc.lookat((2.2, 1.6, 3.0), (0, 0.1, 0)), mc.persp(55.0, RW / RH, 0.1, 50.0), np.float32((2.2, 1.6, 3.0))


def pixel_rays(V, P, W, H, ox=0.5, oy=0.5):
    """pinhole rays through (x + ox, y + oy) of every pixel, float64 rounded to float32 (generatePinholeRay)"""
    vi, pi = np.linalg.inv(np.asarray(V, np.float64)), np.linalg.inv(np.asarray(P, np.float64))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = (xs + ox) / W * 2.0 - 1.0, (ys + oy) / H * 2.0 - 1.0
    cam = (np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pi.T)[..., :3]
    d = cam @ vi[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(vi[:3, 3], d.shape)
    n = W * H
    return o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32), np.full(n, 0.001, np.float32), np.full(n, 10000.0, np.float32)


def raster_mask(meshes):
    """(comparable [H,W] bool, reference primitive id [H,W]): a pixel is compared when its centre ray is not fragile and the rays
    through its four corners see what the centre sees, so that no projected edge of what is visible there comes within half a pixel
    of the centre"""
    V, P, _ = raster_camera()
    centre = nr.trace(meshes, *pixel_rays(V, P, RW, RH))
    same = ~centre["fragile"]
    for ox in (0.0, 1.0):
        for oy in (0.0, 1.0):
            c = nr.trace(meshes, *pixel_rays(V, P, RW, RH, ox, oy))
            same &= (c["prim"] == centre["prim"]) & ~c["fragile"]
    return same.reshape(RH, RW), centre["prim"].reshape(RH, RW)
