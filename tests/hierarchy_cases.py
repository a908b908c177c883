"""The scenes of the hierarchy tests (test_hierarchy_cpu.py, test_gpu_hierarchy.py), numpy only and small on purpose: each builds in
well under a second.  Splat scenes are lists of (arrays as SplatSet.from_arrays takes them, M); mesh scenes are lists of
mesh_cases.mesh dicts.  Every scene is centred on the origin and at least as wide as its coordinates are large, so that a centre's fp32
rounding stays far below a Morton cell (np_hierarchy.NEAR); where a group's own splats do not span such a box, anchors do."""
import functools

import numpy as np

import mesh_cases as mc
import np_hierarchy as nh
import trace_cases as tc

KMR = np.float32(0.0113)           # MgsFrameParams::kernel_min_response, the default
CULL = np.float32(1.0 / 255.0)     # alpha_cull_threshold, the default
PROXIES = [(deg, 1) for deg in nh.DEGREES] + [(deg, 0) for deg in nh.DEGREES]   # (kernel_degree, kernel_adaptive_clamping)
COUNTS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4096, 4097)               # around every 8-ary boundary, up to five levels
T0 = np.array([1000.0, -700.0, 300.0])
EXCUSED_CAP = 0.02


def morton_frame(parts):
    """(box_lo, box_inv_ext) fp32 as the library documents its Morton frame (include/mgs.h): the union of the instances' transformed
    LOCAL boxes (the eight corners of each set's or mesh's box of finite points, in double), not the box of the world points.
    parts: [(points [n, 3] in model space, M)].  The CPU test predicts the excused pairs in this frame."""
    wl, wh = np.full(3, np.inf), np.full(3, -np.inf)
    for pts, M in parts:
        pts = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
        pts = pts[np.isfinite(pts).all(1)]
        if not pts.shape[0]:
            continue
        M = np.eye(4) if M is None else np.asarray(M, np.float32).astype(np.float64)
        b = np.stack([pts.min(0), pts.max(0)])
        corners = np.array([[b[(k >> a) & 1, a] for a in range(3)] for k in range(8)])
        w = corners @ M[:3, :3].T + M[:3, 3]
        wl, wh = np.minimum(wl, w.min(0)), np.maximum(wh, w.max(0))
    ext = wh - wl
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(wl <= wh, wl, 0.0).astype(np.float32), np.where(ext > 0, 1.0 / ext, 0.0).astype(np.float32)


def sigmoid32(x):
    return (np.float32(1) / (np.float32(1) + np.exp(-np.asarray(x, np.float32)))).astype(np.float32)


def logit(p):
    return np.log(p / (1.0 - p))


def cloud(n, seed, half=1.0, log_scale=-3.0, spread=0.35):
    """n splats that all have a leaf (density >= 0.27), no SH, inside the cells of the Morton frame [-half, half]^3 that framed()
    gives them"""
    r = np.random.Generator(np.random.PCG64(seed))
    rot = r.standard_normal((n, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    # a tenth of a cell away from every boundary: under the identity no leaf can floor differently in fp32 (np_hierarchy.NEAR)
    pos = -half + (r.integers(0, 1023, (n, 3)) + r.uniform(0.1, 0.9, (n, 3))) * (2.0 * half / 1023.0)
    return dict(positions=pos.astype(np.float32), f_dc=r.standard_normal((n, 3)).astype(np.float32),
                f_rest=np.zeros((n, 0), np.float32), opacity=r.uniform(-1.0, 3.0, n).astype(np.float32),
                scale=(log_scale + r.standard_normal((n, 3)) * spread).astype(np.float32), rotation=rot)


def framed(a, half=1.0):
    """a with two more splats behind it, on the corners of [-half, half]^3 and far below the cull threshold: the Morton frame is the
    union of the sets' boxes, culled splats included, so they span the frame without putting a leaf on its corner, where the
    quantised coordinate is exactly the cell boundary 1023"""
    c = cloud(2, 98)
    c["positions"] = np.array([[-half] * 3, [half] * 3], np.float32)
    c["opacity"][:] = -9.0
    return cat(a, c)


def cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def cancelling_transform():
    """x -> R (x - T0), R a rotation by 30 degrees about an oblique axis: every term of M p is about 1e3, their sum is about 1"""
    M = tc.trs((1.0, 1.0, 1.0), (1.0, 2.0, 0.5), 30.0, (0.0, 0.0, 0.0)).astype(np.float64)
    M[:3, 3] = -M[:3, :3] @ T0
    return M.astype(np.float32)


def anchors(span=250.0):
    """two splats on opposite corners of a cube: they give the Morton frame its width"""
    a = cloud(2, 99, log_scale=-1.0, spread=0.0)
    a["positions"] = np.array([[-span] * 3, [span] * 3], np.float32)
    return a


def count_scene(n):
    if n == 0:   # three splats, all below the cull threshold: a build with no leaf
        a = cloud(3, 100)
        a["opacity"][:] = -9.0
        return [(a, tc.I4)]
    return [(framed(cloud(n, 100 + n, log_scale=-3.0 if n < 100 else -4.5)), tc.I4)]


def _a_isotropic():
    a = cloud(300, 1)
    a["scale"][:] = a["scale"][:, :1]
    a["rotation"][:] = (1, 0, 0, 0)
    return [(framed(a), tc.I4)]


def _b_anisotropic():
    r = np.random.Generator(np.random.PCG64(2))
    a = cloud(300, 2, log_scale=-2.0)
    axis = r.integers(0, 3, 300)
    a["scale"][np.arange(300), axis] -= np.float32(np.log(1e4))                       # 1e4 between axes: discs, and
    a["scale"][np.arange(0, 300, 2), (axis[::2] + 1) % 3] -= np.float32(np.log(1e4))  # needles
    a["rotation"] = (a["rotation"] * (10.0 ** r.uniform(-3, 3, (300, 1)))).astype(np.float32)   # unnormalised, |q| in 1e-3 .. 1e3
    return [(framed(a), tc.I4)]


def _c_affine():
    a = cloud(1000, 3, half=0.6)   # (no snapping survives these transforms: enough leaves for the cap to hold at three sigma)
    return [(a, tc.trs((0.3, 2.5, 1.0), (1, 1, 0), 50.0, (-0.5, 0.4, 0.1))), (a, tc.SHEAR), (a, tc.MIRROR)]


D_N = 2000


def _d_cancelling():
    r = np.random.Generator(np.random.PCG64(4))
    a = cloud(D_N, 4)
    a["positions"] = (T0 + r.uniform(-1.0, 1.0, (D_N, 3))).astype(np.float32)
    a["scale"] = np.log(10.0 ** r.uniform(-5.0, -2.0, (D_N, 1)) / 3.0 * r.uniform(0.5, 1.0, (D_N, 3))).astype(np.float32)   # extents 1e-5 .. 1e-2
    return [(a, cancelling_transform()), (anchors(), tc.I4)]


E_CULL_FROM = 40   # group e: alpha_cull is the density the device holds for this splat (caller's index), so that one splat is AT it


def _e_thresholds():
    a = cloud(260, 5)
    steps = np.linspace(-4e-6, 4e-6, 80)
    a["opacity"][:80] = logit(float(CULL) * 1.5 * (1.0 + steps)).astype(np.float32)            # at, just below and just above alpha_cull
    a["opacity"][80:240] = logit(float(KMR) / nh.CLAMP * (1.0 + np.linspace(-8e-6, 8e-6, 160))).astype(np.float32)   # kmr / density crosses 0.97
    return [(framed(a), tc.I4)]


F_BAD, F_HUGE = 8, 8   # splats 0 .. 7 have no leaf; splat 8 has one


def _f_nonfinite():
    a = cloud(200, 6)
    a["opacity"][:F_BAD + 1] = 2.0
    a["scale"][F_HUGE] = (50.0, 49.0, 48.0)    # half extents of 1e21 .. 1e22: finite in fp32, though their squares are not: a leaf
    a["scale"][0] = 88.0                       # exp(88) r overflows fp32
    a["scale"][1, 1] = 89.0                    # expf overflows
    a["scale"][2] = (120.0, -3.0, -3.0)
    a["positions"][3, 1] = np.nan
    a["positions"][4, 0] = np.inf
    a["scale"][5, 2] = np.nan
    a["rotation"][6] = 0.0                     # no direction to normalise
    a["rotation"][7, 2] = np.nan
    return [(framed(a), tc.I4)]


def _g_planar():
    a = framed(cloud(260, 7))
    a["positions"][:, 2] = 0.25
    return [(a, tc.I4)]


def _g_collinear():
    a = framed(cloud(120, 8))
    a["positions"][:, 1], a["positions"][:, 2] = 0.125, -0.25
    return [(a, tc.I4)]


def _g_single():
    return [(cloud(1, 9), tc.I4)]


def _h_two_instances():
    a = framed(cloud(300, 10))
    # a fiftieth of a cell apart: both instances' splats stay inside their cells, share their codes, and their ids interleave
    return [(a, tc.I4), (a, tc.trs((1.0, 1.0, 1.0), (0, 1, 0), 0.0, (4e-5, -4e-5, 4e-5)))]


def _i_duplicates():
    a = cloud(150, 11)
    return [(framed(cat(a, {k: v[:50] for k, v in a.items()})), tc.I4)]


@functools.lru_cache(maxsize=None)
def splat_groups():
    return {"a_isotropic": _a_isotropic(), "b_anisotropic": _b_anisotropic(), "c_affine": _c_affine(), "d_cancelling": _d_cancelling(),
            "e_thresholds": _e_thresholds(), "f_nonfinite": _f_nonfinite(), "g_planar": _g_planar(), "g_collinear": _g_collinear(),
            "g_single": _g_single(), "h_two_instances": _h_two_instances(), "i_duplicates": _i_duplicates()}


def storage_planes(arrays, order, density=None):
    """the planes np_hierarchy takes, in storage order: `order` = storage index -> caller's index; density as the device holds it
    (caller's order), or the fp32 sigmoid of the opacity where no device is at hand"""
    d = sigmoid32(arrays["opacity"]) if density is None else np.asarray(density, np.float32)
    return dict(centers=arrays["positions"][order], scales=arrays["scale"][order], quats=arrays["rotation"][order], density=d[order])


# ---- triangles


def soup(n, seed, half=1.0, size=0.05, frame=True):
    r = np.random.Generator(np.random.PCG64(seed))
    # centroids inside the cells of the Morton frame [-B, B]^3, a fifth of a cell away from every boundary
    B = half + 2 * size
    c = (-B + (r.integers(50, 973, (n, 1, 3)) + r.uniform(0.2, 0.8, (n, 1, 3))) * (2.0 * B / 1023.0))
    off = r.uniform(-size, size, (n, 3, 3))
    tri = c + off - off.mean(1, keepdims=True)
    if frame:   # one more triangle, exactly degenerate (a repeated vertex: no leaf), from corner to corner of the frame
        tri = np.concatenate([tri, [[[-B, -B, -B], [B, B, B], [B, B, B]]]])
    tri = tri.astype(np.float32)
    return mc.mesh(tri.reshape(-1, 3), np.arange(3 * tri.shape[0]).reshape(-1, 3), material_ids=np.zeros(tri.shape[0], np.uint32))


def count_mesh(n):
    if n == 0:   # two triangles, both exactly degenerate: a build with no leaf
        return [mc.mesh([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0.5, 0.5, 0.5]], [[0, 1, 2], [3, 3, 1]])]
    if n == 512:   # a grid: 2 * 16 * 16 triangles that share vertices
        return [mc.grid_mesh(seed=3, n=17)]
    return [soup(n, 200 + n)]


def _axis_parallel():
    """triangles in planes x = k, y = k, z = k, the planes through 0 among them"""
    tris = []
    for ax in range(3):
        for k in (0.0, -0.5, 0.7):
            for j in range(4):
                t = np.array([[0.1 * j, 0.2, 0.0], [0.1 * j + 0.3, 0.25, 0.0], [0.1 * j, 0.6, 0.0]]) - 0.31
                t[:, 2] = k
                tris.append(np.roll(t, ax + 1, axis=1))
    p = np.array(tris, np.float32).reshape(-1, 3)
    return mc.mesh(p, np.arange(p.shape[0]).reshape(-1, 3))


def _slivers():
    r = np.random.Generator(np.random.PCG64(31))
    n = 40
    a = r.uniform(-1, 1, (n, 3))
    d = r.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = np.cross(d, r.standard_normal((n, 3)))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    p = np.stack([a, a + d, a + 0.5 * d + 1e-6 * e], 1).astype(np.float32)       # aspect 1e6
    return mc.mesh(p.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3))


def _degenerate():
    """exactly degenerate: a repeated vertex, three collinear points on a lattice (every product exact).  Nearly: the third point one
    ulp off the line"""
    f = np.float32
    up = np.nextafter(f(0.5), f(1))
    p = np.array([[0, 0, 0], [0.5, 0.25, 0.125], [0.5, 0.25, 0.125],          # 0: repeated vertex
                  [0, 0, 0], [0.25, 0.25, 0.5], [0.5, 0.5, 1.0],              # 1: collinear
                  [0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.25, 0.5, 0.75],    # 2: a point
                  [0, 0, 0], [0.25, 0.25, 0.5], [up, 0.5, 1.0],               # 3: one ulp off the line: a leaf
                  [0, 0, 0], [1.0, 0, 0], [0.5, np.float32(1e-30), 0]], np.float32)   # 4: height 1e-30: a leaf
    return mc.mesh(p, np.arange(15).reshape(-1, 3))


MESH_VALID = {"degenerate": [False, False, False, True, True]}


@functools.lru_cache(maxsize=None)
def mesh_content():
    """one scene: -> (meshes, names).  The cancelling instance's vertices lie near T0 in model space and near the origin in the world"""
    near_t0 = soup(60, 22, frame=False)
    near_t0 = dict(near_t0, positions=(near_t0["positions"].astype(np.float64) + T0).astype(np.float32), transform=cancelling_transform())
    m1 = dict(soup(50, 24, frame=False), material_ids=(np.arange(50) % 2).astype(np.uint32))
    m2 = dict(soup(50, 26, frame=False), material_ids=(2 + np.arange(50) % 2).astype(np.uint32), transform=tc.trs((1.3, 0.8, 1.0), (0, 0, 1), 20.0, (0.2, -0.1, 0.3)))
    meshes = [_axis_parallel(), _slivers(), _degenerate(), near_t0, dict(soup(30, 23, frame=False), visible=False), m1, m2]
    return meshes, ("axis_parallel", "slivers", "degenerate", "cancelling", "hidden", "materials_a", "materials_b")
