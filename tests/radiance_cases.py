"""The cases of the per-splat radiance tests (test_radiance_cpu.py, test_gpu_radiance.py): scenes in which one pixel shows one splat's
shaded colour, and that colour in float64.  numpy and the CPU oracle's storage preparation only; imports no device code.

The read-out.  Frames are rendered with MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED (every accepted fragment has alpha 1) into an RGBA32F
target, and no two footprints overlap: the pixel under a splat's centre then holds 1 * 1 * colour + 0, the output of the shading site
itself.  Every splat sits at the centre of a pixel of its own 16 x 16 cell, is isotropic in model space and ~1 px wide at its widest, so
its footprint stays inside the cell's inner 14 x 14 pixels: BORDER (every other pixel of the frame) must stay at alpha 0, the read
pixels at alpha 1.  The builder asserts the premises from the float64 projection: the centre >= 0.25 px from every edge of its pixel,
the read pixel where it was put, and |b1| + |b2| <= 6 px on both axes.

Scenes.  A scene is made for ONE camera pose (the positions are un-projected from that camera).  "four": the four sets of SH degree
3, 0, 1, 2 (15, 0, 3, 8 f_rest coefficients per channel; the degree-0 set has no SH plane) as four instances under different
transforms; "twenty": twenty instances (above the compositor's inline table of 16) of twenty small sets whose degrees cycle.
Instance 0 of "four" (degree 3) has an EXACTLY representable transform: the rotation by 120 degrees about (1, 1, 1) (a cyclic
permutation of the axes: a rotation about a non-axis vector), a non-uniform power-of-two scale and a dyadic translation; its
positions are snapped to 2^-12.  With the dyadic eyes of the six axis poses its model-space camera position and the view
direction of the splat at the image centre (255 x 191: that pixel's ray is the optical axis) are exact coordinate axes in fp32 and in
float64 alike, and so are the directions of the axis and octant rays of the ray-query batch.  The other instances rotate about other
non-axis vectors with non-uniform scales in [0.25, 4].

Tolerance.  unit(...) is u = 2^-23 (|base| + sum_k |c_k| BMAX[k]) per value, BMAX[k] the supremum of basis function k over the unit
sphere, the sum over the coefficients of the effective degree min(set, frame).  test_radiance_cpu.py measures the oracle's fp32
shading against the float64 reference in these units (K_REF) and holds it; the device bar is K * u with K = 4 K_REF rounded up to a
power of two (the margin is for fused multiply-adds, the hardware reciprocal square root and another summation order)."""
import functools

import numpy as np

import np_reference as npr
import trace_cases as tc

W, H = 255, 191
CELL, X0, Y0, NX, NY = 16, 7, 7, 15, 11          # cell (i, j) covers x in [X0 + 16 i, +16), y in [Y0 + 16 j, +16); cell (7, 5) holds pixel (127, 95)
N = NX * NY
FOV, NEAR, FAR = 60.0, 0.1, 100.0
FORMATS = {"f32": 0, "f16": 1, "u8": 2}          # MgsStorageFormat, SH and rgba alike
CPC = {0: 0, 1: 3, 2: 8, 3: 15}
SNAP = 2.0 ** -12
K_REF = 1.5                                      # test_radiance_cpu.py::test_oracle_fp32_against_float64 measures 1.400 and holds this figure
K = 8                                            # 4 * K_REF rounded up to a power of two (the cap is 64)

# sup over the unit sphere of |basis k| (the constants of np_reference.py)
_C1, _C2, _C3 = npr.SH_C1, npr.SH_C2, npr.SH_C3
BMAX = np.array([_C1, _C1, _C1,
                 abs(_C2[0]) / 2, abs(_C2[1]) / 2, 2 * _C2[2], abs(_C2[3]) / 2, _C2[4],            # |xy| <= 1/2; 2zz - xx - yy = 2 at z = 1
                 abs(_C3[0]),                                                                     # (3xx - yy) y = sin 3 phi in the xy plane
                 _C3[1] / 3 ** 1.5,                                                               # |xyz| <= 3^-3/2
                 abs(_C3[2]) * (8 / 3) * np.sqrt(4 / 15),                                         # (5zz - 1) sqrt(1 - zz) at zz = 11/15
                 2 * _C3[3],                                                                      # z (5zz - 3) = 2 at z = 1
                 abs(_C3[4]) * (8 / 3) * np.sqrt(4 / 15),
                 _C3[5] * 2 / 3 ** 1.5,                                                           # (1 - zz) z at zz = 1/3
                 abs(_C3[6])])

# name -> (eye, forward, up): dyadic eyes, exact axes; two diagonals
POSES = {
    "+x": ((-4.5, 0.5, -0.25), (1, 0, 0), (0, 1, 0)),
    "-x": ((4.5, -0.25, 0.5), (-1, 0, 0), (0, 1, 0)),
    "+y": ((0.5, -4.5, 0.25), (0, 1, 0), (0, 0, 1)),
    "-y": ((-0.25, 4.5, -0.5), (0, -1, 0), (0, 0, 1)),
    "+z": ((0.25, 0.5, -4.5), (0, 0, 1), (0, 1, 0)),
    "-z": ((-0.5, 0.25, 4.5), (0, 0, -1), (0, 1, 0)),
    "diag_a": ((3.0, 2.5, 3.5), (-3.0, -2.5, -3.5), (0, 1, 0)),
    "diag_b": ((-3.5, -2.0, 3.0), (4.0, 2.0, -3.5), (0, 1, 0)),
}
POSE_NAMES = list(POSES)
EXTRAS_POSE = "+x"        # the SH-only frames, the rasteriser's extras and the ray queries
TWENTY_POSE = "diag_a"


def camera(pose):
    """(V, P, eye) of a pose, math convention, float32; V is exact for the axis poses"""
    eye, f, up = (np.asarray(a, np.float64) for a in POSES[pose])
    V = tc.lookat(eye, eye + f, up)
    return V, tc.persp(FOV, W / H, NEAR, FAR), eye.astype(np.float32)


def _exact_transform():
    M = np.eye(4)
    M[:3, :3] = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64) @ np.diag([0.5, 2.0, 1.0])
    M[:3, 3] = (1.0, -0.5, 0.25)
    return M.astype(np.float32)


def four_layout():
    """[(set degree, transform)] of the four-instance scene"""
    return [(3, _exact_transform()),
            (0, tc.trs((0.25, 0.4, 0.3), (0, 1, 0), 25.0, (0.5, 0.75, -1.0))),
            (1, tc.trs((4.0, 2.5, 3.0), (0, 1, 1), -50.0, (-1.0, 0.25, 0.5))),
            (2, tc.trs((0.8, 1.3, 2.0), (1, 2, 0.5), 35.0, (-0.5, -0.75, 1.0)))]


def twenty_layout():
    out = []
    for k in range(20):
        s = 0.25 * 16.0 ** (((7 * k) % 20) / 19.0)                     # 0.25 .. 4
        scale = np.clip((s, s * (0.7 + 0.05 * (k % 5)), s * (1.3 - 0.04 * (k % 7))), 0.25, 4.0)
        out.append(((3, 0, 1, 2)[k % 4], tc.trs(scale, (1 + k % 3, 2 - k % 2, 0.5 + k % 4), 17.0 * k + 9.0,
                                                (0.3 * (k % 5) - 0.6, 0.25 * (k % 3) - 0.25, 0.2 * (k % 7) - 0.6))))
    return out


def _instance_of_cell(k, n_inst):
    return (k + 2) % n_inst      # the centre cell (k = 82) belongs to instance 0 in both layouts


def _colours(rng, n, degree, pose_index):
    """f_dc ~ N(0, 1); f_rest amplitude 0.3 in every band (no decay); every other splat has exactly ONE non-zero coefficient, its
    (coefficient, channel) rotating with the splat and the pose; every fourth has a base colour clamped to 0 (f_dc = -3), so that its
    radiance is the SH sum alone, negative about as often as not"""
    cpc = CPC[degree]
    f_dc = rng.standard_normal((n, 3)).astype(np.float32)
    f_dc[2::4] = -3.0
    if cpc == 0:
        return f_dc, None, np.full(n, -1)
    f_rest = (rng.standard_normal((n, 3, cpc)) * 0.3).astype(np.float32)        # planar [channel][coefficient], as a .ply holds it
    single = np.full(n, -1)
    for i in range(1, n, 2):
        combo = (i // 2 + 23 * pose_index) % (3 * cpc)
        k, ch = combo // 3, combo % 3
        v = f_rest[i, ch, k]
        f_rest[i] = 0.0
        f_rest[i, ch, k] = np.float32(np.copysign(0.35 + abs(v), v))
        single[i] = combo
    return f_dc, f_rest.reshape(n, 3 * cpc), single


@functools.lru_cache(maxsize=None)
def scene(kind, pose):
    """dict(sets=[(arrays, M)] per instance in creation order, degrees, cell[n] (the cell of every splat, global caller order),
    single[n] (combo index of a one-coefficient splat or -1), V, P, eye).  Do not modify the result."""
    layout = four_layout() if kind == "four" else twenty_layout()
    V, P, eye = camera(pose)
    Vi = np.linalg.inv(V.astype(np.float64))
    fx, fy = float(P[0, 0]), float(P[1, 1])
    pose_index = POSE_NAMES.index(pose)
    rng = np.random.Generator(np.random.PCG64(1000 + 17 * pose_index + (0 if kind == "four" else 500)))
    cells = [[k for k in range(N) if _instance_of_cell(k, len(layout)) == q] for q in range(len(layout))]
    sets, cell_of, single_of = [], [], []
    for q, (degree, M) in enumerate(layout):
        ks = np.array(cells[q])
        n = ks.size
        i, j = ks % NX, ks // NX
        px = X0 + CELL * i + 6 + (ks * 5) % 4 + 0.5        # a pixel centre 6..9 pixels into the cell
        py = Y0 + CELL * j + 6 + (ks * 3) % 4 + 0.5
        px[ks == 82], py[ks == 82] = 127.5, 95.5           # the image centre
        z = 2.5 + 3.0 * ((ks * 7) % N) / N                 # view depth 2.5 .. 5.5
        ndc = np.stack([px / W * 2 - 1, py / H * 2 - 1], 1)
        view = np.stack([ndc[:, 0] * z / fx, ndc[:, 1] * z / fy, -z, np.ones(n)], 1)
        Mi = np.linalg.inv(M.astype(np.float64))
        model = (view @ Vi.T) @ Mi.T
        pos = model[:, :3]
        if kind == "four" and q == 0:
            pos = np.round(pos / SNAP) * SNAP
        pos = pos.astype(np.float32)
        # isotropic in model space; the widest world axis is 1 px at the splat's depth
        amax = np.linalg.norm(M[:3, :3].astype(np.float64), axis=0).max()
        sigma = z / (fy * 0.5 * H) / amax
        f_dc, f_rest, single = _colours(rng, n, degree, pose_index)
        arrays = dict(positions=pos, f_dc=f_dc, f_rest=f_rest, opacity=np.full(n, 4.0, np.float32),
                      scale=np.log(np.repeat(sigma[:, None], 3, 1)).astype(np.float32),
                      rotation=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
        sets.append((arrays, M))
        cell_of.append(ks)
        single_of.append(np.where(single >= 0, single + 100 * degree, -1))
    return dict(sets=sets, degrees=[d for d, _ in layout], cell=np.concatenate(cell_of), single=np.concatenate(single_of),
                V=V, P=P, eye=eye, kind=kind, pose=pose)


@functools.lru_cache(maxsize=None)
def prepared(kind, pose, fmt):
    """the oracle's PreparedSet of every instance: the planes as the device holds them after commit(fmt, fmt)"""
    from oracle import binding as ob
    return [ob.PreparedSet(a, sh_format=FORMATS[fmt], rgba_format=FORMATS[fmt]) for a, _ in scene(kind, pose)["sets"]]


def _planes(ps):
    """(rgba [n,4], sh [n,15,3]) float64 of a PreparedSet"""
    n = ps.count
    sh = np.zeros((n, 45))
    if ps.sh_stride:
        sh[:, :ps.sh_stride] = ps.sh[:ps.sh_stride * n].reshape(n, ps.sh_stride)
    return ps.rgba.reshape(n, 4).astype(np.float64), sh.reshape(n, 15, 3)


def in_units(err, u):
    """|error| / u; where u is 0 (a base colour clamped to 0 and no coefficient) only an exact result is 0, anything else is inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u > 0, err / u, np.where(err == 0, 0.0, np.inf))


def unit(rgba, sh, degree, sh_only):
    """u per splat and channel [n,3]"""
    base = np.full((rgba.shape[0], 3), 0.5) if sh_only else np.abs(rgba[:, :3])
    ncoef = (degree + 1) ** 2 - 1
    return 2.0 ** -23 * (base + (np.abs(sh[:, :ncoef]) * BMAX[:ncoef, None]).sum(1))


@functools.lru_cache(maxsize=None)
def geometry(kind, pose):
    """float64 projection of every splat (global caller order): dict(center_px [n,2], read [n,2] (x, y) int, b1, b2, valid, dist [n],
    centre_norm [n]); asserts the premises of the read-out"""
    sc = scene(kind, pose)
    out = {k: [] for k in ("center_px", "b1", "b2", "valid", "dist", "centre_norm")}
    for (a, M), ps in zip(sc["sets"], prepared(kind, pose, "f32")):
        n = ps.count
        pr = npr.project(ps.positions.reshape(n, 3), ps.cov6.reshape(n, 6), ps.rgba.reshape(n, 4), np.zeros((n, 45)), 0, M, sc["V"], sc["P"],
                         sc["eye"], W, H, sh_degree=0)
        for k in ("center_px", "b1", "b2", "valid"):
            out[k].append(pr[k])
        world = ps.positions.reshape(n, 3).astype(np.float64) @ M[:3, :3].astype(np.float64).T + M[:3, 3].astype(np.float64)
        out["dist"].append(np.linalg.norm(world - sc["eye"].astype(np.float64), axis=1))
        out["centre_norm"].append(np.linalg.norm(world, axis=1))
    g = {k: np.concatenate(v) for k, v in out.items()}
    c = g["center_px"]
    g["read"] = np.floor(c).astype(np.int64)
    frac = c - np.floor(c)
    assert g["valid"].all()
    assert (np.minimum(frac, 1 - frac) >= 0.25).all(), "a centre lies within 0.25 px of a pixel edge"
    assert (np.abs(g["b1"]) + np.abs(g["b2"]) <= 6.0).all(), "a footprint reaches out of its cell's interior"
    i, j = sc["cell"] % NX, sc["cell"] // NX
    off = g["read"] - np.stack([X0 + CELL * i, Y0 + CELL * j], 1)
    assert ((off >= 6) & (off <= 9)).all(), "a read pixel left the middle of its cell"
    assert np.unique(sc["cell"]).size == N
    assert g["dist"].min() >= 2.0 and g["centre_norm"].max() <= 8.0 and np.linalg.norm(sc["eye"]) <= 8.0
    return g


@functools.lru_cache(maxsize=None)
def border_mask():
    """[H,W] bool: every pixel that is not one of a cell's inner 14 x 14"""
    m = np.ones((H, W), bool)
    for j in range(NY):
        for i in range(NX):
            m[Y0 + CELL * j + 1:Y0 + CELL * j + 15, X0 + CELL * i + 1:X0 + CELL * i + 15] = False
    return m


@functools.lru_cache(maxsize=None)
def reference(kind, pose, fmt, sh_degree, sh_only=False):
    """(rgb [n,3] float64, u [n,3]) of every splat for the frame's camera: np_reference.project on the dequantised planes"""
    sc = scene(kind, pose)
    rgb, us = [], []
    for (a, M), ps, sd in zip(sc["sets"], prepared(kind, pose, fmt), sc["degrees"]):
        n = ps.count
        rgba, sh = _planes(ps)
        assert ps.sh_degree == sd and (ps.sh_stride == 0) == (sd == 0)
        if sh_only:
            rgba = rgba.copy()
            rgba[:, :3] = 0.5
        pr = npr.project(ps.positions.reshape(n, 3), ps.cov6.reshape(n, 6), rgba, sh.reshape(n, 45), sd, M, sc["V"], sc["P"], sc["eye"], W, H,
                         sh_degree=sh_degree)
        rgb.append(pr["rgba"][:, :3])
        us.append(unit(rgba, sh, min(sd, sh_degree), sh_only))
    return np.concatenate(rgb), np.concatenate(us)


# ---- the ray-query batch: one ray per splat of scene("four", EXTRAS_POSE), aimed at its centre ------------------------------------------
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OCTANTS = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
# model-space offset origin -> centre of the exact rays of instance 0 (scale 0.5, 2, 1 along model x, y, z): 2.5 world units for the axes
_EXACT_LEN = np.array([5.0, 1.25, 2.5])


@functools.lru_cache(maxsize=None)
def rays():
    """dict(origin [n,3] float32, direction [n,3] float32 (world, unit), model_dir [n,3] float64 (the direction the reference uses:
    normalize(centre - M^-1 origin) from the float32 origin), intended [n,3] (the model-space direction asked for), exact [n] bool).
    Origins: instance 0 gets the six axes and the eight octant diagonals exactly, every instance a seeded spread over the sphere, the
    other instances the axes and diagonals as closely as their float32 origin allows.  Asserted: every ray is >= 2 long, starts within
    8 of the world origin, and stays more than 3.5 sigma (of that splat's widest axis) away from every other splat in front of its own."""
    sc = scene("four", EXTRAS_POSE)
    rng = np.random.Generator(np.random.PCG64(77))
    focal = float(sc["P"][1, 1]) * 0.5 * H
    worlds = []
    for (a, M) in sc["sets"]:
        M64 = M.astype(np.float64)
        worlds.append(a["positions"].astype(np.float64) @ M64[:3, :3].T + M64[:3, 3])
    allw = np.concatenate(worlds)
    sig_w = np.linalg.norm(allw - sc["eye"].astype(np.float64), axis=1) / focal      # >= every splat's largest world sigma (depth <= distance)
    fixed = [np.asarray(d, np.float64) for d in AXES + OCTANTS]
    O, D, MD, IN, EX = [], [], [], [], []
    for q, (a, M) in enumerate(sc["sets"]):
        M64 = M.astype(np.float64)
        Mi = np.linalg.inv(M64)
        p = a["positions"].astype(np.float64)
        n = p.shape[0]

        def make(i, d, exact):
            """the ray of splat i with the model-space direction d, or None when it is not isolated or starts too far out"""
            if exact:
                off = d * _EXACT_LEN if np.abs(d).sum() == 1 else d * 1.25
            else:
                d = d / np.linalg.norm(d)
                off = d * (2.25 / np.linalg.norm(M64[:3, :3] @ d))
            o = ((p[i] - off) @ M64[:3, :3].T + M64[:3, 3]).astype(np.float32)
            dw = worlds[q][i] - o.astype(np.float64)
            length = np.linalg.norm(dw)
            dw /= length
            rel = allw - o.astype(np.float64)
            t = np.maximum(rel @ dw, 0.0)
            miss = np.linalg.norm(rel - t[:, None] * dw, axis=1)
            # what could be walked before the aimed-at splat: every other splat whose closest point lies in front of it (hits are walked in
            # the order of that point; behind the first accepted hit, alpha 1, nothing counts).  3.5 sigma: response 0.002, the
            # acceptance threshold is kernel_min_response = 0.0113 (2.99 sigma)
            other = (np.linalg.norm(allw - worlds[q][i], axis=1) > 1e-9) & (rel @ dw < length + 0.25)
            if not (miss[other] > 3.5 * sig_w[other]).all() or length < 2.0 or np.linalg.norm(o) > 8.0:
                return None
            md = p[i] - (np.append(o.astype(np.float64), 1.0) @ Mi.T)[:3]
            assert not exact or np.array_equal(md, off), "an exact ray's model-space offset is not exact"
            return o, dw.astype(np.float32), md / np.linalg.norm(md), d / np.linalg.norm(d), exact

        got = [None] * n
        order = np.argsort(np.linalg.norm(worlds[q], axis=1), kind="stable")
        for d in fixed:                                  # each fixed direction goes to the first free splat (nearest the origin first) it suits
            for i in order:
                if got[i] is None:
                    got[i] = make(i, d, q == 0)
                    if got[i] is not None:
                        break
            else:
                raise AssertionError(f"no splat of instance {q} suits the direction {d}")
        for i in range(n):
            for attempt in range(50):
                if got[i] is not None:
                    break
                got[i] = make(i, rng.standard_normal(3), False)
            assert got[i] is not None, (q, i)
        for g in got:
            for lst, v in zip((O, D, MD, IN, EX), g):
                lst.append(v)
    r = dict(origin=np.array(O, np.float32), direction=np.array(D, np.float32), model_dir=np.array(MD), intended=np.array(IN), exact=np.array(EX))
    e = r["exact"]
    assert e.sum() == 14
    assert np.abs(r["model_dir"] - r["intended"]).max() <= 1e-6
    return r


@functools.lru_cache(maxsize=None)
def ray_reference(fmt, sh_degree, sh_only=False):
    """(rgb [n,3], u [n,3]) of the ray batch: np_reference.project's formula with cam_model replaced by the ray's model-space origin"""
    sc = scene("four", EXTRAS_POSE)
    md = rays()["model_dir"]
    rgb, us, at = [], [], 0
    for ps, sd in zip(prepared("four", EXTRAS_POSE, fmt), sc["degrees"]):
        n = ps.count
        rgba, sh = _planes(ps)
        base = np.full((n, 3), 0.5) if sh_only else rgba[:, :3].copy()
        deg = min(sd, sh_degree)
        if deg >= 1:
            base = base + npr.sh_radiance(sh, deg, md[at:at + n])
        rgb.append(base)
        us.append(unit(rgba, sh, deg, sh_only))
        at += n
    return np.concatenate(rgb), np.concatenate(us)
