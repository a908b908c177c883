"""The scenes of the blend tests (tests/test_blend_cpu.py, tests/test_gpu_blend.py, tests/_child_blend.py): every case is built for
one structure of k_composite's blend walk.  Constants of k_composite.hip: region 32x16 px, quarter (wave) 16x8 px; a batch holds 288
records, blending starts at 32 staged, a stage-A round scans 512 list entries; the additive mode: 448 per batch, starts at 192.

All sets have SH degree 0 (no f_rest): the colour is 0.5 + 0.2820948 f_dc as committed, so the blend test does not test shading.

  layers        eight screen-filling splats of opacity 0.8 (T = 0.2^k: 3.4e-4 after the 5th, 6.9e-5 after the 6th, clear of 1e-4 on
                every pixel), bright splats in alternating saturated colours behind.  A wave that retires at 1e-3 loses the 5th layer.
  hole          the front is eight layers of small discs of opacity 0.5 on a 2-px grid (a gaussian has no sharp edge, so a gap a
                few pixels wide cannot be cut into a screen-filling splat) with the discs within 3.2 px of one pixel left out:
                behind the front 101 of that quarter's 128 pixels are saturated and the hole's own T is 0.16, so the quarter stays
                live for hundreds of records; its neighbours retire.  Bright records behind the hole.
  second_batch  600 faint records over one region, which never saturates: more than 288 (and 448, and one stage-A round of 512)
                staged records reach it.  No record may be lost or doubled at a boundary.
  faint         opacities between 1/255 and 3/255: the alpha <= 1/255 rule decides most fragments, nothing saturates.
  partial       333x217: the last region column and row hold pixels outside the image, which start saturated; opaque splats.
  crowded       fragment_cases' natural case with the gaussian on.
  mixed_sets    two different sets, one instance each, under a TRS and under a mirrored transform (negative determinant), in
                fp32, fp16 (mixed_sets_f16) and uint8 (mixed_sets_u8) storage of colour and opacity: the blend is fed what the
                committed scene holds after quantisation, concatenated by global id.
"""
import functools

import numpy as np

from vk_gaussian_splatting_amd import synth
import fragment_cases as fc
import np_blend as nb
import occluder_levels as ol

MIXED = {"mixed_sets": (0, 0), "mixed_sets_f16": (1, 1), "mixed_sets_u8": (2, 2)}   # name -> (sh_format, rgba_format) of the commit
CASES = ["layers", "hole", "second_batch", "faint", "partial", "crowded"] + list(MIXED)
SURFACE_CASES = ["layers", "hole", "partial", "crowded", "mixed_sets", "mixed_sets_u8"]   # cases whose pixels cross depth_iso_threshold
CHILD_CASES = ["second_batch", "hole"]                      # rendered on both binning paths and with the smallest bins as well
ISO = 0.7
HOLE = (40, 20)      # the live pixel of "hole": region (1,1), quarter (0,0) = x 32..47, y 16..23
HOLE_QUARTER = (slice(16, 24), slice(32, 48))
SECOND_BATCH_RECORDS = 600
HOLE_BEHIND = 300      # bright records behind the hole (the last ids of the set)
FRONT_LAYERS = 8


def _f_dc(colour):
    return ((np.asarray(colour, np.float64) - 0.5) / 0.28209479177387814).astype(np.float32)


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p)).astype(np.float32)


SATURATED = [(0.95, 0.05, 0.05), (0.05, 0.95, 0.05), (0.05, 0.05, 0.95)]


def _scene(rows, w, h):
    """rows: (x px, y px, sigma1 px, sigma2 px, angle, distance, opacity, (r, g, b)) -> case dict"""
    a = fc._discs([r[:6] for r in rows], w, h, fc.GRID_EYE_Z)
    a["opacity"] = _logit([r[6] for r in rows])
    a["f_dc"] = _f_dc([r[7] for r in rows])
    return dict(sets=[(a, None)], cam=fc.grid_camera(w, h), W=w, H=h)


def _layer_colour(k):
    return (0.2 + 0.1 * k, 0.9 - 0.1 * k, 0.3 + 0.05 * k)


def _layers():
    w, h = 96, 64
    rows = [(w / 2 + 3.0, h / 2 + 2.0) + fc.OVERSIZED + (4.0 + 0.05 * k, 0.8, _layer_colour(k)) for k in range(FRONT_LAYERS)]
    j = 0
    for y in np.arange(6.0, h, 10.0):
        for x in np.arange(5.0, w, 9.0):
            rows.append((x + 0.3 * (j % 3), y + 0.2 * (j % 5), 5.0, 4.0, 0.4 * j, 5.0 + 0.01 * j, 0.9, SATURATED[j % 3]))
            j += 1
    return _scene(rows, w, h)


def _hole():
    w, h = 64, 32
    rows, j = [], 0
    for k in range(FRONT_LAYERS):
        for y in np.arange(1.0, h, 2.0):
            for x in np.arange(1.0, w, 2.0):
                if np.hypot(x - (HOLE[0] + 0.5), y - (HOLE[1] + 0.5)) < 3.2:
                    continue
                rows.append((x, y, 1.5, 1.5, 0.0, 4.0 + 0.05 * k + 1e-5 * j, 0.5, _layer_colour(k)))
                j += 1
    r = np.random.default_rng(11)
    for j in range(HOLE_BEHIND):
        rows.append((HOLE[0] + 0.5 + r.uniform(-6, 6), HOLE[1] + 0.5 + r.uniform(-4, 4), 3.0, 2.5, 0.3 * j, 5.0 + 0.005 * j, 0.6, SATURATED[j % 3]))
    return _scene(rows, w, h)


def _second_batch():
    w, h = 96, 48
    r = np.random.default_rng(12)
    rows = [(16.0 + r.uniform(-6, 6), 8.0 + r.uniform(-3, 3), 4.0, 3.5, 0.2 * j, 4.0 + 0.002 * j, 0.012, tuple(r.uniform(0.05, 0.95, 3)))
            for j in range(SECOND_BATCH_RECORDS)]
    return _scene(rows, w, h)


def _faint():
    w, h = 96, 64
    r = np.random.default_rng(13)
    rows = [(r.uniform(0, w), r.uniform(0, h), r.uniform(2, 6), r.uniform(2, 6), r.uniform(0, 3), 4.0 + 0.001 * j,
             r.uniform(1.05 / 255, 3.0 / 255), tuple(r.uniform(0.05, 0.95, 3))) for j in range(1500)]
    return _scene(rows, w, h)


def _degree0(c):
    sets = []
    for a, m in c["sets"]:
        a = dict(a)
        a["f_rest"] = np.zeros((a["positions"].shape[0], 0), np.float32)
        sets.append((a, m))
    return dict(c, sets=sets)


@functools.lru_cache(maxsize=None)
def _mixed_sets():
    sets = []
    for n, seed, grow, dense in ((1500, 21, 0.8, 1.0), (1200, 22, 0.6, 2.5)):
        sc = synth.make_scene(n, seed=seed, sh_coeffs_per_channel=0)
        sc["f_rest"] = np.zeros((n, 0), np.float32)
        sc["scale"] = (sc["scale"] + grow).astype(np.float32)
        sc["opacity"] = (sc["opacity"] + dense).astype(np.float32)
        sets.append(sc)
    trs = fc._trs([0.8, 1.2, 1.0], [0.1, 1.0, 0.3], -0.6, [0.6, 0.1, -0.4])
    mirrored = fc._trs([-1.0, 1.1, 0.9], [0.3, 1.0, -0.2], 0.5, [-0.5, 0.0, 0.3])   # determinant < 0
    w, h = 208, 120
    return dict(sets=[(sets[0], trs), (sets[1], mirrored)], cam=fc.orbit_camera(w, h), W=w, H=h)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(sets=[(arrays, transform or None)], cam=(V, P, eye), W, H[, formats=(sh_format, rgba_format) of the commit])"""
    if name in MIXED:
        return dict(_mixed_sets(), formats=MIXED[name])
    if name == "partial":
        return _degree0(fc.case("opaque_gaussian"))
    if name == "crowded":
        return _degree0(fc.case("crowded"))
    return {"layers": _layers, "hole": _hole, "second_batch": _second_batch, "faint": _faint}[name]()


class Ref:
    """The float64 side of one case, from the oracle alone: instances, the sorted stream (nearest first), the key depths, the colours
    as the oracle holds them, the oracle's own projected records as a splat table.  Built once per process, never modified."""

    def __init__(self, ob, name):
        c = case(name)
        self.name, self.c, self.W, self.H = name, c, c["W"], c["H"]
        V, P, eye = c["cam"]
        shf, rgbaf = c.get("formats", (0, 0))
        prepared = {id(a): ob.PreparedSet(a, sh_format=shf, rgba_format=rgbaf) for a, _ in c["sets"]}
        self.inst = ob.make_instances([(prepared[id(a)], m) for a, m in c["sets"]])
        self.frame_kw = dict(view=V, proj=P, camera_pos=eye, width=c["W"], height=c["H"], sh_degree=0)
        self.counts = [prepared[id(a)].count for a, _ in c["sets"]]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)])
        self.total = int(self.offsets[-1])
        self.rgba = np.concatenate([prepared[id(a)].rgba.reshape(-1, 4) for a, _ in c["sets"]]).astype(np.float64)
        frame = ob.make_frame(**self.frame_kw)
        keys, ids = ob.key_cull(frame, self.inst)
        ks, order = ob.sort_stable(keys, ids)
        self.order_btf = order                       # the sorted stream: far to near
        self.order = order[::-1].copy()              # nearest first
        self.key_depth = np.full(self.total, np.inf, np.float32)
        self.key_depth[order] = ol.depths_of_btf_keys(ks)
        rec = np.zeros((self.order.size, 7))
        self.ndc_z = np.zeros(self.total)
        keep = np.zeros(self.order.size, bool)
        for j, g in enumerate(self.order):
            k = int(np.searchsorted(self.offsets, g, side="right") - 1)
            q = ob.project(frame, self.inst, k, int(g - self.offsets[k]))
            if q.valid:
                keep[j] = True
                rec[j] = [q.center_px[0], q.center_px[1], q.basis1[0], q.basis1[1], q.basis2[0], q.basis2[1], q.rgba[3]]
                self.ndc_z[g] = q.ndc_z
        self.table = self.table_of(self.order[keep], rec[keep])
        # world normals as the oracle holds them (not quantised), and how far another fp32 evaluation may lie from them
        self.normals, self.normal_err = np.zeros((self.total, 3)), np.zeros(self.total)
        for k, (a, m) in enumerate(c["sets"]):
            o, n = int(self.offsets[k]), self.counts[k]
            for i in range(n):
                self.normals[o + i] = ob.splat_normal(frame, self.inst, k, i, quantize=False)
            M = np.eye(4) if m is None else np.asarray(m, np.float64)
            local = (np.linalg.inv(M) @ np.append(np.asarray(eye, np.float64), 1.0))[:3] - np.asarray(a["positions"], np.float64)
            q = np.asarray(a["rotation"], np.float64)
            w_, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
            inv = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y), 2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z),
                            2 * (y * z - w_ * x), 2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
            self.normal_err[o:o + n] = nb.normal_allowance(np.exp(np.asarray(a["scale"], np.float64)), np.einsum("nr,nrc->nc", local, inv))
        self._memo = {}

    def table_of(self, ids, rec):
        """a splat table from projected records [n, >= 7] (centre, basis 1, basis 2, opacity) of the global ids `ids`"""
        return nb.table_from_records(ids, rec[:, 0:2], rec[:, 2:4], rec[:, 4:6], rec[:, 6], self.key_depth[np.asarray(ids, np.int64)])

    def median_level(self):
        return ol.pick_level(self.key_depth[np.isfinite(self.key_depth)], 0.5)

    def background(self):
        return ol.random_background(self.W, self.H, 5)

    def blend(self, table=None, colours=None, order=None, occluder=False, iso=None, normals=False, **kw):
        """np_blend.blend of this case (memoised for the oracle's own table): occluder: at the median level over background()"""
        key = (occluder, iso, normals, tuple(sorted(kw.items()))) if table is None and colours is None else None
        if key is not None and key in self._memo:
            return self._memo[key]
        b = nb.blend(self.table if table is None else table, self.order if order is None else order, self.rgba[:, :3] if colours is None else colours, self.W, self.H,
                     delta=fc.DELTA, depth_level=float(self.median_level()) if occluder else None,
                     bg=self.background() if occluder else None, iso=iso, normals=self.normals if normals else None,
                     normal_err=self.normal_err if normals == "other" else None, **kw)
        if key is not None:
            self._memo[key] = b
        return b

    def simulate(self, order=None, occluder=False, **kw):
        return nb.simulate(self.table, self.order if order is None else order, self.rgba[:, :3], self.W, self.H,
                           depth_level=float(self.median_level()) if occluder else None, bg=self.background() if occluder else None, **kw)


_refs = {}


def reference(ob, name):
    if name not in _refs:
        _refs[name] = Ref(ob, name)
    return _refs[name]
