"""Scenes of the indirect traced frames (mgs_render_traced_indirect): trace_mesh_cases' meshes with mirror and glass materials, flat
reflectors only (a direction error of one ulp then grows linearly with the path's length).  Frames are at most 48 x 40.

b1      a mirror floor under a splat blob, one point light, hard shadows: the lit splats' reflection (the raw integrated normal at b = 1)
b2_N    two facing mirrors and an emissive box between them, max_bounces N = 1, 3, 16; 37 x 29 (no multiple of 16 in either axis)
b3      a glass slab (ior 1.5, coloured Tf) in front of a blob over the mirror floor
b4_far  b1 with its only light out of range of every mesh point: nothing bounces
b4_head b1 without lights: the headlight
b5      splats partially in front of the mirror (T carried into the bounce), min_mesh_composite_transmittance 0.5"""
import functools

import numpy as np

import np_lighting as nl
import np_trace_bounce as ntb
import trace_cases as tc
import trace_lit_cases as tlc
import trace_mesh_cases as tmc

MIRROR = dict(ambient=(0.02, 0.02, 0.03), diffuse=(0.1, 0.12, 0.1), specular=(0.8, 0.7, 0.6), emission=(0.0, 0.0, 0.0), shininess=32.0)
MIRROR_B = dict(MIRROR, specular=(0.5, 0.8, 0.9))
GLASS = dict(ambient=(0.01, 0.01, 0.01), diffuse=(0.05, 0.05, 0.05), specular=(0.0, 0.0, 0.0), emission=(0.0, 0.0, 0.0), shininess=8.0)
REFLECT = dict(transmittance=(0.0, 0.0, 0.0), ior=1.0, illum=1)
REFRACT = dict(transmittance=(0.9, 0.8, 0.7), ior=1.5, illum=2)
NONE = dict(transmittance=(0.0, 0.0, 0.0), ior=1.0, illum=0)


def prism(h):
    """a right-angle glass prism, flat normals: the entry face z = 0 (normal +z, x and y in [-h, h]), the exit face y = -h, the
    hypotenuse from (y = h, z = 0) to (y = -h, z = -2h) at 45 degrees to both, and the two caps x = -h, x = h"""
    s = np.sqrt(0.5)
    faces = [([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], (0, 0, 1)),
             ([[-h, -h, -2 * h], [h, -h, -2 * h], [h, -h, 0], [-h, -h, 0]], (0, -1, 0)),
             ([[-h, h, 0], [h, h, 0], [h, -h, -2 * h], [-h, -h, -2 * h]], (0, s, -s))]
    pos, nrm, idx = [], [], []
    for corners, n in faces:
        b = len(pos)
        pos += corners
        nrm += [n] * 4
        idx += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    for x, sign in ((-h, -1.0), (h, 1.0)):
        b = len(pos)
        pos += [[x, -h, 0], [x, h, 0], [x, -h, -2 * h]]
        nrm += [(sign, 0, 0)] * 3
        idx += [[b, b + 1, b + 2]]
    return dict(positions=np.float32(pos), indices=idx, normals=np.float32(nrm), material_ids=[k % 2 for k in range(len(idx))],
                materials=tmc.MATERIALS, transform=None, visible=True)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: trace_mesh_cases' lit case plus bounce (per mesh instance a list of bounce materials, or None) and max_bounces"""
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    far = nl.default_light(position=(0.3, 9.0, 0.2), range=2.0, intensity=4.0)
    floor = tmc.placed(tmc.FLOOR, materials=[MIRROR, MIRROR_B])
    out = {}
    out["b1"] = dict(tlc._case([(tlc.blob(), None)], [point]), meshes=[floor], bounce=[[REFLECT, REFLECT]], max_bounces=3)
    left = tmc.placed(tmc.quad([[-0.9, -0.6, 0.9], [-0.9, -0.6, -0.9], [-0.9, 0.9, -0.9], [-0.9, 0.9, 0.9]], (1.0, 0.0, 0.0)), materials=[MIRROR, MIRROR_B])
    right = tmc.placed(tmc.quad([[0.9, -0.6, -0.9], [0.9, -0.6, 0.9], [0.9, 0.9, 0.9], [0.9, 0.9, -0.9]], (-1.0, 0.0, 0.0)), materials=[MIRROR_B, MIRROR])
    glow = tmc.placed(tmc.BOX, materials=[tmc.MAT_GLOW, tmc.MAT_SHADED])
    for nb in (1, 3, 16):
        out[f"b2_{nb}"] = dict(tlc._case([], [point], W=37, H=29, eye=(0.0, 0.2, 0.6), target=(-0.9, 0.12, 0.55)), meshes=[left, right, glow],
                               bounce=[[REFLECT, REFLECT], [REFLECT, REFLECT], None], max_bounces=nb)
    slab = tmc.box((-0.9, -0.3, 0.7), (-0.1, 0.7, 0.85))
    slab = tmc.placed(slab, materials=[GLASS, GLASS])
    # the prism's entry face looks at the camera: the primary rays cross it nearly head-on and meet the hypotenuse near 45 degrees,
    # beyond the critical angle of ior 1.5 (41.8 degrees)
    tilt = np.degrees(np.arctan2(1.65, 2.6))
    wedge = tmc.placed(prism(0.2), tc.trs((1.0, 1.0, 1.0), (1, 0, 0), -tilt, (0.5, 0.25, 0.9)), materials=[GLASS, GLASS])
    out["b3"] = dict(tlc._case([(tlc.blob(), None)], [point]), meshes=[floor, slab, wedge],
                     bounce=[[REFLECT, NONE], [REFRACT, REFRACT], [REFRACT, REFRACT]], max_bounces=4)
    out["b4_far"] = dict(tlc._case([(tlc.blob(), None)], [far]), meshes=[floor], bounce=[[REFLECT, REFLECT]], max_bounces=3)
    out["b4_head"] = dict(tlc._case([(tlc.blob(), None)], []), meshes=[floor], bounce=[[REFLECT, REFLECT]], max_bounces=2)
    # three lights: the last one IN RANGE is not the last of the table, whose last light is out of range of every mesh point
    side = nl.default_light(position=(-1.2, 0.9, 0.8), range=10.0, intensity=2.0, color=(1.0, 0.8, 0.6))
    out["b4_three"] = dict(tlc._case([(tlc.blob(), None)], [point, side, far]), meshes=[floor], bounce=[[REFLECT, REFLECT]], max_bounces=2)
    veil = tlc.blob(centre=(0.0, -0.2, 0.9), opacity=0.0, seed=5, n=40)
    for spp in (4, 18, 32):
        out["b5" if spp == 18 else f"b5_{spp}"] = dict(
            tlc._case([(tlc.join(tlc.blob(), veil), None)], [point], W=33, H=27, trace=dict(samples_per_pass=spp)), meshes=[floor],
            bounce=[[REFLECT, REFLECT]], max_bounces=2, mesh_min_T=0.5)
    out["b5_fisheye"] = dict(tlc._case([(tlc.join(tlc.blob(), veil), None)], [point], W=33, H=27,
                                       frame=dict(camera_model=1, fov_rad=1.0, dof_mode=1, focus_dist=2.5, aperture=0.004)), meshes=[floor],
                             bounce=[[REFLECT, REFLECT]], max_bounces=2, mesh_min_T=0.5)
    # the bare mirror: no lights (the headlight shades the floor, so it bounces), a splat material that is emission alone (the
    # bounce's splat surface keeps its radiance): the bounce adds specular x what the reflected ray's walk integrates
    glowing = dict(ambient=(0.0, 0.0, 0.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0), emission=(1.0, 1.0, 1.0), shininess=0.0)
    # (min_transmittance 0: the bounce's walk ends on maxComponent(specular * S) and the ray query's on S; with the cut at 0 both
    # walk every hit, and the two sums can be held to each other)
    out["bare"] = dict(tlc._case([(tlc.blob(), None)], [], materials=[glowing], trace=dict(min_transmittance=0.0)), meshes=[floor], bounce=[[REFLECT, REFLECT]], max_bounces=1)
    for c in out.values():
        c.setdefault("mesh_min_T", 0.0)
        c["sets"] = [(a, np.eye(4, dtype=np.float32) if M is None else M) for a, M in c["sets"]]
    return out


# the cases the child also renders with fp16 / uint8 colour and SH storage: k_trace_bounce<1, KB> and <2, KB> at KB 18, 4 and 32
STORAGE_CASES = ("b1", "b5_4", "b5_32")


def restate_with(c, inst, **over):
    L = c.get("light", {})
    kw = dict(tlc._trace_kw(c), **over)
    bounce = kw.pop("bounce", c["bounce"])
    return ntb.frame(inst, c["meshes"], [m["materials"] for m in c["meshes"]], bounce, c["V"], c["P"], c["W"], c["H"], c["eye"], c.get("lights"),
                     c.get("materials"), max_bounces=kw.pop("max_bounces", c["max_bounces"]), mesh_min_T=c["mesh_min_T"],
                     shadows=L.get("shadows_mode", 0), offset=L.get("particle_shadow_offset", 0.2),
                     threshold=L.get("particle_shadow_transmittance_threshold", 0.8), strength=L.get("particle_shadow_color_strength", 0.0), **kw)


@functools.lru_cache(maxsize=None)
def restate(name):
    """the restatement of a case from its arrays alone; computed once and shared: do not modify the result"""
    c = cases()[name]
    return restate_with(c, [(ntb.ntl.prepare_set(a), M) for a, M in c["sets"]])
