"""Scenes of the traced frames with mesh hits (mgs_frame_set_trace_meshes): splats from trace_lit_cases, small meshes with two materials.
Frames are at most 48 x 40.

u1  a blob straddling an upright quad over the splat floor: splats behind the quad are cut, splats in front weight it by T
u2  meshes only, no splat set committed
u3  threshold 0.5 under a dense and a thin blob
u4  an invisible instance plus instances under mesh_ray_cases.NONUNIFORM / MIRRORED
u5  the upright quad plus a box through a fisheye lens with depth of field
l1  a blob over a mesh floor under a point light: the splats' shadow falls on the mesh
l2  a mesh box's shadow on the splat floor
l3  a box on a floor quad under a directional light, no splats: mesh shadows on meshes, the floor under the box included
l4  a spot light whose range ends on the mesh floor; no lights (the headlight); an emission-only triangle beside a shaded one
l5  a translucent veil in front of a lit mesh, and a cloud too thin for the iso threshold: discarded, the mesh shows at full weight
l6  samples_per_pass 4 / 18 / 32, a specular material with shininess 64
u2 and l3 also hold tests/golden/meshes/fixture.obj (38 triangles, the loader's two materials, one of them emission only) under a
scale and a rotation."""
import functools

import numpy as np

import mesh_cases as mc
import mesh_ray_cases as mrc
import np_lighting as nl
import np_trace_mesh as ntm
import trace_cases as tc
import trace_lit_cases as tlc

MAT_SHADED = dict(ambient=(0.1, 0.12, 0.14), diffuse=(0.7, 0.6, 0.5), specular=(0.0, 0.0, 0.0), emission=(0.0, 0.0, 0.0), shininess=0.0)
MAT_GLOW = dict(ambient=(0.0, 0.0, 0.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0), emission=(0.3, 0.5, 0.2), shininess=0.0)
MATERIALS = [MAT_SHADED, MAT_GLOW]


def quad(corners, normal, transform=None):
    """two triangles over four corners (counter-clockwise), one material each"""
    return dict(positions=np.float32(corners), indices=[[0, 1, 2], [0, 2, 3]], normals=np.float32([normal] * 4), material_ids=[0, 1],
                materials=MATERIALS, transform=transform, visible=True)


def box(lo, hi):
    """twelve triangles, face normals, the materials alternating"""
    lo, hi = np.float32(lo), np.float32(hi)
    pos, nrm, idx = [], [], []
    for axis in range(3):
        for side, sign in ((lo, -1.0), (hi, 1.0)):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3, np.float32)
            n[axis] = sign
            base = len(pos)
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = np.zeros(3, np.float32)
                p[axis], p[u], p[v] = side[axis], (hi if a else lo)[u], (hi if b else lo)[v]
                pos.append(p)
                nrm.append(n)
            idx += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return dict(positions=np.float32(pos), indices=idx, normals=np.float32(nrm), material_ids=[k % 2 for k in range(12)], materials=MATERIALS,
                transform=None, visible=True)


UPRIGHT = quad([[-0.6, -0.6, 0.0], [0.6, -0.6, 0.0], [0.6, 0.8, 0.0], [-0.6, 0.8, 0.0]], (0.0, 0.0, 1.0))
FLOOR = quad([[-1.4, -0.5, 1.4], [1.4, -0.5, 1.4], [1.4, -0.5, -1.4], [-1.4, -0.5, -1.4]], (0.0, 1.0, 0.0))
BOX = box((-0.25, -0.5, -0.2), (0.2, 0.0, 0.25))


MAT_SPEC = dict(MAT_SHADED, specular=(0.5, 0.5, 0.5), shininess=64.0)


def fixture(transform):
    """the fixture as the loader reads it (positions, normals, material ids and the MTL's materials), placed by `transform`"""
    from vk_gaussian_splatting_amd import capi
    v = capi.Mesh.load_obj(mc.FIXTURE).view()
    return dict(positions=v["positions"], indices=v["indices"], normals=v["normals"], material_ids=v["material_ids"],
                materials=[dict(m) for m in v["materials"]], transform=np.asarray(transform, np.float32), visible=True)


def placed(mesh, transform=None, visible=True, materials=None):
    return dict(mesh, transform=transform, visible=visible, materials=materials or mesh["materials"])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: trace_cases' / trace_lit_cases' dict plus meshes (np_mesh_rays dicts with `materials`) and mesh_min_T; a case with
    `lights` is a frame of mgs_render_traced_lit"""
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(1.2, -1.0, -0.2), intensity=1.0)   # the box's shadow falls on the floor's shaded triangle
    spot = nl.default_light(type=nl.LIGHT_SPOT, position=(0.0, 1.0, 0.0), direction=(0.0, -1.0, 0.0), range=1.6, intensity=3.0,
                            inner_cone_deg=25.0, outer_cone_deg=40.0)   # 1.5 above the floor: the range ends 0.56 from the axis
    eye, target = (0.0, 1.3, 2.6), (0.0, -0.35, 0.0)
    scene = tlc.join(tlc.floor(), tlc.blob())
    dense = tlc.blob(centre=(-0.3, 0.15, 0.5), opacity=4.0, seed=3)
    thin = tlc.blob(centre=(0.3, 0.15, 0.5), opacity=-2.0, seed=4)
    veil = tlc.blob(centre=(-0.3, 0.15, 0.5), opacity=0.0, seed=5, n=40)
    out = {}
    out["u1"] = dict(tc._case([(scene, None)], eye, target, W=48, H=40), meshes=[UPRIGHT])
    out["u2"] = dict(tc._case([], eye, target, W=37, H=29), meshes=[UPRIGHT, BOX, fixture(tc.trs((0.3, 0.3, 0.3), (0, 1, 0), 25.0, (0.85, -0.3, 0.4)))])
    out["u3"] = dict(tc._case([(tlc.join(dense, thin), None)], eye, target, W=48, H=40), meshes=[UPRIGHT], mesh_min_T=0.5)
    out["u4"] = dict(tc._case([(scene, None)], eye, target, W=48, H=40),
                     meshes=[placed(UPRIGHT, visible=False), placed(UPRIGHT, mrc.NONUNIFORM), placed(BOX, mrc.MIRRORED)])
    out["u5"] = dict(tc._case([(scene, None)], eye, target, W=41, H=37,
                              frame=dict(camera_model=1, fov_rad=1.0, dof_mode=1, focus_dist=2.5, aperture=0.004)), meshes=[UPRIGHT, BOX])
    out["l1"] = dict(tlc._case([(tlc.blob(), None)], [point]), meshes=[FLOOR])
    low = nl.default_light(position=(1.5, 0.6, 0.5), range=10.0, intensity=4.0)   # low in the +x: the box throws a long shadow
    out["l2"] = dict(tlc._case([(tlc.floor(), None)], [low]), meshes=[BOX])
    out["l3"] = dict(tlc._case([], [sun]), meshes=[FLOOR, BOX, fixture(tc.trs((0.3, 0.3, 0.3), (0, 1, 0), 25.0, (-0.8, -0.32, 0.3)))])   # (lifted off the floor quad: no coplanar pair)
    out["l4_spot"] = dict(tlc._case([(tlc.blob(), None)], [spot]), meshes=[FLOOR])
    out["l4_headlight"] = dict(tlc._case([(tlc.blob(), None)], []), meshes=[FLOOR])
    out["l5"] = dict(tlc._case([(tlc.join(veil, thin), None)], [point]), meshes=[UPRIGHT])
    for spp in (4, 18, 32):
        out[f"l6_{spp}"] = dict(tlc._case([(tlc.blob(), None)], [point], trace=dict(samples_per_pass=spp), W=33, H=27),
                                meshes=[placed(FLOOR, materials=[MAT_SPEC, MAT_GLOW])])
    for c in out.values():
        c.setdefault("mesh_min_T", 0.0)
        c["sets"] = [(a, np.eye(4, dtype=np.float32) if M is None else M) for a, M in c["sets"]]
    return out


def restate_with(c, inst, **over):
    L = c.get("light", {})
    kw = dict(tlc._trace_kw(c), **over)
    return ntm.frame(inst, c["meshes"], [m["materials"] for m in c["meshes"]], c["V"], c["P"], c["W"], c["H"], c["eye"], c.get("lights"),
                     c.get("materials"), lit="lights" in c, mesh_min_T=c["mesh_min_T"], shadows=L.get("shadows_mode", 0),
                     offset=L.get("particle_shadow_offset", 0.2), threshold=L.get("particle_shadow_transmittance_threshold", 0.8),
                     strength=L.get("particle_shadow_color_strength", 0.0), **kw)


@functools.lru_cache(maxsize=None)
def restate(name):
    """the restatement of a case from its arrays alone; computed once and shared: do not modify the result"""
    c = cases()[name]
    return restate_with(c, [(ntm.ntl.prepare_set(a), M) for a, M in c["sets"]])
