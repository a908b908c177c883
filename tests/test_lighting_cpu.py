"""CPU tests of the deferred lighting feature: the C ABI declares and exports the entry points, the ctypes layer mirrors them, the
numpy restatement (np_lighting.py) does what the shaders say on hand-computed pixels, project files carry lights and materials,
and — from the reference's own G-buffer — the ambiguity cap holds for the GPU test's cases and the float32-vs-float64 difference
that sets the GPU bar is what lighting_cases.py records."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, lookat, persp
import lighting_cases as lc
import np_lighting as nl
import occluder_levels as ol

HEADER = os.path.join(ROOT, "include", "mgs.h")
LIB = os.path.join(ROOT, "vk_gaussian_splatting_amd", "csrc", "libmgs.so")
NEW = ("mgs_light_default", "mgs_material_default", "mgs_scene_set_lights", "mgs_instance_set_material")


# ---- 1. header / exports / ctypes ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_lighting_entry_points():
    hdr = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    assert re.search(r"int32_t\s+lighting_mode\s*;", hdr) and "reserved_" not in hdr.split("typedef struct MgsFrameParams")[1].split("} MgsFrameParams")[0]
    assert re.search(r"MGS_STAGE_LIGHT\s*=\s*7\b", hdr) and re.search(r"MGS_STAGE_COUNT\s*=\s*8\b", hdr)
    assert re.search(r"#define\s+MGS_MAX_LIGHTS\s+64\b", hdr)
    assert "PARITY UNPINNED" in hdr.upper()
    lib = ctypes.CDLL(LIB)
    for name in NEW:
        assert hasattr(lib, name), f"{name} not exported by libmgs.so"


def test_capi_mirrors_the_structures_and_defaults():
    from vk_gaussian_splatting_amd import capi
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS
    assert ctypes.sizeof(capi.FrameParams) == 288
    assert ctypes.sizeof(capi.Light) == 15 * 4 and ctypes.sizeof(capi.Material) == 13 * 4
    p = capi.default_params(64, 48)
    assert p.lighting_mode == 0 == capi.LIGHTING_DISABLED
    assert capi.FrameParams.lighting_mode.offset == 284
    assert (capi.LIGHTING_DIRECT, capi.LIGHTING_INDIRECT) == (1, 2)
    assert (capi.LIGHT_DIRECTIONAL, capi.LIGHT_POINT, capi.LIGHT_SPOT) == (0, 1, 2)
    l = capi.make_light()  # wavefront.h:81-93
    assert l.type == 1 and list(l.color) == [1, 1, 1] and l.intensity == 1.0 and list(l.position) == [0, 0, 0]
    assert l.range == 10.0 and list(l.direction) == [0, 0, -1] and (l.inner_cone_deg, l.outer_cone_deg) == (30.0, 45.0)
    assert l.attenuation_mode == 2
    m = capi.make_material()  # splat_set_vk.cpp:128-135
    assert list(m.ambient) == list(m.diffuse) == list(m.specular) == [0, 0, 0] and list(m.emission) == [1, 1, 1] and m.shininess == 0.0
    d = nl.default_light()
    for k in ("type", "intensity", "range", "inner_cone_deg", "outer_cone_deg", "attenuation_mode"):
        assert getattr(l, k) == d[k]
    for method in ("set_lights", "set_material", "download_consolidated_depth"):
        assert callable(getattr(capi.Scene, method))


def test_null_handle_is_an_error_not_a_crash():
    lib = ctypes.CDLL(LIB)
    lib.mgs_scene_set_lights.restype = ctypes.c_int
    lib.mgs_scene_set_lights.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.mgs_instance_set_material.restype = ctypes.c_int
    lib.mgs_instance_set_material.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mgs_last_error.restype = ctypes.c_char_p
    assert lib.mgs_scene_set_lights(None, None, 0) == -1
    assert b"null handle" in lib.mgs_last_error()
    buf = (ctypes.c_float * 13)()
    assert lib.mgs_instance_set_material(None, 0, buf) == -1
    assert b"null handle" in lib.mgs_last_error()
    lib.mgs_light_default(None)
    lib.mgs_material_default(None)  # tolerated


# ---- 2. the restatement on hand-computed pixels ----------------------------------------------------------------------------
EYE = np.array([0.0, 0.0, 5.0], np.float32)
V1 = lookat(EYE, [0, 0, 0], [0, 1, 0])
P1 = persp(60.0, 1.0, 0.1, 100.0)
BASE = np.array([0.5, 0.25, 1.0], np.float32)


def one_pixel(lights, mats, world=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), nw=1.0, pid=0, alpha=0.3, dtype=np.float64):
    """a 1x1 frame whose only pixel looks along the view axis; the picked depth is chosen so that the reconstructed world
    position is `world` (on the view axis: x = y = 0)"""
    clip = P1.astype(np.float64) @ (V1.astype(np.float64) @ np.array([world[0], world[1], world[2], 1.0]))
    depth = np.array([[clip[2] / clip[3]]], np.float32)
    img = np.array([[[BASE[0], BASE[1], BASE[2], alpha]]], np.float32)
    nrm = np.array([[[normal[0] * nw, normal[1] * nw, normal[2] * nw, nw]]], np.float32)
    ids = np.array([[pid]], np.uint32)
    return nl.light_frame(img, depth, ids, nrm, V1, P1, EYE, lights, mats, [0], dtype=dtype)


DIFF = nl.default_material(diffuse=(1, 1, 1), emission=(0, 0, 0), shininess=8.0)


def test_world_position_reconstruction():
    # a point light exactly `d` above the surface point, attenuation mode 3: the result depends on d^2 alone
    r = one_pixel([nl.default_light(position=(0, 0, 2.0), range=10.0, attenuation_mode=3)], [DIFF])
    assert np.allclose(r.lit[0, 0, :3], BASE * (1.0 / (4.0 + 0.01)), rtol=2e-5)  # the picked depth is an fp32 value
    assert r.lit[0, 0, 3] == 1.0


@pytest.mark.parametrize("mode,expect", [(0, 1.0), (1, 1.0 - 2.0 / 10.0), (2, 1.0 / (1.0 + 4.0)), (3, 1.0 / (4.0 + 0.01))])
def test_point_light_attenuation_modes(mode, expect):
    r = one_pixel([nl.default_light(position=(0, 0, 2.0), range=10.0, attenuation_mode=mode, intensity=3.0, color=(1, 0.5, 0.25))], [DIFF])
    assert np.allclose(r.lit[0, 0, :3], BASE * np.array([1, 0.5, 0.25]) * 3.0 * expect, rtol=2e-5)


def test_directional_light_and_ndotl():
    s = 1 / math.sqrt(2)
    r = one_pixel([nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(0.0, -2.0, -2.0), intensity=2.0)], [DIFF])
    assert np.allclose(r.lit[0, 0, :3], BASE * 2.0 * s, rtol=1e-6)  # L = -normalize(direction), N.L = cos 45
    r = one_pixel([nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(0.0, 0.0, 1.0))], [DIFF])
    assert np.array_equal(r.lit[0, 0, :3], np.zeros(3))  # lit from behind: max(N.L, 0)


def test_range_cull_and_its_ambiguity():
    far = one_pixel([nl.default_light(position=(0, 0, 2.0), range=1.5, attenuation_mode=0)], [DIFF])
    assert np.array_equal(far.lit[0, 0, :3], np.zeros(3)) and far.lit[0, 0, 3] == 1.0 and not far.mask[0, 0]
    edge = one_pixel([nl.default_light(position=(0, 0, 2.0), range=2.0 * (1 + 2e-6), attenuation_mode=0)], [DIFF])
    assert edge.mask[0, 0] and np.allclose(edge.lit[0, 0, :3], BASE, rtol=1e-5) and np.array_equal(edge.alt[0, 0, :3], np.zeros(3))
    lin = one_pixel([nl.default_light(position=(0, 0, 2.0), range=2.0 * (1 + 2e-6), attenuation_mode=1)], [DIFF])
    assert not lin.mask[0, 0]  # linear attenuation reaches zero at the range: continuous


def test_spot_cones():
    def spot(offset_deg):
        # light 2 above the point, its axis tilted by offset_deg from the straight-down direction
        a = math.radians(offset_deg)
        return nl.default_light(type=nl.LIGHT_SPOT, position=(0, 0, 2.0), direction=(math.sin(a), 0.0, -math.cos(a)), inner_cone_deg=20.0,
                                outer_cone_deg=40.0, range=10.0, attenuation_mode=0)
    inside = one_pixel([spot(10.0)], [DIFF]).lit[0, 0, :3]
    assert np.allclose(inside, BASE, rtol=1e-6)
    outside = one_pixel([spot(50.0)], [DIFF]).lit[0, 0, :3]
    assert np.array_equal(outside, np.zeros(3))
    between = one_pixel([spot(30.0)], [DIFF]).lit[0, 0, :3]
    c = lambda d: math.cos(math.radians(d))
    t = (c(30.0) - c(40.0)) / (c(20.0) - c(40.0))  # smoothstep on the cosines, angles in degrees
    assert np.allclose(between, BASE * t * t * (3 - 2 * t), rtol=1e-5)


def test_specular_term_and_minimum_shininess():
    # light and camera both on the normal: V.R = 1, pow(1, s) = 1, specular = (2 + s) / (2 * 3.14159265)
    for s, s_eff in ((2.0, 4.0), (32.0, 32.0), (2000.0, 2000.0)):
        m = nl.default_material(specular=(1, 1, 1), emission=(0, 0, 0), shininess=s)
        r = one_pixel([nl.default_light(position=(0, 0, 2.0), attenuation_mode=0, intensity=0.5)], [m])
        assert np.allclose(r.lit[0, 0, :3], BASE * ((2.0 + s_eff) / (2.0 * 3.14159265)) * 0.5, rtol=1e-5), s


def test_headlight_default_material_invalid_id_and_pass_through():
    # empty table: a point light at the camera, intensity 1, no attenuation, infinite range
    r = one_pixel([], [DIFF])
    assert np.allclose(r.lit[0, 0, :3], BASE, rtol=1e-6)
    # the splat sets' default material is fully emissive and needs no shading: colour == base colour exactly, alpha 1
    r = one_pixel(lc.LIGHTS_MIXED, [nl.default_material()])
    assert np.array_equal(r.lit[0, 0], np.array([BASE[0], BASE[1], BASE[2], 1.0]))
    for dt in (np.float32, np.float64):
        assert np.array_equal(one_pixel([], [nl.default_material()], dtype=dt).lit[0, 0, :3], BASE)
    # invalid id: diffuse = base colour, ambient 0.1, no specular, whatever the instance's material says
    m = nl.default_material(diffuse=(0, 0, 0), specular=(1, 1, 1), emission=(5, 5, 5))
    r = one_pixel([], [m], pid=nl.INVALID_ID)
    assert np.allclose(r.lit[0, 0, :3], 0.1 + BASE, rtol=1e-6)
    # normal.w below the threshold: colour and alpha pass through
    r = one_pixel(lc.LIGHTS_MIXED, [DIFF], nw=0.0009)
    assert np.array_equal(r.lit[0, 0], np.array([BASE[0], BASE[1], BASE[2], np.float32(0.3)], np.float64)) and not r.shaded[0, 0]
    r = one_pixel(lc.LIGHTS_MIXED, [DIFF], nw=0.001 * (1 + 1e-6))
    assert r.mask[0, 0]


def test_ambient_is_counted_once_per_light():
    m = nl.default_material(ambient=(0.25, 0.25, 0.25), emission=(0, 0, 0))
    behind = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(0, 0, 1.0))  # contributes nothing but its ambient share
    for k in (1, 3):
        r = one_pixel([behind] * k, [m])
        assert np.allclose(r.lit[0, 0, :3], BASE * 0.25 * k, rtol=1e-6)


def test_material_of_the_owning_instance_and_need_shading():
    mats = [nl.default_material(diffuse=(1, 0, 0), emission=(0, 0, 0)), nl.default_material(diffuse=(0, 1, 0), emission=(0, 0, 0))]
    clip = P1.astype(np.float64) @ (V1.astype(np.float64) @ np.array([0, 0, 0, 1.0]))
    img = np.tile(np.array([BASE[0], BASE[1], BASE[2], 0.5], np.float32), (1, 2, 1))
    depth = np.full((1, 2), clip[2] / clip[3], np.float32)
    nrm = np.tile(np.array([0, 0, 1, 1], np.float32), (1, 2, 1))
    r = nl.light_frame(img, depth, np.array([[99, 100]], np.uint32), nrm, V1, P1, EYE, [], mats, [0, 100])
    assert r.lit[0, 0, 1] == 0 and r.lit[0, 0, 0] > 0 and r.lit[0, 1, 0] == 0 and r.lit[0, 1, 1] > 0
    assert not nl.need_shading(nl.default_material()) and nl.need_shading(nl.default_material(ambient=(0.001, 0.001, 0.001)))
    assert not nl.need_shading(nl.default_material(diffuse=(0.0005, 0.0005, 0.0005)))


def test_consolidated_depth():
    picked = np.array([[0.0, 0.00005, 0.5, 0.9, 0.7]], np.float32)
    d, mask = nl.consolidate_depth(picked)
    assert np.array_equal(d, np.array([[1.0, 1.0, 0.5, 0.9, 0.7]], np.float32)) and not mask.any()
    occ = np.array([[0.6, 0.6, 0.6, 0.6, 0.7]], np.float32)
    d, mask = nl.consolidate_depth(picked, occ)
    assert np.array_equal(d, np.array([[0.6, 0.6, 0.5, 0.6, 0.7]], np.float32))  # LESS: equal depths keep the geometry's
    assert mask[0, 4] and not mask[0, :4].any()


def test_target_rounding_helpers():
    x = np.array([[[0.5, 1.7, -0.2, 1.0]]], np.float64)
    assert np.array_equal(nl.to_target(x, "u8"), np.array([[[128, 255, 0, 255]]], np.uint8))
    assert nl.to_target(x, "f16").dtype == np.float16 and nl.from_target(nl.to_target(x, "u8"))[0, 0, 0] == np.float32(128) / np.float32(255)
    ok, _ = lc.pixel_ok(nl.to_target(x, "f16"), x, "f16", 0.0)
    assert ok.all()


# ---- 3. project files ------------------------------------------------------------------------------------------------------
def test_project_files_carry_lights_and_materials(tmp_path):
    from vk_gaussian_splatting_amd import project
    mat = {"ambient": [0.1, 0.2, 0.3], "diffuse": [0.4, 0.5, 0.6], "specular": [0.7, 0.8, 0.9], "emission": [0.0, 0.0, 0.0], "shininess": 12.0}
    splats = {"splatSets": [{"id": 0, "path": "a.ply"}],
              "splats": [{"splatSetId": 0, "name": "a", "position": [0, 0, 0], "rotation": [0, 0, 0], "scale": [1, 1, 1], "material": mat},
                         {"splatSetId": 0, "name": "b"}]}
    v5 = dict(splats, version=5, renderer={"lightingMode": 1},
              lights={"nextNamingNumber": 3,
                      "assets": [{"id": 7, "type": 2, "color": [1, 0.5, 0.25], "intensity": 3.0, "range": 7.0, "innerConeAngle": 10.0,
                                  "outerConeAngle": 25.0, "attenuationMode": 1, "proxyScale": 2.0}],
                      "instances": [{"assetId": 7, "name": "s", "translation": [1, 2, 3], "rotation": [0, 90.0, 0]},
                                    {"assetId": 7, "translation": [4, 5, 6], "rotation": [0, 0, 0]}]})
    f = tmp_path / "v5.vkgs"
    f.write_text(json.dumps(v5))
    pr = project.load_project(str(f))
    assert pr.lighting_mode == 1 and len(pr.lights) == 2
    L = pr.lights[0]
    assert L["type"] == 2 and L["color"] == [1, 0.5, 0.25] and L["intensity"] == 3.0 and L["range"] == 7.0
    assert (L["inner_cone_deg"], L["outer_cone_deg"], L["attenuation_mode"]) == (10.0, 25.0, 1) and L["position"] == [1, 2, 3]
    assert np.allclose(L["direction"], [-1.0, 0.0, 0.0], atol=1e-6)  # (0, 0, -1) turned 90 degrees about y
    assert pr.lights[1]["position"] == [4, 5, 6] and pr.lights[1]["direction"] == [0, 0, -1] and pr.lights[1]["range"] == 7.0
    assert pr.instances[0].material == mat and pr.instances[1].material is None
    # ... and they map onto the C structures
    from vk_gaussian_splatting_amd import capi
    cl, cm = capi.make_light(**L), capi.make_material(**mat)
    assert cl.type == 2 and cl.attenuation_mode == 1 and list(cl.position) == [1, 2, 3] and cl.outer_cone_deg == 25.0
    assert np.allclose(list(cm.specular), [0.7, 0.8, 0.9]) and cm.shininess == 12.0
    out = tmp_path / "v5b.vkgs"
    project.save_project(pr, str(out))
    pr2 = project.load_project(str(out))
    assert pr2.extra["lights"] == v5["lights"] and pr2.lights == pr.lights and pr2.instances[0].material == mat and pr2.lighting_mode == 1
    # version 3: "radius" is the range, "position" the translation, no rotation, cone angles and attenuation at their defaults
    v3 = dict(splats, version=3, renderer={"lightingMode": 2},
              lights={"assets": [{"id": 1, "type": 1, "color": [1, 1, 1], "intensity": 2.0, "radius": 4.0, "scale": 0.5}],
                      "instances": [{"assetId": 1, "position": [0, 1, 0]}]})
    f.write_text(json.dumps(v3))
    pr = project.load_project(str(f))
    L = pr.lights[0]
    assert pr.lighting_mode == 2 and L["type"] == 1 and L["position"] == [0, 1, 0] and L["range"] == 4.0 and L["intensity"] == 2.0
    assert (L["inner_cone_deg"], L["outer_cone_deg"], L["attenuation_mode"]) == (30.0, 45.0, 2) and L["direction"] == [0, 0, -1]
    # versions 0-2: a flat list, position and radius on the light itself; "lightingEnabled" instead of lightingMode
    v1 = dict(splats, version=1, renderer={"lightingEnabled": True},
              lights=[{"type": 1, "position": [4, 5, 6], "color": [0.2, 0.3, 0.4], "intensity": 1.5, "radius": 9.0}, {"type": 0, "position": [0, 0, 0]}])
    f.write_text(json.dumps(v1))
    pr = project.load_project(str(f))
    assert pr.lighting_mode == 2 and pr.lights[0]["position"] == [4, 5, 6] and pr.lights[0]["range"] == 9.0 and pr.lights[0]["intensity"] == 1.5
    assert pr.lights[1]["type"] == 0 and pr.lights[1]["color"] == [1, 1, 1] and pr.lights[1]["range"] == 10.0
    assert project.Project().lighting_mode == 0


# ---- 4. the cap and the tolerance, from the reference alone --------------------------------------------------------------------
def oracle_gbuffer(ob, gut, occluder):
    """(image float32[H,W,4] front-to-back colour frame, depth, ids, normal, occluder depth or None) of the oracle for the cases'
    scene and camera"""
    sets = lc.scene_sets()
    V, P, eye = lc.camera_matrices(lambda e, c, u, fov, zn, zf, w, h: (lookat(e, c, u), persp(fov, w / h, zn, zf)))
    fkw = dict(pipeline_3dgut=1) if gut else {}
    inst = ob.make_instances([(ob.PreparedSet(a), m) for a, m in sets])
    fr = ob.make_frame(V, P, eye, lc.W, lc.H, **fkw)
    oks, order = ob.sort_stable(*ob.key_cull(fr, inst))
    z = ol.depths_of_btf_keys(oks)
    surf = ob.render_surface_gut if gut else ob.render_surface
    color = ob.render_gut if gut else (lambda f, i, o: ob.render(f, i, order=o))
    ftb = ob.make_frame(V, P, eye, lc.W, lc.H, front_to_back=1, **fkw)
    occ_depth = None
    if occluder:
        level = ol.pick_level(z, 0.5)
        occ_depth, bg = lc.occluder_images(level)
        keep = order[z <= level]
        d0, i0, n0 = surf(fr, inst, order[::-1].copy(), lc.ISO, normals=True)
        d1, i1, n1 = surf(fr, inst, keep[::-1].copy(), lc.ISO, normals=True)
        c0, c1 = color(ftb, inst, order)[0], color(ftb, inst, keep)[0]
        m = occ_depth < 1.0
        depth, ids, nrm, img = np.where(m, d1, d0), np.where(m, i1, i0), np.where(m[..., None], n1, n0), np.where(m[..., None], c1, c0)
        img = img.copy()
        img[..., :3] += (1.0 - img[..., 3:4]) * bg[..., :3]  # final = splats + T * geometry colour
    else:
        depth, ids, nrm = surf(fr, inst, order[::-1].copy(), lc.ISO, normals=True)
        img = color(ftb, inst, order)[0]
    return img.astype(np.float32), depth, ids, nrm, occ_depth, (V, P, eye)


def test_cap_and_tolerance_from_the_reference_alone(ob):
    worst, memo = 0.0, {}
    for name, (gut, target, lights, mats, occluder) in lc.CASES.items():
        if (gut, occluder) not in memo:
            memo[(gut, occluder)] = oracle_gbuffer(ob, gut, occluder)
        img, depth, ids, nrm, occ_depth, (V, P, eye) = memo[(gut, occluder)]
        stored = nl.from_target(nl.to_target(img, target))  # the pass reads the frame as stored in the target format
        r64 = nl.light_frame(stored, depth, ids, nrm, V, P, eye, lights, mats, lc.inst_prefix(), occ_depth)
        r32 = nl.light_frame(stored, depth, ids, nrm, V, P, eye, lights, mats, lc.inst_prefix(), occ_depth, dtype=np.float32)
        lit = r64.shaded
        assert 0.3 < lit.mean() <= 0.98, (name, lit.mean())  # at least 2 % of the frame passes through
        assert (ids[lit] == nl.INVALID_ID).any() and (ids[lit] < lc.inst_prefix()[1]).any() and ((ids[lit] >= lc.inst_prefix()[1]) & (ids[lit] != nl.INVALID_ID)).any(), name
        share = (r64.mask | r32.mask)[lit].mean()
        keep = lit & ~(r64.mask | r32.mask)
        with np.errstate(invalid="ignore"):
            d = np.abs(r32.lit[..., :3].astype(np.float64) - r64.lit[..., :3]) / np.maximum(1.0, np.abs(r64.lit[..., :3]))
        d = np.where(np.isfinite(d), d, 0.0)[keep]
        print(f"lighting {name}: {lit.mean():.3f} of the pixels lit, ambiguity mask {share:.5f} of them, float32 vs float64 max {d.max():.3e}, "
              f"brightest {np.nanmax(r64.lit[..., :3][keep]):.2f}")
        assert share <= lc.MASK_CAP, (name, share)
        assert np.array_equal(r32.consolidated, r64.consolidated)
        worst = max(worst, float(d.max()))
    print(f"lighting: float32 vs float64 over all cases {worst:.3e}; recorded {lc.F32_VS_F64:.3e}; GPU bar {lc.GPU_BAR:.3e}")
    assert lc.F32_VS_F64 / 2 <= worst <= lc.F32_VS_F64, worst
