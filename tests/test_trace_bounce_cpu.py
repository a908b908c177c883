"""CPU tests of the indirect traced frame (mgs_render_traced_indirect): the header and the exports, every argument error without a
device, the loader's illum rule, and the float64 restatement's own checks (np_trace_bounce.py against np_trace_mesh.py, closed forms,
the fragile cap)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_trace_bounce as ntb
import trace_bounce_cases as tbc
import trace_mesh_cases as tmc
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGILE_CAP = 0.10


def test_header_structs_exports_and_defaults():
    h = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_TRACE_BOUNCES 1", h)
    assert C.sizeof(capi.BounceMaterial) == 32 and C.sizeof(capi.TraceBounceParams) == 16 and C.sizeof(capi.TraceBounceOut) == 272
    lib = capi.load_library()
    for name in ("mgs_bounce_material_default", "mgs_bounce_material_from_mtl", "mgs_mesh_bounce_materials", "mgs_mesh_instance_set_bounce_materials",
                 "mgs_trace_bounce_params_default", "mgs_render_traced_indirect"):
        assert hasattr(lib, name) and name in h and name in capi.EXPORTED_SYMBOLS
    b = capi.TraceBounceParams()
    lib.mgs_trace_bounce_params_default(C.byref(b))
    assert b.max_bounces == 3 and list(b.reserved) == [0, 0, 0]
    m = capi.bounce_material()
    assert list(m.transmittance) == [0.0, 0.0, 0.0] and m.ior == 1.0 and m.illum == 0 and list(m.reserved) == [0, 0, 0]


def _call(p, light=None, trace=None, bounce=None):
    return capi.load_library().mgs_render_traced_indirect(None, C.byref(p), C.byref(trace) if trace else None, C.byref(light) if light else None,
                                                          C.byref(bounce) if bounce else None, None, None, None)


def _params(**over):
    p = capi.default_params(48, 40)
    p.lighting_mode = 2
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _bounce(n, reserved=0):
    b = capi.TraceBounceParams()
    b.max_bounces, b.reserved[1] = n, reserved
    return b


def _last():
    return capi.load_library().mgs_last_error().decode()


def test_lighting_mode_outcomes_without_a_device():
    for mode in (0, 1, 3, -1):
        assert _call(_params(lighting_mode=mode)) == -1 and "null scene" not in _last()
    assert _call(_params()) == -1 and "null scene" in _last()      # indirect: the ranges pass, the null handle is MGS_ERR_INVALID_ARG
    # the other entry points keep answering MGS_LIGHTING_INDIRECT as they did
    assert capi.load_library().mgs_render_traced_lit(None, C.byref(_params()), None, None, None, None) == -8


@pytest.mark.parametrize("n,code", [(0, -1), (-1, -1), (17, -1), (1, None), (16, None)])
def test_max_bounces_range(n, code):
    rc = _call(_params(), bounce=_bounce(n))
    assert rc == -1
    assert ("null scene" in _last()) == (code is None)


def test_refusals_before_the_handle_is_looked_at():
    assert _call(_params(), bounce=_bounce(3, reserved=1)) == -1 and "null scene" not in _last()
    for strategy in (1, 2):
        assert _call(_params(), trace=capi.default_trace_params(trace_strategy=strategy)) == -8 and "null scene" not in _last()
    assert _call(_params(), trace=capi.default_trace_params(trace_strategy=3)) == -1 and "null scene" not in _last()
    assert _call(_params(), capi.default_trace_light_params(shadows_mode=2)) == -8 and "null scene" not in _last()
    assert _call(_params(), capi.default_trace_light_params(shadows_mode=3)) == -1 and "null scene" not in _last()
    assert _call(_params(), trace=capi.default_trace_params(samples_per_pass=33)) == -1 and "null scene" not in _last()
    assert _call(_params(width=0)) == -1 and "null scene" not in _last()
    assert _call(_params(sort_mode=capi.SORT_STOCHASTIC)) == -8 and "null scene" not in _last()


def test_bounce_material_values_are_checked_on_the_host():
    lib = capi.load_library()

    def rc(m):
        arr = (capi.BounceMaterial * 1)(m)
        return lib.mgs_mesh_instance_set_bounce_materials(None, 0, arr, 1)
    assert rc(capi.bounce_material()) == -1 and "null handle" in _last()
    for bad in (capi.bounce_material((float("nan"), 0, 0)), capi.bounce_material((0, float("inf"), 0)), capi.bounce_material(ior=float("nan")),
                capi.bounce_material((0.5, 0.5, 0.5), 0.0, 2), capi.bounce_material((0.5, 0.5, 0.5), -1.0, 3)):
        assert rc(bad) == -1 and "null handle" not in _last()
    m = capi.bounce_material()
    m.reserved[2] = 1
    assert rc(m) == -1 and "null handle" not in _last()
    assert rc(capi.bounce_material(ior=0.0, illum=1)) == -1 and "null handle" in _last()   # ior is read by illum >= 2 alone


@pytest.mark.parametrize("tf,mtl_illum,want", [
    ((0, 0, 0), 0, 0), ((0, 0, 0), 1, 0), ((0, 0, 0), 2, 1), ((0, 0, 0), 3, 1), ((0, 0, 0), 7, 1),
    ((0.5, 0, 0), 0, 2), ((0, 0.5, 0), 2, 2), ((0.2, 0.3, 0.4), 5, 2),
    ((0, 0, 1), 0, 0), ((0, 0, 1), 2, 1)])     # the typo of obj_loader.cpp:54: .x twice, .z never
def test_from_mtl_is_the_loaders_rule(tf, mtl_illum, want):
    m = capi.bounce_material_from_mtl(tf, 1.45, mtl_illum)
    assert m.illum == want and list(m.transmittance) == [np.float32(v) for v in tf] and m.ior == np.float32(1.45)


# ---- the restatement ----
def test_next_ray_closed_forms():
    d = np.array([0.6, -0.8, 0.0])
    n = np.array([0.0, 1.0, 0.0])
    mm = dict(specular=(0.5, 0.25, 1.0))
    T, nd, _ = ntb.next_ray(d, n, mm, tbc.REFLECT, np.ones(3), 0)
    assert np.allclose(nd, (0.6, 0.8, 0.0)) and np.allclose(T, (0.5, 0.25, 1.0))
    # ior 1: the ray goes straight on, T *= Tf
    T, nd, _ = ntb.next_ray(d, n, mm, dict(transmittance=(0.9, 0.8, 0.7), ior=1.0, illum=2), np.ones(3), 0)
    assert np.allclose(nd, d) and np.allclose(T, np.float32([0.9, 0.8, 0.7]))
    # Snell entering glass
    T, nd, _ = ntb.next_ray(d, n, mm, tbc.REFRACT, np.ones(3), 0)
    assert np.isclose(nd[0], 0.6 / 1.5) and nd[1] < 0 and np.isclose(np.linalg.norm(nd), 1.0)
    # inside glass beyond the critical angle (sin = 0.8 > 1 / 1.5): reflected off the flipped normal
    T, nd, fr = ntb.next_ray(np.array([0.8, 0.6, 0.0]), n, mm, tbc.REFRACT, np.ones(3), 1)
    assert np.allclose(nd, (0.8, -0.6, 0.0)) and not fr
    # illum 0 ends the path
    T, nd, _ = ntb.next_ray(d, n, mm, tbc.NONE, np.ones(3), 0)
    assert nd is None and (T == 0).all()


def test_all_illum_zero_is_the_lit_mesh_frame_exactly():
    c = tbc.cases()["b5"]
    inst = [(ntb.ntl.prepare_set(a), M) for a, M in c["sets"]]
    r = tbc.restate_with(c, inst, bounce=[None])
    f = r["first"]
    assert r["rays"].sum() == 0 and np.array_equal(r["image"], f["image"]) and np.array_equal(r["hits"], f["hits"])
    assert np.array_equal(r["shadow_hits"], f["shadow_hits"]) and np.array_equal(r["fragile"], f["fragile"])


def test_bare_mirror_facing_an_emissive_mesh():
    """(b) a mirror pixel whose bounce ray meets an emission-only triangle: the bounce adds specular * emission"""
    c = tbc.cases()["b2_1"]
    r = tbc.restate(c and "b2_1")
    f = r["first"]
    live = r["live"][0]
    assert live.any()
    # one bounce adds to a live pixel what its bounce ray meets and nothing to any other pixel; emission is added unweighted (:1159),
    # so a pixel whose gain equals the glow material's emission met the emission-only triangle, whatever the mirror's specular is
    delta = r["image"][..., :3] - f["image"][..., :3]
    assert (delta[~live] == 0).all() and (delta[live] >= -1e-12).all() and (delta[live] != 0).any()
    glow = np.float32(tmc.MAT_GLOW["emission"]).astype(np.float64)
    met = np.isclose(delta, glow).all(-1) & live
    print("pixels whose bounce met the emission-only triangle:", int(met.sum()), "of", int(live.sum()), "live")
    assert c["max_bounces"] == 1 and met.sum() >= 20
    assert np.allclose(delta[met], glow, rtol=0, atol=1e-12)     # the emission itself: a weighting by specular (0.5 .. 0.9) would miss it


def test_rounds_differ_and_end_by_the_count():
    r1, r3, r16 = (tbc.restate(f"b2_{n}") for n in (1, 3, 16))
    assert np.array_equal(r1["rays"][:1], r3["rays"][:1]) and np.array_equal(r3["rays"][:3], r16["rays"][:3])
    assert not np.array_equal(r1["image"], r3["image"]) and not np.array_equal(r3["image"], r16["image"])
    assert r16["rays"][15] > 0          # the facing mirrors keep a path alive to the last round: the count ends it


def test_no_light_in_range_means_no_bounce_and_the_headlight_bounces():
    assert tbc.restate("b4_far")["rays"].sum() == 0
    assert tbc.restate("b4_head")["rays"][0] > 0


def test_glass_case_refracts_through_the_slab_and_reflects_inside_the_prism():
    """(d) in a frame: paths that enter the prism head-on meet its hypotenuse beyond the critical angle and take the reflection
    fallback; paths through the slab enter and leave it (two mesh hits in a row) and go on"""
    r = tbc.restate("b3")
    tir = r["tir"] & ~r["fragile"]
    print("b3: pixels with a total internal reflection on their path:", int(tir.sum()), "rays", r["rays"].tolist())
    assert tir.sum() >= 10
    assert (r["live"][2] & tir).sum() >= 10          # such a path is alive after the reflection: it left the hypotenuse inside the glass
    assert r["rays"][1] > 0 and r["mesh_hits"][0] > 0 and r["mesh_hits"][1] > 0


def test_parallel_slab_with_ior_one_scales_what_lies_behind_it_by_tf_squared():
    """(c) with the headlight (with no light in range the path would end at the slab, :1186-1187).  A slab of ior 1 leaves the ray as
    it is, so the floor point behind it is the frame's without the slab, seen along the same direction, and its shading is linear in
    T = Tf * Tf.  The slab's material lies just above the needShading threshold (|diffuse| = 0.0011 > 0.001, red alone, no ambient,
    no specular): under the headlight (intensity 1, no attenuation) each interface adds at most 0.0011 * T to red and nothing else."""
    import trace_lit_cases as tlc
    faint = dict(ambient=(0.0, 0.0, 0.0), diffuse=(0.0011, 0.0, 0.0), specular=(0.0, 0.0, 0.0), emission=(0.0, 0.0, 0.0), shininess=0.0)
    clear = dict(transmittance=(0.9, 0.8, 0.7), ior=1.0, illum=2)
    floor = tmc.placed(tmc.FLOOR, materials=[tmc.MAT_SHADED, tmc.MAT_SHADED])
    slab = tmc.placed(tmc.box((-0.7, 0.1, -0.7), (0.7, 0.2, 0.7)), materials=[faint, faint])

    def run(meshes, bounce):
        c = dict(tlc._case([], [], W=24, H=20), meshes=meshes, bounce=bounce, max_bounces=3, mesh_min_T=0.0)
        return tbc.restate_with(c, [])
    a, b = run([floor, slab], [None, [clear, clear]]), run([floor], [None])
    through = a["live"][1] & ~a["fragile"] & ~b["fragile"] & b["mesh"]["hit"]     # two interfaces crossed, a floor point behind them
    assert through.sum() >= 40 and a["rays"][2] == 0
    tf = np.float32(clear["transmittance"]).astype(np.float64)
    diff = a["image"][through, :3] - tf * tf * b["image"][through, :3]
    assert (b["image"][through, :3] > 0.05).all()                                # the floor is lit: the product is not held on zeros
    # the floor point is reached over three segments in place of one; np_mesh_rays carries the hit records' fp32 rounding (u = 2^-24,
    # coordinates below 4), so the point moves by at most 3 * 8 u * 4 = 6e-6, and the shading (values below 1, a light 2 away) by less
    # than that per unit of length: slack 1e-5
    slack = 1e-5
    assert (diff[:, 0] >= -slack).all() and (diff[:, 0] <= 0.0011 * (1.0 + tf[0]) + slack).all()
    assert np.abs(diff[:, 1:]).max() <= slack
    print("slab: pixels", int(through.sum()), "red excess max", float(diff[:, 0].max()), "green / blue worst", float(np.abs(diff[:, 1:]).max()))


def test_loader_reads_tf_ni_illum_and_leaves_the_view_alone(tmp_path):
    obj, mtl = tmp_path / "m.obj", tmp_path / "m.mtl"
    mtl.write_text("newmtl mirror\nKd 0.1 0.1 0.1\nKs 0.8 0.8 0.8\nillum 3\n"
                   "newmtl glass\nKd 0.2 0.2 0.2\nTf 0.9 0.8 0.7\nNi 1.5\nillum 7\n"
                   "newmtl typo\nKd 0.3 0.3 0.3\nKt 0 0 1\nNi 1.3\nillum 1\n"
                   "newmtl plain\nKd 0.4 0.4 0.4\n")
    obj.write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nusemtl mirror\nf 1 2 3\nusemtl glass\nf 2 4 3\nusemtl typo\nf 1 2 4\nusemtl plain\nf 1 4 3\n")
    m = capi.Mesh.load_obj(str(obj))
    b = m.bounce_materials()
    assert [x.illum for x in b] == [1, 2, 0, 0]
    assert list(b[1].transmittance) == [np.float32(0.9), np.float32(0.8), np.float32(0.7)] and b[1].ior == np.float32(1.5)
    assert list(b[2].transmittance) == [0.0, 0.0, 1.0] and b[2].ior == np.float32(1.3)       # read, and left non-refractive by the typo
    assert b[0].ior == 1.0 and b[3].ior == 1.0 and list(b[3].transmittance) == [0.0, 0.0, 0.0]
    v = m.view()
    assert len(v["materials"]) == 4 and v["materials"][1]["diffuse"] == (np.float32(0.2),) * 3 and list(v["material_ids"]) == [0, 1, 2, 3]
    # the same file without the three statements gives the same view: they reach nothing MgsMeshView returns
    mtl.write_text("newmtl mirror\nKd 0.1 0.1 0.1\nKs 0.8 0.8 0.8\nnewmtl glass\nKd 0.2 0.2 0.2\nnewmtl typo\nKd 0.3 0.3 0.3\nnewmtl plain\nKd 0.4 0.4 0.4\n")
    w = capi.Mesh.load_obj(str(obj)).view()
    assert all(np.array_equal(v[k], w[k]) for k in ("positions", "normals", "indices", "material_ids")) and v["materials"] == w["materials"]


def test_meshes_from_arrays_and_the_ingest_fixture():
    import mesh_cases as mc
    m = capi.Mesh.from_arrays(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), [[0, 1, 2]], None, [0], [capi.make_material(), capi.make_material()])
    b = m.bounce_materials()
    assert len(b) == 2 and all(x.illum == 0 and x.ior == 1.0 and list(x.transmittance) == [0.0, 0.0, 0.0] for x in b)
    f = capi.Mesh.load_obj(mc.FIXTURE)
    v = f.view()
    assert len(f.bounce_materials()) == len(v["materials"])
    # the fixture's view is what the mesh tests' golden numbers pin (tests/test_mesh_cpu.py passes untouched); here: the counts
    assert v["indices"].shape == (38, 3) and len(v["materials"]) == 2


@pytest.mark.parametrize("name", list(tbc.cases()))
def test_fragile_share_is_capped(name):
    r = tbc.restate(name)
    share = (r["fragile"] & r["ok"]).sum() / max(r["ok"].sum(), 1)
    print(f"{name}: fragile {share:.4f}, rays {r['rays'].tolist()}")
    assert share <= FRAGILE_CAP
