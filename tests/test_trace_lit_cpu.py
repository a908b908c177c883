"""CPU tests of lit traced frames (mgs_render_traced_lit): the header and the exports, every argument error without a device, and the
float64 restatement's own checks (np_trace_lit.py against np_trace.py / np_lighting.py, the closed-form ramp, the fragile cap)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_lighting as nl
import np_trace_lit as ntl
import trace_lit_cases as lc
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_structs_and_exports():
    h = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_TRACE_LIGHTING 1", h)
    assert C.sizeof(capi.TraceLightParams) == 32 and C.sizeof(capi.TraceLightOut) == 40
    lib = capi.load_library()
    for name in ("mgs_trace_light_params_default", "mgs_render_traced_lit", "mgs_trace_download_shadow_hits"):
        assert hasattr(lib, name) and name in h
    d = capi.default_trace_light_params()
    assert (d.shadows_mode, d.particle_shadow_offset, d.particle_shadow_transmittance_threshold, d.particle_shadow_color_strength) == \
        (0, np.float32(0.2), np.float32(0.8), 0.0)


def _call(p, light=None, trace=None):
    return capi.load_library().mgs_render_traced_lit(None, C.byref(p), C.byref(trace) if trace else None, C.byref(light) if light else None, None, None)


def _params(**over):
    p = capi.default_params(48, 40)
    p.lighting_mode = 1
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_lighting_mode_outcomes_without_a_device():
    assert _call(_params(lighting_mode=2)) == -8                      # indirect: MGS_ERR_UNSUPPORTED
    assert _call(_params(lighting_mode=0)) == -1 and _call(_params(lighting_mode=7)) == -1
    assert _call(_params()) == -1                                      # direct: the ranges pass, the null handle is MGS_ERR_INVALID_ARG
    assert "null scene" in capi.load_library().mgs_last_error().decode()
    # mgs_render_traced keeps refusing lit frames
    assert capi.load_library().mgs_render_traced(None, C.byref(_params()), None, None) == -8


@pytest.mark.parametrize("field,value,code", [
    ("shadows_mode", 2, -8), ("shadows_mode", 3, -1), ("shadows_mode", -1, -1),
    ("particle_shadow_offset", -0.1, -1), ("particle_shadow_offset", float("inf"), -1), ("particle_shadow_offset", float("nan"), -1),
    ("particle_shadow_transmittance_threshold", 1.0, -1), ("particle_shadow_transmittance_threshold", -0.1, -1),
    ("particle_shadow_color_strength", 1.5, -1), ("particle_shadow_color_strength", -0.5, -1)])
def test_light_param_ranges(field, value, code):
    assert _call(_params(), capi.default_trace_light_params(**{field: value})) == code
    assert "null scene" not in capi.load_library().mgs_last_error().decode()


def test_trace_param_ranges_still_checked():
    assert _call(_params(), trace=capi.default_trace_params(samples_per_pass=33)) == -1
    assert _call(_params(width=0)) == -1


def test_single_occluder_gives_the_closed_form_ramp():
    a = lc.blob(n=1, radius=0.0, opacity=0.0)
    a["scale"][:] = np.log(0.3)
    a["rotation"][:] = (1, 0, 0, 0)
    a["positions"][:] = (0, 0, 0)
    per = ntl._per_inst([(ntl.prepare_set(a), np.eye(4))], 0.0113, 1.0 / 255.0, True)
    res, hits, _ = ntl.shadow_ray(per, np.array([0.0, -2.0, 0.0]), np.array([0.0, 1.0, 0.0]), 5.0, 18, 0.25, 0.0)
    alpha = 0.5  # sigmoid(0) x response 1 on the axis
    assert hits == 1 and np.allclose(res, ((1 - alpha) - 0.25) / 0.75, atol=1e-12)
    res, _, _ = ntl.shadow_ray(per, np.array([0.0, -2.0, 0.0]), np.array([0.0, 1.0, 0.0]), 5.0, 18, 0.8, 0.0)
    assert np.all(res == 0.0)                                          # below the threshold: black
    res, hits, _ = ntl.shadow_ray(per, np.array([0.0, -2.0, 0.0]), np.array([0.0, 1.0, 0.0]), 1.5, 18, 0.25, 0.0)
    assert hits == 0 and np.all(res == 1.0)                            # the occluder is behind the light


def test_default_materials_and_no_shadows_reproduce_the_traced_frame():
    c = lc.cases()["l13_shadows_off"]
    inst = [(ntl.prepare_set(a), M) for a, M in c["sets"]]
    r = ntl.lit(inst, c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], [nl.default_material()], shadows=0)
    s = r["surface"]
    assert np.array_equal(r["image"][s], r["base"]["image"][s]) and s.any() and (~s).any()
    assert not r["image"][~s].any()


def test_all_lights_in_range_equals_the_deferred_pass():
    """With all lights in range and shadows off the restatement equals np_lighting.light_frame fed with the traced outputs, to 1e-9.
    light_frame reads its inputs the way the deferred raster pass does (fp32 radiance and normal, the position rebuilt from the
    fp32 ndc depth); lit(deferred_inputs=True) shades from the same four inputs, so that the comparison is of the shading — the
    material, emission, the loop over the lights and the range rule — and not of one fp32 ulp of ndc z (1.8e-6 in the image when
    the restatement keeps its float64 position origin + t * direction)."""
    c = lc.cases()["l13_shadows_off"]
    inst = [(ntl.prepare_set(a), M) for a, M in c["sets"]]
    r = ntl.lit(inst, c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"], shadows=0, deferred_inputs=True)
    b = r["base"]
    ref = nl.light_frame(b["image"], b["depth"], b["id"].astype(np.uint32), b["normal"], c["V"], c["P"], c["eye"], c["lights"], c["materials"], [0])
    assert (r["rays"] == 0).all() and all(np.linalg.norm(np.asarray(L["position"]) - 0) < L["range"] - 5 for L in c["lights"])  # in range everywhere
    s = r["surface"] & ref.shaded  # (light_frame also shades pixels with weight but no iso hit; the traced pass discards those)
    assert s.sum() > 1000 and not (r["surface"] & ~ref.shaded).any()
    err = np.abs(ref.lit[..., :3] - r["image"][..., :3])[s]
    print("max |restatement - light_frame| =", err.max(), "over", int(s.sum()), "pixels")
    assert err.max() <= 1e-9


def test_own_position_path_against_the_deferred_pass():
    """The restatement as the lit frame uses it (position = origin + t * direction, view direction = the ray's) against light_frame,
    which rebuilds the position from the fp32 ndc depth through fp32-rounded inverse matrices.  The bound: the depth's own fp32
    tolerance as np_trace reports it (depth_tol, in ndc z) moves the rebuilt position along the ray by depth_tol * dt/dz; with the
    lights' intensity and attenuation the shading's slope in the position is below 8 per unit length in this scene (intensity 4,
    distance >= 1.4: |d/dx (4 / (1 + x^2))| <= 8 x / (1 + x^2)^2 < 1.4, times radiance <= 1.5 and the normalisations), so
    8 * the largest position shift.  Measured 1.8e-6."""
    name = "l13_shadows_off"
    c, r = lc.cases()[name], lc.restate(name)
    b = r["base"]
    ref = nl.light_frame(b["image"], b["depth"], b["id"].astype(np.uint32), b["normal"], c["V"], c["P"], c["eye"], c["lights"], c["materials"], [0])
    s = r["surface"] & ref.shaded & ~r["fragile"]
    Vm, Pm = np.asarray(c["V"], np.float64), np.asarray(c["P"], np.float64)
    cam = np.asarray(c["eye"], np.float64)
    ys, xs = np.nonzero(s)
    clip = np.stack([(xs + 0.5) / c["W"] * 2 - 1, (ys + 0.5) / c["H"] * 2 - 1, b["depth"][s], np.ones(ys.size)], -1)
    def world(z):
        v = np.linalg.inv(Pm) @ np.concatenate([clip[:, :2], z[:, None], clip[:, 3:]], 1).T
        return (np.linalg.inv(Vm) @ (v / v[3]))[:3].T
    eps32 = 2.0 ** -23
    shift = np.linalg.norm(world(b["depth"][s] * (1 + eps32) + b["depth_tol"][s]) - world(b["depth"][s]), axis=1) + 8 * eps32 * np.abs(cam).sum()
    err = np.abs(ref.lit[..., :3] - r["image"][..., :3])[s].max(-1)
    print("max |restatement - light_frame| =", err.max(), "bound", (8 * shift).min(), "..", (8 * shift).max())
    assert (err <= 8 * shift).all()


def test_translucent_case_reaches_the_ramp_and_the_tint():
    r0, r5, r1 = (lc.restate("l07_translucent_" + t) for t in ("s0", "s05", "s1"))
    ok = ~r0["fragile"] & ~r5["fragile"] & ~r1["fragile"]
    T = r0["shadow_T"][..., 0, 0]
    inside = ok & (T > 0.0) & (T < 1.0)
    print("pixels with T inside (0, 1):", int(inside.sum()))
    assert inside.sum() >= 100                                        # the occluders leave T inside (threshold, 1): the ramp's open interval
    for a, b in ((r0, r5), (r5, r1)):                                 # the tint changes non-fragile pixels: the SH branch is live
        d = np.abs(a["image"][..., :3] - b["image"][..., :3]).max(-1)
        assert (d[inside] > 1e-4).sum() >= 50
    assert np.ptp(r1["shadow_T"][inside][:, 0], axis=-1).max() > 1e-3  # ... and is per channel


def test_k_cut_changes_non_fragile_pixels():
    a, b = lc.restate("l08_kcut_4"), lc.restate("l08_kcut_18")
    ok = ~a["fragile"] & ~b["fragile"]
    assert (a["shadow_hits"] != b["shadow_hits"])[ok].sum() >= 100 and a["shadow_hits"].max() == 4 and b["shadow_hits"].max() > 4
    assert (np.abs(a["image"] - b["image"])[ok].max(-1) > 1e-3).sum() >= 100
    assert lc.restate("l08_kcut_1")["shadow_hits"].max() == 1 and lc.restate("l08_kcut_32")["shadow_hits"].max() > 18


def test_offset_changes_non_fragile_pixels():
    a, b = lc.restate("l09_offset_0"), lc.restate("l09_offset_02")
    ok = ~a["fragile"] & ~b["fragile"]
    assert (np.abs(a["image"] - b["image"])[ok].max(-1) > 1e-3).sum() >= 100
    assert (a["shadow_hits"][ok] > 0).sum() >= 100 and (b["shadow_hits"][ok] > 0).sum() <= 10


def test_cases_reach_what_they_are_for():
    r = lc.restate("l17_fallback_normal")
    assert r["fallback"].sum() >= 50                                      # the -rayDirection normal of surfaceFinalFiltering
    n4 = r["base"]["normal"][r["surface"]]
    assert (np.abs(np.linalg.norm(n4[:, :3], axis=1) - 0.2) > 10 * (1e-4 * n4[:, 3] + 64 * ntl.U)).all()  # ten margins = a hundred times the estimated error
    r = lc.restate("l12_thin_cloud")
    assert (~r["surface"] & (r["base"]["hits"] > 0)).sum() >= 300 and not r["image"][~r["surface"]].any()  # discarded to (0,0,0,0)
    r = lc.restate("l04_range")
    assert 0 < r["rays"].sum() < r["surface"].sum()                       # the range ends across the floor
    r = lc.restate("l03_spot")
    lit_px = r["image"][..., :3].sum(-1)[r["surface"]]
    dark = np.percentile(lit_px, 10)                                      # outside the cone: the ambient term alone
    assert (lit_px < 1.2 * dark).sum() > 100 and (lit_px > 2.0 * dark).sum() > 100  # the cone's edge crosses the floor
    assert lc.restate("l05_three")["rays"].max() == 3 and len(lc.cases()["l15_deep"]["sets"][0][0]["positions"]) == 4097
    assert lc.restate("l14_fisheye_dof")["base"]["image"][0, 0, 3] == 1.0  # a corner outside the fisheye circle


@pytest.mark.parametrize("name", sorted(lc.cases()))
def test_fragile_pixels_within_cap(name):
    r = lc.restate(name)
    print(name, "fragile", r["fragile"].mean(), "shadowed pixels", int((r["shadow_hits"] > 0).sum()), "fallback normals", int(r["fallback"].sum()))
    assert r["fragile"].mean() <= 0.05
