"""CPU tests of hybrid frames (mgs_render_hybrid): the header, the export and the binding, every refusal without a device, and the
float64 restatement np_hybrid.py on the CPU oracle's raster G-buffer for every case of hybrid_cases.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import hybrid_cases as hc
import np_lighting as nl
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_export_and_binding():
    h = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_HYBRID 1", h) and re.search(r"int mgs_render_hybrid\(MgsScene", h)
    lib = capi.load_library()
    assert hasattr(lib, "mgs_render_hybrid") and "mgs_render_hybrid" in capi.EXPORTED_SYMBOLS
    P = C.POINTER
    assert lib.mgs_render_hybrid.restype is C.c_int
    assert list(lib.mgs_render_hybrid.argtypes) == [C.c_void_p, P(capi.FrameParams), P(capi.TraceParams), P(capi.TraceLightParams),
                                                    P(capi.FrameOut), P(capi.TraceLightOut)]
    assert callable(capi.Scene.render_hybrid)
    # the out-of-scope lists no longer name the hybrid pipeline; meshes in the traced scene, soft shadows and bounces stay on them
    scope = h[h.index("---- ray-traced splats (MGS_HAS_TRACE)"):h.index("typedef struct MgsTraceParams")]
    assert "the hybrid pipeline" not in scope and "meshes in the traced scene, soft shadows, indirect lighting and bounces" in scope


def _call(p, light=None, trace=None):
    return capi.load_library().mgs_render_hybrid(None, C.byref(p), C.byref(trace) if trace else None, C.byref(light) if light else None, None, None)


def _params(**over):
    p = capi.default_params(48, 40)
    p.lighting_mode = 1
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _err():
    return capi.load_library().mgs_last_error().decode()


def test_lighting_mode_outcomes_without_a_device():
    assert _call(_params(lighting_mode=2)) == -8 and "null scene" not in _err()   # indirect: MGS_ERR_UNSUPPORTED
    for mode in (0, 7, -1):
        assert _call(_params(lighting_mode=mode)) == -1 and "null scene" not in _err() and "mgs_render" in _err()
    for pipeline in (0, 1):
        assert _call(_params(pipeline=pipeline)) == -1 and "null scene" in _err()  # the ranges pass: the null handle is MGS_ERR_INVALID_ARG
    assert capi.load_library().mgs_render_hybrid(None, None, None, None, None, None) == -1


@pytest.mark.parametrize("over,code", [
    (dict(sort_mode=capi.SORT_STOCHASTIC if hasattr(capi, "SORT_STOCHASTIC") else 2), -8),
    (dict(pipeline=0, dof_mode=1), -8),        # the 3DGS hybrid has no lens: mgs_render's own code
    (dict(pipeline=0, camera_model=1), -1),    # ... and no fisheye rays
    (dict(pipeline=2), -1), (dict(width=0), -1), (dict(target_format=9), -1), (dict(kernel_min_response=0.0, pipeline=1), -1),
    (dict(pipeline=1, dof_mode=1, aperture=-1.0), -1)])
def test_frame_param_refusals(over, code):
    assert _call(_params(**over)) == code
    assert "null scene" not in _err()


@pytest.mark.parametrize("field,value,code", [
    ("shadows_mode", 2, -8), ("shadows_mode", 3, -1), ("shadows_mode", -1, -1),
    ("particle_shadow_offset", -0.1, -1), ("particle_shadow_offset", float("nan"), -1),
    ("particle_shadow_transmittance_threshold", 1.0, -1), ("particle_shadow_color_strength", 1.5, -1)])
def test_light_param_ranges(field, value, code):
    assert _call(_params(), capi.default_trace_light_params(**{field: value})) == code
    assert "null scene" not in _err()


def test_trace_param_ranges():
    assert _call(_params(), trace=capi.default_trace_params(samples_per_pass=33)) == -1 and "null scene" not in _err()
    assert _call(_params(), trace=capi.default_trace_params(kernel_adaptive_clamping=2)) == -1 and "null scene" not in _err()
    # max_passes and depth_iso_threshold are not read by a hybrid frame (there is no primary walk): whatever they hold passes
    assert _call(_params(), trace=capi.default_trace_params(max_passes=0, depth_iso_threshold=7.0)) == -1 and "null scene" in _err()


# ---- the restatement on the CPU oracle's G-buffer ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated(name):
    """(G-buffer, restatement) of a case; computed once and shared: do not modify"""
    from oracle import binding as ob
    ob.build()
    c = hc.cases()[name]
    g = hc.oracle_gbuffer(ob, c)
    return g, hc.restate_with(c, g, hc.prepared(c))


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_case_on_the_oracle_gbuffer(name):
    g, r = _restated(name)
    st = r["state"]
    share = r["fragile"].mean()
    print(f"{name}: lit {int((st == 3).sum())}, discarded {int((st == 1).sum())}, outside {int((st == 0).sum())}, fragile {share:.4f}, "
          f"worst |float64 - fp32 position| {r['d_pos'].max():.2e}")
    assert share <= hc.FRAGILE_CAP
    assert np.isfinite(r["image"]).all()
    assert not r["image"][st == 1].any()                                           # discarded: (0,0,0,0)
    keep = (st == 0) | (st == 2)
    assert np.array_equal(r["image"][keep], g[0][keep].astype(np.float64))          # left alone
    assert np.array_equal(r["image"][st == 3][:, 3], g[0][st == 3][:, 3].astype(np.float64))  # alpha is the stored pixel's
    if name == "h11_thin_cloud":
        assert (st == 1).all() and g[0][..., 3].max() > 0.02                        # the cloud is drawn, but nothing of it is a surface
    else:
        assert (st == 3).sum() >= 400 and (st == 1).any()
    if name == "h03_fisheye":
        assert (st == 0).sum() >= 400


def test_each_case_does_what_it_is_for():
    lit, off = _restated("h01_3dgs")[1], _restated("h09_shadows_off")[1]
    dark = lit["surface"] & (lit["shadow_hits"] > 0) & ~lit["fragile"]
    assert dark.sum() >= 50 and (off["rays"] == 0).all() and (lit["rays"][lit["surface"]] == 1).all()
    assert (lit["image"][dark][:, :3].sum(1) < off["image"][dark][:, :3].sum(1)).mean() >= 0.95  # shadowed floor pixels are darker
    free = lit["surface"] & (lit["shadow_hits"] == 0)
    assert np.array_equal(lit["image"][free], off["image"][free])
    s0, s1 = _restated("h07_translucent_s0")[1], _restated("h07_translucent_s1")[1]
    tinted = np.abs(s0["image"] - s1["image"]).max(-1) > 1e-4
    assert tinted.sum() >= 20 and np.array_equal(s0["shadow_hits"], s1["shadow_hits"])
    a, b = _restated("h05_three_lights")[1], _restated("h05_without_far")[1]
    assert np.array_equal(a["image"], b["image"]) and np.array_equal(a["rays"], b["rays"])  # out of range: no ambient, no ray
    assert (a["rays"][a["surface"]] == 2).all()
    k4, k32 = _restated("h08_spp_4")[1], _restated("h08_spp_32")[1]
    assert k32["shadow_hits"].sum() > k4["shadow_hits"].sum() and k4["shadow_hits"].max() <= 4
    h6 = _restated("h06_headlight")[1]
    assert (h6["rays"] == 0).all() and h6["surface"].any()
    m = _restated("h10_materials")
    ids, r = m[0][2], m[1]
    blob_px = r["surface"] & (ids >= hc.inst_prefix(hc.cases()["h10_materials"])[1])
    assert blob_px.sum() >= 30 and (r["rays"][blob_px] == 0).all()                   # the default material: emission only, no ray
    assert np.array_equal(r["image"][blob_px], m[0][0][blob_px].astype(np.float64))


def test_invalid_id_passes_through_and_thresholds():
    """a surface without a picked id keeps its stored pixel; depth and normal weight decide at 0.0001 and 0.001"""
    c = hc.cases()["h01_3dgs"]
    g, r0 = _restated("h01_3dgs")
    img, depth, ids, nrm = (a.copy() for a in g)
    ys, xs = np.nonzero(r0["surface"])
    p = [(ys[k], xs[k]) for k in (0, 1, 2, 3)]
    ids[p[0]] = 0xFFFFFFFF
    depth[p[1]] = np.float32(0.0001)          # not > 0.0001
    nrm[p[2]][3] = np.float32(0.001)          # not > 0.001
    nrm[p[3]][:3] = 0.0                       # normalize(0) = NaN: its length is not < 0.001, the reference shades NaN
    r = hc.restate_with(c, (img, depth, ids, nrm), hc.prepared(c), rows=(int(ys[0]), int(ys[3]) + 1))
    assert r["state"][p[0]] == 2 and np.array_equal(r["image"][p[0]], img[p[0]].astype(np.float64))
    assert r["state"][p[1]] == 1 and r["state"][p[2]] == 1 and not r["image"][p[1]].any() and not r["image"][p[2]].any()
    assert r["fragile"][p[1]] and r["fragile"][p[2]]
    assert r["state"][p[3]] == 3 and np.isnan(r["image"][p[3]][:3]).all()


def test_shadows_off_equals_the_deferred_pass():
    """With shadows off and every light in range the hybrid restatement equals np_lighting.light_frame on the same G-buffer, on lit
    pixels with a picked id.  The two differ in the position (origin + |unprojected - origin| * ray direction against the
    unprojected position itself: the ray goes through the pixel centre by the float64 inverse of proj, the unprojection by the
    fp32-rounded one) and in the view direction (the ray's against normalize(position - camera_pos), the fp32 eye): a few 2^-24
    relative in a position of magnitude ~3, i.e. below 1e-6 in an image of values up to 1.  Measured: 3.5e-08."""
    c = hc.cases()["h09_shadows_off"]
    g, r = _restated("h09_shadows_off")
    ref = nl.light_frame(g[0], g[1], g[2], g[3], c["V"], c["P"], c["eye"], c["lights"], c["materials"], hc.inst_prefix(c))
    assert all(np.linalg.norm(np.asarray(L["position"])) < L["range"] - 5 for L in c["lights"])  # in range everywhere
    s = r["surface"] & ref.shaded & (g[2] != 0xFFFFFFFF)
    assert s.sum() > 1000
    err = np.abs(ref.lit[..., :3] - r["image"][..., :3])[s].max()
    print(f"max |hybrid restatement - light_frame| = {err:.3e} over {int(s.sum())} pixels")
    assert err <= 1e-6
