"""Shadow and light queries without a GPU: the header and the binding agree, every refusal fires before the handle is looked at, the
restatement (np_shadow_query.py) reproduces the lit frames' shadow term, and the batches of the GPU tests stay under the fragile cap."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_shadow_query as nsq
import np_trace_lit as ntl
import shadow_query_cases as sq
import trace_lit_cases as lc
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgs_trace_shadow_rays", "mgs_trace_shadow_rays_device", "mgs_shade_points", "mgs_shade_points_device")
INVALID_ARG, UNSUPPORTED = -1, -8


def test_header_declares_the_entry_points_and_the_structs():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_SHADOW_QUERY 1\b", hdr)
    assert "#define MGS_ABI_VERSION 5 " in hdr and "#define MGS_ABI_MINOR 1 " in hdr
    for n in NAMES:
        assert re.search(r"\bint\s+%s\(MgsScene" % n, hdr), n
        assert n in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.ShadowResult) == 16 == capi.SHADOW_RESULT_DTYPE.itemsize
    assert C.sizeof(capi.ShadeResult) == 16 == capi.SHADE_RESULT_DTYPE.itemsize
    assert C.sizeof(capi.SurfacePoint) == 64 == capi.SURFACE_POINT_DTYPE.itemsize == sq.point_batch().dtype.itemsize
    assert "meshes in the traced scene, soft shadows, indirect lighting and bounces" in hdr


def _rays(lib, p, t=None, l=None, q=None, device=False, count=4, rays=True):
    r, res = capi.make_rays(np.zeros((4, 3)), np.tile([0, 0, 1.0], (4, 1))), np.zeros(4, capi.SHADOW_RESULT_DTYPE)
    fn = lib.mgs_trace_shadow_rays_device if device else lib.mgs_trace_shadow_rays
    by = lambda v: C.byref(v) if v is not None else None
    rc = fn(None, r.ctypes.data_as(C.c_void_p) if rays else None, count, by(p), by(t), by(l), by(q), res.ctypes.data_as(C.c_void_p), None)
    return rc, lib.mgs_last_error()


def _points(lib, p, l=None, n_mat=1, device=False, material=0, t=None):
    pts = capi.make_surface_points(np.zeros((4, 3)), np.tile([0, 1.0, 0], (4, 1)), np.tile([0, -1.0, 0], (4, 1)), np.ones((4, 3)), material)
    res = np.zeros(4, capi.SHADE_RESULT_DTYPE)
    mats = (capi.Material * 300)(*[capi.make_material() for _ in range(300)])
    fn = lib.mgs_shade_points_device if device else lib.mgs_shade_points
    by = lambda v: C.byref(v) if v is not None else None
    rc = fn(None, pts.ctypes.data_as(C.c_void_p), 4, mats, n_mat, by(p), by(t), by(l), None, res.ctypes.data_as(C.c_void_p), None, None)
    return rc, lib.mgs_last_error()


def test_refusals_fire_before_the_handle_is_looked_at():
    lib = capi.load_library()
    p = capi.default_params(16, 16)
    hard = lambda **kw: capi.default_trace_light_params(**dict(dict(shadows_mode=1), **kw))
    for device in (False, True):
        # in range: only the NULL scene is left to complain about
        rc, msg = _rays(lib, p, l=hard(), device=device)
        assert rc == INVALID_ARG and b"null scene" in msg
        rc, msg = _rays(lib, p, device=device)  # `light` NULL: the defaults with hard shadows
        assert rc == INVALID_ARG and b"null scene" in msg
        for l, code in ((hard(shadows_mode=2), UNSUPPORTED), (hard(shadows_mode=0), INVALID_ARG), (hard(shadows_mode=3), INVALID_ARG),
                        (hard(shadows_mode=-1), INVALID_ARG), (hard(particle_shadow_transmittance_threshold=1.0), INVALID_ARG),
                        (hard(particle_shadow_color_strength=1.5), INVALID_ARG)):
            rc, msg = _rays(lib, p, l=l, device=device)
            assert rc == code and b"null scene" not in msg, (l.shadows_mode, rc, msg)
        # particle_shadow_offset is not read by the shadow rays
        rc, msg = _rays(lib, p, l=hard(particle_shadow_offset=-1.0), device=device)
        assert rc == INVALID_ARG and b"null scene" in msg
        for s in (1, 2):
            rc, msg = _rays(lib, p, t=capi.default_trace_params(trace_strategy=s), l=hard(), device=device)
            assert rc == UNSUPPORTED and b"null scene" not in msg
        rc, msg = _rays(lib, p, t=capi.default_trace_params(samples_per_pass=33), l=hard(), device=device)
        assert rc == INVALID_ARG and b"null scene" not in msg
        q = capi.RayQueryParams()
        q.reorder = 2
        rc, msg = _rays(lib, p, l=hard(), q=q, device=device)
        assert rc == INVALID_ARG and b"null scene" not in msg
        rc, msg = _rays(lib, p, l=hard(), device=device, rays=False)
        assert rc == INVALID_ARG and b"null scene" not in msg
        rc, msg = _rays(lib, p, l=hard(), device=device, rays=False, count=0)  # count == 0 with NULL arrays passes the checks
        assert rc == INVALID_ARG and b"null scene" in msg
        # light queries
        rc, msg = _points(lib, p, device=device)
        assert rc == INVALID_ARG and b"null scene" in msg
        rc, msg = _points(lib, p, l=hard(), device=device)
        assert rc == INVALID_ARG and b"null scene" in msg
        for kw, code in ((dict(l=hard(shadows_mode=2)), UNSUPPORTED), (dict(l=hard(shadows_mode=3)), INVALID_ARG), (dict(n_mat=0), INVALID_ARG),
                         (dict(n_mat=257), INVALID_ARG), (dict(l=hard(particle_shadow_offset=-1.0)), INVALID_ARG),
                         (dict(t=capi.default_trace_params(trace_strategy=1)), UNSUPPORTED)):
            rc, msg = _points(lib, p, device=device, **kw)
            assert rc == code and b"null scene" not in msg, (kw, rc, msg)
    rc, msg = _points(lib, p, material=1)  # the host variant reads the indices itself
    assert rc == INVALID_ARG and b"null scene" not in msg
    rc, msg = _points(lib, p, material=1, device=True)  # the device variant cannot: an invalid point, not an error
    assert rc == INVALID_ARG and b"null scene" in msg


def test_restatement_reproduces_the_lit_frame_shadow_term():
    """fed the frame's own origins (position + lightDir * offset, t_min 0, t_max lightDist), the query's restatement gives the shadow
    term np_trace_lit.lit computed for the pixel"""
    name = "l01_point"
    c, r = lc.cases()[name], lc.restate(name)
    kw = lc._trace_kw(c)
    pinst = nsq.per_inst([(ntl.prepare_set(a), M) for a, M in c["sets"]], float(np.float32(kw["kernel_min_response"])),
                         float(np.float32(kw["alpha_cull"])), kw["adaptive_clamping"])
    O, D, _ = ntl.rays(np.asarray(c["V"], np.float64), np.asarray(c["P"], np.float64), c["W"], c["H"])
    lp = np.asarray(c["lights"][0]["position"], np.float32).astype(np.float64)
    ys, xs = np.nonzero(r["rays"] == 1)
    assert len(ys) > 500
    seen = 0
    for y, x in list(zip(ys, xs))[::7]:
        pick = int(r["base"]["id"][y, x])
        e = ntl._eval(pinst[0], O[y, x], D[y, x], kw["kernel_degree"])
        pos = O[y, x] + e["t"][int(np.nonzero(e["idx"] == pick)[0][0])] * D[y, x]
        ldist = np.linalg.norm(lp - pos)
        ldir = (lp - pos) / ldist
        T, hits, _ = nsq.shadow_ray(pinst, pos + ldir * np.float32(0.2), ldir, 0.0, ldist, kw["samples_per_pass"], 0.8, 0.0)
        assert hits == r["shadow_hits"][y, x]
        assert np.abs(T - r["shadow_T"][y, x, 0]).max() <= 1e-6  # (the query rounds lightDist to fp32, the frame's restatement does not)
        seen += hits > 0
    assert seen > 5


def test_restatement_rules_of_the_window_the_direction_and_invalid_rays():
    pinst = sq.prepared(sq.MAIN)
    O, D, tmin, tmax = sq.ray_batch("main")
    ref = sq.restate_rays("default")
    bad = np.array(sq.INVALID_AT)
    assert not ref["valid"][bad].any() and ref["valid"].sum() == sq.N - len(bad)
    assert (ref["transmittance"][bad] == 1.0).all() and not ref["hits"][bad].any()
    i = int(np.nonzero(ref["valid"] & (ref["hits"] >= 2) & (tmin == 0) & (tmax < 1e9) & ~ref["fragile"])[0][0])
    full = nsq.shadow_ray(pinst, O[i], D[i], 0.0, tmax[i], 18, 0.0, 0.0)
    # the given direction: scaling it scales t, and nothing else
    s = np.float32(2.0)
    scaled = nsq.shadow_ray(pinst, O[i], D[i] * s, 0.0, tmax[i] / s, 18, 0.0, 0.0)
    assert scaled[1] == full[1] and np.abs(scaled[0] - full[0]).max() <= 1e-6
    # a negative t_min is 0; a window cut from below or from above loses hits
    assert nsq.shadow_ray(pinst, O[i], D[i], -5.0, tmax[i], 18, 0.0, 0.0)[1] == full[1]
    assert nsq.shadow_ray(pinst, O[i], D[i], 0.999 * tmax[i], tmax[i], 18, 0.0, 0.0)[1] < full[1]
    assert nsq.shadow_ray(pinst, O[i], D[i], 0.0, 0.01 * tmax[i], 18, 0.0, 0.0)[1] < full[1]
    # the batch has what the GPU test is to cover
    n = np.linalg.norm(D.astype(np.float64), axis=1)
    ok = ref["valid"]
    assert (np.abs(n[ok] - 1) > 0.1).sum() > 100 and (tmax[ok] == np.float32(1e10)).sum() > 100 and (tmin[ok] > 0).sum() > 100
    assert (np.abs(O[ok]).max(1) > 1.5).sum() > 100
    st = [sq.restate_rays(f"stack_{k}") for k in (1, 4, 18, 32)]
    assert st[0]["hits"].max() == 1 and st[1]["hits"].max() == 4 and st[2]["hits"].max() == 18 and st[3]["hits"].max() > 18


@pytest.mark.parametrize("name", sorted(sq.RAY_CONFIGS))
def test_fragile_share_of_the_ray_batches(name):
    ref = sq.restate_rays(name)
    share = ref["fragile"].mean()
    print(f"{name}: fragile share {share:.4f}")
    assert share <= 0.02


@pytest.mark.parametrize("name", sorted(sq.POINT_CONFIGS))
def test_fragile_share_of_the_point_batches(name):
    ref = sq.restate_points(name)
    print(f"{name}: fragile share {ref['fragile'].mean():.4f}, shadow rays {int(ref['rays'].sum())}")
    assert ref["fragile"].mean() <= 0.02
    assert not ref["range_fragile"].any()  # so that the GPU test holds MgsTraceLightOut::shadow_rays to the restatement's count exactly
    pts = sq.point_batch()
    assert (np.linalg.norm(pts["normal"], axis=1) < 0.2).sum() > 50
    if name == "three_lights":
        emissive = ref["valid"] & (pts["material"] == 0)
        assert not ref["rays"][emissive].any() and ref["rays"][ref["valid"] & (pts["material"] != 0)].min() >= 2  # the point light is out of range for some
        assert (ref["rays"] == 2).sum() > 50 and (ref["rays"] == 3).sum() > 50 and ref["shadow_hits"].sum() > 1000
    if name == "three_lights_spp_4":  # the K-buffer's size decides some of the batch: the case pins k_shade_points<4> apart from <18>
        wide = sq.restate_points("three_lights")
        assert not np.array_equal(ref["shadow_hits"], wide["shadow_hits"]) and not np.array_equal(ref["color"], wide["color"])


@pytest.mark.parametrize("name", sorted(sq.RAY_CONFIGS))
def test_float32_run_of_the_restatement(name):
    """the staleness check of shadow_query_cases.TWIN_DEV: the float32 run's distance from the float64 run on the non-fragile rays"""
    a, b = sq.restate_rays(name), sq.restate_rays(name, True)
    ok = a["valid"] & ~a["fragile"]
    dev = float(np.abs(a["transmittance"] - b["transmittance"])[ok].max())
    print(f"{name}: float32 run {dev:.3e}, entry {sq.TWIN_DEV[name]:.1e}")
    assert np.array_equal(a["hits"][ok], b["hits"][ok])
    assert sq.TWIN_DEV[name] / 3.0 <= dev <= sq.TWIN_DEV[name]
