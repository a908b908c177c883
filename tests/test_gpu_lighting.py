"""GPU tests (-m gpu) of the deferred lighting pass (MgsFrameParams.lighting_mode, k_light.hip) and of the consolidated depth.

The pass is checked against the independent numpy restatement of the reference's shaders (np_lighting.py, float64) applied to the
library's OWN unlit frame and side outputs: what is under test is the pass, the G-buffer has its own tests against the oracle.
The bar comes from the CPU test (tests/test_lighting_cpu.py::test_cap_and_tolerance_from_the_reference_alone): float32 against
float64 of the restatement on the oracle's G-buffer differs by at most lighting_cases.F32_VS_F64 = 1.0e-3 (measured 9.57e-4,
relative to max(1, value)); the kernel gets 4 x that = 4.0e-3 on an RGBA32F target, plus half a unit of the last place on RGBA16F /
RGBA8.  Pixels whose outcome hangs on a comparison (the ambiguity mask, at most 0.5 % of the lit pixels) may take either outcome.
The library is compared with itself, bit for bit, where the subject is plumbing (strips, graph replay, contexts, modes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi
import lighting_cases as lc
import np_lighting as nl
import occluder_levels as ol

pytestmark = pytest.mark.gpu

TARGETS = {"f32": capi.TARGET_RGBA32F, "f16": capi.TARGET_RGBA16F, "u8": capi.TARGET_RGBA8}


@pytest.fixture(scope="module")
def lit_scene():
    scene = mgs.Scene(0)
    for arrays, m in lc.scene_sets():
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), m)
    scene.commit()
    yield scene
    scene.close()


def params(gut=0, target="f32", lighting=capi.LIGHTING_DIRECT, **kw):
    V, P, eye = lc.camera_matrices(mgs.camera_lookat_perspective)
    p = capi.default_params(lc.W, lc.H)
    capi.set_camera(p, V, P, eye)
    p.pipeline, p.target_format, p.lighting_mode = gut, TARGETS[target], lighting
    p.depth_iso_threshold = lc.ISO
    for k, v in kw.items():
        setattr(p, k, v)
    return p, V, P, eye


def apply(scene, lights, mats):
    scene.set_lights([capi.make_light(**l) for l in lights])
    for k, m in enumerate(mats):
        scene.set_material(k, capi.make_material(**m))


def reset(scene):
    apply(scene, [], [nl.default_material(), nl.default_material()])
    scene.clear_occluder()


def unlit_and_lit(scene, p):
    """(unlit frame, depth, ids, normal, lit frame) of the same parameters: surface_outputs = 1 without lighting, then lighting on"""
    mode = p.lighting_mode
    p.lighting_mode, p.surface_outputs = capi.LIGHTING_DISABLED, 1
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    base = scene.download_frame(p).copy()
    depth, ids, nrm = scene.download_surface(p, normals=True)
    p.lighting_mode, p.surface_outputs = mode, 0
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    lit = scene.download_frame(p).copy()
    d2, i2, n2 = scene.download_surface(p, normals=True)  # a lit frame is rendered as if surface_outputs = 1
    assert np.array_equal(d2, depth) and np.array_equal(i2, ids) and np.array_equal(n2.view(np.uint32), nrm.view(np.uint32))
    return base, depth, ids, nrm, lit


def check_against_restatement(name, base, depth, ids, nrm, lit, V, P, eye, lights, mats, target, occ_depth=None):
    r = nl.light_frame(nl.from_target(base), depth, ids, nrm, V, P, eye, lights, mats, lc.inst_prefix(), occ_depth)
    shaded = r.shaded
    # pass-through pixels keep the first frame's bits; lit pixels have alpha 1
    assert np.array_equal(lit[~shaded & ~r.mask_color], base[~shaded & ~r.mask_color]), name
    share = r.mask_color[shaded].mean()
    ok_a, err = lc.pixel_ok(lit, r.lit, target, lc.GPU_BAR)
    ok_b, _ = lc.pixel_ok(lit, r.alt, target, lc.GPU_BAR)
    outside = ~r.mask_color
    worst = float(err[outside][..., :3].max())
    print(f"lighting {name}: {shaded.mean():.3f} lit, mask {share:.5f}, max error outside the mask {worst:.3e} (bar {lc.GPU_BAR:.1e} + half ulp), "
          f"{int((~ok_a & outside).sum())} pixels outside the bar, {int((r.mask_color & ~(ok_a | ok_b)).sum())} masked pixels matching neither outcome")
    assert share <= lc.MASK_CAP, (name, share)
    assert (ok_a | ~outside).all(), (name, worst)
    assert ((ok_a | ok_b) | outside).all(), name
    assert (ids[shaded] == nl.INVALID_ID).any() and (~shaded).mean() >= 0.02, name  # the cases hold what they were built for
    return r


# ---- 1. the pass against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.CASES))
def test_lit_frame_matches_the_restatement(lit_scene, ob, name):
    gut, target, lights, mats, occluder = lc.CASES[name]
    scene = lit_scene
    p, V, P, eye = params(gut, target)
    apply(scene, lights, mats)
    occ_depth = None
    if occluder:
        insts = [(a, scene.storage_order(i, a["positions"].shape[0]), m) for i, (a, m) in enumerate(lc.scene_sets())]
        oks, _, _, _ = ob.storage_sorted_stream(ob.make_frame(V, P, eye, lc.W, lc.H), insts)
        occ_depth, bg = lc.occluder_images(ol.pick_level(ol.depths_of_btf_keys(oks), 0.5))
        scene.upload_occluder(occ_depth, bg)
    base, depth, ids, nrm, lit = unlit_and_lit(scene, p)
    r = check_against_restatement(name, base, depth, ids, nrm, lit, V, P, eye, lights, mats, target, occ_depth)
    # consolidated depth: comparisons of fp32 values, exact
    cons = scene.download_consolidated_depth(p)
    assert np.array_equal(cons, r.consolidated), name
    if occluder:
        assert (cons == occ_depth).any() and (cons < occ_depth).any()
    else:
        assert (cons == 1.0).any() and (cons < 1.0).any()
    reset(scene)


def test_cpu_sort_mode(lit_scene):
    scene = lit_scene
    p, V, P, eye = params(0, "f32", sort_mode=capi.SORT_CPU_ASYNC, cpu_sort_blocking=1)
    apply(scene, lc.LIGHTS_MIXED, lc.MATS_A)
    base, depth, ids, nrm, lit = unlit_and_lit(scene, p)
    check_against_restatement("cpu sort", base, depth, ids, nrm, lit, V, P, eye, lc.LIGHTS_MIXED, lc.MATS_A, "f32")
    reset(scene)


# ---- 2. defining properties, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["f32", "f16", "u8"])
def test_default_materials_leave_the_colours_alone(lit_scene, target):
    """the splat sets' default material is fully emissive and needs no shading: whatever the lights, a lit frame keeps the colour of
    every pixel whose splat was picked, bit for bit, and sets its alpha to 1.0; pixels without a surface are untouched"""
    scene = lit_scene
    reset(scene)
    scene.set_lights([capi.make_light(**l) for l in lc.LIGHTS_MIXED])
    p, V, P, eye = params(0, target)
    base, depth, ids, nrm, lit = unlit_and_lit(scene, p)
    shaded = ~(nrm[..., 3] < np.float32(0.001))
    one = {"f32": np.float32(1), "f16": np.float16(1), "u8": np.uint8(255)}[target]
    # (pixels with a surface but without a picked splat take the SHADER's default material, which is shaded — ambient 0.1, diffuse =
    #  base colour, deferred_shading.comp.slang:98-129 — whatever the instances' materials are: the property holds where an id was picked)
    keep = ~shaded | (ids != nl.INVALID_ID)
    assert np.array_equal(lit[..., :3][keep], base[..., :3][keep]) and (keep & shaded).mean() > 0.5
    changed = shaded & (ids == nl.INVALID_ID)
    assert changed.any() and (nl.from_target(lit)[..., :3][changed] >= nl.from_target(base)[..., :3][changed]).all()
    assert (lit[..., 3][shaded] == one).all() and np.array_equal(lit[..., 3][~shaded], base[..., 3][~shaded])
    assert shaded.any() and (~shaded).any() and (base[..., 3][shaded] != one).any()
    reset(scene)


def test_direct_and_indirect_render_the_same_frame_and_off_restores_the_unlit_bytes(lit_scene):
    scene = lit_scene
    apply(scene, lc.LIGHTS_MIXED, lc.MATS_A)
    p, V, P, eye = params(0, "f16", lighting=capi.LIGHTING_DISABLED)
    scene.render(p)
    unlit = scene.download_frame(p).copy()
    p.lighting_mode = capi.LIGHTING_DIRECT
    scene.render(p)
    a = scene.download_frame(p).copy()
    p.lighting_mode = capi.LIGHTING_INDIRECT
    scene.render(p)
    b = scene.download_frame(p).copy()
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16)) and not np.array_equal(a.view(np.uint16), unlit.view(np.uint16))
    p.lighting_mode = capi.LIGHTING_DISABLED
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), unlit.view(np.uint16))
    with pytest.raises(mgs.MgsError) as e:  # ... and that frame asked for no surface outputs
        scene.download_consolidated_depth(p)
    assert e.value.code == capi.ERR_STATE
    reset(scene)


@pytest.mark.parametrize("gut", [0, 1])
def test_strips_equal_the_full_frame(lit_scene, gut):
    scene = lit_scene
    apply(scene, lc.LIGHTS_MIXED, lc.MATS_A)
    p, V, P, eye = params(gut, "f32")
    scene.render(p)
    full = scene.download_frame(p).copy()
    rows = (lc.H + 15) // 16
    got = np.zeros_like(full)
    for r0, r1 in ((0, 3), (3, 11), (11, rows)):  # three uneven strips
        p.strip_row_begin, p.strip_row_end = r0, r1
        scene.render(p)
        got[r0 * 16:r1 * 16] = scene.download_frame(p)[r0 * 16:r1 * 16]
    assert np.array_equal(got.view(np.uint32), full.view(np.uint32))
    reset(scene)


def test_graph_replay_equals_plain_launches():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_lighting.py")
    out = {}
    for mode, extra in (("graph", {}), ("plain", {"MGS_GRAPH": "0"})):
        r = subprocess.run([sys.executable, child], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        out[mode] = [l for l in r.stdout.splitlines() if l.startswith("FRAMES_SHA1")]
    assert out["graph"] and out["graph"] == out["plain"]


def test_a_frame_context_equals_its_scene_and_lights_change_between_replays(lit_scene):
    scene = lit_scene
    apply(scene, lc.LIGHTS_MIXED, lc.MATS_A)
    p, V, P, eye = params(0, "f32")
    scene.render(p)
    ref = scene.download_frame(p).copy()
    ctx = scene.frame_context()
    try:
        for _ in range(2):  # the second frame replays the context's captured graph
            ctx.render(p)
            assert np.array_equal(ctx.download_frame(p).view(np.uint32), ref.view(np.uint32))
        with pytest.raises(mgs.MgsError) as e:
            ctx.set_lights([])
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(mgs.MgsError) as e:
            ctx.set_material(0, capi.make_material())
        assert e.value.code == capi.ERR_STATE
        # a light changed on the scene reaches the context's next (replayed) frame, and changing it back restores the bits
        dimmer = [dict(l) for l in lc.LIGHTS_MIXED]
        dimmer[0]["intensity"] = 0.1
        scene.set_lights([capi.make_light(**l) for l in dimmer])
        for h in (ctx, scene):
            h.render(p)
            assert not np.array_equal(h.download_frame(p).view(np.uint32), ref.view(np.uint32))
        scene.set_lights([capi.make_light(**l) for l in lc.LIGHTS_MIXED])
        for h in (ctx, scene):
            h.render(p)
            assert np.array_equal(h.download_frame(p).view(np.uint32), ref.view(np.uint32))
    finally:
        ctx.close()
    reset(scene)


def test_alpha_sum_with_lighting(lit_scene):
    scene = lit_scene
    apply(scene, [], lc.MATS_B)
    p, V, P, eye = params(0, "f32", alpha_mode=capi.ALPHA_SUM)
    base, depth, ids, nrm, lit = unlit_and_lit(scene, p)
    shaded = ~(nrm[..., 3] < np.float32(0.001))
    assert (lit[..., 3][shaded] == 1.0).all() and (base[..., 3][shaded] != 1.0).any()
    reset(scene)


# ---- 3. temporal accumulation --------------------------------------------------------------------------------------------------
def test_temporal_accumulation_averages_lit_samples(lit_scene, ob):
    scene = lit_scene
    apply(scene, lc.LIGHTS_MIXED, lc.MATS_B)
    p, V, P, eye = params(0, "f32")

    def sample_lights(k):  # another light set per sample, so that the four lit frames differ
        ls = [dict(l) for l in lc.LIGHTS_MIXED]
        ls[0]["intensity"] = 0.2 + 0.4 * k
        return [capi.make_light(**l) for l in ls]
    singles = []
    for k in range(4):
        scene.set_lights(sample_lights(k))
        p.frame_sample_id = k
        scene.render(p)
        singles.append(scene.download_frame(p).astype(np.float32))
    assert not np.array_equal(singles[0], singles[3])
    p.temporal_sampling = 1
    main = np.zeros_like(singles[0])
    for k in range(4):
        scene.set_lights(sample_lights(k))
        p.frame_sample_id = k
        scene.render(p)
        got = scene.download_frame(p).astype(np.float32)
        main = ob.post_accumulate(main, singles[k], k)
        assert np.abs(got - main).max() <= 1e-3, k  # the bar of test_gpu_stochastic.py::test_temporal_accumulation_matches_post_comp
    reset(scene)


# ---- 4. consolidated depth and errors ----------------------------------------------------------------------------------------
def test_consolidated_depth_without_lighting(lit_scene):
    scene = lit_scene
    p, V, P, eye = params(0, "f16", lighting=capi.LIGHTING_DISABLED, surface_outputs=1)
    scene.render(p)
    depth, ids = scene.download_surface(p)
    want, _ = nl.consolidate_depth(depth)
    assert np.array_equal(scene.download_consolidated_depth(p), want)
    occ = np.full((lc.H, lc.W), 0.99, np.float32)
    occ[:, ::3] = 1.0
    scene.upload_occluder(occ)
    scene.render(p)
    depth, ids = scene.download_surface(p)
    want, _ = nl.consolidate_depth(depth, occ)
    assert np.array_equal(scene.download_consolidated_depth(p), want) and (want == np.float32(0.99)).any() and (want < np.float32(0.99)).any()
    scene.clear_occluder()
    p.surface_outputs = 0
    scene.render(p)
    with pytest.raises(mgs.MgsError) as e:
        scene.download_consolidated_depth(p)
    assert e.value.code == capi.ERR_STATE


def test_errors(lit_scene):
    scene = lit_scene
    p, V, P, eye = params(0, "f16", sort_mode=capi.SORT_STOCHASTIC)
    with pytest.raises(mgs.MgsError) as e:
        scene.render(p)
    assert e.value.code == capi.ERR_UNSUPPORTED
    p, V, P, eye = params(0, "f16", lighting=3)
    with pytest.raises(mgs.MgsError) as e:
        scene.render(p)
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(mgs.MgsError) as e:
        scene.set_lights([capi.make_light()] * 65)
    assert e.value.code == capi.ERR_INVALID_ARG
    scene.set_lights([capi.make_light()] * 64)
    with pytest.raises(mgs.MgsError) as e:
        scene.set_lights([capi.make_light(type=3)])
    assert e.value.code == capi.ERR_INVALID_ARG
    with pytest.raises(mgs.MgsError) as e:
        scene.set_material(2, capi.make_material())
    assert e.value.code == capi.ERR_INVALID_ARG
    scene.set_lights([])


def test_stage_time_of_the_pass(lit_scene):
    scene = lit_scene
    p, V, P, eye = params(0, "f16", collect_timings=1)
    scene.render(p)
    ms = scene.timings_all()
    assert ms[capi.STAGE_LIGHT] > 0.0 and ms[5] >= ms[capi.STAGE_LIGHT] and ms[4] >= 0.0
    p.lighting_mode = capi.LIGHTING_DISABLED
    scene.render(p)
    assert scene.timings_all()[capi.STAGE_LIGHT] == 0.0
