"""child process of test_gpu_trace_soft.py: soft shadows (MGS_SHADOWS_SOFT) in a fresh process.   usage: _child_trace_soft.py OUT.npz
Every case of trace_soft_cases.py at frame_sample_id 0 (traced: frame RGBA32F, hit counts, shadow hits, picked ids, counters; hybrid:
the unlit raster G-buffer and the hybrid frame), then on s01_penumbra: sample ids 0..15, two runs, every strip row on its own, a frame
context, temporal accumulation, the radii's interface, and hard / unlit / raster frames before and after."""
import os
import sys

os.environ["MGS_SOFT_SHADOWS"] = "1"  # before the library reads its switches
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import np_lighting as nl  # noqa: E402
import trace_soft_cases as sc  # noqa: E402

out = sys.argv[1]


def build(case):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit()
    for m in case.get("meshes", []):  # a lit frame with trace meshes
        mesh = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m["material_ids"], [capi.make_material(**x) for x in m["materials"]])
        k = scene.add_mesh_instance(mesh, m["transform"])
        scene.set_mesh_visible(k, m["visible"])
    if "meshes" in case:
        scene.set_trace_meshes(True, case["mesh_min_T"])
    scene.set_lights([capi.make_light(**L) for L in case["lights"]])
    scene.set_light_radii(case["radii"])
    for k, m in enumerate(case["materials"]):
        scene.set_material(k, capi.make_material(**m))
    return scene


def params(case, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format = capi.TARGET_RGBA32F
    for k, v in dict(case["frame"], **over).items():
        setattr(p, k, v)
    return p


def lit(h, case, p=None, **light_over):
    p = p or params(case)
    o, lo = h.render_traced_lit(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**dict(case["light"], **light_over)),
                                want_stats=True)
    return h.download_frame(p), h.trace_hit_counts(p), h.trace_shadow_hits(p), o, lo


def code_of(fn):
    try:
        fn()
        return 0
    except mgs.MgsError as e:
        return e.code


res = {}
for name, case in sc.cases().items():
    scene = build(case)
    p = params(case)
    if case["hybrid"]:
        pu = params(case, lighting_mode=0, surface_outputs=1)
        scene.render(pu)
        g = (scene.download_frame(pu),) + scene.download_surface(pu, normals=True)
        o, lo = scene.render_hybrid(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]), want_stats=True)
        for k, key in enumerate(("image", "depth", "id", "normal")):
            res[f"{name}_u_{key}"] = g[k]
        res.update({f"{name}_image": scene.download_frame(p), f"{name}_shadow_hits": scene.trace_shadow_hits(p), f"{name}_shadow_rays": lo.shadow_rays,
                    f"{name}_shadow_accepted": lo.shadow_accepted_hits, f"{name}_light_ms": lo.light_ms})
        # radii 0 under SOFT is the hard hybrid frame
        scene.set_light_radii([0.0] * len(case["lights"]))
        scene.render_hybrid(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]))
        a = scene.download_frame(p).tobytes()
        scene.render_hybrid(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**dict(case["light"], shadows_mode=1)))
        res[f"{name}_zero_radii_is_hard"] = a == scene.download_frame(p).tobytes()
        scene.close()
        continue
    img, hits, sh, o, lo = lit(scene, case, p)
    _, ids = scene.download_surface(p)
    res.update({f"{name}_image": img, f"{name}_hits": hits, f"{name}_shadow_hits": sh, f"{name}_id": ids, f"{name}_shadow_rays": lo.shadow_rays,
                f"{name}_shadow_accepted": lo.shadow_accepted_hits, f"{name}_light_ms": lo.light_ms})
    if "meshes" in case:  # a second sample
        s1 = lit(scene, case, params(case, frame_sample_id=1))
        res[f"{name}_sample1_image"], res[f"{name}_sample1_shadow_hits"] = s1[0], s1[2]
    if name == "s06_mesh":  # the same frame twice; every strip row; radii 0 against the hard frame
        res["s06_same_twice"] = lit(scene, case, p)[0].tobytes() == img.tobytes()
        full_sh = sh
        for r in range(3):
            s_img, _, s_sh, _, _ = lit(scene, case, params(case, strip_row_begin=r, strip_row_end=r + 1))
            y0, y1 = 16 * r, min(16 * r + 16, case["H"])
            res[f"s06_strip_{r}"] = s_img[y0:y1].tobytes() == img[y0:y1].tobytes() and np.array_equal(s_sh[y0:y1], full_sh[y0:y1])
        hard = lit(scene, case, p, shadows_mode=1)
        scene.set_light_radii([0.0] * len(case["lights"]))
        zero = lit(scene, case, p)
        res["s06_zero_radii_is_hard"] = zero[0].tobytes() == hard[0].tobytes() and np.array_equal(zero[2], hard[2])
    if name == "s05_fisheye_dof":  # a second sample: lens and light draw from separate states
        res["s05_sample1_image"] = lit(scene, case, params(case, frame_sample_id=1))[0]
    if name == "s01_penumbra":
        n = len(case["lights"])
        pu = params(case, lighting_mode=0)
        scene.render_traced(pu, None)
        unlit_before = scene.download_frame(pu).tobytes()
        scene.render(pu)
        raster_before = scene.download_frame(pu).tobytes()
        hard_before = lit(scene, case, p, shadows_mode=1)
        samples = [lit(scene, case, params(case, frame_sample_id=k)) for k in range(16)]
        res["s01_samples"] = np.stack([s[0] for s in samples])
        res["s01_sample1_shadow_hits"], res["s01_sample1_hits"] = samples[1][2], samples[1][1]
        res["s01_sample1_shadow_rays"] = samples[1][4].shadow_rays
        b = lit(scene, case, p)
        res["same_twice"] = img.tobytes() == b[0].tobytes() == samples[0][0].tobytes() and np.array_equal(sh, b[2]) and np.array_equal(hits, b[1])
        res["second_rebuilt"] = b[3].bvh_rebuilt
        for r in range(3):
            s_img, _, s_sh, _, _ = lit(scene, case, params(case, strip_row_begin=r, strip_row_end=r + 1))
            y0, y1 = 16 * r, min(16 * r + 16, case["H"])
            res[f"strip_{r}"] = s_img[y0:y1].tobytes() == img[y0:y1].tobytes() and np.array_equal(s_sh[y0:y1], sh[y0:y1])
        ctx = scene.frame_context()
        c = lit(ctx, case, p)
        res["context_same"] = c[0].tobytes() == img.tobytes() and np.array_equal(c[2], sh)
        res["context_rebuilt"] = c[3].bvh_rebuilt
        res["context_setter_code"] = code_of(lambda: ctx.set_light_radii([0.5] * n))
        ctx.close()
        res["accumulated"] = np.stack([lit(scene, case, params(case, frame_sample_id=k, temporal_sampling=1))[0] for k in range(3)])
        # the radii's interface
        res["count_mismatch_code"] = code_of(lambda: scene.set_light_radii([0.5] * (n + 1)))
        res["negative_code"] = code_of(lambda: scene.set_light_radii([-0.5] * n))
        res["nan_code"] = code_of(lambda: scene.set_light_radii([float("nan")] * n))
        res["same_after_refusals"] = lit(scene, case, p)[0].tobytes() == img.tobytes()
        scene.set_light_radii([1.0] * n)
        one = lit(scene, case, p)[0].tobytes()
        res["radius_one_differs"] = one != img.tobytes()
        scene.set_light_radii(case["radii"])
        scene.set_lights([capi.make_light(**L) for L in case["lights"]])  # resets every radius to 1.0
        res["set_lights_resets"] = lit(scene, case, p)[0].tobytes() == one
        scene.set_light_radii(case["radii"])
        scene.set_light_radii(None)  # NULL, 0: the defaults
        res["null_restores"] = lit(scene, case, p)[0].tobytes() == one
        scene.set_light_radii([0.0] * n)
        zero = lit(scene, case, p)
        res["zero_radii_is_hard"] = zero[0].tobytes() == hard_before[0].tobytes() and np.array_equal(zero[2], hard_before[2])
        sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), intensity=1.0)
        scene.set_lights([capi.make_light(**sun)])  # (radius 1.0: a directional light draws nothing)
        res["directional_is_hard"] = lit(scene, case, p)[0].tobytes() == lit(scene, case, p, shadows_mode=1)[0].tobytes()
        scene.set_lights([capi.make_light(**L) for L in case["lights"]])
        scene.set_light_radii(case["radii"])
        # the entry points that stay without soft shadows
        t = capi.default_trace_params(**case["trace"])
        soft = capi.default_trace_light_params(**case["light"])
        res["indirect_code"] = code_of(lambda: scene.render_traced_indirect(params(case, lighting_mode=2), t, soft, 2))
        pts = capi.make_surface_points(np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, -1.0, 0.0]]), np.ones((1, 3)), np.zeros(1, np.int64))
        res["shade_points_code"] = code_of(lambda: scene.shade_points(pts, [capi.make_material()], p, t, soft))
        res["same_after_all"] = lit(scene, case, p)[0].tobytes() == img.tobytes()
        # the other paths after soft frames
        hard_after = lit(scene, case, p, shadows_mode=1)
        res["hard_same_after"] = hard_after[0].tobytes() == hard_before[0].tobytes() and np.array_equal(hard_after[2], hard_before[2])
        scene.render_traced(pu, None)
        res["unlit_same_after"] = scene.download_frame(pu).tobytes() == unlit_before
        scene.render(pu)
        res["raster_same_after"] = scene.download_frame(pu).tobytes() == raster_before
    scene.close()
np.savez(out, **res)
