"""child process of test_gpu_trace_lit.py: mgs_render_traced_lit in a fresh process.   usage: _child_trace_lit.py OUT.npz
Every case of trace_lit_cases.py (frame RGBA32F, hit counts, shadow hits, picked ids, both Out structs), then on l01_point: two runs,
every strip row on its own, a frame context, a changed light and material, and mgs_render_traced / mgs_render before and after."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import trace_lit_cases as lc  # noqa: E402

out = sys.argv[1]


def build(case, fmt=None):
    scene = mgs.Scene(0)
    for k, (arrays, M) in enumerate(case["sets"]):
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit(*([fmt, fmt] if fmt is not None else []))
    scene.set_lights([capi.make_light(**L) for L in case["lights"]])
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
    t = capi.default_trace_params(**case["trace"])
    l = capi.default_trace_light_params(**dict(case["light"], **light_over))
    o, lo = h.render_traced_lit(p, t, l, want_stats=True)
    return h.download_frame(p), h.trace_hit_counts(p), h.trace_shadow_hits(p), o, lo


res = {}
for name, case in lc.cases().items():
    scene = build(case)
    p = params(case)
    img, hits, sh, o, lo = lit(scene, case, p)
    _, ids = scene.download_surface(p)
    res.update({f"{name}_image": img, f"{name}_hits": hits, f"{name}_shadow_hits": sh, f"{name}_id": ids,
                f"{name}_shadow_rays": lo.shadow_rays, f"{name}_shadow_accepted": lo.shadow_accepted_hits, f"{name}_light_ms": lo.light_ms,
                f"{name}_rebuilt": o.bvh_rebuilt})
    if name == "l13_shadows_off":  # default materials, shadows off: the unlit traced frame on pixels with a surface
        for k in range(len(case["materials"])):
            scene.set_material(k, capi.make_material())
        a = lit(scene, case, p)[0]
        pu = params(case, lighting_mode=0, surface_outputs=1)
        scene.render_traced(pu, capi.default_trace_params(**case["trace"]))
        res["unlit_equal_image_lit"], res["unlit_equal_image_unlit"] = a, scene.download_frame(pu)
    if name == "l14_fisheye_dof":  # temporal accumulation over three samples against the frames traced singly
        res["dof_singles"] = np.stack([lit(scene, case, params(case, frame_sample_id=k))[0] for k in range(3)])
        res["dof_accumulated"] = np.stack([lit(scene, case, params(case, frame_sample_id=k, temporal_sampling=1))[0] for k in range(3)])
    if name == "l07_translucent_s1":  # the three target formats of one frame, then quantised SH / colour storage
        for tag, fmt in (("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):
            res[f"target_{tag}"] = lit(scene, case, params(case, target_format=fmt))[0]
        for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
            q = build(case, fmt)
            arrays = case["sets"][0][0]
            n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
            res[f"store_{tag}_rgba"] = q.download_set(0, 2, 4 * n).reshape(n, 4)
            sh = np.zeros((n, 15, 3), np.float32)
            sh[:, :cpc] = q.download_set(0, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
            res[f"store_{tag}_sh"] = sh
            qi, qh, qs, _, _ = lit(q, case, p)
            res[f"store_{tag}_image"], res[f"store_{tag}_hits"], res[f"store_{tag}_shadow_hits"] = qi, qh, qs
            q.close()
    if name == "l01_point":
        pu = params(case, lighting_mode=0)
        scene.render_traced(pu, None)
        try:  # the shadow hits belong to the last traced frame only when that frame was lit
            scene.trace_shadow_hits(pu)
            res["stale_shadow_hits_refused"] = False
        except mgs.MgsError:
            res["stale_shadow_hits_refused"] = True
        unlit_before = scene.download_frame(pu).tobytes()
        scene.render(pu)
        raster_before = scene.download_frame(pu).tobytes()
        b = lit(scene, case, p)
        res["same_twice"] = img.tobytes() == b[0].tobytes() and np.array_equal(sh, b[2]) and np.array_equal(hits, b[1])
        res["second_rebuilt"] = b[3].bvh_rebuilt
        scene.render_traced(pu, None)
        res["unlit_same_after"] = scene.download_frame(pu).tobytes() == unlit_before
        scene.render(pu)
        res["raster_same_after"] = scene.download_frame(pu).tobytes() == raster_before
        for r in range(3):
            s_img, _, s_sh, _, _ = lit(scene, case, params(case, strip_row_begin=r, strip_row_end=r + 1))
            y0, y1 = 16 * r, min(16 * r + 16, case["H"])
            res[f"strip_{r}"] = s_img[y0:y1].tobytes() == img[y0:y1].tobytes() and np.array_equal(s_sh[y0:y1], sh[y0:y1])
        ctx = scene.frame_context()
        c = lit(ctx, case, p)
        res["context_same"] = c[0].tobytes() == img.tobytes() and np.array_equal(c[2], sh)
        res["context_rebuilt"] = c[3].bvh_rebuilt
        ctx.close()
        moved = dict(case["lights"][0], position=(-0.6, 1.2, 0.4))
        scene.set_lights([capi.make_light(**moved)])
        d = lit(scene, case, p)
        res["light_changed_frame"], res["light_changed_rebuilt"] = d[0].tobytes() != img.tobytes(), d[3].bvh_rebuilt
        scene.set_material(0, capi.make_material(**dict(case["materials"][0], diffuse=(0.2, 0.9, 0.2))))
        e = lit(scene, case, p)
        res["material_changed_frame"], res["material_changed_rebuilt"] = e[0].tobytes() != d[0].tobytes(), e[3].bvh_rebuilt
        res["working_bytes"] = scene.memory_usage()[1]
    scene.close()
np.savez(out, **res)
