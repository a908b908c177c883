"""child process of test_gpu_hybrid.py: mgs_render_hybrid in a fresh process.   usage: _child_hybrid.py OUT.npz
Every case of hybrid_cases.py: the unlit mgs_render frame with surface outputs (image and the three surfaces), then the hybrid frame
(image, surfaces, shadow hits, counters); then the target formats, quantised storage, temporal accumulation, strips, a frame
context and the other pipelines before and after."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import hybrid_cases as hc  # noqa: E402

out = sys.argv[1]


def build(case, fmt=None):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
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


def unlit(h, case, **over):
    """(image, depth, ids, normal) of mgs_render with lighting off and the surface outputs on"""
    pu = params(case, **dict(over, lighting_mode=0, surface_outputs=1))
    o = h.render(pu, want_stats=True)
    return (h.download_frame(pu),) + h.download_surface(pu, normals=True) + (o,)


def hybrid(h, case, **over):
    """(image, depth, ids, normal, shadow hits, FrameOut, TraceLightOut)"""
    p = params(case, **over)
    o, lo = h.render_hybrid(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]), want_stats=True)
    return (h.download_frame(p),) + h.download_surface(p, normals=True) + (h.trace_shadow_hits(p), o, lo)


def put(res, tag, u, hy):
    for k, key in enumerate(("image", "depth", "id", "normal")):
        res[f"{tag}_u_{key}"], res[f"{tag}_h_{key}"] = u[k], hy[k]
    res[f"{tag}_shadow_hits"] = hy[4]
    res[f"{tag}_shadow_rays"], res[f"{tag}_shadow_accepted"], res[f"{tag}_light_ms"] = hy[6].shadow_rays, hy[6].shadow_accepted_hits, hy[6].light_ms
    res[f"{tag}_error_flags"], res[f"{tag}_sorted"], res[f"{tag}_u_sorted"] = hy[5].error_flags, hy[5].sorted_count, u[4].sorted_count


res = {}
for name, case in hc.cases().items():
    scene = build(case)
    u = unlit(scene, case)
    wb1 = scene.memory_usage()[1]
    hy = hybrid(scene, case)
    put(res, name, u, hy)
    if name == "h01_3dgs":
        res["working_bytes_growth"] = scene.memory_usage()[1] - wb1
        p = params(case)
        pu = params(case, lighting_mode=0)
        scene.render(pu)
        raster_before = scene.download_frame(pu).tobytes()
        tl = lambda: scene.render_traced_lit(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]), want_stats=True)
        o1, _ = tl()
        traced_before, traced_hits_before = scene.download_frame(p).tobytes(), scene.trace_shadow_hits(p).copy()
        b = hybrid(scene, case)
        res["same_twice"] = b[0].tobytes() == hy[0].tobytes() and np.array_equal(b[4], hy[4])
        try:  # no primary walk: a hybrid frame leaves no hit counts
            scene.trace_hit_counts(p)
            res["hit_counts_refused"] = False
        except mgs.MgsError:
            res["hit_counts_refused"] = True
        o2, _ = tl()
        res["traced_lit_rebuilt_after_hybrid"] = o2.bvh_rebuilt
        res["traced_lit_same_after"] = scene.download_frame(p).tobytes() == traced_before and np.array_equal(scene.trace_shadow_hits(p), traced_hits_before)
        scene.render(pu)
        res["raster_same_after"] = scene.download_frame(pu).tobytes() == raster_before
        full = hybrid(scene, case)
        for r in range(3):
            s = hybrid(scene, case, strip_row_begin=r, strip_row_end=r + 1)
            y0, y1 = 16 * r, min(16 * r + 16, case["H"])
            res[f"strip_{r}"] = s[0][y0:y1].tobytes() == full[0][y0:y1].tobytes() and np.array_equal(s[4][y0:y1], full[4][y0:y1])
        scene.upload_occluder(np.ones((case["H"], case["W"]), np.float32))  # a bound occluder: refused, with the unbind hint
        try:
            hybrid(scene, case)
            res["occluder_refusal"] = "rendered"
        except mgs.MgsError as e:
            res["occluder_refusal"] = f"{e.code} {e}"
        scene.clear_occluder()
        res["same_after_refusal"] = hybrid(scene, case)[0].tobytes() == hy[0].tobytes()
        ctx = scene.frame_context()
        ctx.render_traced_lit(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]))
        co, _ = ctx.render_traced_lit(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]), want_stats=True)
        c = hybrid(ctx, case)
        res["context_same"] = c[0].tobytes() == hy[0].tobytes() and np.array_equal(c[4], hy[4])
        res["context_rebuilt"] = co.bvh_rebuilt
        ctx.close()
    if name == "h02_3dgut":  # a handle whose light-pass scratch exists already: the hybrid frame adds the normalised normal alone
        p = params(case)
        q = build(case)
        q.render_traced_lit(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"]))
        unlit(q, case)  # (the raster working set of the frame)
        mid = q.memory_usage()[1]
        hybrid(q, case)
        res["working_bytes_after_traced_lit"] = q.memory_usage()[1] - mid
        q.close()
    if name == "h09_shadows_off":  # the deferred raster pass on the same scene
        pl = params(case)
        scene.render(pl)
        res["h09_deferred_image"] = scene.download_frame(pl)
    if name == "h04_dof":  # temporal accumulation over three samples against the frames rendered singly
        res["dof_singles"] = np.stack([hybrid(scene, case, frame_sample_id=k)[0] for k in range(3)])
        res["dof_accumulated"] = np.stack([hybrid(scene, case, frame_sample_id=k, temporal_sampling=1)[0] for k in range(3)])
    if name == "h07_translucent_s1":
        for tag, fmt in (("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):  # the G-buffer of a frame of that format
            put(res, "target_" + tag, unlit(scene, case, target_format=fmt), hybrid(scene, case, target_format=fmt))
        for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
            q = build(case, fmt)
            arrays = case["sets"][0][0]
            n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
            res[f"store_{tag}_rgba"] = q.download_set(0, 2, 4 * n).reshape(n, 4)
            sh = np.zeros((n, 15, 3), np.float32)
            sh[:, :cpc] = q.download_set(0, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
            res[f"store_{tag}_sh"] = sh
            put(res, "store_" + tag, unlit(q, case), hybrid(q, case))
            q.close()
    scene.close()
np.savez(out, **res)
