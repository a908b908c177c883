"""child process of test_gpu_trace.py: mgs_render_traced in a fresh process.   usage: _child_trace.py MODE OUT.npz [CASE]
MODE case:   one case of trace_cases.py: the frame (RGBA32F), hit counts, side outputs and MgsTraceOut
MODE extras: determinism, strips, rebuild rules, a frame context, the error codes, the raster path before and after
MODE formats: c_two_instances with quantised SH / colour storage at three K-buffer sizes, the three target formats, temporal
             accumulation of four depth-of-field frames, and every strip row of a 36-row frame on its own"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import trace_cases as tc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]


def build(case):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    if case["sets"]:
        scene.commit()
    return scene


def params(case, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format, p.surface_outputs = capi.TARGET_RGBA32F, 1
    for k, v in dict(case["frame"], **over).items():
        setattr(p, k, v)
    return p


def traced(scene, case, p=None, **trace_over):
    p = p or params(case)
    t = capi.default_trace_params(**dict(case["trace"], **trace_over))
    o = scene.render_traced(p, t, want_stats=True)
    return scene.download_frame(p), scene.trace_hit_counts(p), o


if mode == "case":
    case = tc.cases()[sys.argv[3]]
    scene = build(case)
    p = params(case)
    img, hits, o = traced(scene, case, p)
    depth, ids, nrm = scene.download_surface(p, normals=True)
    n0 = case["sets"][0][0]["positions"].shape[0] if case["sets"] else 0
    order0 = scene.storage_order(0, n0) if n0 else np.zeros(0, np.uint32)  # instance 0: storage index -> caller's index
    np.savez(out, image=img, hits=hits, depth=depth, id=ids, normal=nrm, storage_order_0=order0,
             **{"out_" + k: v for k, v in o.as_dict().items()})
    scene.close()
elif mode == "formats":
    res = {}
    case = tc.cases()["c_two_instances"]
    p = params(case)
    for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
        scene = mgs.Scene(0)
        for arrays, M in case["sets"]:
            scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
        scene.commit(fmt, fmt)
        for k, (arrays, _) in enumerate(case["sets"]):
            n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
            res[f"{tag}_rgba_{k}"] = scene.download_set(k, 2, 4 * n).reshape(n, 4)
            sh = np.zeros((n, 15, 3), np.float32)  # the set's own stride is 3 * cpc floats per splat, [coef][rgb]
            sh[:, :cpc] = scene.download_set(k, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
            res[f"{tag}_sh_{k}"] = sh
        for spp in (18, 4, 32):
            img, hits, _ = traced(scene, case, p, samples_per_pass=spp)
            _, ids = scene.download_surface(p)
            res[f"{tag}_image_{spp}"], res[f"{tag}_hits_{spp}"], res[f"{tag}_id_{spp}"] = img, hits, ids
        scene.close()
    scene = build(case)
    # the same frame to the three target formats
    for tag, fmt in (("f32", capi.TARGET_RGBA32F), ("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):
        res[f"target_{tag}"], res[f"target_{tag}_hits"], _ = traced(scene, case, params(case, target_format=fmt))
    # temporal accumulation: four depth-of-field samples singly, then accumulated by the library
    dof = dict(dof_mode=1, focus_dist=3.0, aperture=0.01)
    res["dof_singles"] = np.stack([traced(scene, case, params(case, frame_sample_id=k, **dof))[0] for k in range(4)])
    res["dof_accumulated"] = np.stack([traced(scene, case, params(case, frame_sample_id=k, temporal_sampling=1, **dof))[0] for k in range(4)])
    # every strip row of the 36-row frame on its own (the last one is a partial tile row) against the full frame; the camera is
    # tilted so that the splats reach the last rows (with the case's own camera rows 30..35 are empty)
    tilted = dict(case, V=tc.lookat(case["eye"], (0.0, -0.9, 0.0)))
    full_img, full_hits, _ = traced(scene, tilted)
    for r in range(3):
        s_img, s_hits, _ = traced(scene, tilted, params(tilted, strip_row_begin=r, strip_row_end=r + 1))
        y0, y1 = 16 * r, min(16 * r + 16, case["H"])
        res[f"strip_{r}"] = s_img[y0:y1].tobytes() == full_img[y0:y1].tobytes() and np.array_equal(s_hits[y0:y1], full_hits[y0:y1])
    res["last_rows_hits"] = full_hits[32:].max(axis=1)
    scene.close()
    np.savez(out, **res)
else:
    res = {}
    case = tc.cases()["c_two_instances"]
    scene = build(case)
    p = params(case)
    a_img, a_hits, o1 = traced(scene, case, p)
    b_img, b_hits, o2 = traced(scene, case, p)
    res["first_rebuilt"], res["second_rebuilt"] = o1.bvh_rebuilt, o2.bvh_rebuilt
    res["same_frame_twice"] = a_img.tobytes() == b_img.tobytes() and np.array_equal(a_hits, b_hits)
    res["scene_bytes_has_bvh"] = scene.memory_usage()[0]
    # a second, freshly built scene: two builds of the same inputs
    scene2 = build(case)
    c_img, c_hits, _ = traced(scene2, case, p)
    res["same_after_rebuild"] = a_img.tobytes() == c_img.tobytes() and np.array_equal(a_hits, c_hits)
    scene2.close()
    # a change of the proxy's parameters rebuilds, changing it back rebuilds again to the same frame
    _, _, o3 = traced(scene, case, p, kernel_adaptive_clamping=0)
    d_img, d_hits, o4 = traced(scene, case, p)
    res["proxy_change_rebuilt"] = o3.bvh_rebuilt == 1 and o4.bvh_rebuilt == 1
    res["same_after_second_build"] = a_img.tobytes() == d_img.tobytes() and np.array_equal(a_hits, d_hits)
    # strip rows [1, 2)
    ps = params(case, strip_row_begin=1, strip_row_end=2)
    s_img, s_hits, _ = traced(scene, case, ps)
    res["strip_equal"] = s_img[16:32].tobytes() == a_img[16:32].tobytes() and np.array_equal(s_hits[16:32], a_hits[16:32])
    # a frame context traces over the scene's hierarchy
    traced(scene, case, p)
    ctx = scene.frame_context()
    x_img, x_hits, ox = traced(ctx, case, p)
    res["context_equal"] = x_img.tobytes() == a_img.tobytes() and np.array_equal(x_hits, a_hits)
    res["context_rebuilt"] = ox.bvh_rebuilt
    # a transform change rebuilds; the frame is saved for the comparison with the restatement
    M2 = tc.trs((1.2, 0.9, 1.0), (0, 0, 1), 15.0, (0.5, 0.2, -0.3))
    scene.set_transform(1, M2)
    m_img, m_hits, om = traced(scene, case, p)
    _, _, om2 = traced(scene, case, p)
    res["moved_rebuilt"], res["moved_again_rebuilt"] = om.bvh_rebuilt, om2.bvh_rebuilt
    res["moved_image"], res["moved_hits"], res["moved_M"] = m_img, m_hits, M2
    # the raster path before and after a traced frame
    pr = capi.default_params(case["W"], case["H"])
    capi.set_camera(pr, case["V"], case["P"], case["eye"])
    pr.target_format = capi.TARGET_RGBA32F
    scene.render(pr)
    r0 = scene.download_frame(pr)
    traced(scene, case, p)
    scene.render(pr)
    r1 = scene.download_frame(pr)
    res["raster_unchanged"] = r0.tobytes() == r1.tobytes() and bool(r0.any())

    # error codes
    def code(fn):
        try:
            fn()
            return 0
        except mgs.MgsError as e:
            return e.code

    res["err_lighting"] = code(lambda: traced(scene, case, params(case, lighting_mode=1)))
    res["err_stochastic"] = code(lambda: traced(scene, case, params(case, sort_mode=3)))
    scene.upload_occluder(np.ones((case["H"], case["W"]), np.float32))
    res["err_occluder"] = code(lambda: traced(scene, case, p))
    scene.clear_occluder()
    res["err_spp"] = code(lambda: traced(scene, case, p, samples_per_pass=40))
    res["err_passes"] = code(lambda: traced(scene, case, p, max_passes=0))
    res["err_kmr"] = code(lambda: traced(scene, case, params(case, kernel_min_response=0.0)))
    fresh = mgs.Scene(0)
    fresh.add_instance(mgs.SplatSet.from_arrays(**case["sets"][0][0]))
    res["err_uncommitted"] = code(lambda: traced(fresh, case, p))
    fresh.close()
    ctx.close()
    scene.close()
    np.savez(out, **res)
print("child ok")
