"""child process of test_gpu_trace.py: mgs_render_traced in a fresh process.   usage: _child_trace.py MODE OUT.npz [CASE]
MODE case:   one case of trace_cases.py: the frame (RGBA32F), hit counts, side outputs and MgsTraceOut
MODE extras: determinism, strips, rebuild rules, a frame context, the error codes, the raster path before and after"""
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
    np.savez(out, image=img, hits=hits, depth=depth, id=ids, normal=nrm, **{"out_" + k: v for k, v in o.as_dict().items()})
    scene.close()
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
