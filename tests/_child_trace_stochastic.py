"""child process of test_gpu_trace_stochastic.py: mgs_render_traced with a stochastic trace strategy in a fresh process.
usage: _child_trace_stochastic.py MODE OUT.npz [CASE]
MODE case:      one case of trace_stochastic_cases.py: pass-stochastic frames for the two sample ids, one any-hit frame, one any-hit frame
                with MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED added to the case's flags, side outputs
MODE mechanics: determinism, strips, a frame context, strategy switches, explicit strategy 0 against trace = NULL
MODE stat:      the running mean of N_STAT samples of both strategies (temporal accumulation), downloaded once each"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import trace_stochastic_cases as sc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]


def build(case, res=None):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    if case["sets"]:
        if case["commit"] == "u8":
            scene.commit(capi.FORMAT_UINT8, capi.FORMAT_UINT8)
            for k, (arrays, _) in enumerate(case["sets"]):  # what the device holds, for the restatement
                n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
                res[f"rgba_{k}"] = scene.download_set(k, 2, 4 * n).reshape(n, 4)
                sh = np.zeros((n, 15, 3), np.float32)
                sh[:, :cpc] = scene.download_set(k, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
                res[f"sh_{k}"] = sh
        else:
            scene.commit()
    return scene


def params(case, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format, p.surface_outputs = capi.TARGET_RGBA32F, 1
    for k, v in dict(case["frame"], **over).items():
        setattr(p, k, v)
    return p


def traced(scene, case, strategy, p=None, **trace_over):
    p = p or params(case)
    t = capi.default_trace_params(**dict(case["trace"], trace_strategy=strategy, **trace_over))
    o = scene.render_traced(p, t, want_stats=True)
    depth, ids, nrm = scene.download_surface(p, normals=True)
    return dict(image=scene.download_frame(p), hits=scene.trace_hit_counts(p), depth=depth, id=ids, normal=nrm,
                accepted_hits=o.accepted_hits, max_passes_used=o.max_passes_used, bvh_rebuilt=o.bvh_rebuilt)


def same(a, b, rows=slice(None)):
    return all(a[k][rows].tobytes() == b[k][rows].tobytes() for k in ("image", "hits", "depth", "id", "normal"))


res = {}
if mode == "case":
    case = sc.cases()[sys.argv[3]]
    scene = build(case, res)
    for sid in sc.SAMPLE_IDS:
        for k, v in traced(scene, case, 1, params(case, frame_sample_id=sid)).items():
            res[f"pass{sid}_{k}"] = v
    for k, v in traced(scene, case, 2).items():
        res[f"any_{k}"] = v
    for k, v in traced(scene, case, 2, params(case, debug_flags=case["frame"].get("debug_flags", 0) | 4)).items():
        res[f"anyopaque_{k}"] = v
    n0 = case["sets"][0][0]["positions"].shape[0] if case["sets"] else 0
    res["storage_order_0"] = scene.storage_order(0, n0) if n0 else np.zeros(0, np.uint32)
    scene.close()
elif mode == "mechanics":
    case = sc.cases()["b_cloud_k18"]
    scene = build(case)
    p = params(case)
    first = traced(scene, case, 0)
    res["first_rebuilt"] = first["bvh_rebuilt"]
    scene.render_traced(p, None)
    res["explicit_0_equals_null"] = scene.download_frame(p).tobytes() == first["image"].tobytes()
    res["switch_rebuilt"] = 0
    for s in (1, 2):
        a = traced(scene, case, s)
        b = traced(scene, case, s)
        other = traced(scene, case, s, params(case, frame_sample_id=1))
        res["switch_rebuilt"] += a["bvh_rebuilt"] + b["bvh_rebuilt"] + other["bvh_rebuilt"]
        res[f"s{s}_same_twice"] = same(a, b)
        res[f"s{s}_other_sample_differs"] = a["image"].tobytes() != other["image"].tobytes()
        top = traced(scene, case, s, params(case, strip_row_begin=0, strip_row_end=1))
        res[f"s{s}_strip"] = same(top, a, slice(0, 16))   # a 12-row frame has one strip row; [1, ...) is empty and traces nothing
        ctx = scene.frame_context()
        c = traced(ctx, case, s)
        res[f"s{s}_context"] = same(c, a) and c["bvh_rebuilt"] == 0
        ctx.close()
        res[f"s{s}_max_passes_used"] = a["max_passes_used"]
        res[f"s{s}_accepted_equals_sum"] = int(a["accepted_hits"]) == int(a["hits"].sum())
    scene.close()
    # two strip rows: a 20 x 24 frame of the same scene; rows [0, 1) and [1, 2) against the full frame
    tall = dict(case, H=24, P=sc.tc.persp(50.0, 20 / 24))
    scene = build(tall)
    for s in (1, 2):
        full = traced(scene, tall, s)
        r0 = traced(scene, tall, s, params(tall, strip_row_begin=0, strip_row_end=1))
        r1 = traced(scene, tall, s, params(tall, strip_row_begin=1, strip_row_end=2))
        res[f"s{s}_two_strips"] = same(r0, full, slice(0, 16)) and same(r1, full, slice(16, 24)) and bool(full["hits"][16:].any())
    scene.close()
elif mode == "stat":
    case = sc.cases()[sc.STAT_CASE]
    scene = build(case)
    for s in (1, 2):
        t0 = time.perf_counter()
        t = capi.default_trace_params(**dict(case["trace"], trace_strategy=s, min_transmittance=0.0))
        for k in range(sc.N_STAT):
            p = params(case, frame_sample_id=k, temporal_sampling=1, surface_outputs=0)
            scene.render_traced(p, t)
        res[f"mean_{s}"] = scene.download_frame(p)
        res[f"seconds_{s}"] = time.perf_counter() - t0
    scene.close()
np.savez(out, **res)
print("child ok")
