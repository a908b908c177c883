"""child process of test_gpu_shadow_query.py: shadow and light queries in a fresh process.   usage: _child_shadow_query.py MODE OUT.npz
MODE rays:   every configuration of shadow_query_cases.RAY_CONFIGS on the device, reorder off and on, the host variant, the storage
             formats with the tint on
MODE points: every configuration of POINT_CONFIGS on the device, reorder off and on, the host variant
MODE edges:  a scene without instances, count == 0, a bound occluder and sensor, a query between two lit frames, a moved instance"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import shadow_query_cases as sq  # noqa: E402
import trace_cases as tc  # noqa: E402
import trace_lit_cases as lc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
STATS = ("node_visits", "candidate_tests", "accepted_hits", "max_passes_used", "invalid_rays", "bvh_rebuilt")
LSTATS = ("shadow_rays", "shadow_node_visits", "shadow_candidate_tests", "shadow_accepted_hits")


def build(name, fmt=None, lights=None):
    scene = mgs.Scene(0)
    for arrays, M in sq.scene(name):
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit(*([fmt, fmt] if fmt is not None else []))
    if lights is not None:
        scene.set_lights([capi.make_light(**L) for L in lights])
    return scene


def params(**over):
    p = capi.default_params(16, 16)
    capi.set_camera(p, np.eye(4), np.eye(4), sq.CAMERA)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1).copy()).cuda()


def light_params(cfg):
    return capi.default_trace_light_params(shadows_mode=1, particle_shadow_transmittance_threshold=cfg["threshold"],
                                           particle_shadow_color_strength=cfg["strength"])


def rays_device(handle, dev, n, cfg, reorder):
    res = torch.full((n * 4 + 8,), -7.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o = handle.trace_shadow_rays_device(dev.data_ptr(), n, params(debug_flags=cfg.get("debug", 0)), res.data_ptr(),
                                        capi.default_trace_params(samples_per_pass=cfg.get("spp", 18)), light_params(cfg), reorder=reorder, want_stats=True)
    got = res.cpu().numpy()
    assert (got[n * 4:] == np.float32(-7.25)).all(), "the kernel wrote behind the results"
    return got[:n * 4].view(capi.SHADOW_RESULT_DTYPE), o.as_dict()


res = {}
if mode == "rays":
    scenes = {}
    for name, cfg in sq.RAY_CONFIGS.items():
        which = cfg["rays"]
        if which not in scenes:
            scenes[which] = build(sq.MAIN if which == "main" else sq.STACK)
        scene = scenes[which]
        rays = capi.make_rays(*sq.ray_batch(which))
        n, dev = rays.shape[0], on_device(rays)
        for reorder in (0, 1):
            got, o = rays_device(scene, dev, n, cfg, bool(reorder))
            res[f"{name}_{reorder}"] = got
            for k in STATS:
                res[f"{name}_{reorder}_{k}"] = o[k]
            res[f"{name}_{reorder}_reorder_ms"] = o["reorder_ms"]
        host, ho = scene.trace_shadow_rays(rays, params(debug_flags=cfg.get("debug", 0)), capi.default_trace_params(samples_per_pass=cfg.get("spp", 18)),
                                           light_params(cfg), want_stats=True)
        res[f"{name}_host"], res[f"{name}_host_accepted_hits"] = host, ho.trace.accepted_hits
    for s in scenes.values():
        s.close()
    cfg = sq.RAY_CONFIGS["thr0_tint"]
    rays = capi.make_rays(*sq.ray_batch("main"))
    for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
        q = build(sq.MAIN, fmt)
        for k, (arrays, _) in enumerate(sq.scene(sq.MAIN)):
            n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
            res[f"store_{tag}_rgba_{k}"] = q.download_set(k, 2, 4 * n).reshape(n, 4)
            sh = np.zeros((n, 15, 3), np.float32)
            sh[:, :cpc] = q.download_set(k, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
            res[f"store_{tag}_sh_{k}"] = sh
        res[f"store_{tag}"], _ = rays_device(q, on_device(rays), rays.shape[0], cfg, False)
        q.close()
elif mode == "points":
    pts = sq.point_batch()
    n, dev = pts.shape[0], on_device(pts)
    mats = sq.MATERIALS
    for name, cfg in sq.POINT_CONFIGS.items():
        scene = build(sq.MAIN, lights=cfg["lights"])
        lp = capi.default_trace_light_params(shadows_mode=cfg["shadows"])
        tp = capi.default_trace_params(samples_per_pass=cfg["spp"]) if "spp" in cfg else None
        for reorder in (0, 1):
            r = torch.full((n * 4 + 8,), -7.25, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            lo, bad = scene.shade_points_device(dev.data_ptr(), n, mats, params(), r.data_ptr(), tp, lp, reorder=bool(reorder), want_stats=True)
            got = r.cpu().numpy()
            assert (got[n * 4:] == np.float32(-7.25)).all(), "the kernel wrote behind the results"
            res[f"{name}_{reorder}"] = got[:n * 4].view(capi.SHADE_RESULT_DTYPE)
            res[f"{name}_{reorder}_invalid"] = bad
            for k in LSTATS:
                res[f"{name}_{reorder}_{k}"] = getattr(lo, k)
        if name == "no_shadows":
            res["no_shadows_built_a_hierarchy"] = scene.trace_shadow_rays(capi.make_rays(*sq.ray_batch("main"))[:8], params(), want_stats=True)[1].trace.bvh_rebuilt
        good = pts.copy()
        good["material"][sq.INVALID_AT[4]] = 0  # the host variant refuses an index out of range as a whole
        try:
            scene.shade_points(pts, mats, params(), tp, lp)
            res[f"{name}_host_refused"] = False
        except capi.MgsError as e:
            res[f"{name}_host_refused"] = e.code == -1  # MGS_ERR_INVALID_ARG
        host, lo, bad = scene.shade_points(good, mats, params(), tp, lp, want_stats=True)
        res[f"{name}_host"], res[f"{name}_host_invalid"] = host, bad
        scene.close()
else:
    rays = capi.make_rays(*sq.ray_batch("main"))
    pts = sq.point_batch()
    n = rays.shape[0]
    cfg = sq.RAY_CONFIGS["default"]
    # a scene without instances; count == 0
    empty = mgs.Scene(0)
    for reorder in (0, 1):
        got, o = rays_device(empty, on_device(rays), n, cfg, bool(reorder))
        res[f"empty_{reorder}"], res[f"empty_{reorder}_stats"] = got, np.array([o[k] for k in STATS], np.int64)
    res["empty_points"] = empty.shade_points(pts[:300], sq.MATERIALS, params(), None, capi.default_trace_light_params(shadows_mode=1))
    res["zero_rays"] = empty.trace_shadow_rays(rays[:0], params()).shape[0]
    res["zero_points"] = empty.shade_points(pts[:0], sq.MATERIALS, params()).shape[0]
    empty.close()
    # a query between two frames of one handle, with an occluder and a sensor bound for the query only
    case = lc.cases()[sq.MAIN]
    scene = build(sq.MAIN, lights=case["lights"])
    for k, m in enumerate(case["materials"]):
        scene.set_material(k, capi.make_material(**m))
    pf = capi.default_params(case["W"], case["H"])
    capi.set_camera(pf, case["V"], case["P"], case["eye"])
    pf.target_format, pf.lighting_mode = capi.TARGET_RGBA32F, capi.LIGHTING_DIRECT
    lt = capi.default_trace_light_params(shadows_mode=1)
    scene.render_traced_lit(pf, None, lt, want_stats=True)
    before = (scene.download_frame(pf), scene.trace_hit_counts(pf), scene.trace_shadow_hits(pf))
    whole, o = rays_device(scene, on_device(rays), n, cfg, False)
    res["first_rebuilt"] = o["bvh_rebuilt"]
    depth = torch.ones(case["W"] * case["H"], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.set_occluder(depth.data_ptr(), 0, case["W"], case["H"])
    sensor = capi.sensor_model_from_frame(pf)
    scene.set_sensor(sensor)
    bound, _ = rays_device(scene, on_device(rays), n, cfg, True)
    bound_pts = scene.shade_points(pts[:300], sq.MATERIALS, params(), None, lt)
    scene.set_sensor(None)
    scene.set_occluder(0, 0, 0, 0)
    res["bound_equal"] = bound.tobytes() == whole.tobytes()
    res["bound_points_any"] = bool(bound_pts["color"].any())
    after = (scene.download_frame(pf), scene.trace_hit_counts(pf), scene.trace_shadow_hits(pf))
    res["frame_unchanged"] = all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and bool(before[0].any()) and bool(before[2].any())
    m0 = scene.memory_usage()[1]
    # the blob of instance 1 moved far away: the next query rebuilds the hierarchy and no longer sees it
    M = np.array(sq.scene(sq.MAIN)[1][1], np.float32).copy()
    M[:3, 3] += np.float32(50.0)
    scene.set_transform(1, M)
    moved, o = rays_device(scene, on_device(rays), n, cfg, False)
    res["moved_rebuilt"], res["moved"], res["whole"] = o["bvh_rebuilt"], moved, whole
    res["working_bytes"] = m0
    scene.close()
np.savez(out, **res)
print("child ok")
