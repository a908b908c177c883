"""child process of test_gpu_rays.py: ray queries in a fresh process.   usage: _child_rays.py MODE OUT.npz
MODE tied:  generated rays of a 40 x 24 pinhole, fisheye and depth-of-field frame traced as a batch, next to the traced frame itself,
            at samples_per_pass 4, 18 and 32
MODE batch: the batch of ray_cases.py on the device: reorder off and on, reversed and shuffled
MODE shared: one handle through mgs_render_traced, a ray query of that frame's rays, mgs_render_traced_lit, mgs_render_hybrid and
            mgs_render_traced again, with the same parameters: whether each call rebuilt the hierarchy, the first and the last frame
MODE edges: counts around the wave and workgroup sizes with a sentinel behind the results, an all-invalid batch, a scene without
            instances, the host variant, a query on a frame context next to a finished frame, the reorder buffers in working_bytes"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import ray_cases as rc  # noqa: E402
import trace_cases as tc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
case = tc.cases()[rc.SCENE]
STATS = ("node_visits", "candidate_tests", "accepted_hits", "max_passes_used", "invalid_rays")


def build():
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit()
    return scene


def params(W, H, **over):
    p = capi.default_params(W, H)
    capi.set_camera(p, case["V"], tc.persp(50.0, W / H), case["eye"])
    p.target_format, p.surface_outputs = capi.TARGET_RGBA32F, 1
    for k, v in over.items():
        setattr(p, k, v)
    return p


def on_device(rays):
    """the rays as a device array (16-byte aligned: torch's allocations are)"""
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).copy()).cuda()


def query(handle, rays_dev, count, p, trace=None, reorder=False, extra=0):
    """mgs_trace_rays_device into a fresh result array of count + extra entries, pre-filled with a sentinel; waits (want_stats)"""
    res = torch.full(((count + extra) * 12,), -7.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _, o = handle.trace_rays((rays_dev.data_ptr() if rays_dev is not None else 0, count), p, trace, reorder=reorder, want_stats=True,
                             results=res.data_ptr())
    return res.cpu().numpy().view(capi.RAY_RESULT_DTYPE), o.as_dict()


if mode == "tied":
    res = {}
    scene = build()
    W, H = 40, 24
    cams = dict(pinhole={}, fisheye=dict(camera_model=1, fov_rad=2.4), dof=dict(dof_mode=1, focus_dist=3.0, aperture=0.01, frame_sample_id=2))
    for cam, over in cams.items():
        p = params(W, H, **over)
        rays = torch.zeros(W * H * 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        scene.generate_rays(p, rays.data_ptr())
        for spp in (4, 18, 32):
            t = capi.default_trace_params(samples_per_pass=spp)
            got, o = query(scene, rays, W * H, p, t)
            fo = scene.render_traced(p, t, want_stats=True)
            tag = f"{cam}_{spp}"
            res[tag + "_result"] = got
            res[tag + "_image"], res[tag + "_hits"] = scene.download_frame(p), scene.trace_hit_counts(p)
            _, res[tag + "_id"], res[tag + "_normal"] = scene.download_surface(p, normals=True)
            for k in STATS[:4]:
                res[f"{tag}_rays_{k}"], res[f"{tag}_frame_{k}"] = o[k], getattr(fo, k)
            res[tag + "_invalid_rays"] = o["invalid_rays"]
        res[cam + "_rays"] = rays.cpu().numpy().view(capi.RAY_DTYPE)
    scene.close()
    np.savez(out, **res)
elif mode == "batch":
    res = {}
    scene = build()
    p = params(16, 16)
    O, D, tmin, tmax = rc.batch()
    rays = capi.make_rays(O, D, tmin, tmax)
    n = rays.shape[0]
    rng = np.random.Generator(np.random.PCG64(99))
    orders = dict(caller=np.arange(n), reversed=np.arange(n)[::-1].copy(), shuffled=rng.permutation(n))
    for name, perm in orders.items():
        dev = on_device(rays[perm])
        for reorder in (0, 1):
            got, o = query(scene, dev, n, p, reorder=bool(reorder))
            back = np.empty_like(got)
            back[perm] = got                                  # to the caller's order
            res[f"{name}_{reorder}"] = back
            for k in STATS:
                res[f"{name}_{reorder}_{k}"] = o[k]
            res[f"{name}_{reorder}_reorder_ms"] = o["reorder_ms"]
    scene.close()
    np.savez(out, **res)
elif mode == "shared":
    res = {}
    scene = build()
    W, H = case["W"], case["H"]
    p, t = params(W, H), capi.default_trace_params()
    lit = params(W, H, lighting_mode=capi.LIGHTING_DIRECT)
    rays = torch.zeros(W * H * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o = scene.render_traced(p, t, want_stats=True)
    res["first_rebuilt"], res["first_image"], res["first_hits"] = o.bvh_rebuilt, scene.download_frame(p), scene.trace_hit_counts(p)
    scene.generate_rays(p, rays.data_ptr())
    got, q = query(scene, rays, W * H, p, t)
    res["query_rebuilt"], res["query_hits"] = q["bvh_rebuilt"], got["hit_count"].reshape(H, W)
    o, _ = scene.render_traced_lit(lit, t, None, want_stats=True)
    res["lit_rebuilt"] = o.bvh_rebuilt
    scene.render_hybrid(lit, t, None, want_stats=True)
    o = scene.render_traced(p, t, want_stats=True)
    res["last_rebuilt"], res["last_image"], res["last_hits"] = o.bvh_rebuilt, scene.download_frame(p), scene.trace_hit_counts(p)
    scene.close()
    np.savez(out, **res)
else:
    res = {}
    scene = build()
    p = params(16, 16)
    O, D, tmin, tmax = rc.batch()
    ok = np.setdiff1d(np.arange(rc.N), rc.INVALID_AT)
    rays = capi.make_rays(O, D, tmin, tmax)[ok]
    whole, _ = query(scene, on_device(rays[:257]), 257, p)
    for count in (0, 1, 63, 64, 65, 255, 256, 257):
        for reorder in (0, 1):
            dev = on_device(rays[:max(count, 1)])
            got, o = query(scene, dev if count else None, count, p, reorder=bool(reorder), extra=3)
            res[f"count_{count}_{reorder}_equal"] = got[:count].tobytes() == whole[:count].tobytes()
            res[f"count_{count}_{reorder}_sentinel"] = bool((got[count:].view(np.float32) == np.float32(-7.25)).all())
            res[f"count_{count}_{reorder}_hits"] = int(got[:count]["hit_count"].sum()) == int(o["accepted_hits"])
    # nothing but invalid rays
    bad = capi.make_rays(np.zeros((300, 3)), np.tile([0.0, 0.0, 1.0], (300, 1)))
    bad["origin"][0::4, 1] = np.nan
    bad["direction"][1::4, 0] = np.inf
    bad["direction"][2::4] = 0.0
    bad["t_min"][3::4], bad["t_max"][3::4] = 2.0, 1.0
    for reorder in (0, 1):
        got, o = query(scene, on_device(bad), 300, p, reorder=bool(reorder))
        res[f"invalid_{reorder}"] = got
        for k in STATS:
            res[f"invalid_{reorder}_{k}"] = o[k]
    # without the side outputs: the same walk, no pick and no normals
    flat, _ = query(scene, on_device(rays[:257]), 257, params(16, 16, surface_outputs=0))
    res["nosurf_same"] = all(flat[k].tobytes() == whole[k].tobytes() for k in ("radiance", "transmittance", "hit_count", "passes"))
    res["nosurf_empty"] = (not flat["normal"].view(np.uint32).any() and not flat["t_iso"].view(np.uint32).any() and bool((flat["id"] == 0xFFFFFFFF).all())
                           and bool(whole["normal"].any()) and bool((whole["id"] != 0xFFFFFFFF).any()))
    # the host variant
    host, ho = scene.trace_rays(rays[:257], p, want_stats=True)
    res["host_equal"] = host.tobytes() == whole.tobytes()
    res["host_hits"] = int(ho.trace.accepted_hits) == int(whole["hit_count"].sum())
    res["host_reordered_equal"] = scene.trace_rays(rays[:257], p, reorder=True).tobytes() == whole.tobytes()
    res["host_empty"] = scene.trace_rays(rays[:0], p).shape[0]
    # a query on a frame context next to the scene handle's finished traced frame
    pf = params(40, 24)
    scene.render_traced(pf, None, want_stats=True)
    before = (scene.download_frame(pf), scene.trace_hit_counts(pf)) + scene.download_surface(pf, normals=True)
    ctx = scene.frame_context()
    got, _ = query(ctx, on_device(rays[:257]), 257, p)
    res["context_equal"] = got.tobytes() == whole.tobytes()
    after = (scene.download_frame(pf), scene.trace_hit_counts(pf)) + scene.download_surface(pf, normals=True)
    res["frame_unchanged"] = all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and bool(before[0].any())
    # the reorder buffers belong to the handle (a fresh context: nothing of its working set has grown yet for ray queries)
    m0 = ctx.memory_usage()[1]
    dev = on_device(rays[:3000])
    query(ctx, dev, 3000, p, reorder=True)
    m1 = ctx.memory_usage()[1]
    query(ctx, dev, 3000, p, reorder=True)
    m2 = ctx.memory_usage()[1]
    res["working_bytes"] = np.array([m0, m1, m2], np.int64)
    ctx.close()
    scene.close()
    # a scene without instances
    empty = mgs.Scene(0)
    for reorder in (0, 1):
        got, o = query(empty, on_device(rays[:100]), 100, p, reorder=bool(reorder))
        res[f"empty_{reorder}"] = got
        res[f"empty_{reorder}_stats"] = np.array([o[k] for k in STATS], np.int64)
    empty.close()
    np.savez(out, **res)
print("child ok")
