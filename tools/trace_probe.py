#!/usr/bin/env python3
"""trace_probe — MgsTraceOut and the stage times of the traced pipeline for synthetic scenes.

  python tools/trace_probe.py syn:<n> [syn:<n> ...] [--size W H] [--warmup 3] [--repeats 10] [--samples-per-pass 18] [--trace-strategy full|pass|anyhit] [--lit] [--hybrid] [--rays N [N ...]] [--shadow-rays N [N ...]] [--mesh-rays N [N ...] [--mesh file.obj]] [--trace-meshes [--indirect]] [--hybrid-meshes] [--json OUT.json]

Per scene: one traced frame that builds the hierarchy (build_ms), then --warmup frames, then --repeats timed frames of the benchmark
orbit's pose 5; prints the median, minimum and maximum traced frame time (HIP events around the traversal), node visits and candidate
tests per ray, and writes everything as JSON.  --trace-strategy: MgsTraceParams::trace_strategy of the unlit frames (the lit
and hybrid ones take the sorted strategy alone).  --lit adds lit frames (mgs_render_traced_lit, a diffuse material) with 0 / 1 / 4 point
lights and shadows off / on: the median light_ms and MgsTraceLightOut per shadow ray; in a process started with MGS_SOFT_SHADOWS=1 also a
"soft" row per light count: hard and soft light_ms on the same scene, pose and lights, alternated frame by frame.  --hybrid (with --lit) renders the same lit
scenes through mgs_render_hybrid as well: the raster frame's time, light_ms and the shadow counters beside the traced ones.
--rays N adds ray queries (mgs_trace_rays_device) of about N rays, for every N given: a RANDOM batch (origins uniform in the ball of
the camera's distance, each aimed at a random point of the inner half of that ball: neighbouring lanes share nothing) and a CAMERA
batch (mgs_trace_generate_rays of the probe's camera at the frame size of the scene's aspect with about N pixels, row-major), each
with reorder off and on: the median trace_ms and reorder_ms and the visits per ray; and mgs_render_traced's trace_ms of that same
frame, whose lanes are 8 x 8 pixels where the row-major batch's are 64 x 1.
--shadow-rays N adds shadow queries (mgs_trace_shadow_rays_device) of N rays toward one point light above the scene, for every N
given: a RANDOM batch (origins uniform in the ball of the camera's distance) and a COHERENT one (origins on a regular grid of the
plane below the scene, row-major), each with reorder off and on: the median trace_ms and reorder_ms and the rays per second.
--mesh-rays N [--mesh file.obj] needs no syn: scene: mesh ray queries (mgs_trace_mesh_rays_device) of about N rays against the mesh
(default: tests/golden/meshes/fixture.obj) instanced on a 3 x 3 grid: a CAMERA batch (mgs_trace_generate_rays) and a RANDOM batch,
closest and occlusion mode, reorder off and on: MgsMeshRayOut with the median trace_ms and reorder_ms, and the build time.
--trace-meshes (with a syn: scene) adds the mesh (--mesh, default the fixture) on a 3 x 3 grid to the scene and measures unlit frames
and lit frames (one point light, hard shadows) with mgs_frame_set_trace_meshes off and on: trace_ms, light_ms and both MgsMeshRayOut
blocks of mgs_trace_mesh_stats.  shadow.trace_ms is the mesh composite kernel's time, which traces the occlusion rays of the mesh
points; the occlusion rays of the splat surface run inside light_ms, while shadow.hits counts the occluded rays of both.
--indirect (with --trace-meshes) adds mgs_render_traced_indirect: on that scene with every bounce material illum 0 (max_bounces 3 and
16: what the rounds without a live pixel cost next to the lit frame), then with a mirror floor under the grid (max_bounces 1 and 3):
MgsTraceBounceOut with the median bounce_ms, the live pixels per bounce and their share of the frame.
--hybrid-meshes (with a syn: scene) adds the same grid and measures hybrid frames (3DGS surface, one point light, hard shadows) with
mgs_frame_set_hybrid_meshes off and on: the medians of the mesh depth pre-pass, the raster frame, light_ms and the mesh composite.
Needs an MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402


def random_rays(n, radius, seed=1):
    """n incoherent rays as a RAY_DTYPE array: origins uniform in the ball of `radius`, aimed at random points of the ball of radius / 2"""
    rng = np.random.Generator(np.random.PCG64(seed))

    def ball(r):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * (r * rng.random((n, 1)) ** (1.0 / 3.0))

    o, target = ball(radius), ball(0.5 * radius)
    d = target - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    return capi.make_rays(o, d)


def probe_mesh_rays(path, n, W, H, warmup, repeats):
    """the eight mesh-ray runs of --mesh-rays for one batch size: (camera, random) x (closest, occlusion) x (reorder off, on)"""
    import torch
    scene = mgs.Scene(0)
    mesh = capi.Mesh.load_obj(path)
    pos = mesh.view()["positions"]
    ext = float(np.abs(pos).max()) * 2.5
    for i in range(9):
        M = np.eye(4, dtype=np.float32)
        M[0, 3], M[2, 3] = (i % 3 - 1) * ext, (i // 3 - 1) * ext
        scene.add_mesh_instance(mesh, M)
    eye = np.float32([2.0 * ext, 1.5 * ext, 2.5 * ext])
    w, h = camera_frame_size(n, W, H)
    pc = capi.default_params(w, h)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, w, h)
    capi.set_camera(pc, V, P, eye)
    cam = torch.empty(w * h * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.generate_rays(pc, cam.data_ptr())
    scene.sync()
    rnd = torch.from_numpy(random_rays(n, float(np.linalg.norm(eye))).view(np.float32).copy()).cuda()
    out = dict(requested=n, mesh=os.path.basename(path), instances=9, runs=[])
    for batch, dev, count in (("camera", cam, w * h), ("random", rnd, n)):
        hits = torch.empty(count * 16, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for mode, tag in ((capi.MESH_RAYS_CLOSEST, "closest"), (capi.MESH_RAYS_OCCLUSION, "occlusion")):
            for reorder in (False, True):
                tms, rms = [], []
                for k in range(warmup + repeats):
                    o = scene.trace_mesh_rays_device(dev.data_ptr(), count, hits.data_ptr(), mode=mode, reorder=reorder, want_stats=True)
                    if o.bvh_rebuilt:
                        out["build_ms"] = float(o.build_ms)
                    if k >= warmup:
                        tms.append(o.trace_ms)
                        rms.append(o.reorder_ms)
                d = {k: v for k, v in o.as_dict().items() if not k.endswith("_ms")}
                d.update(batch=batch, mode=tag, reorder=int(reorder), rays=count, trace_ms_median=float(np.median(tms)), trace_ms_min=float(min(tms)),
                         trace_ms_max=float(max(tms)), reorder_ms_median=float(np.median(rms)), node_visits_per_ray=o.node_visits / count,
                         triangle_tests_per_ray=o.triangle_tests / count)
                out["runs"].append(d)
    out["scene_bytes"] = scene.memory_usage()[0]
    scene.close()
    mesh.close()
    return out


def add_mesh_grid(scene, path):
    """the mesh on a 3 x 3 grid, once per scene (--trace-meshes and --hybrid-meshes share it): the grid's spacing"""
    if getattr(scene, "_probe_grid", None) is None:
        mesh = capi.Mesh.load_obj(path)
        ext = float(np.abs(mesh.view()["positions"]).max()) * 2.5
        for i in range(9):
            M = np.eye(4, dtype=np.float32)
            M[0, 3], M[2, 3] = (i % 3 - 1) * ext, (i // 3 - 1) * ext
            scene.add_mesh_instance(mesh, M)
        scene._probe_grid = (mesh, ext)
    return scene._probe_grid[1]


def probe_hybrid_meshes(scene, p, t, path, warmup, repeats):
    """--hybrid-meshes: hybrid frames (3DGS surface, one point light, hard shadows) of the scene plus the mesh on the 3 x 3 grid, with
    mgs_frame_set_hybrid_meshes off and on: the medians of the mesh depth pre-pass (primary.trace_ms: both kernels), the raster frame,
    light_ms (hand-over and light pass) and the mesh composite (shadow.trace_ms)"""
    add_mesh_grid(scene, path)
    scene.set_material(0, capi.make_material(ambient=(0.1, 0.1, 0.1), diffuse=(0.8, 0.8, 0.8), emission=(0.0, 0.0, 0.0)))
    scene.set_lights([capi.make_light(position=(4.0, 6.0, 3.0), range=1000.0, attenuation_mode=0)])
    lp = capi.default_trace_light_params(shadows_mode=1)
    out = dict(mesh=os.path.basename(path), instances=9, runs=[])
    p.lighting_mode, p.collect_timings = 1, 1
    for on in (0, 1):
        scene.set_hybrid_meshes(bool(on))
        pre, ras, lms, cms = [], [], [], []
        for k in range(warmup + repeats):
            fo, lo = scene.render_hybrid(p, t, lp, want_stats=True)
            primary, shadow = scene.trace_mesh_stats() if on else (None, None)
            if k >= warmup:
                ras.append(fo.stage_ms[5]), lms.append(lo.light_ms)
                pre.append(primary.trace_ms if on else 0.0), cms.append(shadow.trace_ms if on else 0.0)
        d = dict(hybrid_meshes=on, prepass_ms_median=float(np.median(pre)), raster_ms_median=float(np.median(ras)), light_ms_median=float(np.median(lms)),
                 light_ms_min=float(min(lms)), light_ms_max=float(max(lms)), composite_ms_median=float(np.median(cms)), shadow_rays=int(lo.shadow_rays))
        if on:
            d["primary"], d["shadow"] = primary.as_dict(), shadow.as_dict()
            d["note"] = "prepass: k_trace_mesh_primary and the depth plane; composite: the mesh shading kernel; the splat surface's mesh occlusion rays are inside light_ms"
        out["runs"].append(d)
    p.lighting_mode, p.collect_timings = 0, 0
    scene.set_hybrid_meshes(False)
    return out


def probe_trace_meshes(scene, p, t, path, eye, warmup, repeats, indirect=False):
    """--trace-meshes: unlit and lit frames of the scene plus the mesh on a 3 x 3 grid, the setting off and on"""
    ext = add_mesh_grid(scene, path)
    scene.set_material(0, capi.make_material(ambient=(0.1, 0.1, 0.1), diffuse=(0.8, 0.8, 0.8), emission=(0.0, 0.0, 0.0)))
    scene.set_lights([capi.make_light(position=(4.0, 6.0, 3.0), range=1000.0, attenuation_mode=0)])
    lp = capi.default_trace_light_params(shadows_mode=1)
    out = dict(mesh=os.path.basename(path), instances=9, runs=[])
    for on in (0, 1):
        scene.set_trace_meshes(bool(on))
        for lit in (0, 1):
            p.lighting_mode = lit
            tms, lms = [], []
            for k in range(warmup + repeats):
                if lit:
                    o, lo = scene.render_traced_lit(p, t, lp, want_stats=True)
                else:
                    o, lo = scene.render_traced(p, t, want_stats=True), None
                if k >= warmup:
                    tms.append(o.trace_ms)
                    lms.append(lo.light_ms if lit else 0.0)
            d = dict(trace_meshes=on, lit=lit, trace_ms_median=float(np.median(tms)), trace_ms_min=float(min(tms)), trace_ms_max=float(max(tms)),
                     light_ms_median=float(np.median(lms)), light_ms_min=float(min(lms)), shadow_rays=int(lo.shadow_rays) if lit else 0)
            if on:
                primary, shadow = scene.trace_mesh_stats()
                d["primary"], d["shadow"] = primary.as_dict(), shadow.as_dict()
                d["note"] = "shadow.trace_ms: the mesh composite kernel; the splat surface's mesh occlusion rays are inside light_ms"
            out["runs"].append(d)
    if indirect:
        out["indirect"] = probe_indirect(scene, p, t, lp, ext, warmup, repeats)
    p.lighting_mode = 0
    scene.set_trace_meshes(False)
    return out


def probe_indirect(scene, p, t, lp, ext, warmup, repeats):
    """--indirect (with --trace-meshes, the setting on): mgs_render_traced_indirect.  First on the scene as it is, every bounce
    material illum 0: against the lit frame above, the price of max_bounces rounds without a live pixel.  Then with a mirror floor
    under the grid, max_bounces 1 and 3: bounce_ms, the live pixels per bounce and their share of the frame."""
    pixels = p.width * p.height
    p.lighting_mode = 2

    def run(nb):
        tms, lms, cms, bms = [], [], [], []
        for k in range(warmup + repeats):
            o, lo, bo = scene.render_traced_indirect(p, t, lp, nb, want_stats=True)
            _, shadow = scene.trace_mesh_stats()
            if k >= warmup:
                tms.append(o.trace_ms), lms.append(lo.light_ms), cms.append(shadow.trace_ms), bms.append(bo.bounce_ms)
        rays = list(bo.rays)[:nb]
        return dict(max_bounces=nb, trace_ms_median=float(np.median(tms)), light_ms_median=float(np.median(lms)),
                    composite_ms_median=float(np.median(cms)), bounce_ms_median=float(np.median(bms)), bounce_ms_min=float(min(bms)),
                    bounce_ms_max=float(max(bms)), rays=rays, mesh_hits=list(bo.mesh_hits)[:nb], live_fraction=[r / pixels for r in rays],
                    particle_hits=int(bo.particle_hits), shadow_rays=int(lo.shadow_rays))
    out = dict(empty=[run(3), run(16)])
    s = 2.0 * ext
    y = -0.6 * ext
    floor = capi.Mesh.from_arrays(np.float32([[-s, y, s], [s, y, s], [s, y, -s], [-s, y, -s]]), [[0, 1, 2], [0, 2, 3]], np.float32([[0, 1, 0]] * 4), [0, 0],
                                  [capi.make_material(ambient=(0.02, 0.02, 0.02), diffuse=(0.1, 0.1, 0.1), specular=(0.8, 0.8, 0.8), shininess=32.0)])
    inst = scene.add_mesh_instance(floor, None)
    scene.set_mesh_bounce_materials(inst, [capi.bounce_material(illum=1)])
    out["mirror_floor"] = [run(1), run(3)]
    out["note"] = "bounce_ms: the hand-over of bounce 0 (which shades the bouncing pixels again) and max_bounces rounds"
    return out


def camera_frame_size(n, W, H):
    """the frame of the aspect W : H with about n pixels"""
    h = max(int(round((n * H / W) ** 0.5)), 1)
    return max(n // h, 1), h


def probe_rays(scene, p, t, n, eye, W, H, warmup, repeats):
    """the four ray-query runs of --rays for one batch size, and the traced frame the camera batch corresponds to"""
    import torch

    def timed(rays_ptr, count, reorder):
        res = torch.empty(count * 12, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tms, rms = [], []
        for k in range(warmup + repeats):
            _, o = scene.trace_rays((rays_ptr, count), p, t, reorder=reorder, want_stats=True, results=res.data_ptr())
            if k >= warmup:
                tms.append(o.trace.trace_ms)
                rms.append(o.reorder_ms)
        return dict(reorder=int(reorder), rays=count, trace_ms_median=float(np.median(tms)), trace_ms_min=float(min(tms)), trace_ms_max=float(max(tms)),
                    reorder_ms_median=float(np.median(rms)), reorder_ms_min=float(min(rms)), node_visits_per_ray=o.trace.node_visits / count,
                    candidate_tests_per_ray=o.trace.candidate_tests / count, accepted_hits_per_ray=o.trace.accepted_hits / count,
                    invalid_rays=int(o.invalid_rays))

    out = dict(requested=n)
    rnd = torch.from_numpy(random_rays(n, float(np.linalg.norm(eye))).view(np.float32).copy()).cuda()
    out["random"] = [timed(rnd.data_ptr(), n, r) for r in (False, True)]
    w, h = camera_frame_size(n, W, H)
    pc = capi.default_params(w, h)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, w, h)
    capi.set_camera(pc, V, P, eye)
    cam = torch.empty(w * h * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.generate_rays(pc, cam.data_ptr())
    scene.sync()
    out["camera"] = [timed(cam.data_ptr(), w * h, r) for r in (False, True)]
    fms = []
    for k in range(warmup + repeats):
        o = scene.render_traced(pc, t, want_stats=True)
        if k >= warmup:
            fms.append(o.trace_ms)
    out["camera_frame"] = dict(width=w, height=h, trace_ms_median=float(np.median(fms)), trace_ms_min=float(min(fms)), trace_ms_max=float(max(fms)),
                               node_visits_per_ray=o.node_visits / (w * h))
    return out


def probe_shadow_rays(scene, p, t, n, eye, warmup, repeats):
    """the four shadow-query runs of --shadow-rays for one batch size: unit directions toward a point light, t_max = its distance"""
    import torch
    radius = float(np.linalg.norm(eye))
    light = np.array((0.3 * radius, 1.2 * radius, 0.2 * radius))
    rng = np.random.Generator(np.random.PCG64(2))
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    side = max(int(np.ceil(n ** 0.5)), 1)
    g = np.linspace(-radius, radius, side)
    gx, gz = np.meshgrid(g, g)
    batches = dict(random=v * (radius * rng.random((n, 1)) ** (1.0 / 3.0)),
                   coherent=np.stack([gx.ravel(), np.full(side * side, -0.5 * radius), gz.ravel()], 1)[:n])
    lp = capi.default_trace_light_params(shadows_mode=1)
    out = dict(requested=n)
    for name, o in batches.items():
        d = light[None] - o
        dist = np.linalg.norm(d, axis=1)
        dev = torch.from_numpy(capi.make_rays(o, d / dist[:, None], 0.0, dist).view(np.float32).copy()).cuda()
        res = torch.empty(n * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out[name] = []
        for reorder in (False, True):
            tms, rms = [], []
            for k in range(warmup + repeats):
                q = scene.trace_shadow_rays_device(dev.data_ptr(), n, p, res.data_ptr(), t, lp, reorder=reorder, want_stats=True)
                if k >= warmup:
                    tms.append(q.trace.trace_ms)
                    rms.append(q.reorder_ms)
            med = float(np.median(tms))
            out[name].append(dict(reorder=int(reorder), rays=n, trace_ms_median=med, trace_ms_min=float(min(tms)), reorder_ms_median=float(np.median(rms)),
                                  rays_per_second=n / (med * 1e-3) if med > 0 else 0.0, node_visits_per_ray=q.trace.node_visits / n,
                                  accepted_hits_per_ray=q.trace.accepted_hits / n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*")
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--samples-per-pass", type=int, default=18)
    ap.add_argument("--trace-strategy", choices=["full", "pass", "anyhit"], default="full")
    ap.add_argument("--lit", action="store_true")
    ap.add_argument("--hybrid", action="store_true")
    ap.add_argument("--rays", type=int, nargs="+", default=[])
    ap.add_argument("--shadow-rays", type=int, nargs="+", default=[])
    ap.add_argument("--mesh-rays", type=int, nargs="+", default=[])
    ap.add_argument("--mesh", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "meshes", "fixture.obj"))
    ap.add_argument("--trace-meshes", action="store_true")
    ap.add_argument("--hybrid-meshes", action="store_true")  # hybrid frames with mgs_frame_set_hybrid_meshes off and on, on the mesh grid
    ap.add_argument("--indirect", action="store_true")  # with --trace-meshes: MgsTraceBounceOut of mgs_render_traced_indirect
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H = a.size
    if not a.scenes and not a.mesh_rays:
        ap.error("give at least one syn:<n> scene, or --mesh-rays N")
    results = []
    for nr in a.mesh_rays:
        r = dict(mesh_ray_queries=probe_mesh_rays(a.mesh, nr, W, H, a.warmup, a.repeats), repeats=a.repeats, warmup=a.warmup)
        print(json.dumps(r))
        results.append(r)
    for name in a.scenes:
        if not name.startswith("syn:"):
            ap.error("scenes are syn:<n>")
        n = int(name[4:])
        scene = mgs.Scene(0)
        scene.add_instance(mgs.SplatSet.from_arrays(**synth.make_scene(n)))
        scene.commit()
        eye = synth.orbit_pose(5)
        V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
        p = capi.default_params(W, H)
        capi.set_camera(p, V, P, eye)
        t = capi.default_trace_params(samples_per_pass=a.samples_per_pass, trace_strategy=["full", "pass", "anyhit"].index(a.trace_strategy))
        first = scene.render_traced(p, t, want_stats=True)
        for _ in range(a.warmup):
            scene.render_traced(p, t, want_stats=True)
        ms = []
        for _ in range(a.repeats):
            o = scene.render_traced(p, t, want_stats=True)
            ms.append(o.trace_ms)
        rays = W * H
        r = dict(scene=name, width=W, height=H, samples_per_pass=a.samples_per_pass, trace_strategy=a.trace_strategy, splats=n, leaves=int(o.leaves), nodes=int(o.nodes),
                 build_ms=float(first.build_ms), first_trace_ms=float(first.trace_ms), trace_ms_median=float(np.median(ms)),
                 trace_ms_min=float(min(ms)), trace_ms_max=float(max(ms)), repeats=a.repeats, warmup=a.warmup,
                 node_visits_per_ray=o.node_visits / rays, candidate_tests_per_ray=o.candidate_tests / rays,
                 accepted_hits_per_ray=o.accepted_hits / rays, max_passes_used=int(o.max_passes_used),
                 scene_bytes=scene.memory_usage()[0])
        if a.rays:
            if a.trace_strategy != "full":
                ap.error("--rays: ray queries take --trace-strategy full only")
            r["ray_queries"] = [probe_rays(scene, p, t, nr, eye, W, H, a.warmup, a.repeats) for nr in a.rays]
        if a.shadow_rays:
            tq = capi.default_trace_params(samples_per_pass=a.samples_per_pass)
            r["shadow_queries"] = [probe_shadow_rays(scene, p, tq, nr, eye, a.warmup, a.repeats) for nr in a.shadow_rays]
        if a.lit:
            p.lighting_mode = 1
            t.trace_strategy = capi.TRACE_STRATEGY_FULL_ANYHIT
            scene.set_material(0, capi.make_material(ambient=(0.1, 0.1, 0.1), diffuse=(0.8, 0.8, 0.8), emission=(0.0, 0.0, 0.0)))
            spots = [(4.0, 6.0, 3.0), (-5.0, 5.0, 2.0), (2.0, 7.0, -5.0), (-3.0, 4.0, -4.0)]
            r["lit"] = []
            for nl in (0, 1, 4):
                scene.set_lights([capi.make_light(position=q, range=1000.0, attenuation_mode=0) for q in spots[:nl]])
                for shadows in (0, 1):
                    lp = capi.default_trace_light_params(shadows_mode=shadows)
                    lms = []
                    for k in range(a.warmup + a.repeats):
                        _, lo = scene.render_traced_lit(p, t, lp, want_stats=True)
                        if k >= a.warmup:
                            lms.append(lo.light_ms)
                    sr = max(int(lo.shadow_rays), 1)
                    r["lit"].append(dict(lights=nl, shadows=shadows, light_ms_median=float(np.median(lms)), light_ms_min=float(min(lms)),
                                         shadow_rays=int(lo.shadow_rays), node_visits_per_shadow_ray=lo.shadow_node_visits / sr,
                                         candidate_tests_per_shadow_ray=lo.shadow_candidate_tests / sr,
                                         accepted_hits_per_shadow_ray=lo.shadow_accepted_hits / sr))
                    if a.hybrid:  # the same lights over the rasterised (3DGS) surface
                        p.collect_timings = 1
                        hms, fms = [], []
                        for k in range(a.warmup + a.repeats):
                            fo, lo = scene.render_hybrid(p, t, lp, want_stats=True)
                            if k >= a.warmup:
                                hms.append(lo.light_ms)
                                fms.append(fo.stage_ms[5])
                        p.collect_timings = 0
                        sr = max(int(lo.shadow_rays), 1)
                        r["lit"][-1]["hybrid"] = dict(raster_ms_median=float(np.median(fms)), light_ms_median=float(np.median(hms)),
                                                      light_ms_min=float(min(hms)), shadow_rays=int(lo.shadow_rays),
                                                      node_visits_per_shadow_ray=lo.shadow_node_visits / sr,
                                                      candidate_tests_per_shadow_ray=lo.shadow_candidate_tests / sr,
                                                      accepted_hits_per_shadow_ray=lo.shadow_accepted_hits / sr)
            if os.environ.get("MGS_SOFT_SHADOWS", "0") not in ("", "0"):
                # soft against hard (MGS_SHADOWS_SOFT, every light's radius 1.0: a disk of 0.5): the same scene, pose and lights,
                # alternated frame by frame in this process; the sample id advances with the frame as an accumulating caller's does
                r["soft"] = []
                for nl in (1, 4):
                    scene.set_lights([capi.make_light(position=q, range=1000.0, attenuation_mode=0) for q in spots[:nl]])
                    ms, last = {1: [], 2: []}, {}
                    for k in range(a.warmup + a.repeats):
                        p.frame_sample_id = k
                        for mode in (1, 2):
                            _, lo = scene.render_traced_lit(p, t, capi.default_trace_light_params(shadows_mode=mode), want_stats=True)
                            last[mode] = lo
                            if k >= a.warmup:
                                ms[mode].append(lo.light_ms)
                    p.frame_sample_id = 0
                    row = dict(lights=nl, radius=1.0)
                    for mode, tag in ((1, "hard"), (2, "soft")):
                        lo, sr = last[mode], max(int(last[mode].shadow_rays), 1)
                        row[tag] = dict(light_ms_median=float(np.median(ms[mode])), light_ms_min=float(min(ms[mode])), light_ms_max=float(max(ms[mode])),
                                        shadow_rays=int(lo.shadow_rays), node_visits_per_shadow_ray=lo.shadow_node_visits / sr,
                                        candidate_tests_per_shadow_ray=lo.shadow_candidate_tests / sr,
                                        accepted_hits_per_shadow_ray=lo.shadow_accepted_hits / sr)
                    r["soft"].append(row)
            p.lighting_mode = 0
        if a.trace_meshes:
            tq = capi.default_trace_params(samples_per_pass=a.samples_per_pass)
            r["trace_meshes"] = probe_trace_meshes(scene, p, tq, a.mesh, eye, a.warmup, a.repeats, a.indirect)
        if a.hybrid_meshes:
            tq = capi.default_trace_params(samples_per_pass=a.samples_per_pass)
            r["hybrid_meshes"] = probe_hybrid_meshes(scene, p, tq, a.mesh, a.warmup, a.repeats)
        print(json.dumps(r))
        results.append(r)
        scene.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
