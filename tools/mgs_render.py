#!/usr/bin/env python3
"""mgs_render — one frame through the C ABI to .npy / .png (the "tools/mgs_render" caller of SURVEY.md §8b).

  python tools/mgs_render.py scene.ply|scene.spz|scene.splat|syn:<n> out.png [--size W H] [--eye x y z]
                             [--center x y z] [--fov deg] [--flip-y] [--sh-format 0|1|2] [--rgba-format 0|1|2]
                             [--occluder-depth FILE.npy [--background FILE.npy]]
                             [--mesh FILE.obj [--mesh-transform 16 floats]]... [--lighting 1 --mesh-shadows 1]
                             [--lighting 0|1 [--lights FILE.json] [--material a a a d d d s s s e e e shininess]]
                             [--pipeline raster|trace|hybrid [--samples-per-pass N --max-passes N --min-transmittance X]
                              [--lighting 1 [--shadows 1] [--shadow-offset X --shadow-threshold X --shadow-color-strength X]]]
                             [--raster-pipeline 3dgs|3dgut]
                             [--compare-with FRAME.npy [--flip-mode 0|1|2] [--compare-view OUT.png --split 0.5 --left capture --right diff-red-gray]]

--occluder-depth: float32 [H, W] window depth of opaque geometry rasterised with the same camera (1.0 = none); the splats are
depth-tested against it (z <= depth).  --background: float32 [H, W, 4] linear colour of that geometry, shown through the splats.

--lighting 1: deferred direct lighting of the splat surface (MgsFrameParams.lighting_mode).  --lights: a JSON list of light dicts
with the field names of MgsLight (type, color, intensity, position, range, direction, inner_cone_deg, outer_cone_deg,
attenuation_mode; absent fields keep the reference's defaults); without it the headlight at the camera lights the scene.
--material: ambient, diffuse, specular, emission (rgb each) and shininess of the single instance (default: fully emissive).

--mesh ... --lighting 1 --mesh-shadows 1 (raster pipelines): after the mesh pass every mesh pixel is lit with the scene's lights and
shadowed by the splats (mgs_shade_points_device: position from the mesh depth, flat normal and material of the pixel's primitive,
--shadow-* and --samples-per-pass as for the traced frames), the result replaces the occluder's colour image, and the splats are
rendered over it: a mesh floor under a splat object shows the object's shadow.  Needs torch for the device images.

--pipeline trace --lighting 1 [--shadows 1]: a lit traced frame (mgs_render_traced_lit), --lights / --material as for the raster pipelines.
--pipeline hybrid --lighting 1 [--shadows 1]: a hybrid frame (mgs_render_hybrid): the rasterised frame of --raster-pipeline as the
primary surface, lit and shadowed by the traced light pass; --lights / --material / --shadow-* as above, --samples-per-pass of the
shadow rays.  Not combinable with --occluder-depth or --mesh.  --raster-pipeline: 3DGS (default) or 3DGUT, of --pipeline raster and hybrid.
--pipeline trace: the ray-traced pipeline (mgs_render_traced: 3DGRT primary rays over the scene's device-built hierarchy) instead of
the raster one; prints MgsTraceOut.  Not combinable with --occluder-depth.
--pipeline hybrid --lighting 1 --mesh FILE.obj --hybrid-meshes 1 [--mesh-composite-threshold T]: the meshes take part in the hybrid frame
(mgs_frame_set_hybrid_meshes): a traced mesh depth pre-pass in front of the raster frame, splats and meshes shadowing each other.
--pipeline trace --mesh FILE.obj [--lighting 1 --shadows 1]: the meshes take part in the traced frame (mgs_frame_set_trace_meshes): mesh
hits cut the particle walk, meshes are shaded and throw and receive shadows; prints both MgsMeshRayOut blocks.  --trace-meshes 0 leaves
the setting off (the frame of the splats alone); --mesh-composite-threshold X is min_mesh_composite_transmittance.
--trace-strategy full|pass|anyhit: MgsTraceParams::trace_strategy of an unlit traced frame (sorted passes, pass-stochastic, stochastic
any-hit); --accumulate N renders the samples frame_sample_id = 0..N-1 with temporal accumulation and writes the last, the running mean.

--compare-with: float32 [H, W, 3|4] frame made elsewhere (a reference screenshot, another build's frame), uploaded as the capture;
prints MSE / PSNR / FLIP of the rendered frame against it, computed on the device (mgs_compare_metrics).  --compare-view writes
the split view (left | right of --split; modes capture, current, diff-raw, diff-red-gray, diff-red-only, flip).

PNG = linear RGB clamped to [0,1] over a black background, 8 bit, no tonemap — like the reference's
screenshot path (gaussian_splatting_ui.cpp:508-540).  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402


def shade_mesh_pixels(scene, meshes, p, V, P, a):
    """--mesh-shadows 1: light the mesh pixels of the last mesh pass with the scene's light table and shadow them by the splats
    (mgs_shade_points_device), then bind the mesh depth and the new colours as the occluder (mgs_frame_set_occluder).  Positions are
    rebuilt from the mesh depth through the inverse of proj * view; the mesh pass exposes no normals, so they are flat: the face
    normal of the pixel's primitive from the mesh arrays, turned toward the viewer (the pass draws both windings).  The material is
    the primitive's, radiance is 1 (a mesh's colour is its material).  Returns the device images: the caller keeps them alive."""
    import torch
    W, H = p.width, p.height
    depth, _, prim = scene.download_meshes()
    rows, cols = np.nonzero(prim != capi.MESH_NONE)
    face_n, face_m, mats = [], [], []
    for mesh, M in meshes:  # primitive ids are global: the instances' triangles concatenated in creation order
        v = mesh.view()
        M = np.eye(4) if M is None else np.asarray(M, np.float64)
        tri = (v["positions"].astype(np.float64) @ M[:3, :3].T + M[:3, 3])[v["indices"]]
        face_n.append(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
        own = v["materials"] or [dict(ambient=(0.1,) * 3, diffuse=(0.7,) * 3, specular=(1.0,) * 3, emission=(0.0,) * 3, shininess=32.0)]  # the loader's default
        face_m.append(len(mats) + np.minimum(v["material_ids"], len(own) - 1))
        mats += own
    if len(mats) > 256:
        raise SystemExit("--mesh-shadows: the meshes hold more than 256 materials (mgs_shade_points takes 1 to 256)")
    face_n, face_m = np.concatenate(face_n), np.concatenate(face_m)
    depth_dev = torch.from_numpy(depth).cuda()
    color_dev = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    if len(rows):
        ndc = np.stack([(cols + 0.5) / W * 2 - 1, (rows + 0.5) / H * 2 - 1, depth[rows, cols].astype(np.float64), np.ones(len(rows))], 1)  # row 0 = NDC y -1
        world = ndc @ np.linalg.inv(np.asarray(P, np.float64) @ np.asarray(V, np.float64)).T
        pos = world[:, :3] / world[:, 3:4]
        view = pos - np.asarray(a.eye, np.float64)[None]
        view /= np.linalg.norm(view, axis=1, keepdims=True)
        nrm = face_n[prim[rows, cols]]
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
        nrm[(nrm * view).sum(1) > 0] *= -1.0
        pts = capi.make_surface_points(pos, nrm, view, np.ones_like(pos), face_m[prim[rows, cols]])
        pts_dev = torch.from_numpy(pts.view(np.float32).reshape(-1)).cuda()
        res_dev = torch.zeros(len(rows) * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the query runs on the handle's stream
        q = capi.default_params(W, H)
        capi.set_camera(q, V, P, a.eye)
        lp = capi.default_trace_light_params(shadows_mode=1, particle_shadow_offset=a.shadow_offset,
                                             particle_shadow_transmittance_threshold=a.shadow_threshold,
                                             particle_shadow_color_strength=a.shadow_color_strength)
        lo, bad = scene.shade_points_device(pts_dev.data_ptr(), len(rows), mats, q, res_dev.data_ptr(),
                                            capi.default_trace_params(samples_per_pass=a.samples_per_pass), lp, reorder=True, want_stats=True)
        sr = max(int(lo.shadow_rays), 1)
        print(f"{len(rows)} mesh pixels shaded ({bad} invalid), light query {lo.light_ms:.3f} ms on the GPU, {lo.shadow_rays} shadow rays, "
              f"{lo.shadow_node_visits / sr:.1f} node visits and {lo.shadow_accepted_hits / sr:.2f} hits per shadow ray")
        at = (torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda())
        color_dev[at[0], at[1], :3] = res_dev.view(-1, 4)[:, :3]
        color_dev[at[0], at[1], 3] = 1.0
        torch.cuda.synchronize()
    scene.set_occluder(depth_dev.data_ptr(), color_dev.data_ptr(), W, H)
    return depth_dev, color_dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--eye", type=float, nargs=3, default=[1.7, 1.5, 1.7])   # camera_set.h:48-53
    ap.add_argument("--center", type=float, nargs=3, default=[0, 0, 0])
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--flip-y", action="store_true")
    ap.add_argument("--sh-format", type=int, default=0)
    ap.add_argument("--rgba-format", type=int, default=0)
    ap.add_argument("--occluder-depth", default=None, metavar="FILE.npy")
    ap.add_argument("--background", default=None, metavar="FILE.npy")
    ap.add_argument("--mesh", action="append", default=[], metavar="FILE.obj")
    ap.add_argument("--mesh-transform", action="append", type=float, nargs=16, default=[], metavar="M")
    ap.add_argument("--mesh-pick-image", default=None, metavar="OUT.npy")  # --mesh: closest-hit global primitive ids of the primary rays (mgs_trace_mesh_rays_device)
    ap.add_argument("--mesh-shadows", type=int, choices=[0, 1], default=0)  # --mesh --lighting 1: the splats' shadows on the meshes
    ap.add_argument("--trace-meshes", type=int, choices=[0, 1], default=1)  # --pipeline trace --mesh: mgs_frame_set_trace_meshes
    ap.add_argument("--hybrid-meshes", type=int, choices=[0, 1], default=0)  # --pipeline hybrid --mesh: mgs_frame_set_hybrid_meshes
    ap.add_argument("--mesh-composite-threshold", type=float, default=0.0)
    ap.add_argument("--lighting", type=int, choices=[0, 1, 2], default=0)  # 2: --pipeline trace --mesh, mgs_render_traced_indirect
    ap.add_argument("--max-bounces", type=int, default=3)  # --lighting 2
    # --lighting 2: illum ior tf tf tf for every material of the k-th --mesh (illum: the derived model 0 / 1 / 2) in place of what its MTL says
    ap.add_argument("--mesh-bounce", action="append", type=float, nargs=5, default=[], metavar="B")
    ap.add_argument("--lights", default=None, metavar="FILE.json")
    ap.add_argument("--material", type=float, nargs=13, default=None)
    ap.add_argument("--pipeline", choices=["raster", "trace", "hybrid"], default="raster")  # hybrid: the raster surface lit with traced shadow rays
    ap.add_argument("--raster-pipeline", choices=["3dgs", "3dgut"], default="3dgs")  # of --pipeline raster and hybrid
    # --sensor FILE.json with --pipeline raster --raster-pipeline 3dgut: a flat JSON of MgsSensorModel's fields (model, focal_length,
    # principal_point, radial, tangential, thin_prism, fisheye_radial, max_angle); fields left out keep the frame's perfect camera
    ap.add_argument("--sensor", default=None, metavar="FILE.json")
    # --pipeline trace / hybrid --lighting 1: 1 = hard shadow rays through the splats, 2 = soft (one disk sample per light and frame:
    # converge with --accumulate N)
    ap.add_argument("--shadows", type=int, choices=[0, 1, 2], default=0)
    # --shadows 2 with --lights: one radius for every light, in place of the file's "radius" keys (without it: those keys, else 1.0)
    ap.add_argument("--light-radius", type=float, default=None, metavar="R")
    ap.add_argument("--shadow-offset", type=float, default=0.2)
    ap.add_argument("--shadow-threshold", type=float, default=0.8)
    ap.add_argument("--shadow-color-strength", type=float, default=0.0)
    ap.add_argument("--samples-per-pass", type=int, default=18)
    ap.add_argument("--max-passes", type=int, default=200)
    ap.add_argument("--trace-strategy", choices=["full", "pass", "anyhit"], default="full")
    ap.add_argument("--accumulate", type=int, default=1, metavar="N")
    ap.add_argument("--min-transmittance", type=float, default=0.01)
    ap.add_argument("--compare-with", default=None, metavar="FRAME.npy")
    ap.add_argument("--flip-mode", type=int, choices=[0, 1, 2], default=capi.FLIP_REFERENCE)
    ap.add_argument("--compare-view", default=None, metavar="OUT.png")
    ap.add_argument("--split", type=float, default=0.5)
    ap.add_argument("--left", choices=sorted(capi.SHOW_NAMES), default="capture")
    ap.add_argument("--right", choices=sorted(capi.SHOW_NAMES), default="current")
    a = ap.parse_args()
    if a.compare_view and not a.compare_with:
        ap.error("--compare-view needs --compare-with")
    if a.scene.startswith("syn:"):
        ss = mgs.SplatSet.from_arrays(**synth.make_scene(int(a.scene[4:])))
    else:
        ss = mgs.SplatSet.load(a.scene)
    scene = mgs.Scene(0)
    scene.add_instance(ss)
    scene.commit(a.sh_format, a.rgba_format)
    W, H = a.size
    V, P = mgs.camera_lookat_perspective(a.eye, a.center, [0, 1, 0], a.fov, 0.1, 2000.0, W, H, flip_y=a.flip_y)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, a.eye)
    p.collect_timings = 1
    if a.pipeline != "trace":
        p.pipeline = capi.PIPELINE_3DGUT if a.raster_pipeline == "3dgut" else capi.PIPELINE_3DGS
    if a.sensor:
        if a.pipeline != "raster" or a.raster_pipeline != "3dgut" or a.lighting or a.mesh:
            ap.error("--sensor needs --pipeline raster --raster-pipeline 3dgut without --lighting and --mesh (mgs_frame_set_sensor)")
        import json
        with open(a.sensor) as f:
            scene.set_sensor(capi.sensor_model_from_frame(p).update(**json.load(f)))
    if a.pipeline == "hybrid" and (a.occluder_depth or (a.mesh and not a.hybrid_meshes)):
        ap.error("--pipeline hybrid takes no --occluder-depth, and --mesh only with --hybrid-meshes 1 (the traced mesh depth pre-pass)")
    if a.hybrid_meshes and not (a.pipeline == "hybrid" and a.mesh):
        ap.error("--hybrid-meshes 1 needs --pipeline hybrid and --mesh")
    if a.hybrid_meshes and a.shadows == 2:
        ap.error("--hybrid-meshes 1 has hard shadows only (--shadows 1)")
    if a.pipeline == "hybrid" and not a.lighting:
        ap.error("--pipeline hybrid needs --lighting 1 (without lighting it is --pipeline raster)")
    if a.mesh_shadows and not (a.mesh and a.lighting and a.pipeline == "raster"):
        ap.error("--mesh-shadows 1 needs --mesh, --lighting 1 and --pipeline raster")
    if a.background and not a.occluder_depth:
        ap.error("--background needs --occluder-depth")
    if a.occluder_depth:
        depth = np.load(a.occluder_depth)
        back = np.load(a.background) if a.background else None
        if depth.shape != (H, W) or (back is not None and back.shape != (H, W, 4)):
            ap.error(f"--occluder-depth must be [{H}, {W}] and --background [{H}, {W}, 4]")
        scene.upload_occluder(depth, back)
    if (a.lights or a.material) and not a.lighting:
        ap.error("--lights / --material need --lighting 1")
    if a.lighting == 2 and not (a.pipeline == "trace" and a.mesh and a.trace_meshes):
        ap.error("--lighting 2 needs --pipeline trace and --mesh (bounces off mesh materials, mgs_render_traced_indirect)")
    if a.lighting:
        p.lighting_mode = capi.LIGHTING_DIRECT if a.lighting == 1 else 2  # MGS_LIGHTING_INDIRECT
        if a.lights:
            import json
            with open(a.lights) as f:
                lights = json.load(f)  # MgsLight's fields, and "radius" for the soft shadows' disk
            scene.set_lights([capi.make_light(**l) for l in lights])
            if a.light_radius is not None:  # --light-radius wins over the file's "radius" keys
                print(f"--light-radius {a.light_radius}: replaces the radius of all {len(lights)} lights of {a.lights}")
                scene.set_light_radii([a.light_radius] * len(lights))
        elif a.light_radius is not None:
            ap.error("--light-radius needs --lights (without lights the frame has the headlight, which is never shadowed)")
        if a.material:
            m = a.material
            scene.set_material(0, capi.make_material(ambient=m[0:3], diffuse=m[3:6], specular=m[6:9], emission=m[9:12], shininess=m[12]))
    if a.mesh:
        # --mesh FILE.obj [--mesh-transform 16 floats, row by row]: rasterised on the device into this handle's occluder (mgs_meshes_render)
        if a.occluder_depth:
            ap.error("--mesh makes the occluder images itself: do not combine it with --occluder-depth")
        if len(a.mesh_transform) > len(a.mesh):
            ap.error("more --mesh-transform than --mesh")
        meshes = []
        for k, path in enumerate(a.mesh):
            m = np.array(a.mesh_transform[k], np.float32).reshape(4, 4) if k < len(a.mesh_transform) else None
            meshes.append((mgs.Mesh.load_obj(path), m))
            inst = scene.add_mesh_instance(*meshes[-1])
            if a.lighting == 2:  # bounce materials: the OBJ's MTL (Tf / Ni / illum), or --mesh-bounce for all of this mesh's materials
                bm = meshes[-1][0].bounce_materials()
                if k < len(a.mesh_bounce):
                    b = a.mesh_bounce[k]
                    bm = [capi.bounce_material(b[2:5], b[1], int(b[0])) for _ in bm]
                scene.set_mesh_bounce_materials(inst, bm)
    if a.mesh and a.pipeline == "trace":
        # the meshes are traced with the splats: no mesh pass, no occluder (a traced frame refuses a bound one)
        if a.mesh_pick_image:
            ap.error("--mesh-pick-image is for the raster pipelines (a traced frame's hits are mgs_trace_download_mesh_hits)")
        scene.set_trace_meshes(bool(a.trace_meshes), a.mesh_composite_threshold)
    elif a.mesh and a.pipeline == "hybrid":
        # the frame traces its own mesh depth pre-pass: no mesh pass, no caller's occluder (a hybrid frame refuses a bound one)
        if a.mesh_pick_image:
            ap.error("--mesh-pick-image is for the raster pipelines (a hybrid frame's hits are mgs_trace_download_mesh_hits)")
        scene.set_hybrid_meshes(True, a.mesh_composite_threshold)
    elif a.mesh:
        mo = scene.render_meshes(p, want_stats=True)
        print(f"{mo.triangles_in} triangles, {mo.triangles_rasterised} rasterised, {mo.fragments} fragments, {mo.elapsed_ms:.3f} ms on the GPU")
        if a.mesh_pick_image:
            # the frame's primary rays (mgs_trace_generate_rays) against the meshes: uint32 [H, W], 0xFFFFFFFF = nothing hit
            import torch
            rays = torch.empty(p.width * p.height * 8, dtype=torch.float32, device="cuda")
            hits = torch.empty(p.width * p.height * 16, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            scene.generate_rays(p, rays.data_ptr())
            ro = scene.trace_mesh_rays_device(rays.data_ptr(), p.width * p.height, hits.data_ptr(), want_stats=True)
            pick = hits.cpu().numpy().view(capi.MESH_HIT_DTYPE)["primitive_id"].reshape(p.height, p.width)
            np.save(a.mesh_pick_image, pick)
            print(f"mesh pick image: {ro.hits} of {p.width * p.height} rays hit, {ro.leaves} leaves, build {ro.build_ms:.3f} ms, trace {ro.trace_ms:.3f} ms")
        if a.mesh_shadows:
            held = shade_mesh_pixels(scene, meshes, p, V, P, a)  # the occluder's images: keep them until the frame is downloaded
    soft = a.lighting == 1 and a.shadows == 2 and a.pipeline in ("trace", "hybrid")
    if a.shadows == 2 and not soft:
        ap.error("--shadows 2 needs --lighting 1 with --pipeline trace or hybrid")
    if soft and os.environ.get("MGS_SOFT_SHADOWS", "0") in ("", "0"):
        ap.error("--shadows 2: soft shadows are opt-in per process, run with MGS_SOFT_SHADOWS=1")
    if (a.pipeline != "trace" and a.trace_strategy != "full") or (a.accumulate != 1 and not (a.pipeline == "trace" and not a.lighting) and not soft):
        ap.error("--trace-strategy pass / anyhit are for --pipeline trace (unlit); --accumulate for that and for --shadows 2")
    if a.pipeline == "trace":
        if a.occluder_depth:
            ap.error("--pipeline trace takes no --occluder-depth (meshes: --mesh)")
        if a.mesh and a.trace_meshes and a.trace_strategy != "full":
            ap.error("--pipeline trace --mesh needs --trace-strategy full (or --trace-meshes 0)")
        p.collect_timings = 0
        t = capi.default_trace_params(samples_per_pass=a.samples_per_pass, max_passes=a.max_passes, min_transmittance=a.min_transmittance,
                                      trace_strategy=["full", "pass", "anyhit"].index(a.trace_strategy))
        if a.lighting and t.trace_strategy:
            ap.error("--trace-strategy pass / anyhit are for unlit traced frames")
        if a.lighting:  # mgs_render_traced_lit: --lights / --material as for the raster pipelines, shadows by one more ray per light
            lp = capi.default_trace_light_params(shadows_mode=a.shadows, particle_shadow_offset=a.shadow_offset,
                                                 particle_shadow_transmittance_threshold=a.shadow_threshold,
                                                 particle_shadow_color_strength=a.shadow_color_strength)
            if a.lighting == 2:
                o, lo, bo = scene.render_traced_indirect(p, t, lp, a.max_bounces, want_stats=True)
                print(f"bounces {bo.bounce_ms:.3f} ms on the GPU, live pixels per bounce {list(bo.rays)[:a.max_bounces]}, mesh hits "
                      f"{list(bo.mesh_hits)[:a.max_bounces]}, {bo.particle_hits} particle hits")
            else:
                for k in range(max(a.accumulate, 1)):  # soft shadows: the running mean of the samples is the frame after the last
                    if a.accumulate > 1:
                        p.frame_sample_id, p.temporal_sampling = k, 1
                    o, lo = scene.render_traced_lit(p, t, lp, want_stats=True)
            sr = max(int(lo.shadow_rays), 1)
            print(f"light pass {lo.light_ms:.3f} ms on the GPU, {lo.shadow_rays} shadow rays, {lo.shadow_node_visits / sr:.1f} node visits, "
                  f"{lo.shadow_candidate_tests / sr:.1f} candidate tests and {lo.shadow_accepted_hits / sr:.2f} hits per shadow ray")
        else:
            for k in range(max(a.accumulate, 1)):  # the running mean of the samples is the frame after the last
                if a.accumulate > 1:
                    p.frame_sample_id, p.temporal_sampling = k, 1
                o = scene.render_traced(p, t, want_stats=True)
        img = scene.download_frame(p).astype(np.float32)
        if a.mesh and a.trace_meshes:
            pm, sm = scene.trace_mesh_stats()
            print(f"meshes: {pm.triangles} triangles, {pm.leaves} leaves (build {pm.build_ms:.3f} ms); primary rays: {pm.hits} hits, "
                  f"{pm.triangle_tests} triangle tests, {pm.trace_ms:.3f} ms; occlusion rays: {sm.hits} occluded, {sm.triangle_tests} triangle tests, "
                  f"mesh composite {sm.trace_ms:.3f} ms")
        rays = W * H
        print(f"{scene.splat_count} splats, {o.leaves} leaves in {o.nodes} nodes (build {o.build_ms:.3f} ms), {o.node_visits / rays:.1f} node visits and "
              f"{o.candidate_tests / rays:.1f} candidate tests per ray, {o.accepted_hits / rays:.1f} hits per ray, at most {o.max_passes_used} passes, "
              f"{o.trace_ms:.3f} ms on the GPU")
    elif a.pipeline == "hybrid":  # mgs_render_hybrid: the frame of --raster-pipeline as the primary surface, then the traced light pass
        t = capi.default_trace_params(samples_per_pass=a.samples_per_pass)
        lp = capi.default_trace_light_params(shadows_mode=a.shadows, particle_shadow_offset=a.shadow_offset,
                                             particle_shadow_transmittance_threshold=a.shadow_threshold,
                                             particle_shadow_color_strength=a.shadow_color_strength)
        for k in range(max(a.accumulate, 1)):
            if a.accumulate > 1:
                p.frame_sample_id, p.temporal_sampling = k, 1
            o, lo = scene.render_hybrid(p, t, lp, want_stats=True)
        img = scene.download_frame(p).astype(np.float32)
        sr = max(int(lo.shadow_rays), 1)
        print(f"{scene.splat_count} splats, {o.sorted_count} sorted, raster frame {o.stage_ms[5]:.3f} ms and light pass {lo.light_ms:.3f} ms on the GPU, "
              f"{lo.shadow_rays} shadow rays, {lo.shadow_node_visits / sr:.1f} node visits, {lo.shadow_candidate_tests / sr:.1f} candidate tests and "
              f"{lo.shadow_accepted_hits / sr:.2f} hits per shadow ray")
        if a.hybrid_meshes:
            pm, sm = scene.trace_mesh_stats()
            print(f"meshes: {pm.triangles} triangles, {pm.leaves} leaves (build {pm.build_ms:.3f} ms); depth pre-pass: {pm.hits} hits, "
                  f"{pm.triangle_tests} triangle tests, {pm.trace_ms:.3f} ms; occlusion rays: {sm.hits} occluded, {sm.triangle_tests} triangle tests, "
                  f"mesh composite {sm.trace_ms:.3f} ms")
    else:
        o = scene.render(p)
        img = scene.download_frame(p).astype(np.float32)
        print(f"{scene.splat_count} splats, {o.frustum_count} in frustum, {o.sorted_count} sorted, {o.tile_pairs} bin records, "
              f"{o.stage_ms[5]:.3f} ms on the GPU" + (f" ({o.stage_ms[capi.STAGE_LIGHT]:.3f} ms lighting)" if a.lighting else ""))
    if a.out.endswith(".npy"):
        np.save(a.out, img)
    else:
        from PIL import Image
        rgb = np.clip(img[..., :3], 0, 1)
        Image.fromarray((rgb * 255 + 0.5).astype(np.uint8)).save(a.out)
    if a.compare_with:
        scene.compare_capture_upload(np.load(a.compare_with))
        m = scene.compare_metrics(a.flip_mode)
        print(f"against {a.compare_with}: as the reference computes it MSE {m.mse:.6g} PSNR {m.psnr:.2f} dB FLIP {m.flip:.5f}; "
              f"exact MSE {m.mse_exact:.6g} PSNR {m.psnr_exact:.2f} dB FLIP {m.flip_exact:.5f}; {m.elapsed_ms:.3f} ms on the GPU")
        if a.compare_view:
            view = scene.compare_composite(split=a.split, left=a.left, right=a.right)
            if a.compare_view.endswith(".npy"):
                np.save(a.compare_view, view)
            else:
                from PIL import Image
                Image.fromarray((np.clip(view[..., :3], 0, 1) * 255 + 0.5).astype(np.uint8)).save(a.compare_view)


if __name__ == "__main__":
    main()
