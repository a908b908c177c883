"""child process of test_gpu_mesh_rays.py: mesh ray queries in a fresh process.   usage: _child_mesh_rays.py MODE OUT.npz
MODE cases:      every batch of mesh_ray_cases.py (camera rays from mgs_trace_generate_rays): closest and occlusion, reorder off and on,
                 the host variant, a frame context
MODE watertight: the integer grid under the identity and under an integer translation
MODE lifecycle:  rebuild flags, visibility, an empty scene, memory, the pick image next to the mesh pass, and a traced frame, a shadow
                 query and a mesh pass before and after mesh queries on one handle"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import mesh_cases as mc  # noqa: E402
import mesh_ray_cases as mrc  # noqa: E402
import trace_cases as tc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
STATS = ("triangles", "leaves", "nodes", "node_visits", "triangle_tests", "hits", "invalid_rays", "bvh_rebuilt")
keep = []  # the Mesh objects stay alive as long as the scenes


def add_meshes(scene, meshes):
    ids = []
    for m in meshes:
        # (material ids at or above the material count are clamped to 0 by the loader's rule: give the cases' ids their materials)
        mats = m.get("materials") or [capi.make_material(shininess=8.0 + k) for k in range(mrc.MATERIALS)]
        mats = [capi.make_material(**x) if isinstance(x, dict) else x for x in mats]   # (Mesh.view() returns dicts)
        h = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m.get("material_ids"), mats)
        keep.append(h)
        i = scene.add_mesh_instance(h, m.get("transform"))
        if not m.get("visible", True):
            scene.set_mesh_visible(i, False)
        ids.append(i)
    return ids


def on_device(rays):
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).copy()).cuda()


def query(handle, rays, mode=capi.MESH_RAYS_CLOSEST, reorder=False):
    """mgs_trace_mesh_rays_device with a sentinel behind the hits; -> (hits, stats dict, sentinel untouched)"""
    n = rays.shape[0]
    dev = on_device(rays)
    res = torch.full(((n + 2) * 16,), -7.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o = handle.trace_mesh_rays_device(dev.data_ptr(), n, res.data_ptr(), mode=mode, reorder=reorder, want_stats=True)
    h = res.cpu().numpy()
    return h[:n * 16].view(capi.MESH_HIT_DTYPE), o.as_dict(), bool((h[n * 16:] == np.float32(-7.25)).all())


def generated(scene, V, P, W, H, fisheye=False, fov=0.0):
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, np.linalg.inv(np.asarray(V, np.float64))[:3, 3].astype(np.float32))
    p.camera_model, p.fov_rad = int(fisheye), float(fov)
    dev = torch.zeros(W * H * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.generate_rays(p, dev.data_ptr())
    scene.sync()
    r = dev.cpu().numpy().view(capi.RAY_DTYPE)
    return r["origin"].copy(), r["direction"].copy(), r["t_min"].copy(), r["t_max"].copy()


res = {}
if mode == "cases":
    scenes, made = mrc.scenes(), {}
    for name, (sname, parts) in mrc.batches().items():
        if sname not in made:
            made[sname] = mgs.Scene(0)
            add_meshes(made[sname], scenes[sname])
        scene = made[sname]
        gen = {p: generated(scene, *mrc.cameras()[p]) for p in parts if isinstance(p, str)}
        O, D, tmin, tmax = mrc.rays_of(name, gen)
        rays = capi.make_rays(O, D, tmin, tmax)
        res[name + "_rays"] = rays
        for md, tag in ((capi.MESH_RAYS_CLOSEST, "closest"), (capi.MESH_RAYS_OCCLUSION, "occlusion")):
            for reorder in (0, 1):
                h, o, clean = query(scene, rays, md, bool(reorder))
                res[f"{name}_{tag}_{reorder}"] = h
                res[f"{name}_{tag}_{reorder}_stats"] = np.array([o[k] for k in STATS], np.int64)
                res[f"{name}_{tag}_{reorder}_sentinel"] = clean
        host, ho = scene.trace_mesh_rays(rays, want_stats=True)
        res[name + "_host"] = host
        res[name + "_host_stats"] = np.array([ho.as_dict()[k] for k in STATS], np.int64)
        ctx = scene.frame_context()
        res[name + "_context"], _, _ = query(ctx, rays)
        ctx.close()
    for s in made.values():
        s.close()
elif mode == "watertight":
    for tag, shift in (("identity", None), ("translated", mrc.WT_SHIFT)):
        scene = mgs.Scene(0)
        add_meshes(scene, [mrc.watertight_mesh(shift)])
        O, D, tmin, tmax, _, _ = mrc.watertight_rays(shift)
        for reorder in (0, 1):
            res[f"{tag}_{reorder}"], _, _ = query(scene, capi.make_rays(O, D, tmin, tmax), reorder=bool(reorder))
        res[tag + "_occlusion"], _, _ = query(scene, capi.make_rays(O, D, tmin, tmax), capi.MESH_RAYS_OCCLUSION)
        scene.close()
else:
    # ---- lifecycle on a scene with meshes and no splats
    meshes = mrc.scenes()["mid"]
    O, D, tmin, tmax = mrc.rays_of("mid_257")
    rays = capi.make_rays(O, D, tmin, tmax)
    empty = mgs.Scene(0)
    h, o, _ = query(empty, rays)
    res["empty_hits"], res["empty_stats"] = h, np.array([o[k] for k in STATS], np.int64)
    empty.close()
    scene = mgs.Scene(0)
    m0 = scene.memory_usage()[0]
    ids = add_meshes(scene, meshes[:3])
    m1 = scene.memory_usage()[0]
    h1, o1, _ = query(scene, rays)
    m2 = scene.memory_usage()[0]
    h2, o2, _ = query(scene, rays)
    res["first"], res["second"] = h1, h2
    res["rebuilt"] = np.array([o1["bvh_rebuilt"], o2["bvh_rebuilt"]])
    res["scene_bytes"] = np.array([m0, m1, m2, scene.memory_usage()[0]], np.int64)
    res["bvh_bytes_expected"] = 32 * o1["nodes"] + 48 * o1["leaves"]
    scene.set_mesh_visible(ids[2], False)                       # the enclosing box
    h3, o3, _ = query(scene, rays)
    res["hidden"], res["hidden_rebuilt"] = h3, o3["bvh_rebuilt"]
    scene.set_mesh_visible(ids[2], True)
    scene.set_mesh_transform(ids[1], mrc.SHIFTED)
    h4, o4, _ = query(scene, rays)
    res["moved"], res["moved_rebuilt"] = h4, o4["bvh_rebuilt"]
    add_meshes(scene, [dict(meshes[3], visible=True)])
    h5, o5, _ = query(scene, rays)
    res["added"], res["added_rebuilt"], res["added_triangles"] = h5, o5["bvh_rebuilt"], o5["triangles"]
    scene.close()
    # ---- the pick image next to the mesh pass
    scene = mgs.Scene(0)
    fx = mc.fixture_meshes(capi.Mesh.load_obj(mc.FIXTURE).view())
    add_meshes(scene, fx)
    V, P, eye = mrc.raster_camera()
    p = capi.default_params(mrc.RW, mrc.RH)
    capi.set_camera(p, V, P, eye)
    scene.render_meshes(p, want_stats=True)
    res["raster_prim"] = scene.download_meshes()[2]
    g = generated(scene, V, P, mrc.RW, mrc.RH)
    res["pick_rays"] = capi.make_rays(*g)
    res["pick"], _, _ = query(scene, res["pick_rays"])
    scene.close()
    # ---- a traced frame, a shadow query and a mesh pass before and after mesh queries, on one handle with splats and meshes
    case = tc.cases()["two_instances"] if "two_instances" in tc.cases() else list(tc.cases().values())[0]
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit()
    add_meshes(scene, meshes[:2])
    W, H = 40, 24
    pf = capi.default_params(W, H)
    capi.set_camera(pf, case["V"], tc.persp(50.0, W / H), case["eye"])
    pf.target_format, pf.surface_outputs = capi.TARGET_RGBA32F, 1
    srays = capi.make_rays(O[:200], D[:200], 0.0, 50.0)

    def snapshot():
        scene.clear_occluder()   # (the mesh pass binds its images as the occluder, which a traced frame refuses)
        scene.render_traced(pf, None, want_stats=True)
        frame = (scene.download_frame(pf), scene.trace_hit_counts(pf)) + scene.download_surface(pf, normals=True)
        shadow = scene.trace_shadow_rays(srays, pf)
        scene.render_meshes(pf, want_stats=True)
        return frame + (shadow,) + scene.download_meshes()

    before = snapshot()
    frame_kept = (scene.download_frame(pf), scene.trace_hit_counts(pf))
    mq, _, _ = query(scene, rays)
    query(scene, rays, capi.MESH_RAYS_OCCLUSION, True)
    held = (scene.download_frame(pf), scene.trace_hit_counts(pf))       # the handle's frame, untouched by the queries
    res["frame_held"] = all(a.tobytes() == b.tobytes() for a, b in zip(frame_kept, held))
    res["mesh_images_held"] = all(a.tobytes() == b.tobytes() for a, b in zip(before[-3:], scene.download_meshes()))
    after = snapshot()
    res["unchanged"] = all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and bool(before[0].any()) and bool((before[-1] != 0xFFFFFFFF).any())
    res["mixed_hits"] = int(mq["hit"].sum())
    scene.close()
np.savez(out, **res)
print("child ok")
