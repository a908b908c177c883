"""child process of test_gpu_trace_mesh.py: traced frames with mesh hits in a fresh process.   usage: _child_trace_mesh.py MODE OUT.npz
MODE cases:     every case of trace_mesh_cases.py: frame (RGBA32F), hit counts, side outputs, shadow hits, hit records, statistics
MODE storage:   u1 and l1 with fp16 and uint8 splat storage: the frame, and the quantised arrays as the device holds them
MODE exact:     u1 and u5: the frame's hit records and primary statistics next to the mesh ray query on the generated rays, and the
                unlit composite next to the ray query cut at the mesh
MODE lit:       l1 and l3: lit frames with and without shadows, the mesh points under mgs_shade_points, both statistics blocks
MODE unmoved:   setting off / every instance invisible against the scene without meshes; strips; a frame context; target formats;
                mgs_render and the mesh query before and after
MODE lifecycle: rebuilds, visibility, working_bytes, the error codes"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import trace_mesh_cases as tmc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
STATS = ("triangles", "leaves", "nodes", "node_visits", "triangle_tests", "hits", "invalid_rays")
keep = []


def build(case, meshes=True, storage=None):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    if case["sets"]:
        scene.commit(*((storage, storage) if storage is not None else ()))
    ids = []
    for m in (case["meshes"] if meshes else []):
        h = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m["material_ids"], [capi.make_material(**x) for x in m["materials"]])
        keep.append(h)
        ids.append(scene.add_mesh_instance(h, m.get("transform")))
        if not m.get("visible", True):
            scene.set_mesh_visible(ids[-1], False)
    if "lights" in case:
        scene.set_lights([capi.make_light(**L) for L in case["lights"]])
        for k, m in enumerate(case["materials"]):
            scene.set_material(k, capi.make_material(**m))
    return scene, ids


def params(case, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format, p.surface_outputs = capi.TARGET_RGBA32F, 1
    for k, v in dict(case["frame"], **over).items():
        setattr(p, k, v)
    return p


def frame(h, case, p=None, **light_over):
    """-> image, hit counts, depth, ids, normals (, shadow hits of a lit case)"""
    p = p or params(case)
    t = capi.default_trace_params(**case["trace"])
    if "lights" in case:
        h.render_traced_lit(p, t, capi.default_trace_light_params(**dict(case["light"], **light_over)))
    else:
        h.render_traced(p, t)
    r = (h.download_frame(p), h.trace_hit_counts(p)) + tuple(h.download_surface(p, normals=True))
    return r + ((h.trace_shadow_hits(p),) if "lights" in case else ())


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def generated(h, p):
    dev = torch.zeros(p.width * p.height * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h.generate_rays(p, dev.data_ptr())
    h.sync()
    return dev.cpu().numpy().view(capi.RAY_DTYPE).copy()


def stats(o):
    return np.array([o.as_dict()[k] for k in STATS], np.int64)


C = tmc.cases()
res = {}
def record(scene, case, name):
    """one frame of the case with the setting on: everything the comparison with the restatement reads, under the prefix `name`"""
    p = params(case)
    scene.set_trace_meshes(True, case["mesh_min_T"])
    t = capi.default_trace_params(**case["trace"])
    if "lights" in case:
        o, lo = scene.render_traced_lit(p, t, capi.default_trace_light_params(**case["light"]), want_stats=True)
        res[name + "_shadow_hits"], res[name + "_shadow_rays"] = scene.trace_shadow_hits(p), lo.shadow_rays
    else:
        o = scene.render_traced(p, t, want_stats=True)
    res[name + "_image"], res[name + "_hits"] = scene.download_frame(p), scene.trace_hit_counts(p)
    res[name + "_depth"], res[name + "_id"] = scene.download_surface(p)
    res[name + "_accepted"] = o.accepted_hits
    res[name + "_mesh"] = scene.trace_mesh_hits(p)
    prim, shadow = scene.trace_mesh_stats()
    res[name + "_primary"], res[name + "_shadow"] = stats(prim), stats(shadow)


if mode == "cases":
    for name, case in C.items():
        scene, _ = build(case)
        record(scene, case, name)
        scene.close()
elif mode == "storage":
    for name in ("u1", "l1"):
        case = C[name]
        for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
            scene, _ = build(case, storage=fmt)
            for k, (arrays, _) in enumerate(case["sets"]):
                n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
                res[f"{name}_{tag}_rgba_{k}"] = scene.download_set(k, 2, 4 * n).reshape(n, 4)
                sh = np.zeros((n, 15, 3), np.float32)  # the set's own stride is 3 * cpc floats per splat, [coef][rgb]
                sh[:, :cpc] = scene.download_set(k, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
                res[f"{name}_{tag}_sh_{k}"] = sh
            record(scene, case, f"{name}_{tag}")
            scene.close()
elif mode == "exact":
    for name in ("u1", "u5"):
        case = C[name]
        scene, _ = build(case)
        p = params(case)
        scene.set_trace_meshes(True)
        res[name + "_image"], res[name + "_hits"], res[name + "_depth"], res[name + "_id"], _ = frame(scene, case, p)
        res[name + "_mesh"] = scene.trace_mesh_hits(p).reshape(-1)
        prim, shadow = scene.trace_mesh_stats()
        res[name + "_primary"], res[name + "_shadow"] = stats(prim), stats(shadow)
        rays = generated(scene, p)
        res[name + "_rays"] = rays
        q, qo = scene.trace_mesh_rays(rays, want_stats=True)
        res[name + "_query"], res[name + "_query_stats"] = q, stats(qo)
        # the particle walk of the ray query, cut at the mesh hit as a caller cuts it
        cut = rays.copy()
        hit = q["hit"] == 1
        cut["t_max"][hit] = q["t"][hit]
        pu = params(case)
        res[name + "_walk"] = scene.trace_rays(cut, pu, capi.default_trace_params(**case["trace"]))
        scene.set_trace_meshes(False)
        res[name + "_off_image"] = frame(scene, case, p)[0]
        # the threshold: the mesh leaves where the walk's T is at or below it
        scene.set_trace_meshes(True, 0.5)
        res[name + "_thr_image"] = frame(scene, case, p)[0]
        scene.close()
elif mode == "lit":
    for name in ("l1", "l3"):
        case = C[name] if name == "l1" else dict(C[name], meshes=C[name]["meshes"][:2])   # (l3 without the fixture: the test's two materials)
        scene, _ = build(case)
        p = params(case)
        scene.set_trace_meshes(True)
        img, hits, depth, ids, _, sh = frame(scene, case, p)
        prim, shadow = scene.trace_mesh_stats()
        res[name + "_image"], res[name + "_hits"], res[name + "_shadow_hits"], res[name + "_id"] = img, hits, sh, ids
        res[name + "_primary"], res[name + "_shadow"] = stats(prim), stats(shadow)
        mesh = scene.trace_mesh_hits(p).reshape(-1)
        res[name + "_mesh"] = mesh
        res[name + "_noshadow_image"] = frame(scene, case, p, shadows_mode=0)[0]
        rays = generated(scene, params(case, lighting_mode=0))
        res[name + "_rays"] = rays
        # the mesh points under the light query: the splats' shadow on the caller's surface, no mesh occlusion
        pts = capi.make_surface_points(mesh["position"], mesh["normal"], rays["direction"], np.ones((mesh.shape[0], 3), np.float32),
                                       np.where(mesh["hit"] == 1, mesh["material_id"], 0).astype(np.uint32))
        res[name + "_points"] = scene.shade_points(pts, tmc.MATERIALS, params(case, lighting_mode=0), capi.default_trace_params(**case["trace"]),
                                                   capi.default_trace_light_params(**case["light"]))
        # occlusion of the mesh points' light rays by the meshes, through the mesh ray query
        if name == "l3":
            d = np.float32(case["lights"][0]["direction"])   # normalised in fp32 as the library's light table does it
            d = -(d * (np.float32(1.0) / np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
            occ = capi.make_rays(mesh["position"], np.tile(d, (mesh.shape[0], 1)), 0.001, np.float32(1e10) - np.float32(0.001))
            res[name + "_occluded"] = scene.trace_mesh_rays(occ, mode=capi.MESH_RAYS_OCCLUSION)["hit"]
        scene.set_trace_meshes(False)
        res[name + "_off_image"] = frame(scene, case, p)[0]
        scene.close()
elif mode == "unmoved":
    for name in ("u1", "l1"):
        case = C[name]
        bare, _ = build(case, meshes=False)
        ref = frame(bare, case)
        bare.close()
        scene, ids = build(case)
        res[name + "_off_equal"] = same(ref, frame(scene, case))
        scene.set_trace_meshes(True)
        on = frame(scene, case)
        res[name + "_on_differs"] = not same(ref[:1], on[:1])
        for i in ids:
            scene.set_mesh_visible(i, False)
        res[name + "_invisible_equal"] = same(ref, frame(scene, case))
        res[name + "_invisible_all_miss"] = not scene.trace_mesh_hits(params(case))["hit"].any()
        for i in ids:
            scene.set_mesh_visible(i, True)
        # strips: every tile row on its own
        rows = (case["H"] + 15) // 16
        ok = True
        for r in range(rows):
            s = frame(scene, case, params(case, strip_row_begin=r, strip_row_end=r + 1))
            y0, y1 = 16 * r, min(16 * r + 16, case["H"])
            ok = ok and all(a[y0:y1].tobytes() == b[y0:y1].tobytes() for a, b in zip(s, on))
        res[name + "_strips_equal"] = ok
        ctx = scene.frame_context()
        ctx.set_trace_meshes(True)
        res[name + "_context_equal"] = same(on, frame(ctx, case))
        ctx.close()
        for tag, fmt in (("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):
            tf = frame(scene, case, params(case, target_format=fmt))
            res[f"{name}_target_{tag}"] = tf[0]
            res[f"{name}_target_{tag}_side_equal"] = same(tf[1:], on[1:])
        res[name + "_on_image"] = on[0]
        if name == "u1":
            pr = params(case, lighting_mode=0)
            rays = generated(scene, pr)
            scene.set_trace_meshes(False)
            scene.render(pr)
            r0, q0 = scene.download_frame(pr), scene.trace_mesh_rays(rays)
            scene.set_trace_meshes(True)
            frame(scene, case)
            scene.render(pr)
            res["render_and_query_unmoved"] = r0.tobytes() == scene.download_frame(pr).tobytes() and q0.tobytes() == scene.trace_mesh_rays(rays).tobytes()
        scene.close()
    # temporal accumulation of three depth-of-field samples of u5: singly, then accumulated by the library
    case = C["u5"]
    scene, _ = build(case)
    scene.set_trace_meshes(True)
    res["dof_singles"] = np.stack([frame(scene, case, params(case, frame_sample_id=k))[0] for k in range(3)])
    res["dof_accumulated"] = np.stack([frame(scene, case, params(case, frame_sample_id=k, temporal_sampling=1))[0] for k in range(3)])
    scene.close()
else:
    case = C["u1"]
    scene, ids = build(case)
    p = params(case)
    t = capi.default_trace_params(**case["trace"])
    frame(scene, case, p)
    w0 = scene.memory_usage()[1]
    try:
        scene.trace_mesh_hits(p)
        res["state_off"] = 0
    except capi.MgsError as e:
        res["state_off"] = e.code
    scene.set_trace_meshes(True)
    a = frame(scene, case, p)
    res["working_bytes_growth"] = scene.memory_usage()[1] - w0
    res["pixels"] = case["W"] * case["H"]
    r1 = scene.trace_mesh_stats()[0].bvh_rebuilt
    frame(scene, case, p)
    r2 = scene.trace_mesh_stats()[0].bvh_rebuilt
    M = np.eye(4, dtype=np.float32)
    M[0, 3] = 0.3
    scene.set_mesh_transform(ids[0], M)
    b = frame(scene, case, p)
    r3 = scene.trace_mesh_stats()[0].bvh_rebuilt
    frame(scene, case, p)
    r4 = scene.trace_mesh_stats()[0].bvh_rebuilt
    scene.set_mesh_visible(ids[0], False)
    c = frame(scene, case, p)
    r5 = scene.trace_mesh_stats()[0].bvh_rebuilt
    res["rebuilt"] = np.array([r1, r2, r3, r4, r5])
    res["moved_changes"], res["hidden_changes"] = not same(a[:1], b[:1]), not same(b[:1], c[:1])
    codes = []
    for strategy in (1, 2):
        try:
            scene.render_traced(p, capi.default_trace_params(**dict(case["trace"], trace_strategy=strategy)))
            codes.append(0)
        except capi.MgsError as e:
            codes.append(e.code)
    try:
        scene.render_hybrid(params(case, lighting_mode=1), t)
        codes.append(0)
    except capi.MgsError as e:
        codes.append(e.code)
    res["unsupported"] = np.array(codes)
    import ctypes as C_
    bad = []
    for q in (capi.TraceMeshParams(2, 0.0), capi.TraceMeshParams(1, 1.5), capi.TraceMeshParams(1, -0.1), capi.TraceMeshParams(1, 0.0, (C_.c_uint32 * 2)(0, 7))):
        try:
            scene.set_trace_meshes(params=q)
            bad.append(0)
        except capi.MgsError as e:
            bad.append(e.code)
    res["invalid_arg"] = np.array(bad)
    res["still_on_after_refusals"] = same(frame(scene, case, p)[:1], c[:1])
    scene.set_trace_meshes(False)
    scene.render_traced(p, capi.default_trace_params(**dict(case["trace"], trace_strategy=1)))   # off: the strategies run as before
    res["strategy_runs_when_off"] = True
    scene.close()
np.savez(out, **res)
print("child ok")
