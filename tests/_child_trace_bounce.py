"""child process of test_gpu_trace_bounce.py: indirect traced frames in a fresh process.   usage: _child_trace_bounce.py MODE OUT.npz
MODE cases:     every case of trace_bounce_cases.py: frame (RGBA32F), hit counts, side outputs, shadow hits, hit records, statistics
MODE identical: b1 / b3 with every bounce material illum 0, and with every mesh instance invisible, next to mgs_render_traced_lit
MODE unmoved:   the other entry points before and after an indirect frame; strips; a frame context; target formats; accumulation
MODE lifecycle: working_bytes, the setting off, bounce materials and the hierarchy, refusals"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import trace_bounce_cases as tbc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
keep = []


def build(case, bounce=True, storage=None):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    if case["sets"]:
        scene.commit(*((storage, storage) if storage is not None else ()))
    ids = []
    for m in case["meshes"]:
        h = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m["material_ids"], [capi.make_material(**x) for x in m["materials"]])
        keep.append(h)
        ids.append(scene.add_mesh_instance(h, m.get("transform")))
    scene.set_lights([capi.make_light(**L) for L in case["lights"]])
    for k, m in enumerate(case["materials"]):
        scene.set_material(k, capi.make_material(**m))
    if bounce:
        for i, b in zip(ids, case["bounce"]):
            if b:
                scene.set_mesh_bounce_materials(i, [capi.bounce_material(**x) for x in b])
    scene.set_trace_meshes(True, case["mesh_min_T"])
    return scene, ids


def params(case, lighting=2, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format, p.surface_outputs = capi.TARGET_RGBA32F, 1
    for k, v in dict(case["frame"], lighting_mode=lighting, **over).items():
        setattr(p, k, v)
    return p


def knobs(case):
    return capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**case["light"])


def outputs(h, p):
    return (h.download_frame(p), h.trace_hit_counts(p), h.trace_shadow_hits(p)) + tuple(h.download_surface(p, normals=True))


def indirect(h, case, p=None, nb=None, stats=False):
    p = p or params(case)
    t, lt = knobs(case)
    o = h.render_traced_indirect(p, t, lt, case["max_bounces"] if nb is None else nb, want_stats=stats)
    return (outputs(h, p), o) if stats else outputs(h, p)


def lit(h, case, p=None):
    p = p or params(case, lighting=1)
    t, lt = knobs(case)
    h.render_traced_lit(p, t, lt)
    return outputs(h, p)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


C = tbc.cases()
res = {}


def record(scene, case, name):
    """one indirect frame of the case: everything the comparison with the restatement reads, under the prefix `name`"""
    p = params(case)
    (img, hits, sh, depth, ids, nrm), (o, lo, bo) = indirect(scene, case, p, stats=True)
    res[name + "_image"], res[name + "_hits"], res[name + "_shadow_hits"], res[name + "_depth"], res[name + "_id"] = img, hits, sh, depth, ids
    res[name + "_mesh"] = scene.trace_mesh_hits(p)
    res[name + "_accepted"], res[name + "_shadow_accepted"] = o.accepted_hits, lo.shadow_accepted_hits
    res[name + "_rays"], res[name + "_mesh_hits"] = np.array(list(bo.rays), np.int64), np.array(list(bo.mesh_hits), np.int64)
    res[name + "_particle_hits"] = bo.particle_hits


if mode == "cases":
    for name, case in C.items():
        scene, _ = build(case)
        record(scene, case, name)
        scene.close()
elif mode == "storage":
    for cname in tbc.STORAGE_CASES:
        case = C[cname]
        for tag, fmt in (("f16", capi.FORMAT_FLOAT16), ("u8", capi.FORMAT_UINT8)):
            scene, _ = build(case, storage=fmt)
            for k, (arrays, _) in enumerate(case["sets"]):
                n, cpc = arrays["positions"].shape[0], arrays["f_rest"].shape[1] // 3
                res[f"{cname}_{tag}_rgba_{k}"] = scene.download_set(k, 2, 4 * n).reshape(n, 4)
                sh = np.zeros((n, 15, 3), np.float32)  # the set's own stride is 3 * cpc floats per splat, [coef][rgb]
                sh[:, :cpc] = scene.download_set(k, 3, 45 * n)[:3 * cpc * n].reshape(n, cpc, 3)
                res[f"{cname}_{tag}_sh_{k}"] = sh
            record(scene, case, f"{cname}_{tag}")
            scene.close()
elif mode == "bare":
    import torch
    case = C["bare"]
    scene, _ = build(case)
    p = params(case)
    res["indirect"] = indirect(scene, case, p)[0]
    res["mesh"] = scene.trace_mesh_hits(p)
    res["lit"], res["hits"] = lit(scene, case)[:2]
    dev = torch.zeros(p.width * p.height * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pq = params(case, lighting=0)   # (the ray queries read an unlit frame's parameters)
    scene.generate_rays(pq, dev.data_ptr())
    scene.sync()
    prim = dev.cpu().numpy().view(capi.RAY_DTYPE).reshape(p.height, p.width)
    h = res["mesh"]
    d, n = prim["direction"].astype(np.float32), h["normal"].astype(np.float32)
    refl = d - np.float32(2.0) * (d * n).sum(-1, keepdims=True) * n    # reflect(rayDir, worldNrm), in fp32 as the kernel forms it
    rays = capi.make_rays(h["position"].reshape(-1, 3), refl.reshape(-1, 3), 0.001, 10000.0)
    ok = (h["hit"] == 1).reshape(-1)
    rays["direction"][~ok] = (0.0, 0.0, 1.0)
    res["walk"] = scene.trace_rays(rays, pq, knobs(case)[0]).reshape(p.height, p.width)
    scene.close()
elif mode == "identical":
    for name in ("b1", "b3"):
        case = C[name]
        scene, ids = build(case, bounce=False)
        res[name + "_none"] = same(indirect(scene, case), lit(scene, case))
        for i in ids:   # explicit illum 0
            scene.set_mesh_bounce_materials(i, [capi.bounce_material(), capi.bounce_material()])
        (frame0, (o, lo, bo)) = indirect(scene, case, stats=True)
        res[name + "_zero"] = same(frame0, lit(scene, case))
        res[name + "_zero_rays"] = np.array(list(bo.rays), np.int64)
        for i, b in zip(ids, case["bounce"]):
            if b:
                scene.set_mesh_bounce_materials(i, [capi.bounce_material(**x) for x in b])
        res[name + "_differs"] = not same(indirect(scene, case)[:1], lit(scene, case)[:1])
        for i in ids:
            scene.set_mesh_visible(i, False)
        res[name + "_invisible"] = same(indirect(scene, case), lit(scene, case))
        scene.close()
elif mode == "unmoved":
    case = C["b1"]
    scene, ids = build(case)
    pr = params(case, lighting=0, surface_outputs=0)
    t, lt = knobs(case)

    def others():
        scene.render(pr)
        a = scene.download_frame(pr)
        scene.render_traced(pr, t)
        b = scene.download_frame(pr)
        q = scene.trace_mesh_rays(probe_rays)   # the mesh query: closest hits of a few rays down onto the floor and past it
        return (a, b, q) + lit(scene, case)
    g = np.linspace(-1.6, 1.6, 9, dtype=np.float32)
    ox, oz = np.meshgrid(g, g)
    origins = np.stack([ox.ravel(), np.full(ox.size, 1.0, np.float32), oz.ravel()], 1)
    probe_rays = capi.make_rays(origins, np.tile(np.float32([0.05, -1.0, 0.02]), (ox.size, 1)), 0.001, 10000.0)
    before = others()
    full = indirect(scene, case)
    res["others"] = same(before, others())
    # strip rows equal the same rows of the full frame
    ps = params(case, strip_row_begin=1, strip_row_end=2)
    strip = indirect(scene, case, ps)
    res["strip"] = all(x[16:32].tobytes() == y[16:32].tobytes() for x, y in zip(strip[:3], full[:3]))
    # a frame context equals the scene handle
    ctx = scene.frame_context()
    ctx.set_trace_meshes(True, case["mesh_min_T"])
    res["context"] = same(indirect(ctx, case), full)
    ctx.close()
    # target formats: the converted fp32 frame
    for tag, fmt in (("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):
        res["target_" + tag] = indirect(scene, case, params(case, target_format=fmt))[0]
    res["full"] = full[0]
    # temporal accumulation: the running mean of two identical samples is the sample
    acc = []
    for sid in (0, 1):
        acc.append(indirect(scene, case, params(case, temporal_sampling=1, frame_sample_id=sid))[0])
    res["accum0"], res["accum1"] = acc
    scene.close()
elif mode == "lifecycle":
    case = C["b1"]
    scene, ids = build(case)
    p = params(case)
    lit(scene, case)
    w0 = scene.memory_usage()[1]
    indirect(scene, case, p)
    res["growth"] = scene.memory_usage()[1] - w0
    res["pixels"] = case["W"] * case["H"]
    scene.set_mesh_bounce_materials(ids[0], [capi.bounce_material(illum=1)])
    _, (o, lo, bo) = indirect(scene, case, p, stats=True)
    prim, _ = scene.trace_mesh_stats()
    res["rebuilt_after_materials"] = prim.bvh_rebuilt
    codes = {}

    def code(key, fn):
        try:
            fn()
            codes[key] = 0
        except capi.MgsError as e:
            codes[key] = e.code
    scene.set_trace_meshes(False)
    code("setting_off", lambda: indirect(scene, case, p))
    scene.set_trace_meshes(True, case["mesh_min_T"])
    code("direct", lambda: indirect(scene, case, params(case, lighting=1)))
    code("bounces_0", lambda: indirect(scene, case, p, nb=0))
    code("bounces_17", lambda: indirect(scene, case, p, nb=17))
    ctx = scene.frame_context()
    code("context_materials", lambda: ctx.set_mesh_bounce_materials(ids[0], [capi.bounce_material(illum=1)]))
    ctx.close()
    code("bad_ior", lambda: scene.set_mesh_bounce_materials(ids[0], [capi.bounce_material((0.5, 0.5, 0.5), 0.0, 2)]))
    code("no_instance", lambda: scene.set_mesh_bounce_materials(7, [capi.bounce_material()]))
    for k, v in codes.items():
        res["code_" + k] = v
    scene.set_mesh_bounce_materials(ids[0], [capi.bounce_material(**x) for x in case["bounce"][0]])
    res["usable"] = same(indirect(scene, case, p), indirect(scene, case, p))
    scene.close()
else:
    raise SystemExit("unknown mode " + mode)
np.savez(out, **res)
print("child ok")
