"""child process of test_gpu_hierarchy.py: builds the scenes of hierarchy_cases.py and downloads their hierarchies
(mgs_debug_download_hierarchy) in a fresh process.   usage: _child_hierarchy.py MODE OUT.npz
MODE splats: every content group under every proxy (kernel degree x adaptive clamping), the leaf counts, determinism and lifecycle
MODE meshes: the leaf counts, the content scene, determinism and lifecycle"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import hierarchy_cases as hc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
res, keep = {}, []
RAY = capi.make_rays(np.float32([[0, 0, 5]]), np.float32([[0, 0, -1]]), 0.0, 100.0)


def code(fn):
    try:
        fn()
        return 0
    except mgs.MgsError as e:
        return e.code


def put(tag, dl):
    info, nodes, tris = dl
    res[tag + "_info"] = np.concatenate([[info["levels"], info["total_nodes"], info["leaves"], info["primitives"]], info["level_offset"],
                                         info["level_count"]]).astype(np.int64)
    res[tag + "_frame"] = np.concatenate([info["box_lo"], info["box_inv_ext"]])
    res[tag + "_nodes"] = nodes
    if tris is not None:
        res[tag + "_tris"] = tris


def splat_scene(sets):
    scene = mgs.Scene(0)
    made = {}
    for arrays, M in sets:
        if id(arrays) not in made:
            made[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
        scene.add_instance(made[id(arrays)], M)
    scene.commit()
    return scene


def build_splats(scene, degree, adaptive, cull):
    p = capi.default_params(8, 8)
    p.kernel_degree, p.alpha_cull_threshold, p.kernel_min_response = int(degree), float(cull), float(hc.KMR)
    _, o = scene.trace_rays(RAY, p, capi.default_trace_params(kernel_adaptive_clamping=int(adaptive)), want_stats=True)
    return o.as_dict()


def planes(scene, tag, sets):
    """what the device holds: the storage order and the density of every instance's set"""
    for k, (arrays, _) in enumerate(sets):
        n = arrays["positions"].shape[0]
        res[f"{tag}_order_{k}"] = scene.storage_order(k, n)
        res[f"{tag}_density_{k}"] = scene.download_set(k, 2, 4 * n).reshape(n, 4)[:, 3].copy()


def add_meshes(scene, meshes):
    ids = []
    for m in meshes:
        mats = [capi.make_material(shininess=8.0 + k) for k in range(4)]
        h = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m.get("material_ids"), mats)
        keep.append(h)
        i = scene.add_mesh_instance(h, m.get("transform"))
        if not m.get("visible", True):
            scene.set_mesh_visible(i, False)
        ids.append(i)
    return ids


def mesh_query(scene):
    _, o = scene.trace_mesh_rays(RAY, want_stats=True)
    return o.as_dict()


if mode == "splats":
    for name, sets in hc.splat_groups().items():
        scene = splat_scene(sets)
        if name == "a_isotropic":       # lifecycle, on the first scene: nothing built yet
            res["err_before"] = code(lambda: scene.download_hierarchy(0))
        planes(scene, name, sets)
        cull = res[name + "_density_0"][hc.E_CULL_FROM] if name == "e_thresholds" else hc.CULL
        res[name + "_cull"] = np.float32(cull)
        for degree, adaptive in hc.PROXIES:
            o = build_splats(scene, degree, adaptive, cull)
            put(f"{name}_{degree}_{adaptive}", scene.download_hierarchy(0))
            res[f"{name}_{degree}_{adaptive}_out"] = np.array([o["leaves"], o["nodes"], o["bvh_rebuilt"]], np.int64)
        if name == "c_affine":          # determinism: away and back rebuilds twice, to the same bytes; a context reads the scene's tree
            build_splats(scene, 2, 1, cull)
            a = scene.download_hierarchy(0)
            r1 = build_splats(scene, 2, 0, cull)["bvh_rebuilt"]
            r2 = build_splats(scene, 2, 1, cull)["bvh_rebuilt"]
            b = scene.download_hierarchy(0)
            ctx = scene.frame_context()
            c = ctx.download_hierarchy(0)
            res["rebuilt_twice"] = r1 == 1 and r2 == 1
            res["same_after_rebuild"] = a[1].tobytes() == b[1].tobytes() and all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and a[1].size > 0
            res["context_equal"] = a[1].tobytes() == c[1].tobytes() and all(np.array_equal(a[0][k], c[0][k]) for k in a[0])
            ctx.close()
            # lifecycle: a refused capacity leaves the handle usable; the call neither rebuilds nor allocates
            res["err_capacity"] = code(lambda: scene.download_hierarchy(0, node_capacity=a[0]["total_nodes"] - 1))
            res["err_which"] = code(lambda: scene.download_hierarchy(2))
            m0 = scene.memory_usage()
            d = scene.download_hierarchy(0)
            res["usable_after_refusal"] = d[1].tobytes() == a[1].tobytes()
            res["memory_unchanged"] = scene.memory_usage() == m0
            res["rebuilt_after_download"] = build_splats(scene, 2, 1, cull)["bvh_rebuilt"]
        scene.close()
    for n in hc.COUNTS:
        sets = hc.count_scene(n)
        scene = splat_scene(sets)
        o = build_splats(scene, 2, 1, hc.CULL)
        planes(scene, f"count_{n}", sets)
        put(f"count_{n}", scene.download_hierarchy(0))
        res[f"count_{n}_out"] = np.array([o["leaves"], o["nodes"], o["bvh_rebuilt"]], np.int64)
        scene.close()
else:
    meshes, _ = hc.mesh_content()
    scenes = dict(content=meshes, **{f"count_{n}": hc.count_mesh(n) for n in hc.COUNTS})
    for name, ms in scenes.items():
        scene = mgs.Scene(0)
        ids = add_meshes(scene, ms)
        if name == "content":
            res["err_before"] = code(lambda: scene.download_hierarchy(1))
        o = mesh_query(scene)
        put(name, scene.download_hierarchy(1))
        res[name + "_out"] = np.array([o["leaves"], o["nodes"], o["triangles"], o["bvh_rebuilt"]], np.int64)
        if name == "content":
            a = scene.download_hierarchy(1)
            moved = np.eye(4, dtype=np.float32)
            moved[0, 3] = 0.5
            scene.set_mesh_transform(ids[0], moved)
            r1 = mesh_query(scene)["bvh_rebuilt"]
            scene.set_mesh_transform(ids[0], np.eye(4, dtype=np.float32))
            r2 = mesh_query(scene)["bvh_rebuilt"]
            b = scene.download_hierarchy(1)
            ctx = scene.frame_context()
            c = ctx.download_hierarchy(1)
            res["rebuilt_twice"] = r1 == 1 and r2 == 1
            same_info = lambda x, y: all(np.array_equal(x[0][k], y[0][k]) for k in x[0])  # noqa: E731
            res["same_after_rebuild"] = a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[1].size > 0 and same_info(a, b)
            res["context_equal"] = a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes() and same_info(a, c)
            ctx.close()
            res["err_capacity"] = code(lambda: scene.download_hierarchy(1, tri_capacity=a[0]["leaves"] - 1))
            res["err_capacity_nodes"] = code(lambda: scene.download_hierarchy(1, node_capacity=a[0]["total_nodes"] - 1))
            m0 = scene.memory_usage()
            d = scene.download_hierarchy(1)
            res["usable_after_refusal"] = d[1].tobytes() == a[1].tobytes() and d[2].tobytes() == a[2].tobytes()
            res["memory_unchanged"] = scene.memory_usage() == m0
            res["rebuilt_after_download"] = mesh_query(scene)["bvh_rebuilt"]
        scene.close()
np.savez(out, **res)
print("child ok")
