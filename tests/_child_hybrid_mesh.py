"""child process of test_gpu_hybrid_mesh.py: hybrid frames with meshes in a fresh process.   usage: _child_hybrid_mesh.py MODE OUT.npz
MODE cases:  every case of hybrid_mesh_cases.py with mgs_frame_set_hybrid_meshes on: the frame, the raster outputs, shadow hits, hit
             records, the depth plane, both statistics blocks, the light pass's sums; then mgs_render (lighting 0, surface outputs 1)
             on ANOTHER handle with the downloaded plane bound through mgs_frame_upload_occluder: the raster step alone
MODE props:  the defining properties, the byte equalities, formats, accumulation, strips, a frame context and the refusals"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import hybrid_mesh_cases as hmc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
STATS = ("triangles", "leaves", "nodes", "node_visits", "triangle_tests", "hits", "invalid_rays", "bvh_rebuilt")
keep = []


def build(case, meshes=True):
    scene = mgs.Scene(0)
    for arrays, M in case["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit()
    ids = []
    for m in (case["meshes"] if meshes else []):
        h = capi.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m["material_ids"], [capi.make_material(**x) for x in m["materials"]])
        keep.append(h)
        ids.append(scene.add_mesh_instance(h, m.get("transform")))
    scene.set_lights([capi.make_light(**L) for L in case["lights"]])
    for k, m in enumerate(case["materials"]):
        scene.set_material(k, capi.make_material(**m))
    return scene, ids


def params(case, **over):
    p = capi.default_params(case["W"], case["H"])
    capi.set_camera(p, case["V"], case["P"], case["eye"])
    p.target_format = capi.TARGET_RGBA32F
    for k, v in dict(case["frame"], **over).items():
        setattr(p, k, v)
    return p


def hybrid(h, case, light=None, **over):
    """(image, depth, ids, normal, shadow hits, FrameOut, TraceLightOut)"""
    p = params(case, **over)
    o, lo = h.render_hybrid(p, capi.default_trace_params(**case["trace"]), capi.default_trace_light_params(**dict(case["light"], **(light or {}))),
                            want_stats=True)
    return (h.download_frame(p),) + h.download_surface(p, normals=True) + (h.trace_shadow_hits(p), o, lo)


def stats(o):
    return np.array([o.as_dict()[k] for k in STATS], np.int64)


def code(fn):
    try:
        fn()
        return 0
    except mgs.MgsError as e:
        return e.code


C = hmc.cases()
res = {}


def record(scene, case, name, **over):
    scene.set_hybrid_meshes(True, case["mesh_min_T"])
    hy = hybrid(scene, case, **over)
    p = params(case, **over)
    for k, key in enumerate(("image", "depth", "id", "normal", "shadow_hits")):
        res[f"{name}_{key}"] = hy[k]
    res[f"{name}_shadow_rays"], res[f"{name}_shadow_accepted"], res[f"{name}_light_ms"] = hy[6].shadow_rays, hy[6].shadow_accepted_hits, hy[6].light_ms
    res[f"{name}_error_flags"] = hy[5].error_flags
    res[f"{name}_mesh"], res[f"{name}_plane"] = scene.trace_mesh_hits(p), scene.hybrid_mesh_depth(p)
    prim, shadow = scene.trace_mesh_stats()
    res[f"{name}_primary"], res[f"{name}_shadow"] = stats(prim), stats(shadow)
    return hy


def raster_alone(case, name, plane, **over):
    """mgs_render, unlit with the surface outputs, on another handle with `plane` uploaded as its occluder depth"""
    other, _ = build(case, meshes=False)
    other.upload_occluder(plane)
    pu = params(case, **dict(over, lighting_mode=0, surface_outputs=1))
    other.render(pu)
    r = (other.download_frame(pu),) + other.download_surface(pu, normals=True)
    for k, key in enumerate(("image", "depth", "id", "normal")):
        res[f"{name}_u_{key}"] = r[k]
    other.close()


if mode == "cases":
    for name, case in C.items():
        scene, _ = build(case)
        record(scene, case, name)
        raster_alone(case, name, res[f"{name}_plane"])
        if name == "m02_wall":  # the same frame, the setting on, without shadow rays: what the wall's shadow is measured against
            res["m02_wall_shadows_off_image"] = hybrid(scene, case, light=dict(shadows_mode=0))[0]
        scene.close()
elif mode == "props":
    # m01: shadows on against shadows off; the setting off before and after; the old refusals
    case = C["m01_3dgs_floor"]
    scene, ids = build(case)
    off0 = hybrid(scene, case)
    wb0 = scene.memory_usage()[1]
    on = record(scene, case, "m01")
    res["working_bytes_growth"] = scene.memory_usage()[1] - wb0
    res["m01_same_twice"] = hybrid(scene, case)[0].tobytes() == on[0].tobytes()
    res["m01_shadows_off_image"] = hybrid(scene, case, light=dict(shadows_mode=0))[0]
    p = params(case)
    scene.upload_occluder(np.ones((case["H"], case["W"]), np.float32))
    res["occluder_on"] = code(lambda: hybrid(scene, case))
    scene.set_hybrid_meshes(False)
    res["occluder_off"] = code(lambda: hybrid(scene, case))
    scene.clear_occluder()
    res["off_after_on_same"] = hybrid(scene, case)[0].tobytes() == off0[0].tobytes()
    res["mesh_hits_after_off"] = code(lambda: scene.trace_mesh_hits(p))
    res["plane_after_off"] = code(lambda: scene.hybrid_mesh_depth(p))
    scene.set_trace_meshes(True)
    res["trace_meshes_off"] = code(lambda: hybrid(scene, case))
    scene.set_hybrid_meshes(True)
    res["trace_meshes_ignored_when_on"] = hybrid(scene, case)[0].tobytes() == on[0].tobytes()
    scene.set_trace_meshes(False)
    res["soft_on"] = code(lambda: hybrid(scene, case, light=dict(shadows_mode=2)))
    # m10: an invisible instance only equals the setting-off frame byte for byte; a moved mesh rebuilds once
    scene.set_mesh_visible(ids[0], False)
    inv = hybrid(scene, case)
    res["invisible_same"] = all(a.tobytes() == b.tobytes() for a, b in zip(inv[:5], off0[:5]))
    res["invisible_hits_all_miss"] = not scene.trace_mesh_hits(p)["hit"].any()
    scene.set_mesh_visible(ids[0], True)
    hybrid(scene, case)
    res["rebuilt_visible_again"] = scene.trace_mesh_stats()[0].bvh_rebuilt
    hybrid(scene, case)
    res["rebuilt_unchanged"] = scene.trace_mesh_stats()[0].bvh_rebuilt
    M = np.eye(4, dtype=np.float32)
    M[1, 3] = -0.1
    scene.set_mesh_transform(ids[0], M)
    moved = hybrid(scene, case)
    res["rebuilt_moved"] = scene.trace_mesh_stats()[0].bvh_rebuilt
    res["moved_differs"] = moved[0].tobytes() != on[0].tobytes()
    scene.close()
    # m05: temporal accumulation over three samples against the frames rendered singly
    case = C["m05_dof"]
    scene, _ = build(case)
    scene.set_hybrid_meshes(True)
    res["dof_singles"] = np.stack([hybrid(scene, case, frame_sample_id=k)[0] for k in range(3)])
    res["dof_accumulated"] = np.stack([hybrid(scene, case, frame_sample_id=k, temporal_sampling=1)[0] for k in range(3)])
    scene.close()
    # m11: the target formats, with the raster step alone in that format
    case = C["m06_threshold_0"]
    scene, _ = build(case)
    for tag, fmt in (("f16", capi.TARGET_RGBA16F), ("u8", capi.TARGET_RGBA8)):
        record(scene, case, "target_" + tag, target_format=fmt)
        raster_alone(case, "target_" + tag, res[f"target_{tag}_plane"], target_format=fmt)
    scene.close()
    # m12: strips and a frame context
    case = C["m12_deep"]
    scene, _ = build(case)
    scene.set_hybrid_meshes(True)
    full = hybrid(scene, case)
    for r in range(2):
        s = hybrid(scene, case, strip_row_begin=r, strip_row_end=r + 1)
        y0, y1 = 16 * r, min(16 * r + 16, case["H"])
        res[f"strip_{r}"] = s[0][y0:y1].tobytes() == full[0][y0:y1].tobytes() and np.array_equal(s[4][y0:y1], full[4][y0:y1])
    ctx = scene.frame_context()
    res["context_off_by_default"] = ctx.render_hybrid is not None and hybrid(ctx, case)[0].tobytes() != full[0].tobytes()
    ctx.set_hybrid_meshes(True)
    c = hybrid(ctx, case)
    res["context_same"] = c[0].tobytes() == full[0].tobytes() and np.array_equal(c[4], full[4])
    ctx.close()
    scene.close()
np.savez(out, **res)
print("child ok")
