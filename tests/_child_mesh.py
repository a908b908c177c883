"""child process of test_gpu_mesh.py: mgs_meshes_render + mgs_render in a fresh process (MGS_GRAPH and the RCCL double are read
when the library starts).   usage: _child_mesh.py MODE OUT.npz [RANK WORLD IDFILE]
MODE frame:  mesh pass, then mgs_render of the small splat scene for both alpha modes and lighting 0 / 1; saves the frames, and the
             frames of a fresh handle that was handed the downloaded mesh images through mgs_frame_upload_occluder
MODE gather: one rank of a two-rank mgs_render_gathered (full-frame mesh pass first); prints whether it equals the single-handle frame"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import lighting_cases as lc  # noqa: E402
import mesh_cases as mc  # noqa: E402

mode, out = sys.argv[1], sys.argv[2]


def build():
    scene = mgs.Scene(0)
    for arrays, m in lc.scene_sets():
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), m)
    scene.commit()
    return scene


V, P, eye = lc.camera_matrices(mgs.camera_lookat_perspective)
Wf, Hf = 128, 96


def params(alpha, lighting):
    p = capi.default_params(Wf, Hf)
    capi.set_camera(p, V, P, eye)
    p.alpha_mode, p.lighting_mode, p.depth_iso_threshold = alpha, lighting, lc.ISO
    return p


scene = build()
fixture = mgs.Mesh.load_obj(mc.FIXTURE)
scene.add_mesh_instance(fixture, mc.SCALE)
scene.add_mesh_instance(fixture, mc.ROTATE)
if mode == "frame":
    fresh = build()
    res = {}
    for alpha in (capi.ALPHA_COVERAGE, capi.ALPHA_SUM):
        for lighting in (0, 1):
            p = params(alpha, lighting)
            for rep in range(2):  # the second frame replays the captured graph (when graphs are on)
                scene.render_meshes(p)
                scene.render(p)
            key = f"a{alpha}_l{lighting}"
            res["with_" + key] = scene.download_frame(p).view(np.uint16).copy()
            depth, color, _ = scene.download_meshes()
            fresh.upload_occluder(depth, color)
            fresh.render(p)
            res["ref_" + key] = fresh.download_frame(p).view(np.uint16).copy()
            if lighting:
                res["cons_" + key] = scene.download_consolidated_depth(p)
                res["picked_" + key] = scene.download_surface(p)[0]
                res["mdepth_" + key] = depth
    np.savez(out, **res)
else:
    rank, world, idfile = int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    p = params(capi.ALPHA_COVERAGE, 0)
    scene.render_meshes(p)
    scene.render(p)
    full = scene.download_frame(p).view(np.uint16).copy()
    if rank == 0:
        with open(idfile + ".tmp", "wb") as f:
            f.write(capi.comm_unique_id())
        os.replace(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            if time.time() - t0 > 60:
                raise SystemExit("no unique id from rank 0")
            time.sleep(0.01)
    scene.comm_init(rank, world, open(idfile, "rb").read())
    scene.render_meshes(p)
    scene.render_gathered(p)
    print(f"GATHERED_EQUALS_FULL rank {rank}:", bool(np.array_equal(scene.download_frame(p).view(np.uint16), full)), flush=True)
    scene.comm_destroy()
scene.close()
print("CHILD_DONE", flush=True)
