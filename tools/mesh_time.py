#!/usr/bin/env python3
"""Times of the mesh pass: MgsMeshOut.elapsed_ms of three meshes at 1920 x 1080, median of --steps passes after
--warmup, and, with --frame, the serial frame of the synthetic garden scene with and without a preceding pass of the 1 M-triangle grid.
usage: tools/mesh_time.py [--out file.json] [--only quad|grid|subpixel] [--steps 50] [--warmup 20] [--frame]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402

W, H = 1920, 1080
EYE = np.float32([0.0, 0.0, 2.2])
HALF_H = 2.2 * np.tan(np.radians(27.5))  # half the height of the plane z = 0 the camera sees
HALF_W = HALF_H * W / H


def camera():
    V, P = mgs.camera_lookat_perspective(EYE, [0, 0, 0], [0, 1, 0], 55.0, 0.1, 50.0, W, H)
    return V, P, EYE


def flat(pos, idx):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    return dict(positions=pos, indices=np.asarray(idx, np.uint32).reshape(-1, 3), normals=np.tile(np.float32([0, 0, 1]), (pos.shape[0], 1)))


def quad():
    x, y = 1.05 * HALF_W, 1.05 * HALF_H
    return flat([[-x, -y, 0], [x, -y, 0], [x, y, 0], [-x, y, 0]], [[0, 1, 2], [0, 2, 3]])


def grid(nx=943, ny=531, seed=3):
    """(nx - 1) (ny - 1) 2 = 998 520 triangles of about 2 x 2 pixels that cover the frame, vertices jittered"""
    r = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-1.02 * HALF_W, 1.02 * HALF_W, nx, dtype=np.float32), np.linspace(-1.02 * HALF_H, 1.02 * HALF_H, ny, dtype=np.float32))
    jit = (r.random((ny, nx, 2), dtype=np.float32) - 0.5) * np.float32(0.4 * 2.04 * HALF_W / (nx - 1))
    jit[0, :], jit[-1, :], jit[:, 0], jit[:, -1] = 0, 0, 0, 0
    pos = np.stack([x + jit[..., 0], y + jit[..., 1], np.zeros_like(x)], -1).reshape(-1, 3)
    a = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    return flat(pos, np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)], 0))


def subpixel(count=1_000_000, seed=5):
    """`count` triangles of at most half a pixel, anywhere in the frame, depths spread over one unit"""
    r = np.random.default_rng(seed)
    c = (r.random((count, 1, 3), dtype=np.float32) - 0.5) * np.float32([2 * HALF_W, 2 * HALF_H, 1.0])
    px = 2 * HALF_H / H
    tri = c + (r.random((count, 3, 3), dtype=np.float32) - 0.5) * np.float32([0.5 * px, 0.5 * px, 0.0])
    return flat(tri.reshape(-1, 3), np.arange(3 * count).reshape(-1, 3))


MESHES = {"quad": quad, "grid": grid, "subpixel": subpixel}


def params():
    V, P, eye = camera()
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    p.lighting_mode = 1
    return p


def time_mesh(name, steps, warmup):
    m = MESHES[name]()
    scene = mgs.Scene(0)
    mesh = mgs.Mesh.from_arrays(m["positions"], m["indices"], m["normals"])
    scene.add_mesh_instance(mesh)
    p = params()
    for _ in range(warmup):
        scene.render_meshes(p)
    outs = [scene.render_meshes(p, want_stats=True) for _ in range(steps)]
    ms = np.array([o.elapsed_ms for o in outs])
    o = outs[-1]
    _, _, prim = scene.download_meshes()
    scene.close()
    return dict(triangles=int(o.triangles_in), rasterised=int(o.triangles_rasterised), fragments=int(o.fragments), flags=int(o.flags),
                covered_pixels=int((prim != 0xFFFFFFFF).sum()), median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def time_frame(steps, warmup, splats=5_830_000):
    """the benchmark's scene and orbit (bench.py), frames one after the other, each waited for"""
    sc = synth.make_scene(splats, seed=0xC0FFEE + 2)
    scene = mgs.Scene(0)
    scene.add_instance(mgs.SplatSet.from_arrays(**sc))
    scene.commit()
    m = grid()
    scene.add_mesh_instance(mgs.Mesh.from_arrays(m["positions"], m["indices"], m["normals"]), np.diag(np.float32([3, 3, 1, 1])))
    res = {}
    for with_mesh in (False, True):
        ms = []
        for i in range(warmup + steps):
            eye = synth.orbit_pose(i)
            V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
            p = capi.default_params(W, H)
            capi.set_camera(p, V, P, eye)
            t0 = time.perf_counter()
            if with_mesh:
                scene.render_meshes(p)
            scene.render(p, want_stats=True)
            ms.append((time.perf_counter() - t0) * 1e3)
        res["with_mesh_pass_ms" if with_mesh else "splats_only_ms"] = float(np.median(ms[warmup:]))
    scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=sorted(MESHES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frame", action="store_true")
    a = ap.parse_args()
    res = {"width": W, "height": H, "lighting_mode": 1, "steps": a.steps, "warmup": a.warmup}
    for name in ([a.only] if a.only else ["quad", "grid", "subpixel"]):
        res[name] = time_mesh(name, a.steps, a.warmup)
        print(name, json.dumps(res[name]), flush=True)
    if a.frame:
        res["frame"] = time_frame(a.steps, a.warmup)
        print("frame", json.dumps(res["frame"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
