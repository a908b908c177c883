"""What the occluder (mgs_frame_set_occluder) costs and saves, by the library's own stage events:
   python tools/occluder_probe.py [--splats N] [--width W --height H] [--frames F] [--skip S] [--out FILE]
Garden-sized synthetic scene, fp32 storage, GPU-radix sort, serial frames with the six stage events (collect_timings = 2), the first
S frames untimed (the adaptive bin size settles after 24).  Four runs on one scene and one build: nothing bound; depth 1.0
everywhere (the price of the test itself); depth 0.0 everywhere (the early stop); a wall over the left half of the image at the
median depth of the first pose's sorted splats.  Prints ONE JSON object (mean ms per stage and run, ratios to the unbound run)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=5_830_000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--skip", type=int, default=32)
ap.add_argument("--out", default=None)
a = ap.parse_args()
W, H = a.width, a.height
sc = synth.make_scene(a.splats, seed=0xC0FFEE + 2)
scene = mgs.Scene(0)
scene.add_instance(mgs.SplatSet.from_arrays(**sc))
scene.commit()
poses = []
for i in range(64):
    eye = synth.orbit_pose(i)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    poses.append(p)
# median ndc depth of the first pose's sorted splats (back-to-front keys hold -ndc.z, encodeMinMaxFp32)
so = scene.sort_keys(poses[0])
keys, _ = scene.sort_download(so.count)
bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)
z_mid = float(np.median(-bits.view(np.float32)))
wall = np.ones((H, W), np.float32)
wall[:, : W // 2] = z_mid
runs = [("unbound", None), ("depth_1", np.ones((H, W), np.float32)), ("depth_0", np.zeros((H, W), np.float32)), ("wall_left_half", wall)]
names = ["project", "sort", "bin", "pairsort", "composite", "total"]
res = {}
for tag, depth in runs:
    if depth is None:
        scene.clear_occluder()
    else:
        scene.upload_occluder(depth)
    rows = []
    for i in range(a.skip + a.frames):
        p = poses[i % 64]
        p.collect_timings = 2
        scene.render(p)
        scene.sync()
        if i >= a.skip:
            rows.append(scene.timings_all(0)[:6])
    ms = np.array(rows, np.float64)
    st = scene.render(poses[0], want_stats=True)
    res[tag] = {"stage_ms": {n: round(float(ms[:, j].mean()), 5) for j, n in enumerate(names)},
                "composite_ms_min": round(float(ms[:, 4].min()), 5), "composite_ms_max": round(float(ms[:, 4].max()), 5),
                "error_flags": int(st.error_flags)}
scene.close()
base = res["unbound"]["stage_ms"]
for tag in ("depth_1", "depth_0", "wall_left_half"):
    res[tag]["composite_ratio_to_unbound"] = round(res[tag]["stage_ms"]["composite"] / base["composite"], 4)
    res[tag]["total_ratio_to_unbound"] = round(res[tag]["stage_ms"]["total"] / base["total"], 4)
out = {"tool": "tools/occluder_probe.py", "device": "MI355X (gfx950)", "splats": a.splats, "width": W, "height": H,
       "frames": a.frames, "skipped": a.skip, "wall_depth": z_mid, "runs": res}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
