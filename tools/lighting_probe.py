"""What the deferred lighting pass (MgsFrameParams.lighting_mode, k_light.hip) costs, by the library's own stage events:
   python tools/lighting_probe.py [--splats N] [--width W --height H] [--frames F] [--skip S] [--runs a,b,...] [--out FILE]
Garden-sized synthetic scene, fp32 storage, GPU-radix sort, RGBA16F target, serial frames with the stage events (collect_timings = 2),
the first S frames of each run untimed.  Runs on one scene and one build: "surface" = surface_outputs = 1 without lighting (what a lit
frame pays before the pass; run it on the parent commit too: --runs surface works there), "headlight" = lighting with the empty table,
"lights_8" / "lights_64" = that many mixed lights, every instance material shaded (diffuse + specular, shininess 32).  Prints ONE JSON
object: mean ms per stage and run, the pass's compulsory bytes per pixel and their time at the measured copy bandwidth."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=5_830_000)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--skip", type=int, default=32)
ap.add_argument("--runs", default="surface,headlight,lights_8,lights_64")
ap.add_argument("--out", default=None)
a = ap.parse_args()
W, H = a.width, a.height
lit_capable = hasattr(capi, "LIGHTING_DIRECT")
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


def mixed_lights(n):
    rng = np.random.default_rng(7)
    out = []
    for k in range(n):
        pos = rng.uniform(-4.0, 4.0, 3)
        out.append(capi.make_light(type=k % 3, color=rng.uniform(0.2, 1.0, 3), intensity=float(rng.uniform(0.5, 2.0)), position=pos,
                                   direction=-pos, range=float(rng.uniform(3.0, 12.0)), attenuation_mode=k % 4))
    return out


names = ["project", "sort", "bin", "pairsort", "composite", "total", "cull", "light"]
res = {}
for tag in a.runs.split(","):
    lighting = tag != "surface"
    if lighting and not lit_capable:
        continue
    if lighting:
        scene.set_material(0, capi.make_material(ambient=(0.05,) * 3, diffuse=(0.8,) * 3, specular=(0.5,) * 3, emission=(0,) * 3, shininess=32.0))
        scene.set_lights(mixed_lights({"headlight": 0, "lights_8": 8, "lights_64": 64}[tag]))
    rows = []
    for i in range(a.skip + a.frames):
        p = poses[i % 64]
        p.collect_timings = 2
        p.surface_outputs = 0 if lighting else 1
        if lit_capable:
            p.lighting_mode = capi.LIGHTING_DIRECT if lighting else capi.LIGHTING_DISABLED
        scene.render(p)
        scene.sync()
        if i >= a.skip:
            rows.append(scene.timings_all(0))
    ms = np.array(rows, np.float64)
    st = scene.render(poses[0], want_stats=True)
    res[tag] = {"stage_ms": {n: round(float(ms[:, j].mean()), 5) for j, n in enumerate(names)},
                "light_ms_min": round(float(ms[:, 7].min()), 5), "light_ms_max": round(float(ms[:, 7].max()), 5),
                "total_ms_min": round(float(ms[:, 5].min()), 5), "error_flags": int(st.error_flags)}
scene.close()
# compulsory traffic of the pass per pixel: normal 16 B + depth 4 B + id 4 B + RGBA16F pixel read 8 B and written 8 B
bytes_px = 16 + 4 + 4 + 8 + 8
out = {"tool": "tools/lighting_probe.py", "device": "MI355X (gfx950)", "splats": a.splats, "width": W, "height": H, "frames": a.frames,
       "skipped": a.skip, "bytes_per_pixel": bytes_px, "byte_time_ms_at_copy_bandwidth": round(W * H * bytes_px / (COPY_TBS * 1e12) * 1e3, 5),
       "runs": res}
line = json.dumps(out)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
