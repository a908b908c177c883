"""accumulate_probe — the composite stage (compositor + k_post_accumulate) of a temporal-sampling frame in the three target formats.

  python tools/accumulate_probe.py [--size W H] [--splats N] [--warmup 5] [--repeats 30]

A small scene on a large image, so that the pass over the image is most of the stage; per format the median, minimum and maximum of
MGS_STAGE_COMPOSITE with temporal_sampling = 1 (frame_sample_id 1: the lerp path) and the median without it.  Needs an MI355X."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[3840, 2160])
ap.add_argument("--splats", type=int, default=50_000)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=30)
a = ap.parse_args()
W, H = a.size
scene = mgs.Scene(0)
scene.add_instance(mgs.SplatSet.from_arrays(**synth.make_scene(a.splats, seed=123)))
scene.commit()
eye = synth.orbit_pose(5)
V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
for name, fmt in (("rgba32f", capi.TARGET_RGBA32F), ("rgba16f", capi.TARGET_RGBA16F), ("rgba8", capi.TARGET_RGBA8)):
    med = {}
    for temporal in (0, 1):
        p = capi.default_params(W, H)
        capi.set_camera(p, V, P, eye)
        p.collect_timings, p.target_format, p.temporal_sampling, p.frame_sample_id = 1, fmt, temporal, 1
        ms = [list(scene.render(p).stage_ms)[4] for _ in range(a.warmup + a.repeats)][a.warmup:]
        med[temporal] = (float(np.median(ms)), min(ms), max(ms))
    print(f"accumulate {name} {W}x{H}: composite stage with temporal sampling median {med[1][0]:.4f} ms (min {med[1][1]:.4f}, max {med[1][2]:.4f}), "
          f"without {med[0][0]:.4f} ms")
scene.close()
