#!/usr/bin/env python3
"""compare_probe — times mgs_compare_metrics at 1920x1080 on the benchmark's garden-sized frame (fp32 storage, uploaded as the
capture) against its uint8-storage twin: elapsed_ms of each flip mode, median of 20 calls after 5 warm-up calls, with the bytes
each mode has to move.  Writes profiles/compare_times_1920x1080.json (or --out).  Needs an MI355X.

    python tools/compare_probe.py [--splats N] [--out FILE.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/compare_probe.py --out DIR/probe.json`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=5_830_000)  # bench.py's syn_garden
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_times_1920x1080.json"))
    a = ap.parse_args()
    sc = synth.make_scene(a.splats, seed=0xC0FFEE + 2)
    eye = synth.orbit_pose(5)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    s = mgs.Scene(0)
    s.add_instance(mgs.SplatSet.from_arrays(**sc))
    s.commit(capi.FORMAT_FLOAT32, capi.FORMAT_FLOAT32)
    s.render(p)
    cap = s.download_frame(p).astype(np.float32)
    s.close()
    s = mgs.Scene(0)
    s.add_instance(mgs.SplatSet.from_arrays(**sc))
    s.commit(capi.FORMAT_UINT8, capi.FORMAT_UINT8)
    s.render(p)
    s.compare_capture_upload(cap)
    n = W * H
    # bytes each mode must move: capture RGBA32F 16 B + frame RGBA16F 8 B per pixel; approx reads no more from memory (its 3 x 3
    # neighbourhood comes from cache / LDS); reference adds per image luminance (4 written), five row planes (4 read + 20 written),
    # five feature planes (20 + 4 read, 20 written), the image itself twice more (16 | 8), and 40 read by the final pass
    need = {"disabled": 24 * n, "approx": 24 * n, "reference": (24 + 2 * (4 + 24 + 44) + 24 + 40) * n + 24 * n}
    res = {"scene": f"syn_garden N={a.splats}, fp32 storage (capture, RGBA32F upload) against uint8 storage (frame, RGBA16F)", "size": [W, H]}
    for mode, name in ((capi.FLIP_DISABLED, "disabled"), (capi.FLIP_APPROX, "approx"), (capi.FLIP_REFERENCE, "reference")):
        ts = []
        for i in range(25):
            m = s.compare_metrics(mode)
            if i >= 5:
                ts.append(m.elapsed_ms)
        med = float(np.median(ts))
        res[name] = dict(median_ms=med, min_ms=float(min(ts)), max_ms=float(max(ts)), bytes=need[name], tb_per_s=need[name] / med / 1e9,
                         mse_fixed=m.mse_fixed, psnr=m.psnr, psnr_exact=m.psnr_exact, flip=m.flip, flip_exact=m.flip_exact)
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
