"""child process of test_gpu_fragments.test_grid_counts: libmgs reads its switches (MGS_BIN_SHIFT, MGS_DIRECT_BIN, MGS_DB_TRANSPOSE,
MGS_RECT_RIDE, MGS_RIDE_SPLIT) once per process, so every setting renders in its own interpreter.  Usage: _child_fragment_grids.py
OUT.npz.  Renders the cases of fragment_cases.GRID_CASES in the count mode and writes, per case, the alpha plane, the frame's
statistics (sorted_count, tile_pairs, escape_count, error_flags) and the sorted splats' ids and bin rectangles; and shows that a
frame of 257 bin columns is refused and the frame after it holds its counts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fragment_cases as fc  # noqa: E402
import gpu_fragments as gf  # noqa: E402

res = {}
for k, name in enumerate(fc.GRID_CASES):
    scene = gf.build_scene(name)
    alpha, out = gf.render_counts(scene, name)
    ids, rects = gf.sorted_rects(scene, out)
    res[name + "/alpha"], res[name + "/ids"], res[name + "/rects"] = alpha, ids, rects
    res[name + "/stats"] = np.array([out.sorted_count, out.tile_pairs, out.escape_count, out.error_flags], np.int64)
    if k == 0:   # 8224 x 16 px are 257 bin columns of 32 px: refused, and the scene's next frame is whole.  The frame buffer outlives a
        # frame, so it first gets a frame that is no count anywhere (the gaussian on: non-integer alpha under the over-sized splat)
        res["invalid/alpha_before"] = gf.render_alpha(scene, name, alpha_mode=gf.capi.ALPHA_SUM)[0]
        p = gf.capi.default_params(8224, 16)
        gf.capi.set_camera(p, *fc.grid_camera(8224, 16))
        p.target_format, p.alpha_mode, p.debug_flags = gf.capi.TARGET_RGBA32F, gf.capi.ALPHA_SUM, 4
        try:
            scene.render(p)
            res["invalid/code"] = np.int64(0)
        except gf.capi.MgsError as e:
            res["invalid/code"] = np.int64(e.code)
        res["invalid/alpha_after"] = gf.render_counts(scene, name)[0]
    scene.close()
np.savez(sys.argv[1], **res)
print("CHILD_DONE", flush=True)
