"""child process of test_gpu_blend.test_binning_paths_blend_the_same: libmgs reads MGS_DIRECT_BIN and MGS_BIN_SHIFT once per process, so
every setting renders in its own interpreter.  Usage: _child_blend.py OUT.npz.  Renders blend_cases.CHILD_CASES in the default and the
additive alpha mode and writes the RGBA32F frames and error flags."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_cases as bc  # noqa: E402
import gpu_blend as gb  # noqa: E402

res = {}
for name in bc.CHILD_CASES:
    scene = gb.build_scene(name)
    for mode, kw in (("default", {}), ("sum", dict(alpha_mode=gb.capi.ALPHA_SUM))):
        img, out, _ = gb.render(scene, name, **kw)
        res[f"{name}/{mode}"], res[f"{name}/{mode}/flags"] = img, np.int64(out.error_flags)
    scene.close()
np.savez(sys.argv[1], **res)
print("CHILD_DONE", flush=True)
