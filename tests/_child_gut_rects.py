"""child process of test_gpu_gut_records.test_bin_rectangles_with_32x16_px_bins: libmgs reads MGS_BIN_SHIFT once per process, so the
frames with forced bins render in their own interpreter.  Usage: _child_gut_rects.py OUT.npz CASE...  Renders the default 3DGUT frame of
each case of tests/gut_cases.py and writes the sorted ids and their packed bin rectangles (mgs_frame_download_projected_gut)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import gut_cases as gc  # noqa: E402

res = {}
for name in sys.argv[2:]:
    c = gc.case(name)
    scene, sets = mgs.Scene(0), {}
    for arrays, m in c["sets"]:
        if id(arrays) not in sets:
            sets[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
        scene.add_instance(sets[id(arrays)], m)
    scene.commit()
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.pipeline, p.target_format = capi.PIPELINE_3DGUT, capi.TARGET_RGBA32F
    for k, v in c["params"].items():
        setattr(p, k, v)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    ids = scene.sort_download(out.sorted_count)[1][:out.sorted_count]
    res[name + "/ids"], res[name + "/rect"] = ids, scene.download_projected_gut(ids)[1]
    scene.close()
np.savez(sys.argv[1], **res)
print("CHILD_DONE", flush=True)
