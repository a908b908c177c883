"""child process of test_gpu_compare.test_graph_replay_and_gathered_frames: libmgs reads MGS_GRAPH once per process, so each setting
runs in its own interpreter.  Renders a frame, captures it, renders another pose twice (the second frame replays the captured graph
where graphs are on) and once through mgs_render_gathered (one rank over the RCCL test double named by MGS_RCCL_LIB), and prints the
metrics of each as hex so that the parent can compare bits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, synth  # noqa: E402
import lighting_cases as lc  # noqa: E402


def bits(m):
    return " ".join([str(m.mse_fixed), str(m.flip_fixed)] + [np.float64(v).tobytes().hex() for v in (m.mse, m.psnr, m.flip, m.mse_exact, m.psnr_exact, m.flip_exact)])


scene = mgs.Scene(0)
for arrays, mat in lc.scene_sets():
    scene.add_instance(mgs.SplatSet.from_arrays(**arrays), mat)
scene.commit()
W, H = 320, 240


def params(pose):
    eye = synth.orbit_pose(pose)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    return p


scene.render(params(11))
scene.compare_capture()
p = params(13)
for rep in range(2):
    scene.render(p)
    for mode in (0, 1, 2):
        print("METRICS frame", mode, bits(scene.compare_metrics(mode)), flush=True)
scene.comm_init(0, 1, capi.comm_unique_id())
scene.render_gathered(p)
for mode in (0, 1, 2):
    print("METRICS gathered", mode, bits(scene.compare_metrics(mode)), flush=True)
scene.comm_destroy()
scene.close()
print("CHILD_DONE", flush=True)
