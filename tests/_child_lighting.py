"""child process of test_gpu_lighting.test_graph_replay_equals_plain_launches: libmgs reads MGS_GRAPH once per process, so each
setting renders the lit frames of the lighting cases in its own interpreter and prints the SHA-1 of frames and side outputs"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import lighting_cases as lc  # noqa: E402

scene = mgs.Scene(0)
for arrays, m in lc.scene_sets():
    scene.add_instance(mgs.SplatSet.from_arrays(**arrays), m)
scene.commit()
V, P, eye = lc.camera_matrices(mgs.camera_lookat_perspective)
hh = hashlib.sha1()
for name, (gut, target, lights, mats, occluder) in lc.CASES.items():
    if occluder:
        continue
    p = capi.default_params(lc.W, lc.H)
    capi.set_camera(p, V, P, eye)
    p.pipeline = gut
    p.target_format = {"f32": capi.TARGET_RGBA32F, "f16": capi.TARGET_RGBA16F, "u8": capi.TARGET_RGBA8}[target]
    p.lighting_mode = capi.LIGHTING_DIRECT
    scene.set_lights([capi.make_light(**l) for l in lights])
    for k, m in enumerate(mats):
        scene.set_material(k, capi.make_material(**m))
    for _ in range(2):  # the second frame replays the captured graph where graphs are on
        scene.render(p)
        hh.update(np.ascontiguousarray(scene.download_frame(p)).tobytes())
    hh.update(scene.download_consolidated_depth(p).tobytes())
print("FRAMES_SHA1", hh.hexdigest())
