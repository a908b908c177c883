"""How tests/test_gpu_fragments.py and tests/_child_fragments.py render a case of tests/fragment_cases.py on the device."""
import hashlib

import numpy as np

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi
import fragment_cases as fc


def build_scene(name):
    scene = mgs.Scene(0)
    sets = {}
    for arrays, m in fc.case(name)["sets"]:
        if id(arrays) not in sets:
            sets[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
        scene.add_instance(sets[id(arrays)], m)
    scene.commit()
    return scene


def render_alpha(scene, name, **params):
    """(alpha plane float32[H,W] of an RGBA32F frame, FrameOut with the frame's statistics)"""
    c = fc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.target_format = capi.TARGET_RGBA32F
    for k, v in params.items():
        setattr(p, k, v)
    out = scene.render(p, want_stats=True)
    return np.ascontiguousarray(scene.download_frame(p)[..., 3]), out


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
