"""How tests/test_gpu_blend.py and tests/_child_blend.py render a case of tests/blend_cases.py on the device."""
import numpy as np

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi
import blend_cases as bc


def build_scene(name):
    scene = mgs.Scene(0)
    sets = {}
    for arrays, m in bc.case(name)["sets"]:
        if id(arrays) not in sets:
            sets[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
        scene.add_instance(sets[id(arrays)], m)
    scene.commit(*bc.case(name).get("formats", (capi.FORMAT_FLOAT32, capi.FORMAT_FLOAT32)))
    return scene


def params(name, strip=None, **kw):
    c = bc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.target_format = capi.TARGET_RGBA32F
    p.sh_degree = 0
    if strip is not None:
        p.strip_row_begin, p.strip_row_end = strip
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def render(scene, name, strip=None, **kw):
    """(RGBA32F frame [H,W,4], FrameOut with the frame's statistics, the frame's parameters)"""
    p = params(name, strip, **kw)
    out = scene.render(p, want_stats=True)
    return scene.download_frame(p).copy(), out, p
