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


def render_alpha(scene, name, strip=None, **params):
    """(alpha plane float32[H,W] of an RGBA32F frame, FrameOut with the frame's statistics); strip = (r0, r1): only the 16-px tile
    rows [r0, r1) are rendered, the plane's other rows hold whatever the frame buffer held"""
    c = fc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.target_format = capi.TARGET_RGBA32F
    if strip is not None:
        p.strip_row_begin, p.strip_row_end = strip
    for k, v in params.items():
        setattr(p, k, v)
    out = scene.render(p, want_stats=True)
    return np.ascontiguousarray(scene.download_frame(p)[..., 3]), out


def render_counts(scene, name):
    """the count mode (additive alpha, opacity gaussian disabled)"""
    return render_alpha(scene, name, alpha_mode=capi.ALPHA_SUM, debug_flags=4)


def sorted_rects(scene, out):
    """(ids uint32[n], rectangles int64[n, 4] as (x0, y0, x1, y1) in bins) of the last frame's sorted splats, in sorted order"""
    _, ids = scene.sort_download(out.sorted_count)
    _, rect = scene.download_projected(ids)
    return ids, fc.unpack_rects(rect)


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
