"""GPU tests (-m gpu) of the target formats (csrc/target_pixel.h: the one load and the one store of a frame pixel) through every
compositor that writes the frame: the kernels compute the same fp32 pixel whatever the format, so an RGBA16F or RGBA8 frame
must equal the host conversion (np_lighting.to_target, checked by test_lighting_cpu.py::test_target_rounding_helpers) of the
RGBA32F frame of the same configuration bit for bit, and a temporally accumulated frame must equal the same lerp applied to
what was stored.  The frame is 40 x 24: ragged against the 16-pixel tiles, the 32 x 16 regions and the x + 8 second pixel of
k_composite_gut2; the strip cut is its second tile row (8 of 16 pixel rows exist)."""
import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth
import np_lighting as nl

pytestmark = pytest.mark.gpu
W, H = 40, 24
FORMATS = {"f32": capi.TARGET_RGBA32F, "f16": capi.TARGET_RGBA16F, "u8": capi.TARGET_RGBA8}
STRIPS = {"full": (0, 0), "strip": (1, 2)}  # tile rows; (0, 0) = the whole frame
GUT, GS = capi.PIPELINE_3DGUT, capi.PIPELINE_3DGS
DOF = dict(dof_mode=capi.DOF_FIXED_FOCUS, focus_dist=3.0, aperture=0.05)
CONFIGS = {  # name: (frame parameters, occluder bound)
    "3dgut plain (k_composite_gut2, XT 0)": (dict(pipeline=GUT), False),
    "3dgut depth of field (k_composite_gut2, XT 1)": (dict(pipeline=GUT, frame_sample_id=3, **DOF), False),
    "3dgut surface outputs (k_composite_gut, XT 2)": (dict(pipeline=GUT, surface_outputs=1), False),
    "3dgut occluder (k_composite_gut, OCC)": (dict(pipeline=GUT), True),
    "3dgs plain (k_composite)": (dict(pipeline=GS), False),
}


@pytest.fixture(scope="module")
def scene_small():
    sc = synth.make_scene(600, seed=77)
    keep = np.linalg.norm(sc["positions"], axis=1) < 3.0  # the object cluster without the shell of splats around the camera
    sc = {k: np.ascontiguousarray(v[keep]) for k, v in sc.items()}
    assert 300 <= int(keep.sum()) <= 600
    sc["scale"] = sc["scale"] + np.float32(2.5)  # footprints of a pixel and more at this frame size
    scene = mgs.Scene(0)
    scene.add_instance(mgs.SplatSet.from_arrays(**sc))
    scene.commit()
    yield scene
    scene.close()


def frame_params(**kw):
    eye = synth.orbit_pose(5)
    right = np.cross([0.0, 1.0, 0.0], eye)
    centre = 4.0 * right / np.linalg.norm(right)  # looks past the cluster: it fills one side of the frame, the other side is empty
    V, P = mgs.camera_lookat_perspective(eye, [float(c) for c in centre], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def rows_of(strip):
    b, e = STRIPS[strip]
    return (0, H) if e == 0 else (b * 16, min(e * 16, H))


def render(scene, p, fmt, strip):
    p.target_format = FORMATS[fmt]
    p.strip_row_begin, p.strip_row_end = STRIPS[strip]
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    y0, y1 = rows_of(strip)
    return scene.download_frame(p)[y0:y1].copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32 if a.dtype == np.float32 else np.uint8)


def assert_premises(f32, name):
    """no case passes vacuously: the frame is not all zero, a value lies strictly between two RGBA8 steps, a pixel lies outside
    every splat (coverage alpha exactly 0)"""
    v = np.clip(f32, 0.0, 1.0).astype(np.float64) * 255.0
    assert f32.any(), name
    assert (v != np.round(v)).any(), name
    assert (f32[..., 3] == 0.0).any() and (f32[..., 3] > 0.0).any(), name


@pytest.mark.parametrize("strip", list(STRIPS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_f16_and_u8_frames_are_the_host_conversion_of_the_f32_frame(scene_small, name, strip):
    scene = scene_small
    kw, occluder = CONFIGS[name]
    if occluder:  # left half: nothing in front of the splats; right half: geometry in front of all of them; a colour behind both
        depth = np.ones((H, W), np.float32)
        depth[:, W // 2:] = 0.0
        scene.upload_occluder(depth, np.random.default_rng(3).random((H, W, 4), dtype=np.float32))
    try:
        p = frame_params(**kw)
        f32 = render(scene, p, "f32", strip)
        assert f32.dtype == np.float32
        assert_premises(f32, name)
        for fmt in ("f16", "u8"):
            got, want = render(scene, p, fmt, strip), nl.to_target(f32, fmt)
            diff = int((bits(got) != bits(want)).sum())
            print(f"{name} {strip} {fmt}: {diff} of {want.size} channel values differ from the converted f32 frame")
            assert got.dtype == want.dtype and diff == 0, (name, strip, fmt)
    finally:
        if occluder:
            scene.clear_occluder()


@pytest.mark.parametrize("strip", list(STRIPS))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_accumulated_frame_is_the_lerp_of_what_was_stored(scene_small, fmt, strip):
    """k_post_accumulate (post.comp.slang:29-43) on samples 0 and 1: load the stored frame, lerp in fp32 against the fp32
    accumulator, store back.  The weight of sample 1 is 1/2, so the product of the lerp is exact and a fused multiply-add
    rounds like the separate operations.  Depth of field makes the two samples differ.  The strip case starts the pass at the
    strip's first row."""
    scene = scene_small
    p = frame_params(pipeline=GUT, **DOF)
    assert_premises(render(scene, p, "f32", strip), fmt)
    singles = []
    for k in (0, 1):
        p.frame_sample_id = k
        singles.append(nl.from_target(render(scene, p, fmt, strip)))
    assert not np.array_equal(singles[0], singles[1])
    p.temporal_sampling = 1
    p.frame_sample_id = 0
    got0 = render(scene, p, fmt, strip)
    main = singles[0]  # lerp(main, aux1, 1)
    assert np.array_equal(bits(got0), bits(nl.to_target(main, fmt)))
    p.frame_sample_id = 1
    got1 = render(scene, p, fmt, strip)
    main = main + np.float32(0.5) * (singles[1] - main)
    assert main.dtype == np.float32
    diff = int((bits(got1) != bits(nl.to_target(main, fmt))).sum())
    print(f"accumulated {fmt} {strip}: {diff} of {main.size} channel values differ from the lerp of the stored frames")
    assert diff == 0
    assert not np.array_equal(nl.from_target(got1), singles[1])  # (the accumulated frame is not just the last sample)
