"""The cases of the deferred-lighting tests, shared by tests/test_lighting_cpu.py (which establishes the ambiguity cap and the
float32-vs-float64 difference on the oracle's G-buffer) and tests/test_gpu_lighting.py (which holds the kernel to them)."""
import numpy as np

from vk_gaussian_splatting_amd import synth
import np_lighting as nl

W, H = 320, 240
POSE = 11
N_A, N_B = 40000, 20000
MODEL_B = np.array([[1, 0, 0, 0.8], [0, 1, 0, 0.3], [0, 0, 1, -0.5], [0, 0, 0, 1]], np.float32)
ISO = 0.7

MASK_CAP = 0.005  # at most 0.5 % of the lit pixels may hang on a comparison (a condition on the cases, not on the code)

# The largest float32-vs-float64 difference of np_lighting over all cases below on the oracle's G-buffer, outside the ambiguity
# mask, |a - b| / max(1, |b|) over rgb: MEASURED by test_lighting_cpu.py::test_cap_and_tolerance_from_the_reference_alone (which
# fails if the measurement leaves [F32_VS_F64 / 2, F32_VS_F64]).  It comes from shininess 2000: pow multiplies the relative error
# of its base, a dot product of two normalised fp32 vectors, by the exponent.
F32_VS_F64 = 1.0e-3  # measured 9.57e-4 (gs_f32_headlight; 8.4e-4 .. 8.6e-4 on the mixed-light cases with shininess 2000)
# the kernel's bar on an RGBA32F target: 4 x that (another operation order, fma contraction and another pow than numpy's)
GPU_BAR = 4.0 * F32_VS_F64

LIGHTS_MIXED = [
    nl.default_light(type=nl.LIGHT_DIRECTIONAL, color=(1.0, 0.9, 0.8), intensity=0.8, direction=(-0.3, -1.0, -0.2)),
    nl.default_light(type=nl.LIGHT_POINT, color=(0.4, 0.6, 1.0), intensity=1.5, position=(1.0, 2.0, 1.0), range=5.0, attenuation_mode=0),  # its range cuts through the scene
    nl.default_light(type=nl.LIGHT_POINT, color=(1.0, 0.3, 0.3), intensity=2.0, position=(-2.0, 0.5, -1.0), range=8.0, attenuation_mode=1),
    nl.default_light(type=nl.LIGHT_SPOT, color=(0.9, 1.0, 0.7), intensity=6.0, position=(0.0, 4.0, 0.0), direction=(0.0, -1.0, 0.0),
                     inner_cone_deg=20.0, outer_cone_deg=35.0, range=20.0, attenuation_mode=2),
    nl.default_light(type=nl.LIGHT_SPOT, color=(0.6, 0.6, 1.0), intensity=4.0, position=(-3.0, 1.0, 2.0), direction=(3.0, -1.0, -2.0),
                     inner_cone_deg=15.0, outer_cone_deg=40.0, range=6.0, attenuation_mode=3),
]
MATS_A = [nl.default_material(ambient=(0.05, 0.05, 0.05), diffuse=(0.8, 0.8, 0.8), specular=(0.5, 0.5, 0.5), emission=(0, 0, 0), shininess=4.0),
          nl.default_material(ambient=(0, 0, 0), diffuse=(0.6, 0.5, 0.4), specular=(1.0, 1.0, 1.0), emission=(0.2, 0.2, 0.2), shininess=2000.0)]
MATS_B = [nl.default_material(ambient=(0.1, 0.1, 0.2), diffuse=(0.5, 0.7, 0.9), specular=(0.3, 0.3, 0.3), emission=(0, 0, 0), shininess=32.0),
          nl.default_material()]

# name -> (3DGUT pipeline, target, lights, materials, occluder with background)
CASES = {
    "gs_f32_mixed": (0, "f32", LIGHTS_MIXED, MATS_A, False),
    "gs_f16_mixed": (0, "f16", LIGHTS_MIXED, MATS_A, False),
    "gs_u8_mixed": (0, "u8", LIGHTS_MIXED, MATS_B, False),
    "gs_f32_headlight": (0, "f32", [], MATS_A, False),
    "gut_f32_mixed": (1, "f32", LIGHTS_MIXED, MATS_A, False),
    "gut_f16_headlight": (1, "f16", [], MATS_B, False),
    "gs_f32_mixed_occluder": (0, "f32", LIGHTS_MIXED, MATS_B, True),
}


def _open_sky(sc):
    """the synthetic scene without its background shell above y = 0.5: part of the frame sees no splat at all (pixels that pass
    through) and the fringe of the rest never reaches the depth threshold (lit pixels without a picked id)"""
    pos = sc["positions"]
    keep = (np.linalg.norm(pos, axis=1) < 3.9) | (pos[:, 1] < 0.5)
    return {k: np.ascontiguousarray(v[keep]) for k, v in sc.items()}


_SETS = []


def scene_sets():
    """[(arrays, model matrix or None)]: two instances of different splat sets"""
    if not _SETS:
        _SETS.extend([(_open_sky(synth.make_scene(N_A, seed=21)), None), (_open_sky(synth.make_scene(N_B, seed=22)), MODEL_B)])
    return _SETS


def inst_prefix():
    """first global id of each instance"""
    return [0, scene_sets()[0][0]["positions"].shape[0]]


def camera_matrices(lookat_perspective):
    eye = synth.orbit_pose(POSE)
    V, P = lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    return V, P, eye


def occluder_images(level):
    """the caller's geometry of the occluder case: a wall at window depth `level` over the right half, a background gradient"""
    depth = np.ones((H, W), np.float32)
    depth[:, W // 2:] = np.float32(level)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    bg = np.stack([xx / W, yy / H, 0.25 + 0.5 * xx / W, np.ones_like(xx)], -1).astype(np.float32)
    return depth, bg


def half_step(expected_stored):
    """half a unit of the target's last place at each stored value, as a float32 array"""
    a = np.asarray(expected_stored)
    if a.dtype == np.uint8:
        return np.full(a.shape, 0.5 / 255.0, np.float32)
    if a.dtype == np.float16:
        with np.errstate(invalid="ignore", over="ignore"):
            return (np.spacing(np.abs(a)).astype(np.float32) * 0.5)
    return np.zeros(a.shape, np.float32)


def pixel_ok(got_stored, expected, target, bar):
    """per pixel: every channel of the stored frame within bar * max(1, |expected|) + half a unit of the target's last place of the
    expected value rounded to the target"""
    e_st = nl.to_target(expected, target)
    e, g = nl.from_target(e_st), nl.from_target(got_stored)
    with np.errstate(invalid="ignore"):
        tol = bar * np.maximum(1.0, np.abs(e)) + half_step(e_st)
        ok = (np.abs(g - e) <= tol) | (np.isnan(g) & np.isnan(e)) | ((g == e) & np.isinf(e))
    return ok.all(axis=-1), np.where(np.isfinite(e) & np.isfinite(g), np.abs(g - e) / np.maximum(1.0, np.abs(e)), 0.0)
