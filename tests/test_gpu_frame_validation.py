"""GPU test (-m gpu) of mgs_render's parameter validation (validateFrameParams, csrc/api_frame.hip): every rejection, one invalid
field at a time, with its return code and message, and the handle untouched by it — the valid frame rendered after each rejected
call is bit for bit the one rendered before."""
import math

import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth

pytestmark = pytest.mark.gpu

W = H = 64
INVALID_ARG, UNSUPPORTED = capi.ERR_INVALID_ARG, capi.ERR_UNSUPPORTED
GS, GUT = capi.PIPELINE_3DGS, capi.PIPELINE_3DGUT
DOF_MSG = "depth of field needs a finite aperture >= 0 and a finite focus_dist > 0"
RESPONSE_MSG = "alpha_clamp must be in (1/255, 1] and kernel_min_response in [0, 1)"

# (name, pipeline of the otherwise valid frame, the invalid fields, return code, text of mgs_last_error())
CASES = [
    ("target_format_high", GS, dict(target_format=3), INVALID_ARG, "target_format must be MGS_TARGET_RGBA16F / RGBA32F / RGBA8"),
    ("target_format_low", GS, dict(target_format=-1), INVALID_ARG, "target_format must be MGS_TARGET_RGBA16F / RGBA32F / RGBA8"),
    ("pipeline", GS, dict(pipeline=2), INVALID_ARG, "pipeline must be MGS_PIPELINE_3DGS or MGS_PIPELINE_3DGUT"),
    ("camera_model", GS, dict(camera_model=2), INVALID_ARG, "camera_model out of range"),
    ("camera_model_gut", GUT, dict(camera_model=-1), INVALID_ARG, "camera_model out of range"),
    ("extent_method", GUT, dict(extent_method=2), INVALID_ARG, "extent_method out of range"),
    ("alpha_clamp_low", GUT, dict(alpha_clamp=1.0 / 255.0), INVALID_ARG, RESPONSE_MSG),
    ("alpha_clamp_high", GUT, dict(alpha_clamp=1.5), INVALID_ARG, RESPONSE_MSG),
    ("alpha_clamp_nan", GUT, dict(alpha_clamp=math.nan), INVALID_ARG, RESPONSE_MSG),
    ("kernel_min_response_one", GUT, dict(kernel_min_response=1.0), INVALID_ARG, RESPONSE_MSG),
    ("kernel_min_response_negative", GUT, dict(kernel_min_response=-0.5), INVALID_ARG, RESPONSE_MSG),
    ("dof_on_3dgs", GS, dict(dof_mode=capi.DOF_FIXED_FOCUS), UNSUPPORTED, "depth of field is a feature of the 3DGUT pipeline"),
    ("dof_aperture_negative", GUT, dict(dof_mode=capi.DOF_FIXED_FOCUS, aperture=-1.0), INVALID_ARG, DOF_MSG),
    ("dof_aperture_infinite", GUT, dict(dof_mode=capi.DOF_FIXED_FOCUS, aperture=math.inf), INVALID_ARG, DOF_MSG),
    ("dof_focus_zero", GUT, dict(dof_mode=capi.DOF_FIXED_FOCUS, focus_dist=0.0), INVALID_ARG, DOF_MSG),
    ("dof_focus_nan", GUT, dict(dof_mode=capi.DOF_FIXED_FOCUS, focus_dist=math.nan), INVALID_ARG, DOF_MSG),
    ("kernel_degree_6", GUT, dict(kernel_degree=6), INVALID_ARG, "kernel_degree must be one of 0, 1, 2, 3, 4, 5, 8"),
    ("kernel_degree_negative", GUT, dict(kernel_degree=-1), INVALID_ARG, "kernel_degree must be one of 0, 1, 2, 3, 4, 5, 8"),
    ("normal_method", GUT, dict(normal_method=2), INVALID_ARG, "normal_method must be MGS_NORMAL_MAX_DENSITY_PLANE or MGS_NORMAL_ISO_SURFACE"),
    ("sort_mode", GS, dict(sort_mode=2), INVALID_ARG, "sort_mode must be MGS_SORT_GPU_RADIX, MGS_SORT_CPU_ASYNC or MGS_SORT_STOCHASTIC"),
    ("sort_mode_gut", GUT, dict(sort_mode=4), INVALID_ARG, "sort_mode must be MGS_SORT_GPU_RADIX, MGS_SORT_CPU_ASYNC or MGS_SORT_STOCHASTIC"),
    ("dof_mode", GUT, dict(dof_mode=2), INVALID_ARG, "dof_mode / frame_sample_id out of range"),
    ("frame_sample_id", GS, dict(frame_sample_id=-1), INVALID_ARG, "dof_mode / frame_sample_id out of range"),
    ("lighting_mode_high", GS, dict(lighting_mode=3), INVALID_ARG, "lighting_mode must be MGS_LIGHTING_DISABLED, MGS_LIGHTING_DIRECT or MGS_LIGHTING_INDIRECT"),
    ("lighting_mode_low", GUT, dict(lighting_mode=-1), INVALID_ARG, "lighting_mode must be MGS_LIGHTING_DISABLED, MGS_LIGHTING_DIRECT or MGS_LIGHTING_INDIRECT"),
    ("lighting_stochastic", GS, dict(lighting_mode=capi.LIGHTING_DIRECT, sort_mode=capi.SORT_STOCHASTIC), UNSUPPORTED,
     "lighting of MGS_SORT_STOCHASTIC frames is not supported"),
    ("occluder_size", GS, dict(occluder=(H // 2, W)), INVALID_ARG, f"the bound occluder images are {W}x{H // 2}, the frame is {W}x{H}"),
    ("occluder_stochastic", GS, dict(occluder=(H, W), sort_mode=capi.SORT_STOCHASTIC), UNSUPPORTED,
     "MGS_SORT_STOCHASTIC with an occluder bound is not supported"),
]


def valid_params(pipeline):
    eye = synth.orbit_pose(5)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    p.pipeline = pipeline
    return p


def render_bits(scene, p):
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    return scene.download_frame(p).view(np.uint16).copy()


def test_every_rejection_of_mgs_render_leaves_the_handle_as_it_was():
    scene = mgs.Scene(0)
    scene.add_instance(mgs.SplatSet.from_arrays(**synth.make_scene(1000, seed=11)))
    scene.commit()
    try:
        before = {pl: render_bits(scene, valid_params(pl)) for pl in (GS, GUT)}
        for pl in (GS, GUT):
            assert np.count_nonzero(before[pl]) > W * H // 8, "the valid frame shows next to nothing: the comparison would be empty"
        lib = capi.load_library()
        for name, pipeline, fields, code, text in CASES:
            p = valid_params(pipeline)
            fields = dict(fields)
            occluder = fields.pop("occluder", None)
            if occluder:
                scene.upload_occluder(np.ones(occluder, np.float32))
            for k, v in fields.items():
                assert hasattr(p, k), k
                setattr(p, k, v)
            with pytest.raises(mgs.MgsError) as e:
                scene.render(p)
            message = lib.mgs_last_error().decode()
            assert e.value.code == code, (name, e.value.code, message)
            assert text in message and message.startswith("frame: "), (name, message)
            if occluder:
                scene.clear_occluder()
            after = render_bits(scene, valid_params(pipeline))
            assert np.array_equal(after, before[pipeline]), f"{name}: the valid frame after the rejected call differs"
        # the record hooks answer for a frame of their own pipeline only, and for the scene's ids only
        for pl, own, other in ((GS, scene.download_projected, scene.download_projected_gut), (GUT, scene.download_projected_gut, scene.download_projected)):
            render_bits(scene, valid_params(pl))
            rec, rect = own([0, 999])
            assert rec.shape == (2, 24 if pl == GUT else 10) and rect.shape == (2,)
            with pytest.raises(mgs.MgsError) as e:
                other([0])
            assert e.value.code == capi.ERR_STATE and "frame rendered yet" in lib.mgs_last_error().decode()
            with pytest.raises(mgs.MgsError) as e:
                own([0, 1000])
            assert e.value.code == INVALID_ARG and "id out of range" in lib.mgs_last_error().decode()
            assert np.array_equal(render_bits(scene, valid_params(pl)), before[pl])
    finally:
        scene.close()
