"""child process of tests/test_gpu_gut_sensor.py: every frame of the sensor-model tests in one fresh interpreter.
Usage: _child_gut_sensor.py OUT.npz.  For each case of tests/gut_sensor_cases.py the scene is built, the case's sensor is bound
(mgs_frame_set_sensor) and the frames are rendered; what they leave is written to OUT.npz under "<case>/<what>".  The binding rules
(rebinding between replayed frames, unbinding, contexts, the entry points that refuse) are exercised on the `mild` scene and written as
"rules/<what>"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi  # noqa: E402
import gut_sensor_cases as sc  # noqa: E402

UNSUPPORTED = -8
res = {}


def build(name):
    c = sc.case(name)
    scene, sets = mgs.Scene(0), {}
    for arrays, m in c["sets"]:
        if id(arrays) not in sets:
            sets[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
        scene.add_instance(sets[id(arrays)], m)
    scene.commit()
    return scene


def params(name, **kw):
    c = sc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.pipeline, p.target_format, p.sh_degree = capi.PIPELINE_3DGUT, capi.TARGET_RGBA32F, 0
    for k, v in dict(c["params"], **kw).items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def sensor_of(name):
    return capi.sensor_model_from_frame(params(name)).update(**sc.sensor_fields(name))


def refused(call):
    try:
        call()
    except capi.MgsError as e:
        return e.code == UNSUPPORTED and "mgs_frame_set_sensor(handle, NULL)" in str(e)
    return False


for name in sc.CASES:
    c = sc.case(name)
    scene = build(name)
    scene.set_sensor(sensor_of(name))
    # the default frame: the emitted set, the records, the blend of the packed compositor
    p = params(name)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    ids = scene.sort_download(out.sorted_count)[1][:out.sorted_count]
    rec, rect = scene.download_projected_gut(ids)
    res[name + "/ids"], res[name + "/rec"], res[name + "/rect"] = ids, rec, rect
    res[name + "/frustum"] = np.int64(out.frustum_count)
    res[name + "/blend_packed"] = scene.download_frame(p).astype(np.float32)
    p = params(name, surface_outputs=1)
    assert scene.render(p, want_stats=True).error_flags == 0
    res[name + "/blend_tile"] = scene.download_frame(p).astype(np.float32)
    # the count mode (additive alpha, opacity gaussian off): the tile compositor with and without the surface outputs
    p = params(name, alpha_mode=capi.ALPHA_SUM, debug_flags=4)
    assert scene.render(p, want_stats=True).error_flags == 0
    res[name + "/count_plain"] = np.ascontiguousarray(scene.download_frame(p)[..., 3])
    p = params(name, alpha_mode=capi.ALPHA_SUM, debug_flags=4, surface_outputs=1)
    assert scene.render(p, want_stats=True).error_flags == 0
    res[name + "/count_surface"] = np.ascontiguousarray(scene.download_frame(p)[..., 3])
    res[name + "/count_surface_ids"] = scene.download_surface(p)[1]
    # the packed compositor and a stochastic frame with every fragment opaque: the nearest fragment's colour, alpha = "a fragment"
    p = params(name, debug_flags=4)
    assert scene.render(p, want_stats=True).error_flags == 0
    res[name + "/opaque_packed"] = scene.download_frame(p).astype(np.float32)
    p = params(name, debug_flags=4, sort_mode=capi.SORT_STOCHASTIC)
    assert scene.render(p, want_stats=True).error_flags == 0
    res[name + "/opaque_stochastic"] = scene.download_frame(p).astype(np.float32)
    # the sensor's rays
    rays = torch.zeros(c["W"] * c["H"] * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    scene.generate_rays(params(name), rays.data_ptr())
    scene.sync()
    res[name + "/rays"] = rays.cpu().numpy().reshape(c["H"], c["W"], 8)
    scene.close()

# ---- binding rules ----
name = "mild"
scene = build(name)
p = params(name)


def frame(handle, q=p):
    handle.render(q)
    return handle.download_frame(q).astype(np.float32).copy()


plain = frame(scene)
plain2 = frame(scene)                       # (replayed)
scene.set_sensor(sensor_of("mild"))
mild = frame(scene)
mild2 = frame(scene)                        # (replayed with the sensor bound)
scene.set_sensor(sensor_of("strong"))       # rebinding between two replayed frames
strong = frame(scene)
ctx = scene.frame_context()
ctx_plain = frame(ctx)                      # the scene's sensor does not reach its contexts ...
ctx.set_sensor(sensor_of("mild"))
ctx_mild = frame(ctx)
strong_again = frame(scene)                 # ... nor a context's the scene
# the entry points that refuse while a sensor is bound
p3 = params(name, pipeline=capi.PIPELINE_3DGS)
plit = params(name, lighting_mode=1)
res["rules/refuse_3dgs"] = refused(lambda: scene.render(p3))
res["rules/refuse_lit"] = refused(lambda: scene.render(plit))
res["rules/refuse_meshes"] = refused(lambda: scene.render_meshes(p))
res["rules/refuse_traced"] = refused(lambda: scene.render_traced(p))
res["rules/refuse_traced_lit"] = refused(lambda: scene.render_traced_lit(plit))
res["rules/refuse_hybrid"] = refused(lambda: scene.render_hybrid(plit))
after_refusals = frame(scene)               # a refused call leaves the binding and the handle as they were
scene.set_sensor(None)
restored = frame(scene)
works = []
for call in (lambda: scene.render(p3), lambda: scene.render(plit), lambda: scene.render_traced(p), lambda: scene.render_traced_lit(plit),
             lambda: scene.render_hybrid(plit), lambda: scene.render_meshes(p)):
    try:
        call()
        works.append(True)
    except capi.MgsError as e:
        print("after unbinding:", e, flush=True)
        works.append(False)
scene.clear_occluder()                      # (the mesh pass binds its images)
restored_last = frame(scene)
res["rules/works_after_unbinding"] = np.array(works)
for k, v in dict(plain=plain, plain2=plain2, mild=mild, mild2=mild2, strong=strong, ctx_plain=ctx_plain, ctx_mild=ctx_mild, strong_again=strong_again,
                 after_refusals=after_refusals, restored=restored, restored_last=restored_last).items():
    res["rules/" + k] = v
ctx.close()
scene.close()
np.savez(sys.argv[1], **res)
print("CHILD_DONE", flush=True)
