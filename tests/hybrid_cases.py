"""The scenes of the hybrid-frame tests (test_hybrid_cpu.py, test_gpu_hybrid.py), numpy only, built from trace_lit_cases' floor, blob
and fins: frames of 48 x 40 pixels (2.5 workgroup tiles high, partial on both axes; one case is 33 x 25).  A case is one of
trace_lit_cases (sets, V, P, eye, W, H, frame, trace, light, lights, materials) whose frame carries the raster pipeline.
restate_with(case, gbuffer, prepared instances) runs np_hybrid on a G-buffer; oracle_gbuffer(ob, case) makes one on the CPU.
h13 (strip rows: three strips equal the full frame bit for bit) has no scene of its own: it is h01 rendered strip by strip in
_child_hybrid.py (strip_0..2), asserted by test_gpu_hybrid.py::test_determinism_strips_context."""
import functools

import numpy as np

import np_hybrid as nh
import np_lighting as nl
import np_trace_lit as ntl
import trace_cases as tc
import trace_lit_cases as lc

GS, GUT = 0, 1
FRAGILE_CAP = 0.05  # the project's cap


def _case(sets, lights, pipeline, **kw):
    frame = dict(kw.pop("frame", None) or {}, pipeline=pipeline)
    return lc._case(sets, lights, frame=frame, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    scene = lc.join(lc.floor(), lc.blob())
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), intensity=1.0)
    spot = nl.default_light(type=nl.LIGHT_SPOT, position=(-0.2, 1.4, 0.1), direction=(0.1, -1.0, 0.0), range=10.0, intensity=5.0,
                            inner_cone_deg=14.0, outer_cone_deg=24.0)
    far = nl.default_light(position=(6.0, 7.0, 5.0), range=1.0, intensity=50.0)  # nothing of the scene is within its range
    c = {}
    c["h01_3dgs"] = _case([(scene, tc.I4)], [point], GS)
    c["h02_3dgut"] = _case([(scene, tc.I4)], [point], GUT)
    c["h03_fisheye"] = _case([(scene, tc.I4)], [point], GUT, frame=dict(camera_model=1, fov_rad=1.4))
    c["h04_dof"] = _case([(scene, tc.I4)], [point], GUT, frame=dict(dof_mode=1, focus_dist=2.9, aperture=0.004))
    c["h05_three_lights"] = _case([(scene, tc.I4)], [dict(sun, intensity=0.5), spot, far], GS)
    c["h05_without_far"] = _case([(scene, tc.I4)], [dict(sun, intensity=0.5), spot], GS)
    c["h06_headlight"] = _case([(scene, tc.I4)], [], GUT)
    thin = lc.join(lc.floor(), lc.blob(opacity=-2.6, n=12, log_scale=-1.9))
    for tag, st in (("s0", 0.0), ("s1", 1.0)):
        c["h07_translucent_" + tag] = _case([(thin, tc.I4)], [point], GUT,
                                            light=dict(particle_shadow_transmittance_threshold=0.3, particle_shadow_color_strength=st))
    stack = lc.join(lc.floor(), lc.blob(n=60, centre=(0.0, 0.45, 0.0), radius=0.5, opacity=-2.2, seed=21, log_scale=-1.8))
    for k in (4, 32):
        c[f"h08_spp_{k}"] = _case([(stack, tc.I4)], [point], GS, light=dict(particle_shadow_transmittance_threshold=0.05), trace=dict(samples_per_pass=k))
    c["h09_shadows_off"] = _case([(scene, tc.I4)], [point], GS, light=dict(shadows_mode=0))
    c["h10_materials"] = _case([(lc.floor(), tc.trs((1.1, 1.0, 1.1), (0, 1, 0), 20.0, (0.05, 0.0, -0.05))),
                                (lc.blob(), tc.trs((1.2, 1.2, 1.2), (0, 1, 0), 30.0, (0.2, 0.0, 0.0)))], [point], GUT,
                               materials=[dict(lc.SHADED, specular=(0.5, 0.5, 0.5), shininess=64.0), nl.default_material()])
    # a cloud too thin to reach the iso threshold: no pixel has a picked depth, every pixel is discarded
    c["h11_thin_cloud"] = _case([(lc.blob(n=30, centre=(0.0, 0.0, 0.0), radius=1.2, opacity=-3.5, seed=31, log_scale=-2.0), tc.I4)], [point], GS)
    deep = lc.join(lc.floor(n_side=62, half=1.3, seed=15), lc.blob(n=253, seed=16, radius=0.35, log_scale=-3.3))
    deep["scale"][:62 * 62] += np.log(np.float32(0.14))  # 4097 leaves: the shadow rays walk five levels
    c["h12_deep"] = _case([(deep, tc.I4)], [point], GUT, W=33, H=25)
    return c


def prepared(case):
    return [(ntl.prepare_set(a), M) for a, M in case["sets"]]


def restate_with(c, gbuffer, inst, rows=None):
    """gbuffer = (image as stored, picked depth, ids in the caller's order, integrated normal)"""
    L = c["light"]
    kw = lc._trace_kw(c)
    kw.update(no_gauss=bool(c["frame"].get("debug_flags", 0) & 4), sh_only=bool(c["frame"].get("debug_flags", 0) & 2))
    image, depth, ids, normal = gbuffer
    return nh.lit(image, depth, ids, normal, inst, c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"],
                  shadows=L.get("shadows_mode", 0), offset=L.get("particle_shadow_offset", 0.2),
                  threshold=L.get("particle_shadow_transmittance_threshold", 0.8), strength=L.get("particle_shadow_color_strength", 0.0),
                  rows=rows, **kw)


def inst_prefix(case):
    return np.cumsum([0] + [a["positions"].shape[0] for a, _ in case["sets"]])[:-1]


def oracle_gbuffer(ob, case):
    """the CPU oracle's raster frame of the case: (image float32, picked depth, ids, integrated normal)"""
    f = dict(tc.FRAME_DEFAULTS, **{k: v for k, v in case["frame"].items() if k in tc.FRAME_DEFAULTS})
    gut = case["frame"]["pipeline"] == GUT
    kw = dict(camera_model=f["camera_model"], fov_rad=f["fov_rad"] or None, dof_mode=f["dof_mode"], focus_dist=f["focus_dist"],
              aperture=f["aperture"], frame_sample_id=f["frame_sample_id"], kernel_degree=f["kernel_degree"],
              kernel_min_response=f["kernel_min_response"], alpha_clamp=f["alpha_clamp"], pipeline_3dgut=1 if gut else 0)
    inst = ob.make_instances([(ob.PreparedSet(a), M) for a, M in case["sets"]])
    V, P, eye, W, H = case["V"], case["P"], case["eye"], case["W"], case["H"]
    fr = ob.make_frame(V, P, eye, W, H, **kw)
    _, order = ob.sort_stable(*ob.key_cull(fr, inst))
    ftb = ob.make_frame(V, P, eye, W, H, front_to_back=1, **kw)
    if gut:
        depth, ids, nrm = ob.render_surface_gut(fr, inst, order[::-1].copy(), 0.7, normals=True)
        img = ob.render_gut(ftb, inst, order)[0]
    else:
        depth, ids, nrm = ob.render_surface(fr, inst, order[::-1].copy(), 0.7, normals=True)
        img = ob.render(ftb, inst, order=order)[0]
    return img.astype(np.float32), depth, ids, nrm
