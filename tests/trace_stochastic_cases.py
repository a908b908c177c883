"""The scenes of the stochastic trace strategies' tests (test_trace_stochastic_cpu.py, test_gpu_trace_stochastic.py), numpy only.
A case is a case of trace_cases.py (same keys) plus "commit": None or "u8" (SH and colours committed as uint8).  Frames are 20 x 12:
a partial 16-pixel tile and partial 8 x 8 wave tiles on both axes.  ray_hits(name) runs the restatement's per-ray part once per
process; do not modify its result."""
import functools

import numpy as np

import np_trace
import np_trace_stochastic as nts
import trace_cases as tc

W, H = 20, 12


def _case(sets, eye, commit=None, W=W, H=H, **kw):
    return dict(tc._case(sets, eye, W=W, H=H, **kw), commit=commit)


def ties():
    """200 particles of which 160..199 are bit-identical copies (centre, log-scale, quaternion) of 0..39 with other colours, built like
    trace_cases._ties.  Copies share a Morton code and the commit sort keeps equal codes in the caller's order, so a pair alone cannot
    tell the caller's order from the storage order: the ring case does that."""
    a = tc.cloud(160, 84, log_scale=-1.9)
    a["scale"][:40] += np.float32(0.5)
    a["f_dc"][:40] = 2.5
    a["opacity"][:] = np.maximum(a["opacity"], np.float32(-2.0))
    b = {k: np.concatenate([v, v[:40]]) for k, v in a.items()}
    b["f_dc"][160:] = -2.5
    return b


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["a_faint_k04"] = _case([(tc.cloud(300, 81, log_scale=-1.9, opacity_mean=-1.2), tc.I4)], (0.3, 0.2, 3.0), trace=dict(samples_per_pass=4))
    c["b_cloud_k18"] = _case([(tc.cloud(450, 92, log_scale=-2.0), tc.I4)], (0.3, 0.2, 3.0), trace=dict(samples_per_pass=18))
    c["c_two_instances_k32"] = _case([(tc.cloud(220, 83, log_scale=-1.8, opacity_mean=-1.0), tc.trs((1.4, 0.8, 1.0), (1, 2, 0.5), 35.0, (-0.5, 0.1, 0.0))),
                                      (tc.cloud(180, 85, sh_coeffs=3, log_scale=-2.0), tc.trs((0.8, 0.8, 0.8), (0, 1, 0), -20.0, (0.7, -0.1, -0.4)))],
                                     (0.2, 0.5, 3.4), trace=dict(samples_per_pass=32))
    c["d_fisheye_k04"] = _case([(tc.cloud(400, 86, half=1.5, log_scale=-1.7, opacity_mean=-0.5), tc.I4)], (0.1, 0.2, 2.2),
                               frame=dict(camera_model=1, fov_rad=2.4), trace=dict(samples_per_pass=4))
    c["e_u8_k18"] = _case([(tc.cloud(250, 87, log_scale=-1.9), tc.I4)], (0.3, 0.2, 3.0), commit="u8")
    # without adaptive clamping a faint particle is a candidate (response above the proxy's) that particleProcessHit does not accept
    c["i_no_clamping_k04"] = _case([(tc.cloud(300, 93, log_scale=-1.9, opacity_mean=-2.5), tc.I4)], (0.3, 0.2, 3.0),
                                   trace=dict(samples_per_pass=4, kernel_adaptive_clamping=0))
    c["f_empty"] = _case([], (0.0, 0.0, 3.0))
    c["g_ties"] = _case([(ties(), tc.I4)], (0.3, 0.2, 3.0), frame=dict(debug_flags=4))
    # eight different particles with bit-identical t on the central ray, stored in (nearly) the reverse of the caller's order (trace_cases._ring)
    c["h_ring"] = dict(_case([(tc._ring(), tc.I4)], (0.0, 0.0, 3.0), W=33, H=25, frame=dict(debug_flags=4)), exact_ties=((12, 16, 0, frozenset(range(tc.RING))),))
    return c


def frame_trace(case):
    return dict(tc.FRAME_DEFAULTS, **case["frame"]), dict(tc.TRACE_DEFAULTS, **case["trace"])


def ray_hits_with(case, sets_prepared, **frame_over):
    f, t = frame_trace(case)
    f.update(frame_over)
    return nts.ray_hits(sets_prepared, case["V"], case["P"], case["W"], case["H"], adaptive_clamping=bool(t["kernel_adaptive_clamping"]),
                        kernel_degree=f["kernel_degree"], kernel_min_response=f["kernel_min_response"], alpha_clamp=f["alpha_clamp"],
                        alpha_cull=f["alpha_cull_threshold"], sh_degree=f["sh_degree"], fisheye=f["camera_model"] == 1, fov_rad=f["fov_rad"],
                        thin=f["thin_particle_threshold"], sh_only=bool(f["debug_flags"] & 2), no_gauss=bool(f["debug_flags"] & 4),
                        normal_method=f["normal_method"])


def prepared(case):
    return [(np_trace.prepare_set(a), M) for a, M in case["sets"]]


@functools.lru_cache(maxsize=None)
def ray_hits(name):
    case = cases()[name]
    return ray_hits_with(case, prepared(case))


def pass_sample(name, sample_id, R=None, **over):
    _, t = frame_trace(cases()[name])
    t.update(over)
    return nts.pass_stochastic(R or ray_hits(name), sample_id, samples_per_pass=t["samples_per_pass"], max_passes=t["max_passes"],
                               min_transmittance=t["min_transmittance"], depth_iso_threshold=t["depth_iso_threshold"])


SAMPLE_IDS = (0, 5)
STAT_CASE = "a_faint_k04"      # the convergence test's case: many passes, many rejections
N_STAT = 4096
