"""The scenes of the traced-pipeline tests (test_trace_cpu.py, test_gpu_trace.py), numpy only: every case is small enough for the
float64 brute-force restatement (np_trace.py) to take a second or two.  A case = dict(sets=[(arrays, M)], V, P, eye, W, H,
frame={MgsFrameParams overrides}, trace={MgsTraceParams overrides}); restate(case) runs the restatement once per process."""
import functools

import numpy as np

import np_trace


def lookat(eye, c, up=(0, 1, 0)):
    eye, c, up = (np.asarray(a, np.float64) for a in (eye, c, up))
    f = c - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = s, u, -f
    V[0, 3], V[1, 3], V[2, 3] = -s @ eye, -u @ eye, f @ eye
    return V.astype(np.float32)


def persp(fov_deg, aspect, n=0.1, f=100.0):
    t = np.tan(np.radians(fov_deg) / 2)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[2, 2], P[3, 2], P[2, 3] = 1 / (aspect * t), 1 / t, f / (n - f), -1, -(f * n) / (f - n)
    return P


def cloud(n, seed, half=1.0, log_scale=-2.4, sh_coeffs=15, opacity_mean=0.5):
    rng = np.random.Generator(np.random.PCG64(seed))
    rot = rng.standard_normal((n, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    return dict(positions=rng.uniform(-half, half, (n, 3)).astype(np.float32),
                f_dc=rng.standard_normal((n, 3)).astype(np.float32),
                f_rest=(rng.standard_normal((n, 3 * sh_coeffs)) * 0.12).astype(np.float32),
                opacity=(rng.standard_normal(n) * 1.5 + opacity_mean).astype(np.float32),
                scale=(log_scale + rng.standard_normal((n, 3)) * 0.35).astype(np.float32), rotation=rot)


def trs(scale, axis, angle_deg, translation):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(angle_deg)), np.sin(np.radians(angle_deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(scale)
    M[:3, 3] = translation
    return M.astype(np.float32)


I4 = np.eye(4, dtype=np.float32)


def _case(sets, eye, target=(0, 0, 0), W=48, H=36, fov=50.0, frame=None, trace=None):
    V = lookat(eye, target)
    return dict(sets=sets, V=V, P=persp(fov, W / H), eye=np.asarray(eye, np.float32), W=W, H=H, frame=dict(frame or {}), trace=dict(trace or {}))


def _special_d():
    a = cloud(500, 41)
    a["scale"][0] = (np.log(1.5), np.log(0.004), np.log(0.004))   # a needle through the cloud
    a["positions"][0] = (0.1, 0.05, 0.0)
    a["opacity"][0] = 3.0
    a["scale"][1] = np.log(2.5)                                    # one scene-sized splat
    a["positions"][1] = (0.0, 0.0, -0.5)
    a["opacity"][1] = -1.5
    return a


def _special_l():
    a = cloud(300, 43)
    a["opacity"][5] = -9.0            # density far below the cull threshold: no leaf, no hit
    a["positions"][5] = (0.0, 0.0, 0.9)
    a["scale"][5] = np.log(0.5)
    a["scale"][6, 1] = np.nan         # non-finite bound: no leaf, no hit
    return a


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["a_outside"] = _case([(cloud(800, 11, log_scale=-2.7), I4)], (0.3, 0.4, 3.2), W=64, H=48)
    c["b_inside"] = _case([(cloud(400, 12, log_scale=-2.1), I4)], (0.05, 0.02, 0.1), target=(0.3, 0.1, -1.0), W=32, H=24, fov=70.0)
    c["c_two_instances"] = _case([(cloud(500, 13), trs((1.6, 0.7, 1.0), (1, 2, 0.5), 35.0, (-0.6, 0.1, 0.0))),
                                  (cloud(400, 14, sh_coeffs=3), trs((0.8, 0.8, 0.8), (0, 1, 0), -20.0, (0.9, -0.1, -0.4)))], (0.2, 0.6, 3.6))
    c["d_needle_and_giant"] = _case([(_special_d(), I4)], (0.4, 0.3, 3.0))
    for n in (1, 7, 9, 64, 65, 513):
        c[f"e_leaves_{n}"] = _case([(cloud(n, 20 + n, half=0.7, log_scale=-1.9 if n < 100 else -2.6), I4)], (0.2, 0.2, 2.6), W=32, H=24)
    c["f_many_passes"] = _case([(cloud(450, 15, log_scale=-2.2), I4)], (0.3, 0.2, 3.0), trace=dict(samples_per_pass=4))
    c["g_out_of_passes"] = _case([(cloud(450, 16, log_scale=-2.1, opacity_mean=-1.0), I4)], (0.3, 0.2, 3.0), trace=dict(samples_per_pass=2, max_passes=3))
    c["h_fisheye"] = _case([(cloud(900, 17, half=1.5), I4)], (0.1, 0.2, 2.2), frame=dict(camera_model=1, fov_rad=2.4))
    for sid in (0, 3):
        c[f"i_dof_{sid}"] = _case([(cloud(600, 18), I4)], (0.3, 0.3, 3.0), W=32, H=24,
                                  frame=dict(dof_mode=1, focus_dist=3.0, aperture=0.01, frame_sample_id=sid))
    for deg in (0, 3):
        c[f"j_degree_{deg}"] = _case([(cloud(600, 19), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(kernel_degree=deg))
    c["k_no_adaptive_clamping"] = _case([(cloud(450, 31), I4)], (0.3, 0.3, 3.0), W=32, H=24, trace=dict(kernel_adaptive_clamping=0))
    c["l_no_leaf"] = _case([(_special_l(), I4)], (0.2, 0.2, 3.0), W=32, H=24)
    c["m_empty"] = _case([], (0.0, 0.0, 3.0), W=32, H=24)
    return c


FRAME_DEFAULTS = dict(kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull_threshold=1.0 / 255.0, sh_degree=3,
                      camera_model=0, fov_rad=0.0, dof_mode=0, focus_dist=1.3, aperture=0.001, frame_sample_id=0)
TRACE_DEFAULTS = dict(samples_per_pass=18, max_passes=200, min_transmittance=0.01, kernel_adaptive_clamping=1, depth_iso_threshold=0.7)


def restate_with(case, sets_prepared, rows=None, **extra):
    f = dict(FRAME_DEFAULTS, **case["frame"])
    t = dict(TRACE_DEFAULTS, **case["trace"])
    dof = (f["focus_dist"], f["aperture"], f["frame_sample_id"]) if f["dof_mode"] else None
    return np_trace.trace(sets_prepared, case["V"], case["P"], case["W"], case["H"], samples_per_pass=t["samples_per_pass"],
                          max_passes=t["max_passes"], min_transmittance=t["min_transmittance"],
                          adaptive_clamping=bool(t["kernel_adaptive_clamping"]), depth_iso_threshold=t["depth_iso_threshold"],
                          kernel_degree=f["kernel_degree"], kernel_min_response=f["kernel_min_response"], alpha_clamp=f["alpha_clamp"],
                          alpha_cull=f["alpha_cull_threshold"], sh_degree=f["sh_degree"], fisheye=f["camera_model"] == 1,
                          fov_rad=f["fov_rad"], dof=dof, rows=rows, **extra)


@functools.lru_cache(maxsize=None)
def restate(name):
    """the restatement of a case from its arrays alone (colours computed here); computed once and shared: do not modify the result"""
    case = cases()[name]
    return restate_with(case, [(np_trace.prepare_set(a), M) for a, M in case["sets"]])
