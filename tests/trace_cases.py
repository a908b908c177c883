"""The scenes of the traced-pipeline tests (test_trace_cpu.py, test_gpu_trace.py), numpy only: every case is small enough for the
float64 brute-force restatement (np_trace.py) to take a few seconds at most.  A case = dict(sets=[(arrays, M)], V, P, eye, W, H,
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


def _big(n, seed, **kw):
    """a cloud in which every particle has a leaf: opacity clipped well above the cull threshold (logit(1/255) = -5.5)"""
    a = cloud(n, seed, **kw)
    a["opacity"] = np.maximum(a["opacity"], np.float32(-4.0))
    return a


def _dead_third(n, seed, **kw):
    a = _big(n, seed, **kw)
    a["opacity"][::3] = -9.0
    return a


def _planar():
    a = cloud(260, 51, log_scale=-2.6)
    a["positions"][:, 2] = 0.25
    return a


def _collinear():
    a = cloud(120, 52, log_scale=-2.5)
    a["positions"][:, 1], a["positions"][:, 2] = 0.125, -0.25     # an axis-parallel line: two axes without extent
    return a


def _coincident():
    a = cloud(64, 53, log_scale=-1.6)
    a["positions"][:] = (0.125, -0.0625, 0.25)
    a["scale"] = (a["scale"] + np.linspace(-1.2, 0.6, 64, dtype=np.float32)[:, None]).astype(np.float32)
    return a


def _ties():
    """340 particles: 300..339 are exact copies (centre, log-scale, quaternion) of 0..39, with other colours and opacities"""
    a = cloud(300, 54, log_scale=-2.3)
    a["scale"][:40] += np.float32(0.5)
    a["f_dc"][:40] = 2.5
    a["opacity"][:40] = 1.0
    b = {k: np.concatenate([v, v[:40]]) for k, v in a.items()}
    b["f_dc"][300:] = -2.5
    b["opacity"][300:] = 2.0
    return b


def _thin():
    """thin_particle_threshold 0.06: a third of the particles have one scale below it, a third two, the rest none; no scale within
    10 % of the threshold (nor of the iso method's 2 % of the largest scale)"""
    a = cloud(300, 55, log_scale=-2.0)
    rng = np.random.Generator(np.random.PCG64(56))
    s = rng.uniform(0.08, 0.2, (300, 3))
    small = rng.uniform(0.02, 0.05, (300, 3))
    s[0::3, 0] = small[0::3, 0]
    s[1::3, 1], s[1::3, 2] = small[1::3, 1], small[1::3, 2]
    a["scale"] = np.log(s).astype(np.float32)
    return a


RING = 8


def _ring():
    """particles 0..7: identity quaternion, one centre z, one log-scale z, on a ring around the z axis; on the ray (0, 0, -1) from
    (0, 0, 3) their t is bit-identical (np_trace: declared ties).  Listed in DESCENDING order of the (y, x) bit interleave that both
    Morton sorts (commit, hierarchy) roughly order them by, so the storage order of the group is close to the reverse of the caller's
    (the GPU test reads the storage order back and asserts that it would choose other hits).  Distinct
    colours and opacities; no two share an x or a y (rows and columns of the frame with a zero direction component).  The rest of the
    cloud stays clear of the axis."""
    a = cloud(120, 67, log_scale=-2.6)
    far = np.hypot(a["positions"][:, 0], a["positions"][:, 1]) > 0.55
    a = {k: v[far] for k, v in a.items()}
    ang = np.radians(10.0 + 45.0 * np.arange(RING))
    xy = np.stack([0.05 * np.cos(ang), 0.05 * np.sin(ang)], 1).astype(np.float32)
    q = np.floor((xy + 0.0625) / 0.125 * 1023.0).astype(np.int64)
    code = np.zeros(RING, np.int64)
    for b in range(10):
        code |= ((q[:, 0] >> b) & 1) << (2 * b) | ((q[:, 1] >> b) & 1) << (2 * b + 1)
    xy = xy[np.argsort(-code)]
    ring = dict(positions=np.concatenate([xy, np.full((RING, 1), 0.25, np.float32)], 1),
                f_dc=np.array([[2, -1, -1], [-1, 2, -1], [-1, -1, 2], [2, 2, -1], [-1, 2, 2], [2, -1, 2], [1.5, 0, -1.5], [-1.5, 1, 0]], np.float32),
                f_rest=np.zeros((RING, 45), np.float32),
                opacity=np.linspace(-1.2, 0.2, RING).astype(np.float32),
                scale=np.tile(np.log(np.array([0.08, 0.08, 0.07], np.float32)), (RING, 1)),
                rotation=np.tile(np.array([1, 0, 0, 0], np.float32), (RING, 1)))
    return {k: np.concatenate([ring[k], a[k]]) for k in a}


SHEAR = np.array([[1, 0.4, 0, 0.2], [0, 1, 0.25, -0.9], [0, 0, 1, 0.1], [0, 0, 0, 1]], np.float32)
MIRROR = np.array([[-1, 0, 0, 0.9], [0, 1, 0, 0.7], [0, 0, 1, -0.2], [0, 0, 0, 1]], np.float32)


def _five_instances():
    a = cloud(220, 57, half=0.6, sh_coeffs=15)
    b = cloud(200, 58, half=0.6, sh_coeffs=8)
    c = cloud(200, 59, half=0.6, sh_coeffs=0)
    d = cloud(150, 60, half=0.6, sh_coeffs=3)
    d["opacity"][:] = -9.0                                         # the whole instance below the cull threshold: no leaf
    return [(a, trs((1.0, 1.0, 1.0), (0, 1, 0), 25.0, (-0.9, 0.6, 0.0))), (b, MIRROR), (a, trs((0.7, 1.2, 0.9), (1, 0, 1), -40.0, (-0.8, -0.7, 0.3))),
            (d, I4), (c, SHEAR)]


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
    # K-buffer sizes: K = 1; K < KB inside the 18-slot buffer; the 32-slot buffer; rays that run out of candidates (few large, faint splats)
    for k in (1, 5, 17, 19, 32):
        c[f"n_spp_{k:02d}"] = _case([(cloud(220, 61, log_scale=-1.5, opacity_mean=-2.2), I4)], (0.3, 0.2, 3.0), W=32, H=24, trace=dict(samples_per_pass=k))
    c["n_spp_32_all_candidates"] = _case([(cloud(220, 61, log_scale=-1.5, opacity_mean=-2.2), I4)], (0.3, 0.2, 3.0), W=32, H=24,
                                         trace=dict(samples_per_pass=32, min_transmittance=0.0))
    # tree sizes: around one sort partition of 4096 keys, and six levels
    for n, ls, wh in ((4095, -3.6, (24, 16)), (4096, -3.6, (24, 16)), (4097, -3.6, (24, 16)), (32769, -5.4, (16, 12))):
        c[f"e_leaves_{n}"] = _case([(_big(n, 70 + n % 7, log_scale=ls), I4)], (0.2, 0.2, 2.6), W=wh[0], H=wh[1])
    c["o_dead_third"] = _case([(_dead_third(13500, 62, log_scale=-4.3), I4)], (0.2, 0.2, 2.6), W=24, H=16)
    # Morton frames without extent
    c["p_planar"] = _case([(_planar(), I4)], (0.3, 0.2, 3.0), W=32, H=24)
    c["p_collinear"] = _case([(_collinear(), I4)], (0.3, 0.2, 3.0), W=32, H=24)
    c["p_coincident"] = _case([(_coincident(), I4)], (0.3, 0.2, 3.0), W=32, H=24)
    # column 16 has d.x == 0, row 12 has d.y == 0; 33 x 25 leaves a partial 8-pixel tile on both axes
    c["q_axis_rays"] = _case([(cloud(500, 63), I4)], (0.0, 0.0, 3.0), W=33, H=25)
    # the same camera, K = 5 below the size of a group of eight DIFFERENT particles with bit-identical t on the central ray
    c["q_axis_ring_ties"] = dict(_case([(_ring(), I4)], (0.0, 0.0, 3.0), W=33, H=25, trace=dict(samples_per_pass=5)),
                                 exact_ties=((12, 16, 0, frozenset(range(RING))),))
    for deg in (1, 4, 5, 8):
        c[f"j_degree_{deg}"] = _case([(cloud(600, 19), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(kernel_degree=deg))
    c["j_degree_0_no_clamping"] = _case([(cloud(600, 19), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(kernel_degree=0),
                                        trace=dict(kernel_adaptive_clamping=0))
    c["r_five_instances"] = _case(_five_instances(), (0.2, 0.4, 3.8), W=32, H=24)
    for k in (32, 18, 4, 1):
        c[f"s_ties_{k:02d}"] = _case([(_ties(), I4)], (0.3, 0.2, 3.0), W=32, H=24, trace=dict(samples_per_pass=k))
    c["t_normal_iso"] = _case([(cloud(450, 64), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(normal_method=1))
    c["t_normal_thin"] = _case([(_thin(), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(thin_particle_threshold=0.06))
    c["t_normal_thin_iso"] = _case([(_thin(), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(thin_particle_threshold=0.06, normal_method=1))
    c["u_sh_only"] = _case([(cloud(450, 65), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(debug_flags=2))
    c["u_no_gaussian"] = _case([(cloud(450, 65), I4)], (0.3, 0.3, 3.0), W=32, H=24, frame=dict(debug_flags=4))
    c["v_iso_threshold_1"] = _case([(cloud(450, 66), I4)], (0.3, 0.3, 3.0), W=32, H=24, trace=dict(depth_iso_threshold=1.0))
    c["v_iso_threshold_0"] = _case([(cloud(450, 66), I4)], (0.3, 0.3, 3.0), W=32, H=24, trace=dict(depth_iso_threshold=0.0))
    return c


FRAME_DEFAULTS = dict(kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull_threshold=1.0 / 255.0, sh_degree=3,
                      camera_model=0, fov_rad=0.0, dof_mode=0, focus_dist=1.3, aperture=0.001, frame_sample_id=0, normal_method=0,
                      thin_particle_threshold=1e-6, debug_flags=0)
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
                          fov_rad=f["fov_rad"], dof=dof, rows=rows, thin=f["thin_particle_threshold"], normal_method=f["normal_method"],
                          sh_only=bool(f["debug_flags"] & 2), no_gauss=bool(f["debug_flags"] & 4),
                          **dict(dict(exact_ties=case.get("exact_ties", ())), **extra))


@functools.lru_cache(maxsize=None)
def restate(name):
    """the restatement of a case from its arrays alone (colours computed here); computed once and shared: do not modify the result"""
    case = cases()[name]
    return restate_with(case, [(np_trace.prepare_set(a), M) for a, M in case["sets"]])
