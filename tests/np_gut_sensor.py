"""The 3DGUT pipeline through a bound sensor model (mgs_frame_set_sensor) in float64: tests/np_gut.py with the point projection and
the pixel rays replaced, nothing else.  The forward maps are restated from the reference's formulas (projectPointPinhole,
projectPointFisheye, evalPolyHorner4, withinResolution, threedgut_camera_projections.h.slang:51-59,78-171; computeMaxAngle,
threedgut_camera_models.h.slang:87-119).  The reference has no inverse of these models: the ray of a pixel is DEFINED by the library
(include/mgs.h, "sensor models") as the direction whose projection is the pixel's centre, found by Newton; here it is iterated to
1e-12 in float64.

np_gut's fragile masks are kept; two conditions are added: a sigma point within the margin of the icD limits, of max_angle or of the
withinResolution border (the margins `sigma_hard` / `sigma_image` of np_gut.project, which now carry the sensor's thresholds), and a
pixel whose inverse is within the margin of having no ray (the `edge` of pixel_rays).

Every map here takes the arithmetic's dtype from its input, and _twin recompiles np_gut's own text over a float32 numpy, so that the
whole restatement also runs in float32: gut_sensor_cases.py measures that run against the float64 one for the bars of the GPU tests.

Test infrastructure only."""
import inspect

import numpy as np

import np_gut

PINHOLE, FISHEYE = 0, 1
NEWTON_ITERS = 8          # the library's fixed iteration count (device_types.h: kSensorNewtonIters)
TOL_PX = 1e-2             # ... and its convergence bound in pixels (kSensorTolPx)
FIELDS = ("model", "focal_length", "principal_point", "radial", "tangential", "thin_prism", "fisheye_radial", "max_angle")


def sensor(model, focal_length, principal_point, radial=(0,) * 6, tangential=(0, 0), thin_prism=(0,) * 4, fisheye_radial=(0,) * 4, max_angle=0.0, round32=True):
    s = dict(model=int(model), focal_length=np.asarray(focal_length, np.float64), principal_point=np.asarray(principal_point, np.float64),
             radial=np.asarray(radial, np.float64), tangential=np.asarray(tangential, np.float64), thin_prism=np.asarray(thin_prism, np.float64),
             fisheye_radial=np.asarray(fisheye_radial, np.float64), max_angle=float(max_angle))
    if not round32:
        return s
    # what the library receives is fp32: the restatement works on the same numbers
    return {k: (np.asarray(v, np.float32).astype(np.float64) if isinstance(v, np.ndarray) else (float(np.float32(v)) if k == "max_angle" else v)) for k, v in s.items()}


def compute_max_angle(W, H, pp, f):
    """computeMaxAngle (threedgut_camera_models.h.slang:87-119)"""
    mdx = pp[0] if pp[0] > 0.5 * W else W - pp[0]
    mdy = pp[1] if pp[1] > 0.5 * H else H - pp[1]
    r = np.hypot(mdx, mdy)
    return max(2.0 * r / f[0], 2.0 * r / f[1]) / 2.0


def from_frame(P, W, H, st):
    """mgs_sensor_model_from_frame: the perfect model of the frame"""
    st3 = dict(st)
    f = np_gut.focal(P, W, H, st3)
    pp = np.array([W, H], np.float64) / 2.0
    return sensor(FISHEYE if st["camera_model"] == 1 else PINHOLE, f, pp, max_angle=np_gut.max_angle(W, H, f), round32=False)


def max_angle_of(sn, W, H):
    return sn["max_angle"] if sn["max_angle"] > 0 else float(np.float32(compute_max_angle(W, H, sn["principal_point"], sn["focal_length"])))


def horner4(k, x):
    return ((k[3] * x + k[2]) * x + k[1]) * x + k[0]


def distort(sn, u, v):
    """computeDistortion (:96-116): (icD u + delta_x, icD v + delta_y, icD)"""
    t = u.dtype.type
    k, tg, tp = (sn[n].astype(u.dtype) for n in ("radial", "tangential", "thin_prism"))
    uu, vv = u * u, v * v
    r2 = uu + vv
    a1, a2, a3 = t(2) * u * v, r2 + t(2) * uu, r2 + t(2) * vv
    icd = (t(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) / (t(1) + r2 * (k[3] + r2 * (k[4] + r2 * k[5])))
    dx = tg[0] * a1 + tg[1] * a2 + r2 * (tp[0] + r2 * tp[1])
    dy = tg[0] * a3 + tg[1] * a1 + r2 * (tp[2] + r2 * tp[3])
    return icd * u + dx, icd * v + dy, icd


def project_points(sn, cam, W, H):
    """projectPoint of the camera-space points cam [n, 3] (right, up, front).  Returns (pixels [n, 2], ok (the model's own validity),
    inside (withinResolution), hard (relative distance from the model's thresholds), soft (... from the image margin), behind,
    fallback (the pinhole's clipped branch was taken))"""
    t = cam.dtype.type
    f, pp = sn["focal_length"].astype(cam.dtype), sn["principal_point"].astype(cam.dtype)
    n = cam.shape[0]
    size = np.linalg.norm(cam.astype(np.float64), axis=1)
    if sn["model"] == FISHEYE:
        amax = t(max_angle_of(sn, W, H))
        rho = np.maximum(np.hypot(cam[:, 0], cam[:, 1]), t(1e-7))
        full = np.arctan2(rho, cam[:, 2])
        th = np.minimum(full, amax)
        th2 = th * th
        delta = th * (horner4(sn["fisheye_radial"].astype(cam.dtype), th2) * th2 + t(1)) / rho
        px = f * cam[:, :2] * delta[:, None] + pp
        ok, hard = th < amax, np.abs(full.astype(np.float64) - float(amax)) / float(amax)
        behind, fallback = np.zeros(n, bool), np.zeros(n, bool)
    else:
        behind = cam[:, 2] <= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2]
            du, dv, icd = distort(sn, u, v)
            valid = (icd > t(0.8)) & (icd < t(1.2))
            clip = t(np.hypot(W, H)) / np.sqrt(u * u + v * v)
            px = np.where(valid[:, None], np.stack([du, dv], 1) * f + pp, np.stack([clip * u, clip * v], 1) + pp)
            px = np.where(behind[:, None], t(0), px)
            icd64 = np.nan_to_num(icd.astype(np.float64), nan=1.0)
        ok = ~behind & valid
        fallback = ~behind & ~valid
        hard = np.minimum(np.abs(cam[:, 2].astype(np.float64)) / size, np.minimum(np.abs(icd64 - 0.8) / 0.8, np.abs(icd64 - 1.2) / 1.2))
        hard = np.where(behind, np.abs(cam[:, 2].astype(np.float64)) / size, hard)
    m = np_gut.MARGIN
    p64 = px.astype(np.float64)
    inside = (px[:, 0] > t(-m * W)) & (px[:, 1] > t(-m * H)) & (px[:, 0] < t(W + m * W)) & (px[:, 1] < t(H + m * H))
    soft = np.minimum(np.minimum(np.abs(p64[:, 0] + m * W), np.abs(p64[:, 0] - W - m * W)) / W,
                      np.minimum(np.abs(p64[:, 1] + m * H), np.abs(p64[:, 1] - H - m * H)) / H)
    return px, ok, inside, hard, soft, behind, fallback


class _Float32Numpy:
    """numpy as the float32 run of the restatement sees it: float64 names float32, and what a constructor would make float64 by
    default (np.zeros(n), np.array([2.0, ...]), np.eye(4)) is float32.  Everything else is numpy itself, which keeps float32 through
    arithmetic with Python scalars."""
    _makers = ("array", "asarray", "zeros", "ones", "full", "eye")

    def __getattr__(self, name):
        if name == "float64":
            return np.float32
        f = getattr(np, name)
        if name not in self._makers:
            return f

        def make(*a, **kw):
            r = f(*a, **kw)
            return r.astype(np.float32) if r.dtype == np.float64 else r
        return make


def _cut(src, old, new, count=1):
    assert src.count(old) == count, (old, src.count(old))
    return src.replace(old, new)


def _twin(float32):
    """np_gut's project, GutFragments and fragments compiled again from their own text, with the point projection taken from a hook
    and the pixels' rays from this module.  float32: the same text over _Float32Numpy — the whole restatement in float32 arithmetic:
    the module's numpy constants become Python floats, and the pixel coordinates (integers, which numpy would promote to float64) are
    cast where they enter the arithmetic.  Every cut asserts that the text it replaces is there."""
    src = inspect.getsource(np_gut.project)
    a, b = src.index("    def cam_project(pts):"), src.index("    pts = [c] + [")
    assert 0 < a < b
    src = src[:a] + "    cam_project = _hook(st, MV, W, H)\n\n" + src[b:]
    ns = dict(vars(np_gut))
    ns["_hook"] = _cam_project_hook
    cls, frag = inspect.getsource(np_gut.GutFragments), inspect.getsource(np_gut.fragments)
    if float32:
        ns.update(np=_Float32Numpy(), _f32=np.float32, GUT_DELTA=float(np_gut.GUT_DELTA), **{k: float(getattr(np_gut, k)) for k in ("W_I", "W_0", "ULPS", "EDGE")})
        cls = _cut(cls, "dx, dy = xx + 0.5 - t[\"c\"][i, 0], yy + 0.5 - t[\"c\"][i, 1]",
                   "dx, dy = _f32(xx + 0.5) - t[\"c\"][i, 0], _f32(yy + 0.5) - t[\"c\"][i, 1]")
    for text in (src, cls, frag):
        exec(compile(text, np_gut.__file__ + " (recompiled by np_gut_sensor)", "exec"), ns)
    ns["pixel_rays"] = pixel_rays
    return ns


def _cam_project_hook(st, MV, W, H):
    sn, dtype, log = st["sensor"], _sensor_dtype(st), st.get("sensor_log")
    keep = np.float32 if st.get("pipeline_dtype") == np.float32 else np.float64

    def cam_project(pts):
        v = pts @ MV[:3, :3].T + MV[:3, 3]
        cam = (v * np.array([1.0, 1.0, -1.0], v.dtype)).astype(dtype)          # RUB -> RUF
        px, ok, inside, hard, soft, behind, fallback = project_points(sn, cam, W, H)
        if log is not None:
            log.append(dict(ok=ok, inside=inside, fallback=fallback, behind=behind))
        return px.astype(keep), ok & inside, behind, hard, np.where(ok, soft, np.inf)

    return cam_project


def _sensor_dtype(st):
    return np.float32 if st.get("pipeline_dtype") == np.float32 else st.get("sensor_dtype", np.float64)


_twins = {}


def _ns(st):
    f32 = st.get("pipeline_dtype") == np.float32
    if f32 not in _twins:
        _twins[f32] = _twin(f32)
    return _twins[f32]


def project(arrays, M, V, P, W, H, st, delta=1e-4):
    """np_gut.project with the sigma points through st["sensor"].  st["sensor_dtype"] (default float64): the arithmetic of the point
    projection alone; st["pipeline_dtype"] = np.float32: the whole restatement in float32 (_twin); st["sensor_log"]: a list that
    receives, per sigma-point slot, which branch every point took.  `dist` (the frustum cull) keeps using V / P and the frame's own
    camera model, as the library does."""
    return _ns(st)["project"](arrays, M, V, P, W, H, st, delta)


# ---- the inverse ----------------------------------------------------------------------------------------------------------------
def _pinhole_step(sn, u, v, qx, qy):
    """residual of the forward map at (u, v) and its 2x2 Jacobian"""
    t = u.dtype.type
    k, tg, tp = (sn[n].astype(u.dtype) for n in ("radial", "tangential", "thin_prism"))
    uu, vv, uv = u * u, v * v, u * v
    r2 = uu + vv
    num = t(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    den = t(1) + r2 * (k[3] + r2 * (k[4] + r2 * k[5]))
    icd = num / den
    fx = icd * u + (tg[0] * (t(2) * uv) + tg[1] * (r2 + t(2) * uu) + r2 * (tp[0] + r2 * tp[1])) - qx
    fy = icd * v + (tg[0] * (r2 + t(2) * vv) + tg[1] * (t(2) * uv) + r2 * (tp[2] + r2 * tp[3])) - qy
    dnum = k[0] + r2 * (t(2) * k[1] + r2 * (t(3) * k[2]))
    dden = k[3] + r2 * (t(2) * k[4] + r2 * (t(3) * k[5]))
    dic = (dnum - icd * dden) / den
    tp0, tp1 = tp[0] + t(2) * r2 * tp[1], tp[2] + t(2) * r2 * tp[3]
    j00 = icd + t(2) * (uu * dic + tg[0] * v + t(3) * tg[1] * u + u * tp0)
    j01 = t(2) * (uv * dic + tg[0] * u + tg[1] * v + v * tp0)
    j10 = t(2) * (uv * dic + tg[0] * u + tg[1] * v + u * tp1)
    j11 = icd + t(2) * (vv * dic + t(3) * tg[0] * v + tg[1] * u + v * tp1)
    return fx, fy, j00, j01, j10, j11, icd


def unproject(sn, px, py, W, H, iters=None, dtype=np.float64):
    """camera-space direction (right, up, BACK: view space) of the image points (px, py), has_ray, edge (relative distance from having no
    ray), residual in pixels.  iters None: iterated until the step is below 1e-12 (at most 100 steps); an integer: the library's
    fixed count."""
    px, py = np.asarray(px, dtype), np.asarray(py, dtype)
    t = px.dtype.type
    f, pp = sn["focal_length"].astype(dtype), sn["principal_point"].astype(dtype)
    qx, qy = (px - pp[0]) * (t(1) / f[0]), (py - pp[1]) * (t(1) / f[1])
    tol = t(TOL_PX / np.abs(sn["focal_length"]).max())
    steps = 100 if iters is None else iters
    with np.errstate(all="ignore"):
        if sn["model"] == FISHEYE:
            k = sn["fisheye_radial"].astype(dtype)
            amax = t(max_angle_of(sn, W, H))
            rq = np.sqrt(qx * qx + qy * qy)
            th = rq.copy()
            slow = np.zeros(th.shape, bool)
            for it in range(steps + 1):
                t2 = th * th
                res = th * (horner4(k, t2) * t2 + t(1)) - rq
                dg = t(1) + t2 * (t(3) * k[0] + t2 * (t(5) * k[1] + t2 * (t(7) * k[2] + t2 * (t(9) * k[3]))))
                if it == NEWTON_ITERS:
                    slow = ~(np.abs(res) <= tol * t(1e-3))
                if it == steps or (iters is None and it >= NEWTON_ITERS and np.nanmax(np.abs(res / dg)) < 1e-12):
                    break
                th = th - res / dg
            ok = (th >= 0) & (th < amax) & (np.abs(res) <= tol) & (dg > 0)
            rr = np.where(rq > 0, t(1) / np.where(rq > 0, rq, t(1)), t(0))
            d = np.stack([np.sin(th) * qx * rr, np.sin(th) * qy * rr, -np.cos(th)], -1)
            edge = np.minimum(np.abs(th.astype(np.float64) - float(amax)) / float(amax), np.abs(dg.astype(np.float64)))
            resid = np.abs(res.astype(np.float64)) * np.abs(sn["focal_length"]).max()
        else:
            u, v = qx.copy(), qy.copy()
            slow = np.zeros(u.shape, bool)
            for it in range(steps + 1):
                fx, fy, j00, j01, j10, j11, icd = _pinhole_step(sn, u, v, qx, qy)
                det = j00 * j11 - j01 * j10
                if it == NEWTON_ITERS:
                    slow = ~((np.abs(fx) <= tol * t(1e-3)) & (np.abs(fy) <= tol * t(1e-3)))
                su, sv = (j11 * fx - j01 * fy) / det, (j00 * fy - j10 * fx) / det
                if it == steps or (iters is None and it >= NEWTON_ITERS and np.nanmax(np.maximum(np.abs(su), np.abs(sv))) < 1e-12):
                    break
                u, v = u - su, v - sv
            ok = (icd > t(0.8)) & (icd < t(1.2)) & (np.abs(fx) <= tol) & (np.abs(fy) <= tol) & (det > 0)
            d = np.stack([u, v, -np.ones_like(u)], -1)
            i64 = np.nan_to_num(icd.astype(np.float64), nan=1.0)
            edge = np.minimum(np.minimum(np.abs(i64 - 0.8) / 0.8, np.abs(i64 - 1.2) / 1.2), np.abs(np.nan_to_num(det.astype(np.float64))))
            resid = np.maximum(np.abs(fx.astype(np.float64) * sn["focal_length"][0]), np.abs(fy.astype(np.float64) * sn["focal_length"][1]))
    d = np.where(ok[..., None], d, np.array([0, 0, -1], dtype))
    # a pixel the long iteration settles while the fixed count has not is within the margin as well
    edge = np.where(slow & ok & (iters is None), 0.0, np.nan_to_num(edge, nan=0.0))   # (the long iteration's own margin: float64 only)
    return d, ok, edge, np.where(ok, np.nan_to_num(resid, nan=np.inf), 0.0)


def forward_pixels(sn, d_cam, W, H):
    """float64 projection of view-space directions [..., 3] (right, up, back): pixels [..., 2] and the model's validity"""
    cam = (np.asarray(d_cam, np.float64) * np.array([1.0, 1.0, -1.0])).reshape(-1, 3)
    px, ok, _, _, _, _, _ = project_points(sn, cam, W, H)
    return px.reshape(d_cam.shape[:-1] + (2,)), ok.reshape(d_cam.shape[:-1])


def pixel_rays(V, P, W, H, st):
    """np_gut.pixel_rays for st["sensor"]: (world direction [H, W, 3], has_ray [H, W], edge [H, W]); rotated and normalised in the
    pipeline's arithmetic"""
    dtype = _sensor_dtype(st)
    out = np.float32 if st.get("pipeline_dtype") == np.float32 else np.float64
    Vi = np.linalg.inv(np.asarray(V, np.float64)).astype(out)
    yy, xx = np.mgrid[0:H, 0:W]
    d, ok, edge, _ = unproject(st["sensor"], xx + 0.5, yy + 0.5, W, H, None if dtype == np.float64 else NEWTON_ITERS, dtype)
    d = d.astype(out) @ Vi[:3, :3].T
    return d / np.sqrt((d * d).sum(-1, keepdims=True)), ok, edge


def fragments(projected, V, P, W, H, st, gaussian=False, delta=1e-4, depth=None):
    """np_gut.fragments with the pixels' rays from the sensor (in the arithmetic of st["pipeline_dtype"])"""
    return _ns(st)["fragments"](projected, V, P, W, H, st, gaussian, delta, depth)
