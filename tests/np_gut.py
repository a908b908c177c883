"""The 3DGUT raster pipeline in float64: what one particle's front end decides and emits, and which particles leave a fragment at
which pixel.  Written from the reference's shaders (threedgut_raster.mesh.slang:111-254, threedgut.h.slang:26-163,
threedgut_camera_projections.h.slang:78-171, threedgut_camera_models.h.slang:87-136, threedgs.h.slang:60-121,
threedgut_raster.frag.slang:87-138, cameras.h.slang:27-82, threedgrt.h.slang:57-127,238-278), column vectors, math-convention
matrices — not from the kernels and not from oracle/mgs_oracle.cpp.

Besides the values, project() names the decision of every particle and the distance of that decision (and of the record's
continuity) from each of its thresholds, so that a comparison with an fp32 implementation can set the particles aside whose
outcome fp32 may legitimately turn: `fragile`.  fragments() does the same per pixel: `borderline_count`.

What the build adds to the shaders and this file restates as well: a quad whose bounding box holds no pixel centre of the frame
(of the strip) is dropped before the sort, and the bin rectangle of the box's pixel window is recorded.

Test infrastructure only."""
import numpy as np

import np_fragments
import np_reference as ref

GUT_DELTA = np.sqrt(3.0)     # sqrt(D + lambda), D 3, alpha 1, beta 2, kappa 0 (threedgut_definitions.h.slang)
W_I, W_0 = 1.0 / 6.0, 2.0    # 1 / (2 (D + lambda));  lambda / (D + lambda) + (1 - alpha^2 + beta); the mean's own weight is 0
DILATION, ALPHA_THRESHOLD, MARGIN = 0.3, 0.01, 0.1
EDGE = 0.02                  # a pixel-edge or cancellation margin is taken relative to EDGE * its scale: with delta = 1e-4 that is
                             # 2e-6 of the scale, some 16 fp32 steps
ULPS = 16 * 2.0 ** -23
REJECTIONS = ("dist", "alpha_cull", "no_valid_point", "det_zero", "wop", "radius", "ev2", "ndc_z", "degenerate",
              "no_pixel_centre", "off_screen", "off_strip")
FIELDS = ("centre", "q", "box", "B", "ro", "opacity")   # the record's fields as the tests compare them


def settings(**kw):
    s = dict(camera_model=0, extent_method=1, ms_antialiasing=0, splat_scale=1.0, alpha_cull=1.0 / 255.0, fov_rad=None,
             strip=None, bin_px=(16, 16), kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, point_cloud=False)
    assert set(kw) <= set(s), set(kw) - set(s)
    s.update(kw)
    return s


def fov_rad(P, st):
    return float(st["fov_rad"]) if st["fov_rad"] is not None else float(2.0 * np.arctan(1.0 / abs(float(np.asarray(P)[1][1]))))


def focal(P, W, H, st):
    """frameInfo.focal (gaussian_splatting.cpp:1239-1251)"""
    if st["camera_model"] == 1:
        return np.array([W, -H], np.float64) / fov_rad(P, st)
    P = np.asarray(P, np.float64)
    return np.array([P[0][0] * 0.5 * W, P[1][1] * 0.5 * H])


def max_angle(W, H, f):
    r = np.hypot(W - 0.5 * W, H - 0.5 * H)   # computeMaxRadius with the principal point at the centre
    return max(2.0 * r / f[0], 2.0 * r / f[1]) / 2.0


def _quat_rows(q):
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], 1),
                     np.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], 1),
                     np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], 1)], 1)  # [n, axis, xyz]


def _edge(v, scale):
    """margin of a value against the nearest integer (a pixel edge of floor / ceil)"""
    return np.abs(v - np.round(v)) / (EDGE * scale)


def project(arrays, M, V, P, W, H, st, delta=1e-4):
    """arrays: positions, scale (log), rotation (w, x, y, z), opacity (logit) of one set; M: the instance's matrix (None: identity).
    Returns a dict of per-particle arrays: emits, reason (index into REJECTIONS, -1 where it emits), fragile, rect_fragile, margins
    (name -> array), n_valid, behind (sigma points with the (0, 0) output), the record (cx, cy, q1, q2, box, B, ro, opacity), half1 / half2,
    window (x0, y0, x1, y1 in pixels), rect (x0, y0, x1, y1 in bins), ndc_z, cerr (what fp32 leaves open of the centre, in pixels)."""
    c = np.asarray(arrays["positions"], np.float64).reshape(-1, 3)
    n = c.shape[0]
    s = np.exp(np.asarray(arrays["scale"], np.float64).reshape(-1, 3))
    R = _quat_rows(np.asarray(arrays["rotation"], np.float64).reshape(-1, 4))
    alpha0 = np.clip(1.0 / (1.0 + np.exp(-np.asarray(arrays["opacity"], np.float64).reshape(-1))), 0.0, 1.0)
    M = np.eye(4) if M is None else np.asarray(M, np.float64)
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    MV = V @ M
    f = focal(P, W, H, st)
    fish = st["camera_model"] == 1
    amax = max_angle(W, H, f)
    mg = {}

    def cam_project(pts):
        v = pts @ MV[:3, :3].T + MV[:3, 3]
        cam = v * np.array([1.0, 1.0, -1.0])          # RUB -> RUF
        size = np.linalg.norm(cam, axis=1)
        if fish:
            rho = np.maximum(np.hypot(cam[:, 0], cam[:, 1]), 1e-7)
            full = np.arctan2(rho, cam[:, 2])
            th = np.minimum(full, amax)
            px = f * cam[:, :2] * (th / rho)[:, None] + np.array([W, H]) / 2.0
            ok, hard = th < amax, np.abs(full - amax) / amax      # the clamp changes the projected point: continuity
            behind = np.zeros(pts.shape[0], bool)
        else:
            behind = cam[:, 2] <= 0
            with np.errstate(divide="ignore", invalid="ignore"):
                px = np.where(behind[:, None], 0.0, cam[:, :2] / cam[:, 2:3] * f + np.array([W, H]) / 2.0)
            ok, hard = ~behind, np.abs(cam[:, 2]) / size           # behind the camera the output is (0, 0): continuity
        inside = (px[:, 0] > -MARGIN * W) & (px[:, 1] > -MARGIN * H) & (px[:, 0] < W + MARGIN * W) & (px[:, 1] < H + MARGIN * H)
        soft = np.minimum(np.minimum(np.abs(px[:, 0] + MARGIN * W), np.abs(px[:, 0] - W - MARGIN * W)) / W,
                          np.minimum(np.abs(px[:, 1] + MARGIN * H), np.abs(px[:, 1] - H - MARGIN * H)) / H)
        return px, ok & inside, behind, hard, np.where(ok, soft, np.inf)

    pts = [c] + [c + sg * GUT_DELTA * s[:, a:a + 1] * R[:, a, :] for a in range(3) for sg in (1.0, -1.0)]
    pts = [pts[0], pts[1], pts[3], pts[5], pts[2], pts[4], pts[6]]   # mean, +delta_a (1..3), -delta_a (4..6): the shader's slots
    pr = [cam_project(p) for p in pts]
    sp = np.stack([p[0] for p in pr], 1)                              # [n, 7, 2]
    valid = np.stack([p[1] for p in pr], 1)
    n_valid = valid.sum(1)
    behind = np.stack([p[2] for p in pr], 1).sum(1)
    mg["sigma_hard"] = np.stack([p[3] for p in pr], 1).min(1)        # cz = 0 (pinhole) / the max angle (fisheye), any point
    soft = np.stack([p[4] for p in pr], 1)
    # the image margin (and with it n_valid) decides only between "some valid point" and none
    mg["sigma_image"] = np.where(n_valid <= 1, np.where(n_valid == 1, np.where(valid, soft, np.inf).min(1), soft.min(1)), np.inf)
    centre = W_I * sp[:, 1:].sum(1)
    d = sp - centre[:, None, :]
    wgt = np.array([W_0] + [W_I] * 6)[None, :]
    cov = np.stack([(wgt * d[..., 0] ** 2).sum(1), (wgt * d[..., 0] * d[..., 1]).sum(1), (wgt * d[..., 1] ** 2).sum(1)], 1)
    cerr = ULPS * np.maximum(np.abs(sp).max((1, 2)), 1.0)

    reason = np.full(n, -1, np.int64)

    def reject(mask, name):
        reason[(reason < 0) & mask] = REJECTIONS.index(name)

    survives, dist_margin = ref.dist_cull(c, M, V, P, W, H, fisheye=fish, focal=f)
    reject(~survives, "dist")
    mg["dist"] = dist_margin
    reject(alpha0 < st["alpha_cull"], "alpha_cull")
    mg["alpha_cull"] = np.abs(alpha0 - st["alpha_cull"]) / st["alpha_cull"]
    reject(n_valid == 0, "no_valid_point")
    alpha = alpha0.copy()
    a, b, dd = cov[:, 0] + DILATION, cov[:, 1], cov[:, 2] + DILATION
    det = a * dd - b * b
    with np.errstate(invalid="ignore", divide="ignore"):
        if st["extent_method"] == 1:
            reject(det == 0.0, "det_zero")
            wop = alpha0 * np.sqrt(np.maximum(0.000025, (cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2) / det)) if st["ms_antialiasing"] else alpha0
            reject(wop < ALPHA_THRESHOLD, "wop")
            mg["wop"] = np.abs(wop - ALPHA_THRESHOLD) / ALPHA_THRESHOLD
            factor = np.minimum(3.33, np.sqrt(2.0 * np.log(np.maximum(wop, 1e-300) / ALPHA_THRESHOLD)))
            mid = 0.5 * (a + dd)
            mg["floor_0.01"] = np.abs(mid * mid - det - 0.01) / np.maximum(0.01, EDGE * mid * mid)
            radius = factor * np.sqrt(mid + np.sqrt(np.maximum(0.01, mid * mid - det)))
            reject(~(radius > 0.0), "radius")
            if st["ms_antialiasing"]:
                alpha = wop
            zero = np.zeros(n)
            h1 = np.stack([np.minimum(factor * np.sqrt(a), radius), zero], 1)
            h2 = np.stack([zero, np.minimum(factor * np.sqrt(dd), radius)], 1)
        else:
            if st["ms_antialiasing"]:
                alpha = alpha0 * np.sqrt(np.maximum((cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2) / det, 0.0))
            half = 0.5 * (a + dd)
            disc = half * half - det
            mg["floor_0.1"] = np.abs(disc - 0.1) / np.maximum(0.1, EDGE * half * half)
            term2 = np.sqrt(np.maximum(0.1, disc))
            ev1, ev2 = half + term2, half - term2
            reject(ev2 <= 0.0, "ev2")
            mg["ev2"] = np.abs(ev2) / half
            if st["point_cloud"]:
                ev1 = ev2 = np.full(n, 0.2)
            mg["b"] = np.abs(np.abs(b) - 0.001) / np.maximum(0.001, EDGE * np.maximum(a, dd))
            e1 = np.stack([np.where(np.abs(b) < 0.001, 1.0, b), ev1 - a], 1)
            # ev1 - a is a difference of nearly equal numbers for a nearly axis-aligned ellipse: fp32 leaves its direction open by
            # this angle (np_fragments.basis_turn has the argument).  A turn by theta moves the quad's axes and box by theta of their
            # size: a particle whose basis may turn by more than delta radians is fragile, like any other relative margin
            turn = ULPS * np.maximum(ev1, a) / np.linalg.norm(e1, axis=1)
            mg["basis_turn"] = delta / np.maximum(turn, 1e-300) * delta
            e1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
            l1 = st["splat_scale"] * np.minimum(3.33 * np.sqrt(ev1), 2048.0)
            l2 = st["splat_scale"] * np.minimum(3.33 * np.sqrt(np.maximum(ev2, 0.0)), 2048.0)
            h1 = e1 * l1[:, None]
            h2 = np.stack([e1[:, 1], -e1[:, 0]], 1) * l2[:, None]
        # depth of the quad: the pinhole projection matrix of the centre; the fixed-function clip of a quad at z = ndc.z, w = 1
        vc = np.concatenate([c, np.ones((n, 1))], 1) @ MV.T
        clip = vc @ P.T
        ndc_z = clip[:, 2] / clip[:, 3]
        reject(~((ndc_z >= 0.0) & (ndc_z <= 1.0)), "ndc_z")
        mg["ndc_z"] = np.minimum(np.abs(ndc_z), np.abs(ndc_z - 1.0))
        n1, n2 = (h1 * h1).sum(1), (h2 * h2).sum(1)
        reject(~((n1 > 0.0) & (n2 > 0.0)), "degenerate")
        # the quad's box, the pixel centres inside it, the bin rectangle
        bex, bey = np.abs(h1[:, 0]) + np.abs(h2[:, 0]), np.abs(h1[:, 1]) + np.abs(h2[:, 1])
        lo = np.stack([centre[:, 0] - bex - 0.5, centre[:, 1] - bey - 0.5], 1)
        hi = np.stack([centre[:, 0] + bex - 0.5, centre[:, 1] + bey - 0.5], 1)
        f0, f1 = np.ceil(lo), np.floor(hi)
        r0, r1 = st["strip"] if st["strip"] is not None else (0, (H + 15) // 16)
        ymin, ymax = float(r0 * 16), float(min(r1 * 16, H) - 1)
        reject(~((f1[:, 0] >= f0[:, 0]) & (f1[:, 1] >= f0[:, 1])), "no_pixel_centre")
        reject(~((f1[:, 0] >= 0) & (f0[:, 0] <= W - 1) & (f1[:, 1] >= 0) & (f0[:, 1] <= H - 1)), "off_screen")
        reject(~((f1[:, 1] >= ymin) & (f0[:, 1] <= ymax)), "off_strip")
        scale = np.maximum(1.0, np.maximum(np.abs(sp).max((1, 2)), np.maximum(bex, bey)))
        edges = np.minimum(np.minimum(_edge(lo[:, 0], scale), _edge(hi[:, 0], scale)), np.minimum(_edge(lo[:, 1], scale), _edge(hi[:, 1], scale)))
        x0, x1 = np.maximum(f0[:, 0], 0.0), np.minimum(f1[:, 0], W - 1.0)
        y0, y1 = np.maximum(f0[:, 1], ymin), np.minimum(f1[:, 1], ymax)
        # an edge matters to the decision where moving it by one pixel turns one of the tests above
        tight = (f1[:, 0] - f0[:, 0] < 1) | (f1[:, 1] - f0[:, 1] < 1) | (f1[:, 0] < 1) | (f0[:, 0] > W - 2) | (f1[:, 1] < ymin + 1) | (f0[:, 1] > ymax - 1)
        mg["pixel_window"] = np.where(tight, edges, np.inf)
        q1, q2 = h1 / n1[:, None], h2 / n2[:, None]
    emits = reason < 0
    window = np.stack([x0, y0, x1, y1], 1)
    window = np.where(emits[:, None], np.nan_to_num(window, nan=0.0, posinf=0.0, neginf=0.0), 0.0).astype(np.int64)
    bx, by = st["bin_px"]
    rect = np.stack([window[:, 0] // bx, window[:, 1] // by, window[:, 2] // bx, window[:, 3] // by], 1)
    # B = S^-1 R N, ro = S^-1 R (M^-1 o - p): the canonical ray of threedgrt.h.slang:57-75 for the model-space ray of frag.slang:117-120
    Mi = np.linalg.inv(M)
    o = np.linalg.inv(V)[:3, 3]
    A = R / s[:, :, None]
    B = A @ Mi[:3, :3]
    ro = np.einsum("nkr,nr->nk", A, (Mi[:3, :3] @ o + Mi[:3, 3])[None, :] - c)
    # the thresholds a rejected particle never reached say nothing about it: a margin counts up to the rejection (dist first)
    order = ["dist", "alpha_cull", "sigma_hard", "sigma_image", "wop", "floor_0.01", "floor_0.1", "ev2", "b", "basis_turn", "ndc_z", "pixel_window"]
    stage = {"dist": 0, "alpha_cull": 1, "sigma_hard": 2, "sigma_image": 2, "wop": 4, "floor_0.01": 5, "floor_0.1": 5, "ev2": 6, "b": 6,
             "basis_turn": 6, "ndc_z": 7, "pixel_window": 9}
    reached = np.where(emits, 99, reason)
    fragile = np.zeros(n, bool)
    for k in order:
        if k in mg:
            mg[k] = np.nan_to_num(np.asarray(mg[k], np.float64), nan=0.0, posinf=np.inf)
            fragile |= (mg[k] < delta) & (reached >= stage[k])
    rect_fragile = fragile | (emits & (edges < delta))
    return dict(emits=emits, reason=reason, fragile=fragile, rect_fragile=rect_fragile, margins=mg, n_valid=n_valid, behind=behind,
                cx=centre[:, 0], cy=centre[:, 1], q1=q1, q2=q2, box=np.stack([bex, bey], 1), B=B.reshape(n, 9), ro=ro, opacity=alpha,
                half1=h1, half2=h2, window=window, rect=rect, ndc_z=ndc_z, cerr=cerr, cov=cov, sigma=sp, opacity_in=alpha0)


def record_deviation(pr, idx, rec):
    """per field of FIELDS, the largest deviation of the records rec[len(idx), 24] (mgs_frame_download_projected_gut's layout) from the
    restatement's particles idx, each on its natural scale: centre, 1/q and box in pixels relative to max(1, quad size); a row of B
    relative to the row's norm; ro relative to |ro|; the opacity relative.  Returns (dict field -> float, dict field -> worst index)."""
    rec = np.asarray(rec, np.float64)
    size = np.maximum(1.0, np.maximum(np.linalg.norm(pr["half1"][idx], axis=1), np.linalg.norm(pr["half2"][idx], axis=1)))
    dev = {}
    dev["centre"] = np.maximum(np.abs(rec[:, 0] - pr["cx"][idx]), np.abs(rec[:, 1] - pr["cy"][idx])) / size
    h = lambda q: q / (q * q).sum(1, keepdims=True)   # noqa: E731  (q = h / |h|^2  <=>  h = q / |q|^2)
    dev["q"] = np.maximum(np.abs(h(rec[:, 2:4]) - pr["half1"][idx]).max(1), np.abs(h(rec[:, 4:6]) - pr["half2"][idx]).max(1)) / size
    dev["box"] = np.abs(rec[:, 6:8] - 0.01 - pr["box"][idx]).max(1) / size   # the record's box is 0.01 px wider (culling only)
    Br, Bw = rec[:, 8:17].reshape(-1, 3, 3), pr["B"][idx].reshape(-1, 3, 3)
    dev["B"] = (np.linalg.norm(Br - Bw, axis=2) / np.linalg.norm(Bw, axis=2)).max(1)
    dev["ro"] = np.linalg.norm(rec[:, 17:20] - pr["ro"][idx], axis=1) / np.linalg.norm(pr["ro"][idx], axis=1)
    dev["opacity"] = np.abs(rec[:, 23] - pr["opacity"][idx]) / pr["opacity"][idx]
    worst = {k: (int(idx[int(np.argmax(v))]) if len(idx) else -1) for k, v in dev.items()}
    return {k: (float(v.max()) if len(idx) else 0.0) for k, v in dev.items()}, worst


# ---- per pixel ------------------------------------------------------------------------------------------------------------------
def pixel_rays(V, P, W, H, st):
    """(world direction [H, W, 3] of every pixel's ray as the reference writes it, has_ray [H, W])"""
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    Vi = np.linalg.inv(V)
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx + 0.5, yy + 0.5                                      # SV_Position
    if st["camera_model"] == 1:                                      # generateFisheyeRay: resolution - 1, no sub-pixel offset
        u, v = px / (W - 1.0) * 2.0 - 1.0, py / (H - 1.0) * 2.0 - 1.0
        r = np.sqrt(u * u + v * v)
        ok = ~(r > 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            phi = np.arccos(np.clip(np.where(np.abs(r) > 1e-9, u / r, 0.0), -1.0, 1.0))
        phi = np.where(v < 0.0, -phi, phi)
        th = r * fov_rad(P, st) * 0.5
        d = np.stack([np.cos(phi) * np.sin(th), -np.sin(phi) * np.sin(th), -np.cos(th)], -1)
        edge = np.abs(r - 1.0)
    else:                                                            # generatePinholeRay(position.xy, float2(0.5)): the double 0.5
        u, v = (px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0
        t = np.stack([u, v, np.ones_like(u), np.ones_like(u)], -1) @ np.linalg.inv(P).T
        d = t[..., :3]
        ok, edge = np.ones((H, W), bool), np.full((H, W), np.inf)
    d = d @ Vi[:3, :3].T
    return d / np.linalg.norm(d, axis=-1, keepdims=True), ok, edge


def response(degree, d2):
    """particleRayMaxKernelResponse<degree> of the SQUARED canonical distance (threedgrt.h.slang:83-127)"""
    d2 = np.maximum(d2, 0.0)
    if degree == 8:
        return np.exp(-0.000685871056241 * d2 ** 4)
    if degree == 5:
        return np.exp(-0.0185185185185 * d2 * d2 * np.sqrt(d2))
    if degree == 4:
        return np.exp(-0.0555555555556 * d2 * d2)
    if degree == 3:
        return np.exp(-0.166666666667 * d2 * np.sqrt(d2))
    if degree == 1:
        return np.exp(-1.5 * np.sqrt(d2))
    if degree == 0:
        return np.maximum(1.0 - 0.329630334487 * np.sqrt(d2), 0.0)
    return np.exp(-0.5 * d2)


def table(projected, delta=1e-4):
    """the emitted particles of all instances (projected = [project(...)] in creation order), ids global"""
    rows, off = [], 0
    for pr in projected:
        i = np.flatnonzero(pr["emits"])
        rows.append(dict(id=i + off, c=np.stack([pr["cx"][i], pr["cy"][i]], 1), q1=pr["q1"][i], q2=pr["q2"][i], box=pr["box"][i],
                         B=pr["B"][i], ro=pr["ro"][i], opacity=pr["opacity"][i], z=pr["ndc_z"][i], cerr=pr["cerr"][i]))
        off += pr["emits"].shape[0]
    return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}


class GutFragments:
    """count, nearest_id (-1: none), borderline_count, nearest_open (the nearest fragment's identity is not settled: it, or one in
    front of it, is borderline, or two candidates' depths tie) — all [H, W]; covering(x, y) for the failure messages"""

    def __init__(self, W, H, t, rays, st, gaussian, delta, depth):
        self.W, self.H, self.table, self.rays, self.st, self.gaussian, self.delta, self.depth = W, H, t, rays, st, gaussian, delta, depth
        self.count = np.zeros((H, W), np.int32)
        self.borderline_count = np.zeros((H, W), np.int32)
        self.nearest_id = np.full((H, W), -1, np.int64)
        self.nearest_open = np.zeros((H, W), bool)
        self._z = np.full((H, W), np.inf)
        self._zopen = np.full((H, W), np.inf)   # nearest borderline fragment that is not counted
        self._frag = []                          # gaussian: (pixel, depth, id, alpha, settled) of every fragment and near miss

    @property
    def borderline(self):
        return self.borderline_count > 0

    def _one(self, i, xx, yy):
        t, st = self.table, self.st
        dirs, ok, redge = self.rays
        dx, dy = xx + 0.5 - t["c"][i, 0], yy + 0.5 - t["c"][i, 1]
        u, v = dx * t["q1"][i, 0] + dy * t["q1"][i, 1], dx * t["q2"][i, 0] + dy * t["q2"][i, 1]
        bu = self.delta + t["cerr"][i] * np.linalg.norm(t["q1"][i])
        bv = self.delta + t["cerr"][i] * np.linalg.norm(t["q2"][i])
        g = dirs[yy, xx] @ t["B"][i].reshape(3, 3).T
        ro = t["ro"][i]
        k = np.cross(g, ro)
        d2 = (k * k).sum(-1) / (g * g).sum(-1)
        # what fp32 leaves open of d2: the cross product of the canonical direction with an origin |ro| radii away
        err = 2.0 * np.sqrt(d2) * ULPS * np.linalg.norm(ro) + self.delta * d2
        dens = t["opacity"][i]
        rcut = max(st["kernel_min_response"], 1.0 / (255.0 * max(dens, 1e-300)))
        live = dens > st["alpha_cull"]
        lo = response(st["kernel_degree"], d2 + err) > rcut * (1.0 + self.delta)
        hi = response(st["kernel_degree"], np.maximum(d2 - err, 0.0)) > rcut * (1.0 - self.delta)
        inq = (np.abs(u) <= 1.0) & (np.abs(v) <= 1.0)
        inq_hi = (np.abs(u) <= 1.0 + bu) & (np.abs(v) <= 1.0 + bv)
        inq_lo = (np.abs(u) <= 1.0 - bu) & (np.abs(v) <= 1.0 - bv)
        keep = inq & (response(st["kernel_degree"], d2) > rcut) & live & ok[yy, xx]
        sure = inq_lo & lo & live & ok[yy, xx] & (redge[yy, xx] > self.delta)
        maybe = inq_hi & hi & live & (ok[yy, xx] | (redge[yy, xx] <= self.delta))
        live_edge = abs(dens - st["alpha_cull"]) <= self.delta * st["alpha_cull"]
        if live_edge:
            sure[:] = False
            maybe = inq_hi & hi
        if self.depth is not None:
            D = self.depth[yy, xx]
            near = np.abs(t["z"][i] - D) <= ULPS   # both are fp32 numbers in [0, 1]: the key depth is good to a few steps of 1
            keep &= t["z"][i] <= D
            sure &= (t["z"][i] <= D) & ~near
            maybe &= (t["z"][i] <= D) | near
        resp = response(st["kernel_degree"], d2)
        return keep, maybe & ~sure, d2, np.minimum(st["alpha_clamp"], resp * dens)

    def blend(self, colours, delta_t=None):
        """the frame with the opacity gaussian on, front to back with the saturation test T >= 1e-4 (threedgut_raster.frag.slang:176-183
        under the FRONT_TO_BACK blend; the build's per-fragment predicate), evaluated twice in float64: with every borderline fragment in
        and with every one out — a fragment whose T lies within delta of 1e-4 counts as borderline for that test too.  colours: [n, 3]
        by global id.  Returns (lo, hi) [H, W, 4]: per channel the smaller and the larger of the two (alpha = 1 - T); self.order_open [H, W] marks the
        pixels where two fragments' depths tie in fp32, whose order is open."""
        assert self.gaussian
        d = self.delta if delta_t is None else delta_t
        pix, z, gid, al, sure = (np.concatenate([f[k] for f in self._frag]) for k in range(5))
        o = np.lexsort((gid, z, pix))
        pix, z, gid, al, sure = pix[o], z[o], gid[o], al[o], sure[o]
        first = np.r_[True, pix[1:] != pix[:-1]]
        # two fragments of a pixel whose depths are within four fp32 steps may be drawn in either order (the sort key is an fp32 depth)
        swap = ~first & (np.abs(z - np.r_[0.0, z[:-1]]) <= 4 * 2.0 ** -23 * np.maximum(np.abs(z), 1e-3))
        self.order_open = np.zeros(self.W * self.H, bool)
        self.order_open[pix[swap]] = True
        self.order_open = self.order_open.reshape(self.H, self.W)
        start = np.maximum.accumulate(np.where(first, np.arange(pix.size), 0))
        rank = np.arange(pix.size) - start
        res = []
        for include, thr in ((True, 1e-4 * (1.0 - d)), (False, 1e-4 * (1.0 + d))):
            T, C = np.ones(self.W * self.H), np.zeros((self.W * self.H, 3))
            for r in range(int(rank.max()) + 1 if pix.size else 0):
                s = np.flatnonzero(rank == r)
                p = pix[s]
                w = np.where((sure[s] | include) & (T[p] >= thr), al[s] * T[p], 0.0)
                C[p] += w[:, None] * colours[gid[s]]
                T[p] -= w
            res.append(np.concatenate([C, (1.0 - T)[:, None]], 1).reshape(self.H, self.W, 4))
        return np.minimum(res[0], res[1]), np.maximum(res[0], res[1])

    def covering(self, x, y):
        """[(global id, squared canonical distance, alpha, borderline)] of the fragments (and near misses) of pixel (x, y), in id order"""
        out = []
        xx, yy = np.array([[x]]), np.array([[y]])
        for i in range(self.table["id"].shape[0]):
            if abs(x + 0.5 - self.table["c"][i, 0]) > self.table["box"][i, 0] + 1 or abs(y + 0.5 - self.table["c"][i, 1]) > self.table["box"][i, 1] + 1:
                continue
            keep, edge, d2, al = self._one(i, xx, yy)
            if keep[0, 0] or edge[0, 0]:
                out.append((int(self.table["id"][i]), float(d2[0, 0]), float(al[0, 0]), bool(edge[0, 0])))
        return out


def fragments(projected, V, P, W, H, st, gaussian=False, delta=1e-4, depth=None):
    """projected: [project(...)] per instance in creation order (the same V, P, W, H and settings).  depth: occluder depth image [H, W]
    or None; a particle then leaves a fragment only where its key depth (the centre's ndc z) is <= depth.  Returns GutFragments."""
    t = table(projected, delta)
    out = GutFragments(W, H, t, pixel_rays(V, P, W, H, st), st, gaussian, delta, None if depth is None else np.asarray(depth, np.float64))
    r0, r1 = st["strip"] if st["strip"] is not None else (0, (H + 15) // 16)
    ya, yb = r0 * 16, min(r1 * 16, H) - 1
    pad = 1.0 + delta
    for i in range(t["id"].shape[0]):
        ex, ey = pad * t["box"][i] + t["cerr"][i]
        x0, x1 = max(0, int(np.floor(t["c"][i, 0] - ex - 0.5))), min(W - 1, int(np.ceil(t["c"][i, 0] + ex - 0.5)))
        y0, y1 = max(ya, int(np.floor(t["c"][i, 1] - ey - 0.5))), min(yb, int(np.ceil(t["c"][i, 1] + ey - 0.5)))
        if x1 < x0 or y1 < y0:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        keep, edge, _, al = out._one(i, xx, yy)
        win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        if gaussian:   # the fragments themselves, for blend()
            m = keep | edge
            out._frag.append((yy[m] * W + xx[m], np.full(int(m.sum()), t["z"][i]), np.full(int(m.sum()), t["id"][i]), al[m], (keep & ~edge)[m]))
        out.count[win] += keep
        out.borderline_count[win] += edge
        z = t["z"][i]
        zw, idw, ow, zo = out._z[win], out.nearest_id[win], out.nearest_open[win], out._zopen[win]
        tie = keep & (np.abs(z - zw) <= 1e-6 * max(abs(z), 1e-3))
        nearer = keep & (z < zw) & ~tie
        ow[nearer] = False
        ow[tie] = True
        idw[nearer] = t["id"][i]
        zw[nearer] = z
        zo[edge] = np.minimum(zo[edge], z)
    # a borderline fragment at or in front of the nearest counted one leaves the nearest open
    out.nearest_open |= np.isfinite(out._zopen) & (out._zopen <= out._z * (1.0 + 1e-6) + 1e-9)
    return out


where, describe = np_fragments.where, np_fragments.describe
