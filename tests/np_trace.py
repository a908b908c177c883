"""Float64 restatement of the traced pipeline (mgs_render_traced): primary rays of the reference's 3DGRT ray tracer.

Test infrastructure only.  Brute force over all particles per ray, no hierarchy; the pass structure exactly as written:
  shaders/threedgrt_raytrace.rgen.slang:159-196    ray, depth of field
  shaders/threedgrt_raytrace.rgen.slang:615-819    passes of samples_per_pass nearest hits, walk, tMin = max(tMin, dist)
  shaders/threedgrt_raytrace.rint.slang:159-172    t of a hit: -dot(o,d)/dot(d,d) in the canonical frame, unnormalised direction
  shaders/threedgrt.h.slang:57-235                 canonical ray, response, particleProcessHit, particleIntegrate
  shaders/particle_as_build.comp.slang:74-87       the response the proxy is circumscribed around
Column-vector form (x' = M x with M the math matrix), i.e. not the form the kernels are written in.

Fragile pixels.  The device evaluates the same formulas in fp32 (unit roundoff u = 2^-24).  A pixel is FRAGILE when a decision
on its ray could flip under that rounding; such pixels are excluded from the exact comparisons (hit count, picked id).  The
margins, with x = om - p the model-space offset of the ray origin from the particle, oc / dc the canonical origin / direction:
  * canonical origin, per axis c:  d_oc[c] = 8 u (|om|_1 + |p|_1 + |x|_1) / s_c   -- om = M^-1 o is four products and three sums of
    terms up to |om|_1 (<= 4 u |om|_1), the subtraction adds u |x|, the rotation three products and two sums (<= 3 u |x|_1), the
    division u; 8 covers the sum with the stored inverse's own rounding (2 u).
  * distance to the ray:  d_d = |d_oc| + 16 u |oc|   -- the cross product with the unit direction moves by at most |d_oc|, and the
    direction itself (two 3x3 products, a division, a normalisation: <= 8 u relative) plus the cross product's own rounding (<= 8 u)
    turn |oc| by 16 u.
  * hit parameter:  d_t = d_d / |dc|   -- t = -(oc . dc) / (dc . dc) carries the same perturbations divided by |dc|.
  * response: evaluated at d - d_d and d + d_d and widened by 16 u relative (the hardware exponential and the products in its
    argument).  A threshold on the response (proxy threshold, kernel_min_response, alpha_cull_threshold / density) between the two
    values makes the pixel fragile.
  * order: two candidate hits of a ray whose t differ by no more than the sum of their d_t, or a hit within d_t of tMin or tMax, make
    the pixel fragile (this covers the K-th slot and the epsT window: both are decided by the order of the hits).
  * transmittance: each accepted hit adds (alpha_hi - alpha_lo) / (1 - alpha) + 4 u to the relative uncertainty of T (kept in double
    on both sides); T within that of min_transmittance or of the iso threshold when it is tested makes the pixel fragile.
  * iso-surface normal (normal_method = 1, computeEllipsoidNormal threedgrt.h.slang:423-537): rem = 9 - dist^2 moves by
    2 dist d_d + d_d^2 (+ 16 u of the 9), half = sqrt(rem) by that over 2 half, the closest approach -b by d_d; rem within its
    margin of 0, or the near root -b - half (or, when that is negative, the far root) within the sum of the two of 0, makes the
    pixel fragile: each is a branch of raySphereIntersection.

Exact ties.  The order margin above would mark every pair of coincident particles fragile, and the device's tie rule could never be
tested.  But two candidates of one ray that belong to the SAME instance and whose centre, log-scale and quaternion are bit-identical
are evaluated by the device from the same bits through the same instruction sequence (evalParticle: one ray, one instance transform,
loadParticle of identical words), so their t is bit-identical on the device whatever it is, and here too.  Such a pair therefore does
not make the pixel fragile through the order rule: its order is decided by the tie rule alone, (t, caller's global id) ascending
(rahit.slang:152-167 inserts by distance; the library orders equal distances by the id in the caller's order), which the sort key of
the candidate list encodes.  Every other margin (thresholds, range, the neighbours that are not its copy) still applies to each of
the two.  A pass ends at tMin = the last walked t and the next collects t > tMin + epsT: the copy of a hit that was walked last in
its pass is never a hit, on either side (at samples_per_pass = 1 no second copy ever is).

Declared ties.  Copies of one particle are stored in the caller's order (the commit sort breaks equal codes by index), so they cannot
tell an order by the caller's id from an order by the storage id.  Different particles can: on a ray whose model-space direction is
(0, 0, dz) exactly, a particle with the identity quaternion has canonical direction (0, 0, dz / s_z), every product with its x and y
components is +-0, and t = -(oc_z dc_z) / (dc_z dc_z) is computed from the ray, the centre's z and the log-scale's z alone: particles
that share those two words have bit-identical t whatever their x, y and other scales (evalParticle: the same instruction sequence on
the same bits; the zeros add exactly).  trace(exact_ties = [(y, x, instance, local ids)]) declares such a group for ONE pixel; there its
members are an exact tie like copies are (their float64 t must be equal here too, which is asserted), and every other margin of
theirs stays.  On every other pixel the group is treated like any particles.
"""
import numpy as np

import np_reference as npr

U = 2.0 ** -24
SH_C0 = 0.28209479177387814
T_MIN, T_MAX, EPS_T = 0.001, 10000.0, 1e-9
INVALID = 0xFFFFFFFF


def prepare_set(arrays, rgba=None, sh=None):
    """the particle data as the device holds it: centres, exp(scale), rotation rows, rgba (0.5 + C0 f_dc, sigmoid(opacity)) and the SH
    record [n][15][3]; rgba [n][4] and sh [n][15][3] (dequantised, caller's order, zero beyond the set's coefficients) may be handed
    in: what mgs_scene_download_set returns for a set committed in a quantised format.  shape[n]: equal for two particles exactly
    when centre, log-scale and quaternion are bit-identical (the exact-tie rule of the module docstring)."""
    pos = np.asarray(arrays["positions"], np.float32).astype(np.float64).reshape(-1, 3)
    n = pos.shape[0]
    s = np.exp(np.asarray(arrays["scale"], np.float32)).astype(np.float64).reshape(-1, 3)
    q = np.asarray(arrays["rotation"], np.float32).astype(np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)  # rotation matrix [n, row, col]
    if rgba is None:
        f_dc = np.asarray(arrays["f_dc"], np.float32).reshape(-1, 3)
        op = np.asarray(arrays["opacity"], np.float32).reshape(-1)
        # the upload clamps to [0, 1] (SplatSetVk::initDataBuffers, src/splat_set_vk.cpp:263-435)
        rgba = np.concatenate([np.clip(np.float32(0.5) + np.float32(SH_C0) * f_dc, 0.0, 1.0),
                               (1.0 / (1.0 + np.exp(-op.astype(np.float64)))).astype(np.float32)[:, None]], 1)
    rgba = np.asarray(rgba, np.float32).astype(np.float64).reshape(-1, 4)
    fr = np.asarray(arrays["f_rest"], np.float32).astype(np.float64).reshape(n, -1)
    cpc = fr.shape[1] // 3
    if sh is None:
        sh = np.zeros((n, 15, 3))
        if cpc:
            sh[:, :cpc, :] = fr.reshape(n, 3, cpc).transpose(0, 2, 1)
    else:
        sh = np.asarray(sh, np.float32).astype(np.float64).reshape(n, 15, 3)
    degree = {0: 0, 3: 1, 8: 2, 15: 3}[cpc]
    raw = np.concatenate([np.asarray(arrays[k], np.float32).reshape(n, -1) for k in ("positions", "scale", "rotation")], 1)
    shape = np.unique(np.ascontiguousarray(raw).view(np.uint32), axis=0, return_inverse=True)[1].reshape(-1) if n else np.zeros(0, np.int64)
    return dict(pos=pos, s=s, R=R, rgba=rgba, sh=sh, degree=degree, n=n, shape=shape)


def response(degree, d):
    """generalised Gaussian in the canonical distance d (threedgrt.h.slang:83-127)"""
    d = np.maximum(d, 0.0)
    if degree == 0:
        return np.maximum(1.0 - 0.329630334487 * d, 0.0)
    return np.exp(-4.5 / 3.0 ** degree * d ** degree)


def rays(V, P, W, H, fisheye=False, fov_rad=None, dof=None, y0=0, y1=None):
    """origin [H,W,3], direction [H,W,3], ok [H,W]; dof = (focus_dist, aperture, frame_sample_id) or None"""
    y1 = H if y1 is None else y1
    vi, pi = np.linalg.inv(np.asarray(V, np.float64)), np.linalg.inv(np.asarray(P, np.float64))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ok = np.ones((H, W), bool)
    if fisheye:
        u, v = xs / (W - 1.0) * 2.0 - 1.0, ys / (H - 1.0) * 2.0 - 1.0
        r = np.sqrt(u * u + v * v)
        ok = ~(r > 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            phic = np.where(np.abs(r) > 1e-9, u / r, 0.0)
        phi = np.arccos(np.clip(phic, -1.0, 1.0))
        phi = np.where(v < 0.0, -phi, phi)
        th = r * fov_rad * 0.5
        cam = np.stack([np.cos(phi) * np.sin(th), -np.sin(phi) * np.sin(th), -np.cos(th)], -1)
    else:
        dx, dy = (xs + 0.5) / W * 2.0 - 1.0, (ys + 0.5) / H * 2.0 - 1.0
        tgt = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ pi.T
        cam = tgt[..., :3]
    d = cam @ vi[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(vi[:3, 3], d.shape).copy()
    if dof is not None:
        focus, aperture, sample = dof
        right, up = vi[:3, 0], vi[:3, 1]
        for y in range(H):
            for x in range(W):
                seed = _xxhash32(x, y, sample)
                seed, a = _rand(seed)
                seed, b = _rand(seed)
                r1, r2 = np.float32(a) * np.float32(6.28318530717958647692), np.float32(b) * np.float32(aperture)
                ap = (np.cos(np.float64(r1)) * right + np.sin(np.float64(r1)) * up) * np.sqrt(np.float64(r2))
                nd = d[y, x] * focus - ap
                o[y, x] += ap
                d[y, x] = nd / np.linalg.norm(nd)
    return o, d, ok


def _xxhash32(px, py, pz):
    m = 0xFFFFFFFF
    p0, p1, p2, p3 = 2246822519, 3266489917, 668265263, 374761393
    h = (pz + p3 + px * p1) & m
    h = (p2 * (((h << 17) | (h >> 15)) & m)) & m
    h = (h + py * p1) & m
    h = (p2 * (((h << 17) | (h >> 15)) & m)) & m
    h = (p0 * (h ^ (h >> 15))) & m
    h = (p1 * (h ^ (h >> 13))) & m
    return h ^ (h >> 16)


def _rand(state):
    m = 0xFFFFFFFF
    prev = (state * 747796405 + 2891336453) & m
    word = (((prev >> ((prev >> 28) + 4)) ^ prev) * 277803737) & m
    r = ((word >> 22) ^ word) & m
    return prev, np.frombuffer(np.uint32(0x3F800000 | (r >> 9)).tobytes(), np.float32)[0] - np.float32(1.0)


def trace(instances, V, P, W, H, samples_per_pass=18, max_passes=200, min_transmittance=0.01, adaptive_clamping=True,
          depth_iso_threshold=0.7, kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull=1.0 / 255.0, sh_degree=3,
          fisheye=False, fov_rad=None, dof=None, thin=1e-6, rows=None, sh_only=False, no_gauss=False, single_sorted_walk=False, normal_method=0,
          reverse_ties=False, exact_ties=()):
    """instances: [(prepared set, M 4x4 math)] in creation order.  Returns dict(image [H,W,4], hits [H,W], depth [H,W], id [H,W],
    normal [H,W,4], fragile [H,W], candidates [H,W], depth_tol [H,W]: the fp32 tolerance of
    the picked depth).  single_sorted_walk: ignore the pass structure, walk all candidates in order
    (what the passes reduce to when K exceeds every ray's candidate count).  normal_method: 0 the max-density plane, 1 the iso
    surface; thin: thin_particle_threshold.  reverse_ties: order exact ties by DESCENDING id (the wrong rule; for the test that shows
    a case can see the rule).  exact_ties: declared ties, see the module docstring.  tie_pair [H,W]: the walk accepted two bit-identical candidates one after the other."""
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    kmr = float(np.float32(kernel_min_response))
    acull, aclamp = float(np.float32(alpha_cull)), float(np.float32(alpha_clamp))
    minT, isoT = float(np.float32(min_transmittance)), float(np.float32(depth_iso_threshold))
    O, D, OK = rays(V, P, W, H, fisheye, fov_rad, dof)
    y0, y1 = (0, H) if rows is None else rows
    img = np.zeros((H, W, 4))
    hits = np.zeros((H, W), np.int64)
    depth = np.zeros((H, W))
    depth_tol = np.zeros((H, W))
    ids = np.full((H, W), INVALID, np.int64)
    nrm = np.zeros((H, W, 4))
    fragile = np.zeros((H, W), bool)
    ncand = np.zeros((H, W), np.int64)
    tie_pair = np.zeros((H, W), bool)
    # per instance and pixel row: every particle against every ray of the row
    per_inst = []
    base = 0
    for ps, M in instances:
        M = np.asarray(M, np.float64)
        Mi, Ri = np.linalg.inv(M), np.linalg.inv(M[:3, :3])
        dens = ps["rgba"][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.minimum(kmr / dens if adaptive_clamping else np.full_like(dens, kmr), 0.97)
        alive = dens > acull  # a particle at or below the cull threshold has no leaf and is never a hit
        alive &= np.isfinite(ps["s"]).all(1) & np.isfinite(ps["pos"]).all(1) & np.isfinite(ps["R"]).all((1, 2))
        per_inst.append((ps, M, Mi, Ri, dens, thr, alive, base))
        base += ps["n"]
    for y in range(y0, y1):
        o_row, d_row, ok_row = O[y], D[y], OK[y]
        cand = [[] for _ in range(W)]  # per pixel: (t, global id, instance, local, d, d_d, d_t)
        frag_row = np.zeros(W, bool)
        for k, (ps, M, Mi, Ri, dens, thr, alive, gbase) in enumerate(per_inst):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                continue
            pos, s, R = ps["pos"][idx], ps["s"][idx], ps["R"][idx]
            om = o_row @ Mi[:3, :3].T + Mi[:3, 3]            # [W,3]
            dm = d_row @ Ri.T                                 # [W,3] unnormalised: t stays the world ray's parameter
            x = om[:, None, :] - pos[None, :, :]             # [W,n,3]
            oc = np.einsum("wnj,njc->wnc", x, R) / s[None]   # R^T x / s
            dc = np.einsum("wj,njc->wnc", dm, R) / s[None]
            dd = (dc * dc).sum(-1)
            t = -(oc * dc).sum(-1) / dd
            cr = np.cross(dc, oc)
            dist = np.sqrt((cr * cr).sum(-1) / dd)
            l1 = np.abs(om).sum(-1)[:, None] + np.abs(pos).sum(-1)[None] + np.abs(x).sum(-1)
            d_oc = 8.0 * U * l1[..., None] / s[None]
            ocn = np.sqrt((oc * oc).sum(-1))
            d_d = np.sqrt((d_oc * d_oc).sum(-1)) + 16.0 * U * ocn
            d_t = d_d / np.sqrt(dd)
            r_mid = response(kernel_degree, dist)
            r_hi = response(kernel_degree, dist - d_d) * (1.0 + 16.0 * U)
            r_lo = response(kernel_degree, dist + d_d) * (1.0 - 16.0 * U)
            th = thr[idx][None]
            inr = (t > T_MIN + EPS_T) & (t < T_MAX + EPS_T)
            is_c = inr & (r_mid > th)
            maybe = ((t + d_t > T_MIN) & (t - d_t < T_MAX + EPS_T)) & (r_hi > th) & ~((t - d_t > T_MIN + EPS_T) & (t + d_t < T_MAX) & (r_lo > th))
            frag_row |= maybe.any(1)  # a proxy or range decision that rounding could flip
            # the walk's own thresholds on the response
            for lim in (np.full_like(th, kmr), acull / dens[idx][None]):
                frag_row |= (is_c & (r_lo <= lim) & (r_hi >= lim)).any(1)
            wi, ni = np.nonzero(is_c)
            for a, b in zip(wi, ni):
                cand[a].append((t[a, b], gbase + idx[b], k, idx[b], dist[a, b], d_d[a, b], d_t[a, b], om[a], dm[a]))
        for xp in range(W):
            if not ok_row[xp]:
                img[y, xp] = (0, 0, 0, 1)
                continue
            c = sorted(cand[xp], key=lambda e: (e[0], -e[1] if reverse_ties else e[1]))
            ncand[y, xp] = len(c)
            fr = bool(frag_row[xp])

            def same_bits(e, f):  # one instance, bit-identical centre, log-scale and quaternion: bit-identical t on the device
                if e[2] == f[2] and per_inst[e[2]][0]["shape"][e[3]] == per_inst[e[2]][0]["shape"][f[3]]:
                    return True
                for ty, tx, tk, tids in exact_ties:  # a declared tie of this pixel
                    if (ty, tx) == (y, xp) and e[2] == f[2] == tk and e[3] in tids and f[3] in tids:
                        assert e[0] == f[0], "a declared exact tie has different t in the restatement"
                        return True
                return False

            for i in range(len(c) - 1):
                if c[i + 1][0] - c[i][0] <= c[i][6] + c[i + 1][6] and not same_bits(c[i], c[i + 1]):
                    fr = True
            T, relT = 1.0, 0.0
            rad = np.zeros(3)
            n_acc = np.zeros(3)
            wsum, iso_d, pick, hc, pick_dt = 0.0, 0.0, INVALID, 0, 0.0
            tmin = T_MIN
            last_acc = None

            def near(Tv, lim):
                return abs(Tv - lim) <= Tv * (relT + 4.0 * U)

            def walk(e):
                nonlocal T, relT, rad, n_acc, wsum, iso_d, pick, pick_dt, hc, fr, last_acc
                tt, gid, k, li, dist, d_d, d_t, om, dm = e
                ps, M, Mi, Ri, dens, thr, alive, gbase = per_inst[k]
                den = dens[li]
                resp = float(response(kernel_degree, dist))
                alpha = min(aclamp, resp * den)
                if not (alpha > acull and resp > kmr):
                    return
                a_hi = min(aclamp, float(response(kernel_degree, dist - d_d)) * den * (1 + 16 * U))
                a_lo = min(aclamp, float(response(kernel_degree, dist + d_d)) * den * (1 - 16 * U))
                if no_gauss:
                    alpha = a_hi = a_lo = 1.0
                v = ps["pos"][li] - om
                v = v / np.linalg.norm(v)
                col = np.full(3, 0.5) if sh_only else ps["rgba"][li, :3].copy()
                deg = min(ps["degree"], sh_degree)
                if deg > 0:
                    col = col + npr.sh_radiance(ps["sh"][li:li + 1], deg, v[None])[0]
                w = alpha * T
                rad += col * w
                T *= 1.0 - alpha
                relT += (a_hi - a_lo) / max(1.0 - alpha, 1e-30) + 4.0 * U
                hc += 1
                if last_acc is not None and last_acc[0] == tt and same_bits(last_acc, e):
                    tie_pair[y, xp] = True
                last_acc = e
                nw, n_frag = _normal_world(ps, li, om, dm, Ri, thin, normal_method, d_d)
                fr = fr or n_frag
                n_acc += nw * w
                wsum += w
                if iso_d == 0.0:
                    if near(T, isoT):
                        fr = True
                    if T < isoT:
                        iso_d, pick, pick_dt = tt, gid, d_t

            if single_sorted_walk:
                for e in c:
                    if near(T, minT):
                        fr = True
                    if T > minT:
                        walk(e)
            else:
                rest = c
                for _ in range(max_passes):
                    if near(T, minT):
                        fr = True
                    if not (tmin <= T_MAX and T > minT):
                        break
                    rest = [e for e in rest if e[0] > tmin + EPS_T]
                    if not rest:
                        break
                    for e in rest[:samples_per_pass]:
                        if near(T, minT):
                            fr = True
                        if T > minT:
                            walk(e)
                            tmin = max(tmin, e[0])
            img[y, xp] = (rad[0], rad[1], rad[2], 1.0 - T)
            hits[y, xp] = hc
            nrm[y, xp] = (n_acc[0], n_acc[1], n_acc[2], wsum)
            if pick != INVALID:
                def ndc_z(tv):
                    clip = P @ (V @ np.append(o_row[xp] + tv * d_row[xp], 1.0))
                    return clip[2] / clip[3], clip
                depth[y, xp], clip = ndc_z(iso_d)
                ids[y, xp] = pick
                # what fp32 may move the picked depth by: the hit's own d_t, plus the rounding of origin + t * direction and of the view
                # transform (8 u of the magnitudes that are summed), taken through ndc z numerically (it is steep close to the camera),
                # plus the projection's products and the division (8 u of the terms of clip z over clip w)
                dt = pick_dt + 8.0 * U * (np.abs(o_row[xp]).sum() + iso_d + np.abs(V[:3, 3]).sum())
                depth_tol[y, xp] = (max(abs(ndc_z(iso_d + dt)[0] - depth[y, xp]), abs(ndc_z(iso_d - dt)[0] - depth[y, xp]))
                                    + 8.0 * U * (np.abs(P[2]) @ np.abs(V @ np.append(o_row[xp] + iso_d * d_row[xp], 1.0))) / abs(clip[3]))
            fragile[y, xp] = fr
    return dict(image=img, hits=hits, depth=depth, id=ids, normal=nrm, fragile=fragile, candidates=ncand, depth_tol=depth_tol,
                tie_pair=tie_pair)


def _normal_world(ps, li, om, dm, Ri, thin, normal_method=0, d_d=0.0):
    """computeEllipsoidNormalMaxDensityPlane (threedgrt.h.slang:358-418) or computeEllipsoidNormal (:423-496, raySphereIntersection
    :502-537 with the canonical ray's NORMALISED direction, radius 3, range [0, inf)) and the inverse-transpose to world space (:218).
    Returns (normal, fragile): fragile when a branch of the iso-surface intersection lies within the hit's fp32 margin d_d."""
    s, R, p = ps["s"][li], ps["R"][li], ps["pos"][li]
    local = om - p
    iso = normal_method == 1
    th = max(0.02 * s.max(), float(np.float32(thin))) if iso else float(np.float32(thin))
    small = s < th
    fragile = bool((np.abs(s - th) <= 8.0 * U * th).any())  # exp(scale) on the device may differ from numpy's by an ulp or two
    fallback = -dm / np.linalg.norm(dm)
    if small.sum() == 0 and not iso:
        g = R @ ((R.T @ local) / (s * s))
        n = g / np.linalg.norm(g)
        if n @ local < 0:
            n = -n
    elif small.sum() == 0:
        oc, dc = (R.T @ local) / s, (R.T @ dm) / s
        dn = dc / np.linalg.norm(dc)
        b = oc @ dn
        cr = np.cross(dn, oc)
        dist2 = cr @ cr
        rem = 9.0 - dist2
        m_rem = 2.0 * np.sqrt(dist2) * d_d + d_d * d_d + 16.0 * U * 9.0
        fragile = fragile or abs(rem) <= m_rem
        n = fallback
        if rem >= 0.0:
            half = np.sqrt(rem)
            m_t = d_d + m_rem / max(2.0 * half, 1e-300) + 16.0 * U * (abs(b) + half)
            t1, t2 = -b - half, -b + half
            fragile = fragile or abs(t1) <= m_t or (t1 < 0.0 and abs(t2) <= m_t)
            tq = t1 if t1 >= 0.0 else t2
            if tq >= 0.0:
                h = oc + tq * dn
                g = R @ (h / np.linalg.norm(h) / s)
                n = g / np.linalg.norm(g)
    elif small.sum() == 1:
        n = R[:, int(np.argmax(small))]
        if n @ local < 0:
            n = -n
    else:
        n = fallback
    wn = Ri.T @ n
    return wn / np.linalg.norm(wn), bool(fragile)


def psnr_rgb(a, b):
    mse = np.mean((np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]) ** 2)
    return 99.0 if mse <= 0 else 10.0 * np.log10(1.0 / mse)
