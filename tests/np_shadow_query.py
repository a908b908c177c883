"""Float64 restatement of the shadow and light queries (mgs_trace_shadow_rays, mgs_shade_points).  Test infrastructure only.  Thin on
purpose: np_trace_lit has the per-instance tables (_per_inst), the shading (_shade64 over np_lighting._shade_direct) and the margins
behind `fragile`; what is restated here is what the queries add to a light pass's shadow ray:
  * the window's lower bound: a candidate needs t > max(t_min, 0); t within its d_t of that bound is fragile;
  * the given-direction rule: the ray is used as given, t runs along the unnormalised direction and t_max plays lightDist (the
    formulas of np_trace_lit._eval hold for any direction: t = -dot(oc, dc) / dot(dc, dc));
  * the invalid-ray rule: a non-finite component, a zero-length direction or t_min > t_max gives (1,1,1) and 0 hits;
  * the loop over the lights for a caller's point (np_trace_lit.lit has it inside its loop over pixels).
Every function takes the arithmetic's dtype: dt = np.float32 is the float32 run of the same text (the transmittance itself stays a
double, as on the device), whose distance from the float64 run sizes the transmittance bar (shadow_query_cases.TWIN_DEV)."""
import numpy as np

import np_lighting as nl
import np_reference as npr
import np_trace_lit as ntl
from np_trace import U, response

per_inst = ntl._per_inst


def valid_rays(O, D, tmin, tmax):
    O, D = np.asarray(O, np.float32), np.asarray(D, np.float32)
    fin = np.isfinite(O).all(1) & np.isfinite(D).all(1) & np.isfinite(tmin) & np.isfinite(tmax)
    with np.errstate(invalid="ignore"):
        return fin & (D != 0).any(1) & (np.asarray(tmin, np.float32) <= np.asarray(tmax, np.float32))


def _eval(pi, o, d, degree, d_o, dt):
    """np_trace_lit._eval in the arithmetic of dt"""
    ps = pi["ps"]
    idx = np.nonzero(pi["alive"])[0]
    pos, s, R = ps["pos"][idx].astype(dt), ps["s"][idx].astype(dt), ps["R"][idx].astype(dt)
    Mi, Ri = pi["Mi"].astype(dt), pi["Ri"].astype(dt)
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    om = Mi[:3, :3] @ o + Mi[:3, 3]
    dm = Ri @ d
    x = om[None] - pos
    oc = np.einsum("nj,njc->nc", x, R) / s
    dc = np.einsum("j,njc->nc", dm, R) / s
    dd = (dc * dc).sum(-1)
    t = -(oc * dc).sum(-1) / dd
    cr = np.cross(dc, oc)
    dist = np.sqrt((cr * cr).sum(-1) / dd)
    l1 = np.abs(om).sum() + np.abs(pos).sum(-1) + np.abs(x).sum(-1)
    d_oc = (8.0 * U * l1[:, None] + d_o * pi["mnorm"]) / s
    d_d = np.sqrt((d_oc * d_oc).sum(-1)) + 16.0 * U * np.sqrt((oc * oc).sum(-1))
    d_t = d_d / np.sqrt(dd)
    return dict(idx=idx, t=t, dist=dist, d_d=d_d, d_t=d_t, om=om, r_mid=response(degree, dist),
                r_hi=response(degree, dist - d_d) * (1.0 + 16.0 * U), r_lo=response(degree, dist + d_d) * (1.0 - 16.0 * U))


def shadow_ray(pinst, o, d, t_min, t_max, K, threshold, strength, d_o=0.0, kernel_degree=2, kmr=0.0113, acull=1.0 / 255.0, aclamp=0.99,
               sh_degree=3, no_gauss=False, sh_only=False, dt=np.float64):
    """np_trace_lit.shadow_ray with the window (max(t_min, 0), fp32(t_max - 0.001)) along the given direction.
    Returns (transmittance[3], accepted hits, fragile)."""
    kmr, acull, aclamp = (float(np.float32(v)) for v in (kmr, acull, aclamp))
    threshold, strength = float(np.float32(threshold)), float(np.float32(strength))
    t_max = float(np.float32(t_max))
    tlo = max(float(np.float32(t_min)), 0.0)
    thi = float(np.float32(np.float32(t_max) - np.float32(0.001)))
    cand, frag = [], False
    for k, pi in enumerate(pinst):
        if not pi["alive"].any():
            continue
        e = _eval(pi, o, d, kernel_degree, d_o, dt)
        th = pi["thr"][e["idx"]]
        t, d_t = e["t"], e["d_t"]
        m_hi = d_t + d_o + 4.0 * U * abs(thi)
        is_c = (t > tlo) & (t < thi) & (e["r_mid"] > th)
        maybe = (t + d_t > tlo) & (t - m_hi < thi) & (e["r_hi"] > th) & ~((t - d_t > tlo) & (t + m_hi < thi) & (e["r_lo"] > th))
        frag |= bool(maybe.any())
        dens = pi["dens"][e["idx"]]
        for lim in (np.full_like(th, kmr), acull / dens):
            frag |= bool((is_c & (e["r_lo"] <= lim) & (e["r_hi"] >= lim)).any())
        for b in np.nonzero(is_c)[0]:
            cand.append((float(t[b]), pi["base"] + e["idx"][b], k, e["idx"][b], e["dist"][b], e["d_d"][b], float(d_t[b]), e["om"]))
    cand.sort(key=lambda c: (c[0], c[1]))
    for i in range(min(len(cand) - 1, K)):
        a, b = cand[i], cand[i + 1]
        same = a[2] == b[2] and pinst[a[2]]["ps"]["shape"][a[3]] == pinst[a[2]]["ps"]["shape"][b[3]]
        if b[0] - a[0] <= a[6] + b[6] and not same:
            frag = True
    T, relT, rad, hits = 1.0, 0.0, np.zeros(3), 0
    for tt, gid, k, li, dist, d_d, d_t, om in cand[:K]:
        if tt >= t_max:
            continue
        pi = pinst[k]
        ps, den = pi["ps"], dt(pi["dens"][li])
        resp = response(kernel_degree, dist)
        alpha = min(aclamp, float(resp * den))
        if alpha > acull and float(resp) > kmr:
            a_hi = min(aclamp, float(response(kernel_degree, dist - d_d)) * float(den) * (1 + 16 * U))
            a_lo = min(aclamp, float(response(kernel_degree, dist + d_d)) * float(den) * (1 - 16 * U))
            if no_gauss:
                alpha = a_hi = a_lo = 1.0
            if strength != 0.0:
                v = ps["pos"][li].astype(dt) - om
                v = v / np.sqrt((v * v).sum())
                col = np.full(3, 0.5) if sh_only else ps["rgba"][li, :3].copy()
                deg = min(ps["degree"], sh_degree)
                if deg > 0:
                    col = col + npr.sh_radiance(ps["sh"][li:li + 1], deg, v[None].astype(np.float64))[0]
                rad += col * float(dt(alpha) * dt(T))
            T *= 1.0 - alpha
            relT += (a_hi - a_lo) / max(1.0 - alpha, 1e-30) + 4.0 * U
            hits += 1
        if abs(T - threshold) <= T * (relT + 4.0 * U):
            frag = True
        if T < threshold:
            T = 0.0
            break
    Tf = min(max(T, 0.0), 1.0)
    scaled = min(max((Tf - threshold) / (1.0 - threshold), 0.0), 1.0)
    mx = rad.max()
    nc = rad / mx if mx > 0.001 else np.ones(3)
    if strength != 0.0 and abs(mx - 0.001) <= mx * (relT + 16.0 * U):
        frag = True
    res = np.clip(scaled * (1.0 + (nc - 1.0) * (strength * (1.0 - scaled))), 0.0, 1.0)
    if abs(res.max() - 0.001) <= Tf * (relT + 4.0 * U) / (1.0 - threshold) + 8.0 * U:
        frag = True
    return res, hits, frag


def shadow_rays(pinst, O, D, tmin, tmax, K=18, threshold=0.8, strength=0.0, **kw):
    """a batch: dict(transmittance [n,3], hits [n], fragile [n], valid [n])"""
    O, D = np.asarray(O, np.float32).astype(np.float64), np.asarray(D, np.float32).astype(np.float64)
    n = O.shape[0]
    ok = valid_rays(O, D, tmin, tmax)
    T, hits, frag = np.ones((n, 3)), np.zeros(n, np.int64), np.zeros(n, bool)
    for i in np.nonzero(ok)[0]:
        T[i], hits[i], frag[i] = shadow_ray(pinst, O[i], D[i], tmin[i], tmax[i], K, threshold, strength, **kw)
    return dict(transmittance=T, hits=hits, fragile=frag, valid=ok)


def shade_points(pinst, pts, materials, lights, camera_pos, shadows=1, offset=0.2, threshold=0.8, strength=0.0, K=18, **kw):
    """pts: a structured array with position, normal, view_dir, radiance, material (capi.SURFACE_POINT_DTYPE's fields); materials,
    lights: np_lighting dicts.  dict(color [n,3], shadow_hits [n], rays [n], fragile [n], range_fragile [n], valid [n]): the loop of
    np_trace_lit.lit.  `rays` is exact wherever range_fragile is not set."""
    f32 = lambda v: float(np.float32(v))
    n = len(pts)
    offset = f32(offset)
    F = {k: np.asarray(pts[k], np.float32).astype(np.float64) for k in ("position", "normal", "view_dir", "radiance")}
    ok = np.isfinite(np.concatenate(list(F.values()), 1)).all(1) & (np.asarray(pts["material"]) < len(materials))
    color, hits, nrays, frag = np.zeros((n, 3)), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    rfrag = np.zeros(n, bool)  # a light's range decision is within its margin: the one thing, with needShading, a point's ray count hangs on
    cam = np.asarray(camera_pos, np.float32).astype(np.float64)
    for i in np.nonzero(ok)[0]:
        pos, nrm, vdir, rad0 = (F[k][i] for k in ("position", "normal", "view_dir", "radiance"))
        m = materials[int(pts["material"][i])]
        mv = lambda key: np.asarray(m[key], np.float32).astype(np.float64)
        color[i] = rad0 * mv("emission")
        if not nl.need_shading(m):
            continue
        nlen = np.linalg.norm(nrm)
        if abs(nlen - 0.2) <= 16.0 * U:  # the length is an fp32 square root of an fp32 dot product of the caller's own numbers
            frag[i] = True
        nn = -vdir if nlen <= 0.2 else nrm
        nn = nn / np.linalg.norm(nn)
        mat = dict(ambient=(rad0 * mv("ambient"))[None], diffuse=(rad0 * mv("diffuse"))[None], specular=(rad0 * mv("specular"))[None],
                   shininess=np.array([f32(m["shininess"])]))
        out = color[i][None].copy()
        if not lights:
            nl._shade_direct(nl.headlight(cam), pos[None], nn[None], mat, vdir[None], out, np.float64, False)
        for L in lights:
            if int(L["type"]) == nl.LIGHT_DIRECTIONAL:
                dirn = np.asarray(L["direction"], np.float32).astype(np.float64)
                ldir, ldist, lp1 = -dirn / np.linalg.norm(dirn), 1e10, 0.0
            else:
                lp = np.asarray(L["position"], np.float32).astype(np.float64)
                to = lp - pos
                ldist, lp1, rng = np.linalg.norm(to), np.abs(lp).sum(), f32(L["range"])
                if abs(ldist - rng) <= 8.0 * U * (np.abs(pos).sum() + lp1):
                    frag[i] = rfrag[i] = True
                if ldist > rng:
                    continue  # skipped entirely: no ambient either
                ldir = to / ldist
            Ls = dict(L, color=np.asarray(L["color"], np.float32).astype(np.float64))
            in_shadow = False
            if shadows and any(pi["alive"].any() for pi in pinst):
                nrays[i] += 1
                d_o = 8.0 * U * (np.abs(pos).sum() + lp1 + offset + 1.0)  # the fp32 light vector, its normalisation and the offset
                res, h, fr = shadow_ray(pinst, pos + ldir * offset, ldir, 0.0, ldist, K, threshold, strength, d_o, **kw)
                hits[i] += h
                frag[i] |= fr
                Ls["color"] = Ls["color"] * res
                in_shadow = res.max() < 0.001
            if in_shadow:
                out += mat["ambient"]
            else:
                ntl._shade64(Ls, pos[None], nn[None], mat, vdir[None], out)
        color[i] = out[0]
    return dict(color=color, shadow_hits=hits, rays=nrays, fragile=frag, range_fragile=rfrag, valid=ok)
