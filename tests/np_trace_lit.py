"""Float64 restatement of a lit traced frame (mgs_render_traced_lit): np_trace.trace for the primary rays, then
  shaders/threedgrt_raytrace.rgen.slang:991-1009    surfaceFinalFiltering
  shaders/threedgrt_raytrace.rgen.slang:1082-1144   evaluateLightingAndShadingParticles
  shaders/threedgrt_raytrace.rgen.slang:1344-1464   traceShadowRayParticle (hard shadows; no mesh in the scene)
  shaders/wavefront.h.slang:33-70,233-280,388-403   computeLightToSurfaceVector, wavefrontComputeShadingDirectOnly
Test infrastructure only.  Shadow rays are evaluated by brute force over all particles with an arbitrary origin and direction; the
shading is np_lighting._shade_direct (the function the raster passes are tested against) with the light's colour multiplied by the
shadow's transmittance, and the inShadow return restated here.

Fragile pixels extend np_trace's (module docstring there; u = 2^-24, d_oc / d_d / d_t as derived there):
  * the shadow origin: position + lightDir * offset.  The primary ray's picked t carries the picked hit's own d_t; origin + t * d, the
    light vector and the offset add 8 u of the magnitudes summed.  d_o = d_t(pick) + 8 u (|o|_1 + t + |pos|_1 + offset) is a WORLD
    length; through the instance's inverse transform it moves the model-space origin by at most |M^-1|_2 d_o, which is added to
    every candidate's d_oc before d_d and d_t are formed as in np_trace.  (The direction's own error, <= 8 u relative, is inside
    np_trace's 16 u |oc| term.)
  * candidate existence: the proxy threshold between the response at d - d_d and at d + d_d, or t within d_t of 0 or within
    d_t + d_o + 4 u lightDist of TMax = lightDist - 0.001 (lightDist itself moves with the origin).  The walk's dist >= lightDist
    test lies 0.001 beyond TMax and is decided with it; for a directional light both are 1e10 in fp32.
  * order: two neighbours among the first K + 1 candidates whose t differ by no more than the sum of their d_t (this is the order
    around the K-th slot and inside the walk); bit-identical particles of one instance are exempt as in np_trace.
  * the walk's thresholds on the response (kernel_min_response, alpha_cull / density) between the two responses.
  * T against the shadow threshold after each slot, and the final max component against 0.001: T carries the relative uncertainty
    np_trace accumulates per accepted hit ((alpha_hi - alpha_lo) / (1 - alpha) + 4 u); the ramp divides it by (1 - threshold).
  * the normal's length against 0.2: the integrated normal is sum(w_i n_i) with unit normals n_i, so its error is at most
    sum(w_i) times the largest relative error of a weight plus that of a normal.  A weight alpha_i T_i carries the relative
    uncertainty np_trace accumulates for T (per hit (alpha_hi - alpha_lo) / (1 - alpha) + 4 u, a few 1e-6 for the responses and
    margins of these scenes, below 1e-5 after the at most 36 hits a ray accepts before T < 0.01), a normal 64 u.  The margin used is
    1e-4 * sum(w_i) + 64 u: ten times that.  test_trace_lit_cpu.py asserts that the case built for the fallback keeps every pixel's
    length at least ten margins (a hundred times the estimate) away from 0.2, so the decision there does not rest on the margin's size.
  * a light's range: |dist - range| <= d_o + 8 u (|pos|_1 + |light|_1).
"""
import numpy as np

import np_lighting as nl
import np_reference as npr
from np_trace import INVALID, U, prepare_set, rays, response, trace, _normal_world  # noqa: F401  (re-exported for the cases)


def _per_inst(instances, kmr, acull, adaptive):
    out, base = [], 0
    for ps, M in instances:
        M = np.asarray(M, np.float64)
        Mi, Ri = np.linalg.inv(M), np.linalg.inv(M[:3, :3])
        dens = ps["rgba"][:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = np.minimum(kmr / dens if adaptive else np.full_like(dens, kmr), 0.97)
        alive = (dens > acull) & np.isfinite(ps["s"]).all(1) & np.isfinite(ps["pos"]).all(1) & np.isfinite(ps["R"]).all((1, 2))
        out.append(dict(ps=ps, Mi=Mi, Ri=Ri, dens=dens, thr=thr, alive=alive, base=base, mnorm=np.linalg.norm(Mi[:3, :3], 2)))
        base += ps["n"]
    return out


def _eval(pi, o, d, degree, d_o=0.0):
    """every live particle of one instance against one world ray: dict of arrays (np_trace's formulas and margins)"""
    ps = pi["ps"]
    idx = np.nonzero(pi["alive"])[0]
    pos, s, R = ps["pos"][idx], ps["s"][idx], ps["R"][idx]
    om = pi["Mi"][:3, :3] @ o + pi["Mi"][:3, 3]
    dm = pi["Ri"] @ d
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


def shadow_ray(per_inst, o, d, light_dist, K, threshold, strength, d_o=0.0, kernel_degree=2, kmr=0.0113, acull=1.0 / 255.0,
               aclamp=0.99, sh_degree=3, no_gauss=False, sh_only=False):
    """traceShadowRayParticle from origin o (the offset already applied) along d.  Returns (transmittance[3], accepted hits, fragile)."""
    tmax = float(np.float32(np.float32(light_dist) - np.float32(0.001)))
    cand, frag = [], False
    for k, pi in enumerate(per_inst):
        if not pi["alive"].any():
            continue
        e = _eval(pi, o, d, kernel_degree, d_o)
        th = pi["thr"][e["idx"]]
        t, d_t = e["t"], e["d_t"]
        m_hi = d_t + d_o + 4.0 * U * tmax
        is_c = (t > 0.0) & (t < tmax) & (e["r_mid"] > th)
        maybe = (t + d_t > 0.0) & (t - m_hi < tmax) & (e["r_hi"] > th) & ~((t - d_t > 0.0) & (t + m_hi < tmax) & (e["r_lo"] > th))
        frag |= bool(maybe.any())
        dens = pi["dens"][e["idx"]]
        for lim in (np.full_like(th, kmr), acull / dens):
            frag |= bool((is_c & (e["r_lo"] <= lim) & (e["r_hi"] >= lim)).any())
        for b in np.nonzero(is_c)[0]:
            cand.append((t[b], pi["base"] + e["idx"][b], k, e["idx"][b], e["dist"][b], e["d_d"][b], d_t[b], e["om"]))
    cand.sort(key=lambda c: (c[0], c[1]))
    for i in range(min(len(cand) - 1, K)):
        a, b = cand[i], cand[i + 1]
        same = a[2] == b[2] and per_inst[a[2]]["ps"]["shape"][a[3]] == per_inst[a[2]]["ps"]["shape"][b[3]]
        if b[0] - a[0] <= a[6] + b[6] and not same:
            frag = True
    T, relT, rad, hits = 1.0, 0.0, np.zeros(3), 0
    for tt, gid, k, li, dist, d_d, d_t, om in cand[:K]:
        if tt >= light_dist:
            continue
        pi = per_inst[k]
        ps, den = pi["ps"], pi["dens"][li]
        resp = float(response(kernel_degree, dist))
        alpha = min(aclamp, resp * den)
        if alpha > acull and resp > kmr:
            a_hi = min(aclamp, float(response(kernel_degree, dist - d_d)) * den * (1 + 16 * U))
            a_lo = min(aclamp, float(response(kernel_degree, dist + d_d)) * den * (1 - 16 * U))
            if no_gauss:
                alpha = a_hi = a_lo = 1.0
            if strength != 0.0:
                v = ps["pos"][li] - om
                v = v / np.linalg.norm(v)
                col = np.full(3, 0.5) if sh_only else ps["rgba"][li, :3].copy()
                deg = min(ps["degree"], sh_degree)
                if deg > 0:
                    col = col + npr.sh_radiance(ps["sh"][li:li + 1], deg, v[None])[0]
                rad += col * (alpha * T)
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


def lit(instances, V, P, W, H, camera_pos, lights, materials, shadows=1, offset=0.2, threshold=0.8, strength=0.0, deferred_inputs=False, **kw):
    """instances / kw as np_trace.trace; lights: np_lighting light dicts (empty: the headlight); materials: one dict per instance.
    Returns dict(image [H,W,4], shadow_hits [H,W], shadow_T [H,W,lights,3], fragile [H,W], surface [H,W] (a lit or discarded-to-
    emission pixel with an iso hit), rays [H,W] (shadow rays the pixel traces), fallback [H,W] (the -rayDirection normal was used),
    base: np_trace's result).
    deferred_inputs: shade from the traced outputs AS THE DEFERRED RASTER PASS READS THEM (np_lighting.light_frame: radiance and
    normal rounded to fp32, the position rebuilt from the fp32 ndc depth through the fp32-rounded inverse matrices, the view
    direction normalize(position - camera)) instead of origin + t * direction and the ray's direction.  Everything after these four
    inputs (material, emission, the loop over the lights, the range rule) is the same code; the self check against light_frame uses it."""
    base = trace(instances, V, P, W, H, **kw)
    f32 = lambda v: float(np.float32(v))
    kmr, acull, aclamp = f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99))
    degree, K = kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18)
    offset, threshold, strength = f32(offset), f32(threshold), f32(strength)
    per_inst = _per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    O, D, OK = rays(np.asarray(V, np.float64), np.asarray(P, np.float64), W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    img = np.zeros((H, W, 4))
    sh_hits = np.zeros((H, W), np.int64)
    sh_T = np.ones((H, W, max(len(lights), 1), 3))
    fragile = base["fragile"].copy()
    surface = np.zeros((H, W), bool)
    nrays = np.zeros((H, W), np.int64)
    fallback = np.zeros((H, W), bool)
    cam = np.asarray(camera_pos, np.float32).astype(np.float64)
    y0, y1 = kw.get("rows") or (0, H)
    for y in range(y0, y1):
        for x in range(W):
            if not OK[y, x]:
                img[y, x] = (0, 0, 0, 1)
                continue
            pick = int(base["id"][y, x])
            if pick == INVALID:
                continue  # discarded: (0,0,0,0)
            surface[y, x] = True
            o, d = O[y, x], D[y, x]
            k = int(np.searchsorted(prefix, pick, side="right") - 1)
            e = _eval(per_inst[k], o, d, degree)
            j = int(np.nonzero(e["idx"] == pick - per_inst[k]["base"])[0][0])
            t_iso, pick_dt = e["t"][j], e["d_t"][j]
            n4 = base["normal"][y, x]
            nlen = np.linalg.norm(n4[:3])
            if abs(nlen - 0.2) <= 1e-4 * n4[3] + 64.0 * U:
                fragile[y, x] = True
            n = -d if nlen <= 0.2 else n4[:3]
            fallback[y, x] = nlen <= 0.2
            n = n / np.linalg.norm(n)
            pos = o + t_iso * d
            rad0 = base["image"][y, x, :3]
            vdir = d
            if deferred_inputs:
                rad0 = rad0.astype(np.float32).astype(np.float64)
                n = n4[:3].astype(np.float32).astype(np.float64)
                n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
                clip = np.array([(x + 0.5) / W * 2.0 - 1.0, (y + 0.5) / H * 2.0 - 1.0, float(np.float32(base["depth"][y, x])), 1.0])
                vp = nl.inverse_f32(P).astype(np.float64) @ clip
                pos = (nl.inverse_f32(V).astype(np.float64) @ (vp / vp[3]))[:3]
                vdir = (pos - cam) / np.linalg.norm(pos - cam)
            m = materials[k]
            mv = lambda key: np.asarray(m[key], np.float32).astype(np.float64)
            color = rad0 * mv("emission")
            img[y, x, 3] = base["image"][y, x, 3]
            if not nl.need_shading(m):
                img[y, x, :3] = color
                continue
            mat = dict(ambient=(rad0 * mv("ambient"))[None], diffuse=(rad0 * mv("diffuse"))[None], specular=(rad0 * mv("specular"))[None],
                       shininess=np.array([f32(m["shininess"])]))
            out = color[None].copy()
            d_o = pick_dt + 8.0 * U * (np.abs(o).sum() + t_iso + np.abs(pos).sum() + offset)
            if not lights:
                nl._shade_direct(nl.headlight(cam), pos[None], n[None], mat, vdir[None], out, np.float64, False)
            for li, L in enumerate(lights):
                if int(L["type"]) == nl.LIGHT_DIRECTIONAL:
                    dirn = np.asarray(L["direction"], np.float32).astype(np.float64)
                    ldir, ldist = -dirn / np.linalg.norm(dirn), 1e10
                else:
                    lp = np.asarray(L["position"], np.float32).astype(np.float64)
                    to = lp - pos
                    ldist = np.linalg.norm(to)
                    rng = f32(L["range"])
                    if abs(ldist - rng) <= d_o + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum()):
                        fragile[y, x] = True
                    if ldist > rng:
                        continue  # skipped entirely: no ambient either
                    ldir = to / ldist
                Ls = dict(L, color=np.asarray(L["color"], np.float32).astype(np.float64))
                in_shadow = False
                if shadows:
                    nrays[y, x] += 1
                    res, hits, fr = shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull, aclamp,
                                               kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
                    sh_hits[y, x] += hits
                    sh_T[y, x, li] = res
                    fragile[y, x] |= fr
                    Ls["color"] = np.asarray(L["color"], np.float32).astype(np.float64) * res
                    in_shadow = res.max() < 0.001
                if in_shadow:
                    out += mat["ambient"]
                else:
                    _shade64(Ls, pos[None], n[None], mat, vdir[None], out)
            img[y, x, :3] = out[0]
    return dict(image=img, shadow_hits=sh_hits, shadow_T=sh_T, fragile=fragile, surface=surface, rays=nrays, fallback=fallback, base=base)


def _shade64(light, pos, n, mat, view_dir, radiance):
    """np_lighting._shade_direct with a light colour that is not rounded to fp32 (the shadow's factor is applied in fp32 on the
    device, whose rounding is within the image tolerance; rounding the product here would only add a second one)"""
    L = dict(light)
    col = np.asarray(light["color"], np.float64)
    # _shade_direct reads light["color"] through np.asarray(..., np.float32); the light's terms are linear in the colour per
    # channel (radiance gains ambient + (diffuse + specular) * colour), so evaluate unit colours and scale
    zero = dict(L, color=(0.0, 0.0, 0.0))
    amb_only = radiance.copy()
    nl._shade_direct(zero, pos, n, mat, view_dir, amb_only, np.float64, False)
    one = np.zeros_like(radiance)
    for c in range(3):
        unit = [0.0, 0.0, 0.0]
        unit[c] = 1.0
        r = radiance.copy()
        nl._shade_direct(dict(L, color=tuple(unit)), pos, n, mat, view_dir, r, np.float64, False)
        one[:, c] = (r - amb_only)[:, c]
    radiance[:] = amb_only + one * col[None]
