"""Float64 restatement of the indirect traced frame (mgs_render_traced_indirect; include/mgs.h, "reflection and refraction bounces").

Test infrastructure only.  Bounce 0 is np_trace_mesh.frame(lit=True): the light term of wavefrontComputeShading is the direct
function's, so its image, hit counts, shadow hits and fragile mask are bounce 0's.  What is restated here:
  shaders/wavefront.h.slang:335-376                 illum's transmittance and new ray (reflect, refract, total internal reflection)
  shaders/threedgrt_raytrace.rgen.slang:1179-1219   the light loop's state rule: a pixel bounces when a light shaded its mesh point
  shaders/threedgrt_raytrace.rgen.slang:230-337     the bounce loop, b up to max_bounces inclusive
  shaders/threedgrt_raytrace.rgen.slang:505-573     the bounce ray's closest mesh hit (np_mesh_rays.trace), the iso surface's reset
  shaders/threedgrt_raytrace.rgen.slang:615-763     the pass walk with carried radiance, double3 T and hit count (walk_ray)
  shaders/threedgrt_raytrace.rgen.slang:1037-1062   evaluateLightingAndShadingForBounce: the splat surface on radiance -
                                                    radianceBeforeParticles with the raw integrated normal, then the mesh
Shadow rays and shading are np_trace_mesh's (its _occluded, _light_vec) and np_trace_lit's (shadow_ray, _shade64, _eval).

Fragile pixels: a pixel is fragile when any bounce of its path is, and stays so.  Per bounce b, with u = 2^-24 and the ray origin's
error d_o = 16 u |origin|_1 + m_t of the hit that made it (np_trace_mesh's mesh point rule), grown by 8 u |origin|_1 per earlier bounce:
  * np_mesh_rays' mask of the closest hit, and the hit asked again with t_min moved in and out by m_e = 64 (d_o + 8 u |origin|_1) (a
    bounce hit with t near tMin: the neighbouring face at a box's edge): a different primitive is fragile.
  * the walk's margins as np_trace_rays has them (window ends with the upper end's own m_t, proxy and response thresholds, order),
    every candidate's d_oc widened by d_o as np_trace_lit does for a shadow ray; T against min_transmittance (the max channel) and
    the iso threshold (the x channel) with the carried relative uncertainty of T.
  * t_iso against t_mesh, T against min_mesh_composite_transmittance, light ranges, the shadow rays: np_trace_mesh's rules.
  * dot(rayDir, worldNrm) against 0 for a refractive material: |dot| <= 64 u (1 + b).
  * the refraction discriminant k against 0: |k| <= 64 u (1 + b) max(1, eta^2).
"""
import numpy as np

import np_lighting as nl
import np_mesh_rays as nr
import np_reference as npr
import np_trace_lit as ntl
import np_trace_mesh as ntm
from np_trace import EPS_T, INVALID, T_MAX, T_MIN, U, _normal_world, response


def illum_of(bounce_materials, inst, mat):
    bm = bounce_materials[inst] if inst < len(bounce_materials) and bounce_materials[inst] else []
    return bm[mat] if mat < len(bm) else dict(transmittance=(0.0, 0.0, 0.0), ior=1.0, illum=0)


def next_ray(d, nrm, mm, bm, T, b):
    """wavefrontComputeShading:335-376 -> (T', direction or None, fragile)"""
    f64 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    illum = int(bm["illum"])
    if illum <= 0:
        return np.zeros(3), None, False
    dn = float(d @ nrm)
    if illum == 1:
        return T * f64(mm["specular"]), d - 2.0 * dn * nrm, False
    ior = float(np.float32(bm["ior"]))
    frag = abs(dn) <= 64.0 * U * (1 + b)
    eta, N = 1.0 / ior, nrm
    if dn > 0.0:
        eta, N = ior, -nrm
    ni = float(N @ d)
    k = 1.0 - eta * eta * (1.0 - ni * ni)
    frag = frag or abs(k) <= 64.0 * U * (1 + b) * max(1.0, eta * eta)
    r = np.zeros(3) if k < 0.0 else eta * d - (eta * ni + np.sqrt(k)) * N
    rl = np.linalg.norm(r)
    nd = r / rl if rl > 0.0 else d - 2.0 * ni * N
    return T * f64(bm["transmittance"]), nd, bool(frag)


def is_tir(d, nrm, bm):
    """the refractive material's ray takes the total-internal-reflection fallback (wavefront.h.slang:370-374)"""
    if int(bm["illum"]) < 2:
        return False
    ior = float(np.float32(bm["ior"]))
    dn = float(d @ nrm)
    eta, ni = (ior, -dn) if dn > 0.0 else (1.0 / ior, dn)
    return 1.0 - eta * eta * (1.0 - ni * ni) < 0.0


def walk_ray(per_inst, o, d, t_hi, m_t, T, relT, rad, d_o, K, max_passes, minT, isoT, degree, kmr, acull, aclamp, sh_degree, thin, normal_method,
             sh_only=False, no_gauss=False):
    """traceRayParticlesInsertionSort on one ray in (T_MIN + EPS_T, t_hi + EPS_T) with carried T [3], relT and radiance [3].
    Returns dict(T, relT, rad, hits, t_iso, pick, pick_dt, normal [3], fragile)."""
    T, rad = np.array(T, np.float64), np.array(rad, np.float64)
    t_hi = min(t_hi, T_MAX)
    cand, fr = [], False
    for k, pi in enumerate(per_inst):
        if not pi["alive"].any():
            continue
        e = ntl._eval(pi, o, d, degree, d_o)
        th = pi["thr"][e["idx"]]
        t, d_t = e["t"], e["d_t"]
        is_c = (t > T_MIN + EPS_T) & (t < t_hi + EPS_T) & (e["r_mid"] > th)
        maybe = ((t + d_t > T_MIN) & (t - d_t - m_t < t_hi + EPS_T) & (e["r_hi"] > th)
                 & ~((t - d_t > T_MIN + EPS_T) & (t + d_t + m_t < t_hi) & (e["r_lo"] > th)))
        fr |= bool(maybe.any())
        dens = pi["dens"][e["idx"]]
        for lim in (np.full_like(th, kmr), acull / dens):
            fr |= bool((is_c & (e["r_lo"] <= lim) & (e["r_hi"] >= lim)).any())
        dm = pi["Ri"] @ d
        for j in np.nonzero(is_c)[0]:
            cand.append((t[j], pi["base"] + e["idx"][j], k, e["idx"][j], e["dist"][j], e["d_d"][j], d_t[j], e["om"], dm))
    cand.sort(key=lambda c: (c[0], c[1]))
    for i in range(len(cand) - 1):
        a, b = cand[i], cand[i + 1]
        same = a[2] == b[2] and per_inst[a[2]]["ps"]["shape"][a[3]] == per_inst[a[2]]["ps"]["shape"][b[3]]
        if b[0] - a[0] <= a[6] + b[6] and not same:
            fr = True
    st = dict(hits=0, t_iso=0.0, pick=INVALID, pick_dt=0.0, n=np.zeros(3))

    def near(Tv, lim):
        return abs(Tv - lim) <= Tv * (relT + 4.0 * U)

    def accept(e):
        nonlocal T, relT, rad, fr
        tt, gid, k, li, dist, d_d, d_t, om, dm = e
        pi = per_inst[k]
        ps, den = pi["ps"], pi["dens"][li]
        resp = float(response(degree, dist))
        alpha = min(aclamp, resp * den)
        if not (alpha > acull and resp > kmr):
            return
        a_hi = min(aclamp, float(response(degree, dist - d_d)) * den * (1 + 16 * U))
        a_lo = min(aclamp, float(response(degree, dist + d_d)) * den * (1 - 16 * U))
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
        T = T * (1.0 - alpha)
        relT += (a_hi - a_lo) / max(1.0 - alpha, 1e-30) + 4.0 * U
        st["hits"] += 1
        nw, n_frag = _normal_world(ps, li, om, dm, pi["Ri"], thin, normal_method, d_d)
        fr = fr or n_frag
        st["n"] = st["n"] + nw * w
        if st["t_iso"] == 0.0:
            if near(T[0], isoT):
                fr = True
            if T[0] < isoT:
                st["t_iso"], st["pick"], st["pick_dt"] = tt, gid, d_t

    tmin, rest = T_MIN, cand
    for _ in range(max_passes):
        if near(T.max(), minT):
            fr = True
        if not (tmin <= t_hi and T.max() > minT):
            break
        rest = [e for e in rest if e[0] > tmin + EPS_T]
        if not rest:
            break
        for e in rest[:K]:
            if near(T.max(), minT):
                fr = True
            if T.max() > minT:
                accept(e)
                tmin = max(tmin, e[0])
    return dict(T=T, relT=relT, rad=rad, hits=st["hits"], t_iso=st["t_iso"], pick=st["pick"], pick_dt=st["pick_dt"], normal=st["n"], fragile=fr)


def frame(instances, meshes, mesh_materials, bounce_materials, V, P, W, H, camera_pos=None, lights=None, materials=None, max_bounces=3,
          mesh_min_T=0.0, shadows=1, offset=0.2, threshold=0.8, strength=0.0, **kw):
    """The indirect frame.  bounce_materials: per mesh instance a list of dict(transmittance, ior, illum) indexed by material id (or
    None / shorter: illum 0).  Everything else as np_trace_mesh.frame(lit=True).  Returns its dict with image, hits, shadow_hits and
    fragile over all bounces, plus rays [max_bounces] / mesh_hits [max_bounces] (non-fragile counts are exact), live [max_bounces,H,W],
    particle_hits, first: np_trace_mesh's frame (bounce 0)."""
    f32 = lambda v: float(np.float32(v))
    f64 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    first = ntm.frame(instances, meshes, mesh_materials, V, P, W, H, camera_pos, lights, materials, lit=True, mesh_min_T=mesh_min_T, shadows=shadows,
                      offset=offset, threshold=threshold, strength=strength, **kw)
    img, hits, sh_hits, fragile = first["image"].copy(), first["hits"].copy(), first["shadow_hits"].copy(), first["fragile"].copy()
    O, D, OK = first["base"]["rays"]
    mesh = first["mesh"]
    lights = list(lights or [])
    cam = None if camera_pos is None else f64(camera_pos)
    minTm, minT, isoT = f32(mesh_min_T), f32(kw.get("min_transmittance", 0.01)), f32(kw.get("depth_iso_threshold", 0.7))
    kmr, acull, aclamp = f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99))
    degree, K = kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18)
    offset, threshold, strength = f32(offset), f32(threshold), f32(strength)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    any_mesh = any(m.get("visible", True) for m in meshes)
    have_particles = any(pi["alive"].any() for pi in per_inst)

    def shade(mat, pos, nrm, vdir, d_o, out, key):
        """the loop over the lights (np_trace_mesh.frame's shade): returns whether a light shaded the point"""
        y, x = key
        if not lights:
            nl._shade_direct(nl.headlight(cam), pos[None], nrm[None], mat, vdir[None], out, np.float64, False)
            return True
        shaded = False
        for L in lights:
            ldir, ldist, rng = ntm._light_vec(L, pos)
            if rng is not None:
                lp = f64(L["position"])
                if abs(ldist - rng) <= d_o + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum()):
                    fragile[y, x] = True
                if ldist > rng:
                    continue
            shaded = True
            res = np.ones(3)
            if shadows:
                occ, ofr = ntm._occluded(meshes, pos[None], ldir[None], np.array([ldist]), np.array([d_o])) if any_mesh else (np.zeros(1, bool), np.zeros(1, bool))
                fragile[y, x] |= bool(ofr[0])
                if occ[0]:
                    res = np.zeros(3)
                elif have_particles:
                    res, h, sfr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull, aclamp,
                                                 kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
                    sh_hits[y, x] += h
                    fragile[y, x] |= bool(sfr)
            if shadows and res.max() < 0.001:
                out += mat["ambient"]
            else:
                ntl._shade64(dict(L, color=f64(L["color"]) * res), pos[None], nrm[None], mat, vdir[None], out)
        return shaded

    def in_range_any(pos):
        if not lights:
            return True
        return any(rng is None or ldist <= rng for _, ldist, rng in (ntm._light_vec(L, pos) for L in lights))

    # ---- bounce 0: what wavefrontComputeShading leaves of T and the ray at every shaded mesh point ----
    state = {}   # (y, x) -> dict(o, d, T, relT, rad, d_o)
    for y in range(H):
        for x in range(W):
            if not OK[y, x] or not first["composited"][y, x]:
                continue
            inst, mat = int(mesh["inst"][y, x]), int(mesh["mat"][y, x])
            mm = mesh_materials[inst][mat]
            pos, nrm = mesh["pos"][y, x], mesh["nrm"][y, x]
            if not nl.need_shading(mm) or not in_range_any(pos):
                continue
            T0 = first["T"][y, x] if first["splat_lit"][y, x] else 1.0
            relT0 = first["base"]["relT"][y, x] if first["splat_lit"][y, x] else 0.0
            Tn, nd, fr = next_ray(D[y, x], nrm, mm, illum_of(bounce_materials, inst, mat), np.full(3, float(np.float32(T0))), 0)
            fragile[y, x] |= fr
            if nd is None:
                continue
            m_t = 32.0 * U * (np.abs(O[y, x]).sum() + mesh["t"][y, x])
            state[(y, x)] = dict(o=pos, d=nd, T=Tn, relT=relT0 + 4.0 * U, rad=img[y, x, :3].copy(), d_o=16.0 * U * np.abs(pos).sum() + m_t)

    n_rays, n_mesh = np.zeros(max_bounces, np.int64), np.zeros(max_bounces, np.int64)
    live = np.zeros((max_bounces, H, W), bool)
    tir = np.zeros((H, W), bool)   # a bounce of the pixel's path took the total-internal-reflection fallback
    particle_hits = 0
    for b in range(1, max_bounces + 1):
        if not state:
            break
        keys = list(state.keys())
        Ob, Db = np.array([state[k]["o"] for k in keys]), np.array([state[k]["d"] for k in keys])
        do = np.array([state[k]["d_o"] for k in keys])
        m_e = 64.0 * (do + 8.0 * U * np.abs(Ob).sum(-1))
        n = len(keys)
        ans = [nr.trace(meshes, Ob, Db, np.maximum(0.001 + s * m_e, 0.0), np.full(n, 10000.0)) for s in (0.0, -1.0, 1.0)]
        mr = ans[0]
        nxt = {}
        for i, key in enumerate(keys):
            y, x = key
            s = state[key]
            live[b - 1, y, x] = True
            n_rays[b - 1] += 1
            o, d = s["o"], s["d"]
            hit, t_mesh = bool(mr["hit"][i]), float(mr["t"][i]) if mr["hit"][i] else np.inf
            fragile[y, x] |= bool(mr["fragile"][i])
            for other in ans[1:]:
                if bool(other["hit"][i]) != hit or (hit and int(other["prim"][i]) != int(mr["prim"][i])):
                    fragile[y, x] = True
            n_mesh[b - 1] += int(hit)
            m_t = 32.0 * U * (np.abs(o).sum() + t_mesh) if hit else 0.0
            before = s["rad"].copy()
            if have_particles:
                w = walk_ray(per_inst, o, d, t_mesh, m_t, s["T"], s["relT"], s["rad"], s["d_o"], K, kw.get("max_passes", 200), minT, isoT, degree, kmr,
                             acull, aclamp, kw.get("sh_degree", 3), kw.get("thin", 1e-6), kw.get("normal_method", 0), kw.get("sh_only", False),
                             kw.get("no_gauss", False))
            else:
                w = dict(T=s["T"], relT=s["relT"], rad=s["rad"], hits=0, t_iso=0.0, pick=INVALID, pick_dt=0.0, normal=np.zeros(3), fragile=False)
            fragile[y, x] |= bool(w["fragile"])
            hits[y, x] += w["hits"]
            particle_hits += w["hits"]
            T, relT, rad = w["T"], w["relT"], w["rad"]
            t_iso, pick = w["t_iso"], w["pick"]
            if pick != INVALID and hit and abs(t_iso - t_mesh) <= w["pick_dt"] + m_t:
                fragile[y, x] = True
            if pick != INVALID and t_iso > 0.0 and t_iso < t_mesh:
                k = int(np.searchsorted(prefix, pick, side="right") - 1)
                m = materials[k]
                delta = rad - before
                out = (delta * f64(m["emission"]))[None].copy()
                if nl.need_shading(m):
                    mat = dict(ambient=(delta * f64(m["ambient"]))[None], diffuse=(delta * f64(m["diffuse"]))[None], specular=(delta * f64(m["specular"]))[None],
                               shininess=np.array([f32(m["shininess"])]))
                    pos = o + t_iso * d
                    shade(mat, pos, w["normal"], d, s["d_o"] + w["pick_dt"] + 8.0 * U * (np.abs(o).sum() + t_iso + np.abs(pos).sum() + offset), out, key)
                rad = out[0] + before
            if hit:
                if abs(T.max() - minTm) <= T.max() * (relT + 4.0 * U):
                    fragile[y, x] = True
                if T.max() > minTm:
                    inst, mat_id = int(mr["inst"][i]), int(mr["mat"][i])
                    mm = mesh_materials[inst][mat_id]
                    rad = rad + f64(mm["emission"])
                    if nl.need_shading(mm):
                        mat = dict(ambient=(T * f64(mm["ambient"]))[None], diffuse=(T * f64(mm["diffuse"]))[None], specular=(T * f64(mm["specular"]))[None],
                                   shininess=np.array([f32(mm["shininess"])]))
                        pos, nrm = mr["pos"][i], mr["nrm"][i]
                        d_o = s["d_o"] + 16.0 * U * np.abs(pos).sum() + m_t
                        out = rad[None].copy()
                        if shade(mat, pos, nrm, d, d_o, out, key):
                            tir[y, x] |= is_tir(d, nrm, illum_of(bounce_materials, inst, mat_id))
                            Tn, nd, fr = next_ray(d, nrm, mm, illum_of(bounce_materials, inst, mat_id), T, b)
                            fragile[y, x] |= fr
                            if nd is not None:
                                nxt[key] = dict(o=pos, d=nd, T=Tn, relT=relT + 4.0 * U, rad=out[0].copy(), d_o=d_o)
                        rad = out[0]
            img[y, x, :3] = rad
        state = nxt
    return dict(first, image=img, hits=hits, shadow_hits=sh_hits, fragile=fragile, rays=n_rays, mesh_hits=n_mesh, live=live,
                particle_hits=particle_hits, first=first, tir=tir)
