"""Float64 restatement of the traced frames with mesh hits (mgs_frame_set_trace_meshes; include/mgs.h, "mesh hits in the traced frames").

Test infrastructure only.  np_mesh_rays.trace answers every mesh ray (primary: closest, window (0.001, 10000); occlusion: window
(0.001, lightDist - 0.001) from the un-offset origin).  walk() is np_trace.trace with ONE change, a per-pixel upper end: the copy exists
because np_trace.py is not edited, and test_trace_mesh_cpu.py holds it equal to np_trace.trace (no meshes) and, through frame(), to
np_trace_lit.lit.  frame() then restates
  shaders/threedgrt_raytrace.rgen.slang:495-553     the mesh hit is the upper end of the particle walk
  shaders/threedgrt_raytrace.rgen.slang:1037-1077   splatIsClosest, the composite condition, the unlit composite
  shaders/threedgrt_raytrace.rgen.slang:1148-1165,1222-1255   evaluateLightingAndShadingMeshes, direct mode
  shaders/threedgrt_raytrace.rgen.slang:1262-1341   traceShadowRayForLight: meshes first, then the particles
  shaders/threedgrt_raytrace.rgen.slang:1490-1502   depth of the primary hit
with np_trace_lit.shadow_ray and _shade64 for the particle shadow ray and the shading.

Fragile pixels: the union of np_trace's (the walk), np_trace_lit's (the shadow rays and the splat surface) and np_mesh_rays's (the
primary mesh ray and every occlusion ray), plus, with u = 2^-24:
  * t_mesh's own fp32 error: m_t = 32 u (|o|_1 + t_mesh): the sheared vertices carry 2 u of |vertex - origin|_1 each, the three edge
    functions and T / det a few u more (test_mesh_rays_cpu.py measures t at a few 1e-7 relative on its cases; 32 u = 1.9e-6).
  * a particle candidate against the upper end: np_trace's window rule with the upper end t_mesh and the candidate's d_t widened by m_t
    (inside walk(): the `maybe` mask and the pass loop use the pixel's end).
  * t_iso against t_mesh (splatIsClosest): |t_iso - t_mesh| <= d_t(pick) + m_t.
  * T against min_mesh_composite_transmittance: np_trace's relative uncertainty of T, |T - lim| <= T (relT + 4 u).
  * a mesh occlusion candidate near either window end, the hit triangle itself near t = 0 included: the ray's origin carries d_o (the
    splat surface: np_trace_lit's d_o; a mesh point: 16 u |pos|_1 + m_t), a length that moves every t along the ray by at most d_o
    over the cosine to the triangle; the occlusion is therefore asked three times, with both ends moved in and out by
    m_e = 64 (d_o + 8 u (|pos|_1 + min(lightDist, |light|_1 + |pos|_1))) (64 covers grazing angles down to 1 / 64), and a pixel whose
    three answers differ is fragile.
  * a light's range at the mesh point: |dist - range| <= d_o + 8 u (|pos|_1 + |light|_1), np_trace_lit's rule with the mesh point's d_o.
"""
import numpy as np

import np_lighting as nl
import np_mesh_rays as nr
import np_reference as npr
import np_trace_lit as ntl
from np_trace import EPS_T, INVALID, T_MAX, T_MIN, U, _normal_world, rays, response


def walk(instances, V, P, W, H, tmax=None, samples_per_pass=18, max_passes=200, min_transmittance=0.01, adaptive_clamping=True,
          depth_iso_threshold=0.7, kernel_degree=2, kernel_min_response=0.0113, alpha_clamp=0.99, alpha_cull=1.0 / 255.0, sh_degree=3,
          fisheye=False, fov_rad=None, dof=None, thin=1e-6, rows=None, sh_only=False, no_gauss=False, single_sorted_walk=False, normal_method=0,
          reverse_ties=False, exact_ties=()):
    """np_trace.trace with a per-pixel upper end: tmax [H,W] (the pixel's t_mesh; inf or None = the frame's 10000) replaces T_MAX in
    the candidates' window, its fragile rule (a candidate's d_t widened by the mesh t's own m_t) and the pass loop.  Returns np_trace's
    dict plus T [H,W], relT [H,W] (the walk's transmittance and its relative uncertainty) and pick_dt [H,W].
    instances: [(prepared set, M 4x4 math)] in creation order.  Returns dict(image [H,W,4], hits [H,W], depth [H,W], id [H,W],
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
    TM = np.full((H, W), T_MAX) if tmax is None else np.minimum(np.asarray(tmax, np.float64), T_MAX)
    MT = np.where(TM < T_MAX, 32.0 * U * (np.abs(O).sum(-1) + TM), 0.0)   # the mesh t's own fp32 error
    Tout, relTout, pick_dt_out = np.ones((H, W)), np.zeros((H, W)), np.zeros((H, W))
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
            tm_row, mt_row = TM[y][:, None], MT[y][:, None]
            inr = (t > T_MIN + EPS_T) & (t < tm_row + EPS_T)
            is_c = inr & (r_mid > th)
            maybe = (((t + d_t > T_MIN) & (t - d_t - mt_row < tm_row + EPS_T)) & (r_hi > th)
                     & ~((t - d_t > T_MIN + EPS_T) & (t + d_t + mt_row < tm_row) & (r_lo > th)))
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
                    if not (tmin <= TM[y, xp] and T > minT):
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
            Tout[y, xp], relTout[y, xp], pick_dt_out[y, xp] = T, relT, pick_dt
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
                tie_pair=tie_pair, T=Tout, relT=relTout, pick_dt=pick_dt_out, rays=(O, D, OK))


def _occluded(meshes, pos, ldir, ldist, d_o):
    """traceShadowRayMesh for n points: (occluded [n] bool, fragile [n] bool); the three windows of the module docstring"""
    n = pos.shape[0]
    if n == 0 or not meshes:
        return np.zeros(n, bool), np.zeros(n, bool)
    far = np.minimum(ldist, 1e10)
    reach = np.where(ldist >= 1e9, 0.0, ldist)
    m_e = 64.0 * (d_o + 8.0 * U * (2.0 * np.abs(pos).sum(-1) + reach))
    ans = []
    for s0, s1 in ((0.0, 0.0), (-1.0, 1.0), (1.0, -1.0)):
        t0 = np.maximum(0.001 + s0 * m_e, 0.0)
        t1 = np.where(ldist >= 1e9, 1e10, far - 0.001 + s1 * m_e)
        r = nr.trace(meshes, pos, ldir, t0, t1)
        ans.append((r["hit"], r["fragile"]))
    occ = ans[0][0]
    frag = ans[0][1] | (ans[1][0] != occ) | (ans[2][0] != occ)
    return occ, frag


def _light_vec(L, pos):
    """computeLightToSurfaceVector: (direction to the light, its distance, range or None)"""
    if int(L["type"]) == nl.LIGHT_DIRECTIONAL:
        dirn = np.asarray(L["direction"], np.float32).astype(np.float64)
        return -dirn / np.linalg.norm(dirn), 1e10, None
    lp = np.asarray(L["position"], np.float32).astype(np.float64)
    to = lp - pos
    ldist = np.linalg.norm(to)
    return to / ldist, ldist, float(np.float32(L["range"]))


def frame(instances, meshes, mesh_materials, V, P, W, H, camera_pos=None, lights=None, materials=None, lit=False, mesh_min_T=0.0, shadows=1,
          offset=0.2, threshold=0.8, strength=0.0, **kw):
    """A traced frame with mesh hits.  meshes: np_mesh_rays mesh dicts; mesh_materials: per mesh a list of material dicts; lit: the
    frame of mgs_render_traced_lit (lights: np_lighting dicts, empty = the headlight; materials: one per splat instance), otherwise
    the unlit frame.  kw as np_trace.trace.
    Returns dict(image, hits, id, depth, depth_tol, fragile, shadow_hits, T, mesh (np_mesh_rays' result reshaped [H,W]), composited
    [H,W], mesh_rays [H,W] / shadow_rays [H,W]: mesh occlusion / particle shadow rays the pixel traces, occluded [H,W]: of them hit,
    range_skipped [H,W]: a light out of range at the mesh point, splat_lit [H,W], base: walk()'s result)."""
    f32 = lambda v: float(np.float32(v))
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    O, D, OK = rays(V, P, W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
    ok = OK.reshape(-1)
    n = int(ok.sum())
    mr = nr.trace(meshes, O.reshape(-1, 3)[ok], D.reshape(-1, 3)[ok], np.full(n, 0.001, np.float32), np.full(n, 10000.0, np.float32))
    mesh = {}
    for k, v in mr.items():
        if np.isscalar(v):
            mesh[k] = v
            continue
        full = np.zeros((W * H,) + v.shape[1:], v.dtype)
        if k == "t":
            full[:] = np.inf
        if k in ("prim", "inst", "mat", "prim2"):
            full[:] = nr.NONE
        full[ok] = v
        mesh[k] = full.reshape((H, W) + v.shape[1:])
    base = walk(instances, V, P, W, H, tmax=mesh["t"], **kw)
    img = base["image"].copy()
    fragile = base["fragile"] | mesh["fragile"]
    depth, depth_tol = base["depth"].copy(), base["depth_tol"].copy()
    sh_hits = np.zeros((H, W), np.int64)
    composited = np.zeros((H, W), bool)
    mesh_rays, shadow_rays, occluded = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    range_skipped, splat_lit = np.zeros((H, W), bool), np.zeros((H, W), bool)
    minT = f32(mesh_min_T)
    kmr, acull, aclamp = f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99))
    degree, K = kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18)
    offset, threshold, strength = f32(offset), f32(threshold), f32(strength)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    cam = None if camera_pos is None else np.asarray(camera_pos, np.float32).astype(np.float64)
    lights = list(lights or [])
    y0, y1 = kw.get("rows") or (0, H)

    def shadow(pos, d_o, L):
        """traceShadowRayForLight at pos for light L -> (transmittance[3], in range, fragile, mesh ray?, occluded?, particle ray?, hits)"""
        ldir, ldist, rng = _light_vec(L, pos)
        fr = False
        if rng is not None:
            lp = np.asarray(L["position"], np.float32).astype(np.float64)
            fr = abs(ldist - rng) <= d_o + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum())
            if ldist > rng:
                return None, False, fr, 0, 0, 0, 0
        if not shadows:
            return np.ones(3), True, fr, 0, 0, 0, 0
        any_mesh = any(m.get("visible", True) for m in meshes)
        occ, ofr = _occluded(meshes, pos[None], ldir[None], np.array([ldist]), np.array([d_o])) if any_mesh else (np.zeros(1, bool), np.zeros(1, bool))
        fr = fr or bool(ofr[0])
        if occ[0]:
            return np.zeros(3), True, fr, int(any_mesh), 1, 0, 0
        if not any(pi["alive"].any() for pi in per_inst):
            return np.ones(3), True, fr, int(any_mesh), 0, 0, 0
        res, hits, sfr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull, aclamp,
                                        kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
        return res, True, fr or sfr, int(any_mesh), 0, 1, hits

    def shade(mat, pos, nrm, vdir, d_o, out, y, x):
        """the loop over the lights of evaluateLightingAndShading{Particles,Meshes}: out[1,3] gains every light's terms"""
        if not lights:
            nl._shade_direct(nl.headlight(cam), pos[None], nrm[None], mat, vdir[None], out, np.float64, False)
        for L in lights:
            res, inrange, fr, mray, occ, pray, hits = shadow(pos, d_o, L)
            fragile[y, x] |= bool(fr)
            if not inrange:
                range_skipped[y, x] = True
                continue
            mesh_rays[y, x] += mray
            occluded[y, x] += occ
            shadow_rays[y, x] += pray
            sh_hits[y, x] += hits
            if shadows and res.max() < 0.001:
                out += mat["ambient"]
            else:
                Ls = dict(L, color=np.asarray(L["color"], np.float32).astype(np.float64) * res)
                ntl._shade64(Ls, pos[None], nrm[None], mat, vdir[None], out)

    for y in range(y0, y1):
        for x in range(W):
            if not OK[y, x]:
                continue
            o, d = O[y, x], D[y, x]
            hit, t_mesh = bool(mesh["hit"][y, x]), mesh["t"][y, x]
            m_t = 32.0 * U * (np.abs(o).sum() + t_mesh) if hit else 0.0
            T, relT = base["T"][y, x], base["relT"][y, x]
            pick = int(base["id"][y, x])
            rgb = img[y, x, :3].copy()
            alpha = img[y, x, 3]
            if lit:
                t_iso = 0.0
                if pick != INVALID:
                    k = int(np.searchsorted(prefix, pick, side="right") - 1)
                    e = ntl._eval(per_inst[k], o, d, degree)
                    j = int(np.nonzero(e["idx"] == pick - per_inst[k]["base"])[0][0])
                    t_iso, pick_dt = e["t"][j], e["d_t"][j]
                    if hit and abs(t_iso - t_mesh) <= pick_dt + m_t:
                        fragile[y, x] = True
                if pick != INVALID and t_iso > 0.0 and t_iso < t_mesh:
                    splat_lit[y, x] = True
                    n4 = base["normal"][y, x]
                    nlen = np.linalg.norm(n4[:3])
                    if abs(nlen - 0.2) <= 1e-4 * n4[3] + 64.0 * U:
                        fragile[y, x] = True
                    nn = -d if nlen <= 0.2 else n4[:3]
                    nn = nn / np.linalg.norm(nn)
                    pos = o + t_iso * d
                    m = materials[k]
                    mv = lambda key: np.asarray(m[key], np.float32).astype(np.float64)
                    out = (rgb * mv("emission"))[None].copy()
                    if nl.need_shading(m):
                        mat = dict(ambient=(rgb * mv("ambient"))[None], diffuse=(rgb * mv("diffuse"))[None], specular=(rgb * mv("specular"))[None],
                                   shininess=np.array([f32(m["shininess"])]))
                        shade(mat, pos, nn, d, pick_dt + 8.0 * U * (np.abs(o).sum() + t_iso + np.abs(pos).sum() + offset), out, y, x)
                    rgb = out[0]
                else:  # surfaceFinalFiltering / not the closest: radiance 0, T = 1
                    rgb, alpha, T, relT = np.zeros(3), 0.0, 1.0, 0.0
            if hit:
                if abs(T - minT) <= T * (relT + 4.0 * U):
                    fragile[y, x] = True
                if T > minT:
                    composited[y, x] = True
                    mm = mesh_materials[int(mesh["inst"][y, x])][int(mesh["mat"][y, x])]
                    mv = lambda key: np.asarray(mm[key], np.float32).astype(np.float64)
                    if not lit:
                        rgb = rgb + T * (mv("emission") + mv("ambient") + mv("diffuse"))
                    else:
                        rgb = rgb + mv("emission")
                        if nl.need_shading(mm):
                            mat = dict(ambient=(T * mv("ambient"))[None], diffuse=(T * mv("diffuse"))[None], specular=(T * mv("specular"))[None],
                                       shininess=np.array([f32(mm["shininess"])]))
                            pos, nrm = mesh["pos"][y, x], mesh["nrm"][y, x]
                            out = rgb[None].copy()
                            shade(mat, pos, nrm, d, 16.0 * U * np.abs(pos).sum() + m_t, out, y, x)
                            rgb = out[0]
                    alpha = 1.0
                if pick == INVALID:
                    def ndc_z(tv):
                        clip = P @ (V @ np.append(o + tv * d, 1.0))
                        return clip[2] / clip[3], clip
                    depth[y, x], clip = ndc_z(t_mesh)
                    dt = m_t + 8.0 * U * (np.abs(o).sum() + t_mesh + np.abs(V[:3, 3]).sum())
                    depth_tol[y, x] = (max(abs(ndc_z(t_mesh + dt)[0] - depth[y, x]), abs(ndc_z(t_mesh - dt)[0] - depth[y, x]))
                                       + 8.0 * U * (np.abs(P[2]) @ np.abs(V @ np.append(o + t_mesh * d, 1.0))) / abs(clip[3]))
            img[y, x] = (rgb[0], rgb[1], rgb[2], alpha)
    return dict(image=img, hits=base["hits"], id=base["id"], depth=depth, depth_tol=depth_tol, fragile=fragile, shadow_hits=sh_hits, T=base["T"],
                mesh=mesh, composited=composited, mesh_rays=mesh_rays, shadow_rays=shadow_rays, occluded=occluded, range_skipped=range_skipped,
                splat_lit=splat_lit, base=base, ok=OK)
