"""Float64 restatement of soft shadows (MGS_SHADOWS_SOFT) in lit traced frames, lit frames with trace meshes and hybrid frames:
np_trace_lit / np_trace_mesh / np_hybrid for everything up to the loop over the lights, then that loop with
  shaders/wavefront.h.slang:33-70     computeLightToSurfaceVector under SHADOWS_MODE == SHADOWS_SOFT
  shaders/wavefront.h.slang:78-92     buildOrthonormalBasis (Frisvad)
  shaders/wavefront.h.slang:95-102    sampleDisk: r first, then theta
  shaders/threedgrt_raytrace.rgen.slang:228   seedRayPass = xxhash32(pixel, frameSampleId)
  shaders/threedgrt_raytrace.rgen.slang:1054,1061   one inout seed for the splat surface's loop and the mesh hit's (mesh_frame)
Test infrastructure only.  Built on np_trace_lit (_per_inst, _eval, shadow_ray, _shade64), np_hybrid (hand_over) and the integer RNG
of np_trace_stochastic (xxhash32, rand).

What is exact and what is not.  The draws are integers: the state after any number of draws and both uniform numbers (23 bits over
2^23) are bit-exact.  theta = fl(fl(2 * 3.14159265) * rand) is ONE fp32 product of two fp32 numbers and is restated with numpy's
fp32 product, so it is exact as well.  Only the disk arithmetic behind them is float64 here against fp32 there.

The sample position's error eps_s (a world length; u = 2^-24):
  * n = normalize(light - pos) carries d_n = 8 u + d_o / dist per component: 8 u for the subtraction, the dot product, the square
    root and the scaling, d_o / dist because the surface position itself is only known to d_o (np_trace_lit's docstring).
  * Frisvad's basis with a = 1 / (1 + n.z): d_a = a^2 d_n.  Every entry is 1 - n.x^2 a, n.x n.y a or a component of n.  Since
    n.x^2 <= 1 - n.z^2 <= 2 (1 + n.z), n.x^2 a <= 2, so n.x^2 d_a <= 2 a d_n and 2 |n.x| a d_n <= 2 a d_n (|n.x| <= 1), plus 4 u for
    the entry's own three operations on values <= 2: an entry moves by at most (4 a + 8) d_n.
  * r = (radius / 2) sqrt(rand): sqrtf and the product are correctly rounded to 1 ulp each, 4 u relative.  cosf / sinf of the exact
    theta: the math library's bound of 2 ulp is 4 u absolute on values <= 1 (this is why the device uses the accurate functions).
  * samplePos = light + r (cos t + sin b): the two products, two sums per component and the final sum add 8 u (|light|_1 + r).
  eps_s = r ((4 a + 8) d_n + 16 u) + 8 u (|light|_1 + r).
eps_s enters exactly where the light's position enters: it is added to d_o for the shadow ray (origin, direction and TMax all move
with the sample: np_trace_lit folds all three into d_o) and to the range margin |lightDist - range| <= d_o + eps_s + 8 u (...).
Fragile pixels in addition to np_trace_lit's:
  * 1 + n.z < 0.01 (a > 100).  The reference switches bases at n.z < -0.9999999, i.e. 1 + n.z < 1e-7, where a = 1e7 multiplies d_n
    ~ 1e-6 to an error of order 10 in a unit vector: no margin holds near that branch.  Below a = 100 the basis moves by at most
    408 d_n ~ 4e-4 relative to the disk, r 408 d_n < 2e-4 world units for the radii of these scenes — the size at which the shadow
    ray's own margins still classify candidates.  The cut also covers "n.z within the margin of -0.9999999" with five decades to
    spare.  It removes a cone of 8 degrees half angle around -z from the light, seen from the surface.
  * the range test with the widened margin above.
A light with radius <= 0 or a directional light takes np_trace_lit's statements in np_trace_lit's order: with all radii 0 the
result equals np_trace_lit.lit bit for bit (test_trace_soft_cpu.py asserts it)."""
import numpy as np

import np_hybrid as nh
import np_mesh_rays as nr
import np_lighting as nl
import np_trace_lit as ntl
from np_trace import INVALID, U, rays, trace
from np_trace_mesh import _occluded, walk
from np_trace_stochastic import rand, xxhash32

F = np.float32
TWO_PI_F32 = F(2.0) * F(3.14159265)
A_CUT = 100.0


def seed_of(x, y, sample_id):
    return xxhash32(int(x), int(y), int(sample_id))


def skip_draws(seed, lights, radii):
    """the state after one whole loop over the lights: two draws per point or spot light with a radius, culled or not"""
    for L, R in zip(lights, radii):
        if int(L["type"]) != nl.LIGHT_DIRECTIONAL and float(F(R)) > 0.0:
            seed, _ = rand(seed)
            seed, _ = rand(seed)
    return seed


def sample_light(L, radius, pos, seed, d_o):
    """computeLightToSurfaceVector, soft -> (seed, ldir, ldist, in_range, fragile, eps_s); ldir None when culled"""
    if int(L["type"]) == nl.LIGHT_DIRECTIONAL:
        dirn = np.asarray(L["direction"], F).astype(np.float64)
        return seed, -dirn / np.linalg.norm(dirn), 1e10, True, False, 0.0
    lp = np.asarray(L["position"], F).astype(np.float64)
    radius = float(F(radius))
    eps, frag, sp = 0.0, False, lp
    if radius > 0.0:
        to_c = lp - pos
        dist_c = np.linalg.norm(to_c)
        n = to_c / dist_c
        seed, u1 = rand(seed)
        seed, u2 = rand(seed)
        if 1.0 + n[2] < 1.0 / A_CUT:
            frag = True
        if n[2] < float(F(-0.9999999)):
            tng, btg = np.array([0.0, -1.0, 0.0]), np.array([-1.0, 0.0, 0.0])
            a = 1.0 / max(1.0 + n[2], 1e-300)
        else:
            a = 1.0 / (1.0 + n[2])
            b = -n[0] * n[1] * a
            tng = np.array([1.0 - n[0] * n[0] * a, b, -n[0]])
            btg = np.array([b, 1.0 - n[1] * n[1] * a, -n[1]])
        r = (radius * 0.5) * np.sqrt(u1)
        theta = float(TWO_PI_F32 * F(u2))
        sp = lp + r * (np.cos(theta) * tng + np.sin(theta) * btg)
        d_n = 8.0 * U + d_o / dist_c
        eps = r * ((4.0 * a + 8.0) * d_n + 16.0 * U) + 8.0 * U * (np.abs(lp).sum() + r)
    to = sp - pos
    ldist = np.linalg.norm(to)
    rng = float(F(L["range"]))
    if abs(ldist - rng) <= d_o + eps + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum()):
        frag = True
    if ldist > rng:
        return seed, None, ldist, False, frag, eps
    return seed, to / ldist, ldist, True, frag, eps


def light_loop(seed, lights, radii, pos, n, vdir, mat, out, d_o, per_inst, shadows, offset, K, threshold, strength, degree, kmr, acull, aclamp, kw):
    """the loop over the lights of evaluateLightingAndShadingParticles at one surface point; out [1,3] gains every light's terms.
    Returns (seed, shadow rays, shadow hits, per-light transmittance [lights,3], fragile)"""
    nrays, hits_sum, frag = 0, 0, False
    sh_T = np.ones((max(len(lights), 1), 3))
    for li, (L, R) in enumerate(zip(lights, radii)):
        seed, ldir, ldist, inr, fr, eps = sample_light(L, R if shadows == 2 else 0.0, pos, seed, d_o)
        frag |= fr
        if not inr:
            continue  # skipped entirely: no ambient either
        Ls = dict(L, color=np.asarray(L["color"], F).astype(np.float64))
        in_shadow = False
        if shadows:
            nrays += 1
            res, hits, fr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o + eps, degree, kmr, acull, aclamp,
                                           kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
            hits_sum += hits
            sh_T[li] = res
            frag |= fr
            Ls["color"] = np.asarray(L["color"], F).astype(np.float64) * res
            in_shadow = res.max() < 0.001
        if in_shadow:
            out += mat["ambient"]
        else:
            ntl._shade64(Ls, pos[None], n[None], mat, vdir[None], out)
    return seed, nrays, hits_sum, sh_T, frag


def _knobs(kw, offset, threshold, strength):
    f32 = lambda v: float(F(v))
    return (f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99)),
            kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18), f32(offset), f32(threshold), f32(strength))


def lit(instances, V, P, W, H, camera_pos, lights, materials, radii=None, sample_id=0, shadows=2, offset=0.2, threshold=0.8, strength=0.0,
        base=None, **kw):
    """np_trace_lit.lit with shadows = 2: radii one per light (None: the default 1.0), sample_id = frame_sample_id (the seed's; the
    lens's is kw["dof"]'s own).  base: np_trace.trace's result when the caller has it (it does not depend on the lights).
    Returns np_trace_lit.lit's dict."""
    radii = [1.0] * len(lights) if radii is None else list(radii)
    base = trace(instances, V, P, W, H, **kw) if base is None else base
    kmr, acull, aclamp, degree, K, offset, threshold, strength = _knobs(kw, offset, threshold, strength)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    O, D, OK = rays(np.asarray(V, np.float64), np.asarray(P, np.float64), W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    img = np.zeros((H, W, 4))
    sh_hits = np.zeros((H, W), np.int64)
    sh_T = np.ones((H, W, max(len(lights), 1), 3))
    fragile = base["fragile"].copy()
    surface = np.zeros((H, W), bool)
    nrays = np.zeros((H, W), np.int64)
    fallback = np.zeros((H, W), bool)
    cam = np.asarray(camera_pos, F).astype(np.float64)
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
            e = ntl._eval(per_inst[k], o, d, degree)
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
            m = materials[k]
            mv = lambda key: np.asarray(m[key], F).astype(np.float64)
            color = rad0 * mv("emission")
            img[y, x, 3] = base["image"][y, x, 3]
            if not nl.need_shading(m):
                img[y, x, :3] = color
                continue
            mat = dict(ambient=(rad0 * mv("ambient"))[None], diffuse=(rad0 * mv("diffuse"))[None], specular=(rad0 * mv("specular"))[None],
                       shininess=np.array([float(F(m["shininess"]))]))
            out = color[None].copy()
            d_o = pick_dt + 8.0 * U * (np.abs(o).sum() + t_iso + np.abs(pos).sum() + offset)
            if not lights:
                nl._shade_direct(nl.headlight(cam), pos[None], n[None], mat, d[None], out, np.float64, False)
            _, nrays[y, x], sh_hits[y, x], sh_T[y, x], fr = light_loop(seed_of(x, y, sample_id), lights, radii, pos, n, d, mat, out, d_o, per_inst,
                                                                      shadows, offset, K, threshold, strength, degree, kmr, acull, aclamp, kw)
            fragile[y, x] |= fr
            img[y, x, :3] = out[0]
    return dict(image=img, shadow_hits=sh_hits, shadow_T=sh_T, fragile=fragile, surface=surface, rays=nrays, fallback=fallback, base=base)


def hybrid_lit(image, depth, ids, normal, instances, V, P, W, H, camera_pos, lights, materials, radii=None, sample_id=0, shadows=2, offset=0.2,
               threshold=0.8, strength=0.0, rows=None, **kw):
    """np_hybrid.lit with shadows = 2: the same seed (rgen.slang:228 runs in hybrid too), one loop per pixel at the handed-over
    position.  Returns np_hybrid.lit's dict."""
    radii = [1.0] * len(lights) if radii is None else list(radii)
    kmr, acull, aclamp, degree, K, offset, threshold, strength = _knobs(kw, offset, threshold, strength)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    ho = nh.hand_over(depth, ids, normal, V, P, W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
    stored = np.asarray(image, F).astype(np.float64)
    img = stored.copy()
    sh_hits = np.zeros((H, W), np.int64)
    nrays = np.zeros((H, W), np.int64)
    fragile = ho["fragile"].copy()
    cam = np.asarray(camera_pos, F).astype(np.float64)
    y0, y1 = rows or (0, H)
    for y in range(y0, y1):
        for x in range(W):
            st = ho["state"][y, x]
            if st == 1:
                img[y, x] = 0.0
            if st != 3:
                continue
            o, d, t, pos, n = ho["O"][y, x], ho["D"][y, x], ho["t"][y, x], ho["pos"][y, x], ho["n"][y, x]
            k = int(np.searchsorted(prefix, int(ids[y, x]), side="right") - 1)
            m = materials[k]
            mv = lambda key: np.asarray(m[key], F).astype(np.float64)
            rad0 = stored[y, x, :3]
            color = rad0 * mv("emission")
            if not nl.need_shading(m):
                img[y, x, :3] = color
                continue
            mat = dict(ambient=(rad0 * mv("ambient"))[None], diffuse=(rad0 * mv("diffuse"))[None], specular=(rad0 * mv("specular"))[None],
                       shininess=np.array([float(F(m["shininess"]))]))
            out = color[None].copy()
            d_o = 2.0 * ho["d_pos"][y, x] + 8.0 * U * (np.abs(o).sum() + t + np.abs(pos).sum() + offset)
            if not lights:
                nl._shade_direct(nl.headlight(cam), pos[None], n[None], mat, d[None], out, np.float64, False)
            _, nrays[y, x], sh_hits[y, x], _, fr = light_loop(seed_of(x, y, sample_id), lights, radii, pos, n, d, mat, out, d_o, per_inst, shadows,
                                                             offset, K, threshold, strength, degree, kmr, acull, aclamp, kw)
            fragile[y, x] |= fr
            img[y, x, :3] = out[0]
    return dict(image=img, shadow_hits=sh_hits, fragile=fragile, state=ho["state"], surface=ho["state"] == 3, rays=nrays, d_pos=ho["d_pos"],
                t=ho["t"])


def mesh_frame(instances, meshes, mesh_materials, V, P, W, H, camera_pos=None, lights=None, materials=None, radii=None, sample_id=0, lit=True,
               mesh_min_T=0.0, shadows=2, offset=0.2, threshold=0.8, strength=0.0, **kw):
    """np_trace_mesh.frame with shadows = 2 (radii one per light, None: 1.0; sample_id = frame_sample_id).  ONE random state per pixel
    serves both loops over the lights (rgen.slang:1054, :1061): the mesh shading continues where the splat surface's loop ended, and
    starts from the fresh seed where that loop did not run.  The result gains both_loops [H,W] and mesh_loop_fresh [H,W].
    np_trace_mesh.frame's own description: A traced frame with mesh hits.  meshes: np_mesh_rays mesh dicts; mesh_materials: per mesh a list of material dicts; lit: the
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
    radii = [1.0] * len(lights) if radii is None else list(radii)
    both_loops, mesh_loop_fresh = np.zeros((H, W), bool), np.zeros((H, W), bool)
    y0, y1 = kw.get("rows") or (0, H)

    def shadow(pos, d_o, L, R, seed):
        """traceShadowRayForLight at pos for light L -> (seed, transmittance[3], in range, fragile, mesh ray?, occluded?, particle ray?, hits)"""
        seed, ldir, ldist, inr, fr, eps = sample_light(L, R if shadows == 2 else 0.0, pos, seed, d_o)
        if not inr:
            return seed, None, False, fr, 0, 0, 0, 0
        d_o = d_o + eps  # the sample's own error moves direction and distance of both shadow rays
        if not shadows:
            return seed, np.ones(3), True, fr, 0, 0, 0, 0
        any_mesh = any(m.get("visible", True) for m in meshes)
        occ, ofr = _occluded(meshes, pos[None], ldir[None], np.array([ldist]), np.array([d_o])) if any_mesh else (np.zeros(1, bool), np.zeros(1, bool))
        fr = fr or bool(ofr[0])
        if occ[0]:
            return seed, np.zeros(3), True, fr, int(any_mesh), 1, 0, 0
        if not any(pi["alive"].any() for pi in per_inst):
            return seed, np.ones(3), True, fr, int(any_mesh), 0, 0, 0
        res, hits, sfr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull, aclamp,
                                        kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
        return seed, res, True, fr or sfr, int(any_mesh), 0, 1, hits

    def shade(mat, pos, nrm, vdir, d_o, out, y, x, seed):
        """the loop over the lights of evaluateLightingAndShading{Particles,Meshes}: out[1,3] gains every light's terms"""
        if not lights:
            nl._shade_direct(nl.headlight(cam), pos[None], nrm[None], mat, vdir[None], out, np.float64, False)
        for L, R in zip(lights, radii):
            seed, res, inrange, fr, mray, occ, pray, hits = shadow(pos, d_o, L, R, seed)
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
        return seed

    for y in range(y0, y1):
        for x in range(W):
            if not OK[y, x]:
                continue
            o, d = O[y, x], D[y, x]
            seed, splat_loop = seed_of(x, y, sample_id), False
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
                        seed = shade(mat, pos, nn, d, pick_dt + 8.0 * U * (np.abs(o).sum() + t_iso + np.abs(pos).sum() + offset), out, y, x, seed)
                        splat_loop = True
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
                            shade(mat, pos, nrm, d, 16.0 * U * np.abs(pos).sum() + m_t, out, y, x, seed)
                            both_loops[y, x], mesh_loop_fresh[y, x] = splat_loop, not splat_loop
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
                splat_lit=splat_lit, base=base, ok=OK, both_loops=both_loops, mesh_loop_fresh=mesh_loop_fresh)
