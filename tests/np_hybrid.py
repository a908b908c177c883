"""Float64 restatement of steps 2 and 3 of a hybrid frame (mgs_render_hybrid) from a given raster G-buffer and the scene's sets:
  shaders/threedgrt_raytrace.rgen.slang:346-460     initRtxStateFromRasterPass (the hand-over)
  shaders/threedgrt_raytrace.rgen.slang:1047-1049   a surface without a picked splat stays unlit
then the shading and the shadow rays of np_trace_lit (its shadow_ray, _per_inst and _shade64 are used as they are).  Test
infrastructure only.  The G-buffer is what the raster pass left: the image as stored in its target format (float), the picked ndc
depth (fp32), the picked ids (caller's global ids) and the integrated normal (fp32 x 4).

state [H,W]: 0 = outside the fisheye circle (the stored pixel stays), 1 = discarded (0,0,0,0), 2 = valid surface without a picked id
(the stored pixel stays), 3 = lit.

Fragile pixels are those of np_trace_lit's shadow ray and range rules with this d_o: the hand-over's position (ray origin + ray
parameter * ray direction) is evaluated in float64 and once more in numpy float32 in the kernel's operation order; d_o = twice the
distance between the two (the factor covers contraction in the compiled kernel) + 8 u (|o|_1 + t + |pos|_1 + offset).  The
unprojection of an ndc depth near 1 is ill-conditioned, so the distance is computed, not assumed.  Also fragile: a picked depth
within 4 ulp of 0.0001, a normal.w within 4 ulp of 0.001, a normal length within 1e-6 of 0.001."""
import numpy as np

import np_lighting as nl
import np_trace_lit as ntl
from np_trace import U, rays

INVALID = 0xFFFFFFFF
F = np.float32


def _unproject32(x, y, z, W, H, Pi, Vi, o32):
    """the pinhole branch of k_hybrid_surface in fp32, operation for operation: (world position, ray parameter)"""
    cx = (F(x) + F(0.5)) / F(W) * F(2.0) - F(1.0)
    cy = (F(y) + F(0.5)) / F(H) * F(2.0) - F(1.0)
    v = [((cx * Pi[r, 0] + cy * Pi[r, 1]) + z * Pi[r, 2]) + Pi[r, 3] for r in range(4)]
    v = [v[0] / v[3], v[1] / v[3], v[2] / v[3], v[3] / v[3]]
    w = [((v[0] * Vi[r, 0] + v[1] * Vi[r, 1]) + v[2] * Vi[r, 2]) + v[3] * Vi[r, 3] for r in range(3)]
    e = [w[k] - o32[k] for k in range(3)]
    return np.array(w, F), np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def hand_over(depth, ids, normal, V, P, W, H, fisheye=False, fov_rad=None, dof=None):
    """dict(state, t, pos (origin + t * direction), n, d_pos (float64 against fp32 distance of pos), fragile, O, D)"""
    V64, P64 = np.asarray(V, F).astype(np.float64), np.asarray(P, F).astype(np.float64)
    O, D, OK = rays(V64, P64, W, H, fisheye, fov_rad, dof)
    Pi32, Vi32 = nl.inverse_f32(P), nl.inverse_f32(V)
    Pi, Vi = Pi32.astype(np.float64), Vi32.astype(np.float64)
    depth = np.asarray(depth, F)
    normal = np.asarray(normal, F)
    state = np.zeros((H, W), np.int64)
    t_out = np.zeros((H, W))
    pos_out = np.zeros((H, W, 3))
    n_out = np.zeros((H, W, 3))
    d_pos = np.zeros((H, W))
    fragile = np.zeros((H, W), bool)
    ulp = lambda v: float(np.spacing(F(v)))
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if not OK[y, x]:
                    continue
                z, n4 = depth[y, x], normal[y, x]
                if abs(float(z) - float(F(0.0001))) <= 4.0 * ulp(0.0001) or abs(float(n4[3]) - float(F(0.001))) <= 4.0 * ulp(0.001):
                    fragile[y, x] = True
                valid = z > F(0.0001)
                n = np.zeros(3)
                if n4[3] > F(0.001):
                    n = n4[:3].astype(np.float64)
                    n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
                nlen = np.sqrt((n * n).sum())
                if abs(nlen - 0.001) <= 1e-6:
                    fragile[y, x] = True
                if not valid or nlen < 0.001:
                    state[y, x] = 1
                    continue
                if int(ids[y, x]) == INVALID:
                    state[y, x] = 2
                    continue
                o, d = O[y, x], D[y, x]
                o32, d32 = o.astype(F), d.astype(F)
                if fisheye:
                    dvz = d @ V64[2, :3]
                    t = ((float(z) * Pi[2, 2] + Pi[2, 3]) / (float(z) * Pi[3, 2] + Pi[3, 3])) / dvz
                    V32 = np.asarray(V, F)
                    dvz32 = (d32[0] * V32[2, 0] + d32[1] * V32[2, 1]) + d32[2] * V32[2, 2]
                    t32 = ((z * Pi32[2, 2] + Pi32[2, 3]) / (z * Pi32[3, 2] + Pi32[3, 3])) / dvz32
                else:
                    clip = np.array([(x + 0.5) / W * 2.0 - 1.0, (y + 0.5) / H * 2.0 - 1.0, float(z), 1.0])
                    vp = Pi @ clip
                    wp = (Vi @ (vp / vp[3]))[:3]
                    t = np.linalg.norm(wp - o)
                    _, t32 = _unproject32(x, y, z, W, H, Pi32, Vi32, o32)
                if not t > 0.0:
                    state[y, x] = 1  # no surface for the light pass (k_trace_light's rule); a t32 of the other sign would be fragile
                    fragile[y, x] |= bool(t32 > 0)
                    continue
                pos = o + t * d
                pos32 = (o32 + F(t32) * d32).astype(np.float64)
                state[y, x] = 3
                t_out[y, x], pos_out[y, x], n_out[y, x] = t, pos, n
                d_pos[y, x] = np.linalg.norm(pos32 - pos)
    return dict(state=state, t=t_out, pos=pos_out, n=n_out, d_pos=d_pos, fragile=fragile, O=O, D=D)


def lit(image, depth, ids, normal, instances, V, P, W, H, camera_pos, lights, materials, shadows=1, offset=0.2, threshold=0.8, strength=0.0,
        rows=None, **kw):
    """image [H,W,4]: the raster frame as stored (any float dtype); instances: [(np_trace.prepare_set(...), M)]; kw: np_trace.trace's
    keywords that matter here (samples_per_pass, adaptive_clamping, kernel_degree, kernel_min_response, alpha_clamp, alpha_cull,
    sh_degree, fisheye, fov_rad, dof, no_gauss, sh_only).  Returns dict(image [H,W,4] float64, shadow_hits, fragile, state, surface
    (lit pixels), rays (shadow rays the pixel traces), d_pos, t)."""
    f32 = lambda v: float(F(v))
    kmr, acull, aclamp = f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99))
    degree, K = kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18)
    offset, threshold, strength = f32(offset), f32(threshold), f32(strength)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    ho = hand_over(depth, ids, normal, V, P, W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
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
                       shininess=np.array([f32(m["shininess"])]))
            out = color[None].copy()
            d_o = 2.0 * ho["d_pos"][y, x] + 8.0 * U * (np.abs(o).sum() + t + np.abs(pos).sum() + offset)
            if not lights:
                nl._shade_direct(nl.headlight(cam), pos[None], n[None], mat, d[None], out, np.float64, False)
            for L in lights:
                if int(L["type"]) == nl.LIGHT_DIRECTIONAL:
                    dirn = np.asarray(L["direction"], F).astype(np.float64)
                    ldir, ldist = -dirn / np.linalg.norm(dirn), 1e10
                else:
                    lp = np.asarray(L["position"], F).astype(np.float64)
                    to = lp - pos
                    ldist = np.linalg.norm(to)
                    rng = f32(L["range"])
                    if abs(ldist - rng) <= d_o + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum()):
                        fragile[y, x] = True
                    if ldist > rng:
                        continue  # skipped entirely: no ambient either
                    ldir = to / ldist
                Ls = dict(L, color=np.asarray(L["color"], F).astype(np.float64))
                in_shadow = False
                if shadows:
                    nrays[y, x] += 1
                    res, hits, fr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull,
                                                   aclamp, kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
                    sh_hits[y, x] += hits
                    fragile[y, x] |= fr
                    Ls["color"] = Ls["color"] * res
                    in_shadow = res.max() < 0.001
                if in_shadow:
                    out += mat["ambient"]
                else:
                    ntl._shade64(Ls, pos[None], n[None], mat, d[None], out)
            img[y, x, :3] = out[0]
    return dict(image=img, shadow_hits=sh_hits, fragile=fragile, state=ho["state"], surface=ho["state"] == 3, rays=nrays, d_pos=ho["d_pos"],
                t=ho["t"])
