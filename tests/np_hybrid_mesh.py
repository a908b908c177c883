"""Float64 restatement of steps 3 to 5 of a hybrid frame with meshes (mgs_frame_set_hybrid_meshes; include/mgs.h, "meshes in the hybrid
frames") from a given raster G-buffer, the per-pixel mesh hit records, the scene's sets, lights and materials:
  shaders/threedgrt_raytrace.rgen.slang:346-460     initRtxStateFromRasterPass with T = 1 - stored alpha (np_hybrid.hand_over)
  shaders/threedgrt_raytrace.rgen.slang:468-478     discardSplatContribution: radiance 0, T = 1
  shaders/threedgrt_raytrace.rgen.slang:1037-1062   splatIsClosest, the composite condition
  shaders/threedgrt_raytrace.rgen.slang:1082-1144, :1222-1341   the two shading loops, every shadow ray asking the meshes first
It composes np_hybrid (hand-over), np_trace_mesh (_occluded, _light_vec: the mesh occlusion ray and its three windows) and np_trace_lit
(shadow_ray, _shade64).  Test infrastructure only.

G-buffer: (image as stored, as float; picked ndc depth fp32; picked ids, caller's; integrated normal fp32 x 4), what the raster pass
left after it was tested against the depth plane.  mesh: dict of [H,W] arrays hit (bool), t, pos [.,3], nrm [.,3], inst, mat and
optionally fragile, as np_mesh_rays.trace reports them or as the device's MgsMeshHit records hold them (from_records).

state [H,W]: np_hybrid's 0 (outside the fisheye circle) / 1 (discarded) / 2 (surface without a pick) / 3 (lit), and 4: a surface with
a pick whose ray parameter is not < t_mesh, settled with its raster colour and its own T.

Fragile pixels: np_hybrid's and np_trace_mesh's rules for the rays this frame traces, plus, with u = 2^-24:
  * t of the surface against t_mesh: |t - t_mesh| <= 2 d_pos + 8 u (|o|_1 + t) + 32 u (|o|_1 + t_mesh), the hand-over's fp32 position
    error (np_hybrid) and the mesh t's own (np_trace_mesh's m_t);
  * T against the threshold: T = 1 - alpha is ONE fp32 subtraction of a stored value, exact in this restatement, so only a T within
    4 u of the threshold is fragile (a discarded pixel's T is the constant 1 and never is);
  * a mesh occlusion hit within np_trace_mesh's margins of the shadow window (its _occluded)."""
import numpy as np

import np_hybrid as nh
import np_lighting as nl
import np_trace_lit as ntl
import np_trace_mesh as ntm
from np_trace import U

F = np.float32


def from_records(rec):
    """the device's MgsMeshHit records [H,W] as the mesh dict"""
    hit = rec["hit"] == 1
    return dict(hit=hit, t=np.where(hit, rec["t"].astype(np.float64), np.inf), pos=rec["position"].astype(np.float64),
                nrm=rec["normal"].astype(np.float64), inst=rec["instance_id"].astype(np.int64), mat=rec["material_id"].astype(np.int64))


def depth_plane(mesh, V, P):
    """step 1's plane in float64 from hit records: (plane [H,W], tol [H,W]); 1.0 on a miss.  tol is mesh_ray_cases' depth_tol rule:
    the position's fp32 error (16 u |pos|_1, the record's rounding) taken through ndc z numerically along the view axis, plus 8 u of the
    terms of clip z over clip w"""
    V, P = np.asarray(V, F).astype(np.float64), np.asarray(P, F).astype(np.float64)
    pos = np.concatenate([mesh["pos"], np.ones(mesh["pos"].shape[:-1] + (1,))], -1)
    view = pos @ V.T
    clip = view @ P.T
    with np.errstate(all="ignore"):
        z = clip[..., 2] / clip[..., 3]
        dv = 16.0 * U * (np.abs(mesh["pos"]).sum(-1) + np.abs(V[:3, 3]).sum())
        def zat(s):
            v2 = view.copy()
            v2[..., 2] += s * dv
            c = v2 @ P.T
            return c[..., 2] / c[..., 3]
        tol = np.maximum(np.abs(zat(1.0) - z), np.abs(zat(-1.0) - z)) + 8.0 * U * (np.abs(view) @ np.abs(P[2])) / np.abs(clip[..., 3]) + 4.0 * U
    return np.where(mesh["hit"], z, 1.0), np.where(mesh["hit"], tol, 0.0)


def frame(image, depth, ids, normal, mesh, meshes, mesh_materials, instances, V, P, W, H, camera_pos, lights, materials, mesh_min_T=0.0,
          shadows=1, offset=0.2, threshold=0.8, strength=0.0, rows=None, **kw):
    """meshes: np_mesh_rays mesh dicts (the occlusion rays); mesh_materials: per mesh a list of material dicts; the rest as np_hybrid.lit.
    Returns dict(image [H,W,4] float64, shadow_hits, fragile, state, T [H,W] (the pixel's transmittance before the threshold),
    composited, settled (state 4), mesh_rays / shadow_rays / occluded [H,W]: mesh occlusion rays, particle shadow rays, occluded rays)."""
    f32 = lambda v: float(F(v))
    kmr, acull, aclamp = f32(kw.get("kernel_min_response", 0.0113)), f32(kw.get("alpha_cull", 1.0 / 255.0)), f32(kw.get("alpha_clamp", 0.99))
    degree, K = kw.get("kernel_degree", 2), kw.get("samples_per_pass", 18)
    offset, threshold, strength, minT = f32(offset), f32(threshold), f32(strength), f32(mesh_min_T)
    per_inst = ntl._per_inst(instances, kmr, acull, kw.get("adaptive_clamping", True))
    prefix = np.array([pi["base"] for pi in per_inst], np.int64)
    ho = nh.hand_over(depth, ids, normal, V, P, W, H, kw.get("fisheye", False), kw.get("fov_rad"), kw.get("dof"))
    stored32 = np.asarray(image, F)
    stored = stored32.astype(np.float64)
    img = stored.copy()
    state = ho["state"].copy()
    fragile = ho["fragile"].copy()
    if "fragile" in mesh:
        fragile |= mesh["fragile"]
    Tout = np.ones((H, W))
    sh_hits = np.zeros((H, W), np.int64)
    composited = np.zeros((H, W), bool)
    mesh_rays, shadow_rays, occluded = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    cam = np.asarray(camera_pos, F).astype(np.float64)
    lights = list(lights or [])
    any_mesh = any(m.get("visible", True) for m in meshes)
    any_splat = any(pi["alive"].any() for pi in per_inst)

    def shade(mat, pos, nrm, vdir, d_o, out, y, x):
        """the loop over the lights of evaluateLightingAndShading{Particles,Meshes} (np_trace_mesh.frame's, restated on this frame's state)"""
        if not lights:
            nl._shade_direct(nl.headlight(cam), pos[None], nrm[None], mat, vdir[None], out, np.float64, False)
        for L in lights:
            ldir, ldist, rng = ntm._light_vec(L, pos)
            if rng is not None:
                lp = np.asarray(L["position"], F).astype(np.float64)
                if abs(ldist - rng) <= d_o + 8.0 * U * (np.abs(pos).sum() + np.abs(lp).sum()):
                    fragile[y, x] = True
                if ldist > rng:
                    continue
            res = np.ones(3)
            if shadows:
                occ = False
                if any_mesh:
                    o_, f_ = ntm._occluded(meshes, pos[None], ldir[None], np.array([ldist]), np.array([d_o]))
                    occ = bool(o_[0])
                    fragile[y, x] |= bool(f_[0])
                    mesh_rays[y, x] += 1
                if occ:
                    occluded[y, x] += 1
                    res = np.zeros(3)
                elif any_splat:
                    shadow_rays[y, x] += 1
                    res, hits, sfr = ntl.shadow_ray(per_inst, pos + ldir * offset, ldir, ldist, K, threshold, strength, d_o, degree, kmr, acull,
                                                    aclamp, kw.get("sh_degree", 3), kw.get("no_gauss", False), kw.get("sh_only", False))
                    sh_hits[y, x] += hits
                    fragile[y, x] |= bool(sfr)
            if shadows and res.max() < 0.001:
                out += mat["ambient"]
            else:
                Ls = dict(L, color=np.asarray(L["color"], F).astype(np.float64) * res)
                ntl._shade64(Ls, pos[None], nrm[None], mat, vdir[None], out)

    y0, y1 = rows or (0, H)
    for y in range(y0, y1):
        for x in range(W):
            st = state[y, x]
            if st == 0:
                continue
            o, d = ho["O"][y, x], ho["D"][y, x]
            hit, t_mesh = bool(mesh["hit"][y, x]), float(mesh["t"][y, x])
            m_t = 32.0 * U * (np.abs(o).sum() + t_mesh) if hit else 0.0
            rgb, alpha = stored[y, x, :3].copy(), stored[y, x, 3]
            T = float(F(1.0) - stored32[y, x, 3])
            if st == 1:
                rgb, alpha, T = np.zeros(3), 0.0, 1.0
            elif st == 3:
                t, pos, n = ho["t"][y, x], ho["pos"][y, x], ho["n"][y, x]
                if hit and abs(t - t_mesh) <= 2.0 * ho["d_pos"][y, x] + 8.0 * U * (np.abs(o).sum() + t) + m_t:
                    fragile[y, x] = True
                if hit and not t < t_mesh:
                    state[y, x] = 4  # splatIsClosest fails: the raster colour, unlit, and its own T
                else:
                    k = int(np.searchsorted(prefix, int(ids[y, x]), side="right") - 1)
                    m = materials[k]
                    mv = lambda key: np.asarray(m[key], F).astype(np.float64)
                    out = (rgb * mv("emission"))[None].copy()
                    if nl.need_shading(m):
                        mat = dict(ambient=(rgb * mv("ambient"))[None], diffuse=(rgb * mv("diffuse"))[None], specular=(rgb * mv("specular"))[None],
                                   shininess=np.array([f32(m["shininess"])]))
                        d_o = 2.0 * ho["d_pos"][y, x] + 8.0 * U * (np.abs(o).sum() + t + np.abs(pos).sum() + offset)
                        shade(mat, pos, n, d, d_o, out, y, x)
                    rgb = out[0]
            Tout[y, x] = T
            if hit:
                if st != 1 and abs(T - minT) <= 4.0 * U:  # (a discarded pixel's T is the constant 1: its comparison is exact)
                    fragile[y, x] = True
                if T > minT:
                    composited[y, x] = True
                    mm = mesh_materials[int(mesh["inst"][y, x])][int(mesh["mat"][y, x])]
                    mv = lambda key: np.asarray(mm[key], F).astype(np.float64)
                    rgb = rgb + mv("emission")
                    if nl.need_shading(mm):
                        mat = dict(ambient=(T * mv("ambient"))[None], diffuse=(T * mv("diffuse"))[None], specular=(T * mv("specular"))[None],
                                   shininess=np.array([f32(mm["shininess"])]))
                        pos, nrm = mesh["pos"][y, x], mesh["nrm"][y, x]
                        out = rgb[None].copy()
                        shade(mat, pos, nrm, d, 16.0 * U * np.abs(pos).sum() + m_t, out, y, x)
                        rgb = out[0]
                    alpha = 1.0
            img[y, x] = (rgb[0], rgb[1], rgb[2], alpha)
    return dict(image=img, shadow_hits=sh_hits, fragile=fragile, state=state, T=Tout, composited=composited, settled=state == 4,
                mesh_rays=mesh_rays, shadow_rays=shadow_rays, occluded=occluded, d_pos=ho["d_pos"], t=ho["t"])
