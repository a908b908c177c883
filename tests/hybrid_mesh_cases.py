"""The scenes of the hybrid frames with meshes (mgs_frame_set_hybrid_meshes; test_hybrid_mesh_cpu.py, test_gpu_hybrid_mesh.py), numpy
only: hybrid_cases' splat clusters over trace_mesh_cases' quads.  Frames are 48 x 40 (m12: 33 x 25).  A case is one of hybrid_cases
plus meshes (np_mesh_rays dicts with `materials`) and mesh_min_T.

m01  3DGS, a point light, a floor quad under a cluster: the splats' shadow on the floor, the floor occluding nothing
m02  a wall between the light and the cluster (mesh shadow on the splats) and in front of part of it (raster alpha 0 behind the mesh:
     discarded, the mesh at T = 1)
m03  3DGUT pinhole          m04  3DGUT fisheye          m05  3DGUT depth of field (the child also accumulates three samples)
m06  translucent splats in front of the floor, thresholds 0 / 0.5 / 1.0
m07  tests/golden/meshes/fixture.obj with its materials (one needs no shading); directional + spot + an out-of-range point light
m08  no lights (the headlight); shadows off
m09  samples_per_pass 4 / 18 / 32
m10  (child only) an invisible instance, a mesh moved between two frames
m11  (child only) m06's scene in RGBA16F and RGBA8
m12  33 x 25 with 4097 splats, the floor and a wall in front of every splat (the child also renders its strips and a frame context)"""
import functools

import numpy as np

import hybrid_cases as hc
import np_hybrid_mesh as nhm
import np_lighting as nl
import trace_cases as tc
import trace_lit_cases as lc
import trace_mesh_cases as tmc

GS, GUT = hc.GS, hc.GUT
FRAGILE_CAP = hc.FRAGILE_CAP

# upright, x in [-0.1, 0.9], between the point light (+x side) and part of the cluster; seen from the eye it also covers part of it
WALL = tmc.quad([[0.12, -0.5, 0.45], [0.9, -0.5, 0.45], [0.9, 0.7, 0.45], [0.12, 0.7, 0.45]], (0.0, 0.0, 1.0))

# in front of every splat of m12 (view depth <= 1.81 against >= 1.95): what it covers is cut entirely, and no splat's key depth lies at
# its plane (a wall that crosses the 4097 splats' depth range has one within the plane's fp32 error on a quarter of its pixels)
WALL_FRONT = tmc.quad([[0.12, -0.5, 1.6], [0.9, -0.5, 1.6], [0.9, 0.7, 1.6], [0.12, 0.7, 1.6]], (0.0, 0.0, 1.0))


def _case(sets, lights, pipeline, meshes, mesh_min_T=0.0, **kw):
    c = hc._case(sets, lights, pipeline, **kw)
    c.update(meshes=meshes, mesh_min_T=mesh_min_T)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    side = nl.default_light(position=(0.6, 0.5, 1.6), range=10.0, intensity=4.0)   # in front of the wall: its shadow falls on the cluster behind it
    sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), intensity=0.5)
    spot = nl.default_light(type=nl.LIGHT_SPOT, position=(-0.2, 1.4, 0.1), direction=(0.1, -1.0, 0.0), range=10.0, intensity=5.0,
                            inner_cone_deg=14.0, outer_cone_deg=24.0)
    far = nl.default_light(position=(6.0, 7.0, 5.0), range=1.0, intensity=50.0)
    blob = lc.blob()
    c = {}
    c["m01_3dgs_floor"] = _case([(blob, tc.I4)], [point], GS, [tmc.FLOOR])
    c["m02_wall"] = _case([(lc.blob(n=40, radius=0.3, seed=13), tc.I4)], [side], GS, [tmc.FLOOR, WALL])
    c["m03_3dgut"] = _case([(blob, tc.I4)], [point], GUT, [tmc.FLOOR])
    c["m04_fisheye"] = _case([(blob, tc.I4)], [point], GUT, [tmc.FLOOR], frame=dict(camera_model=1, fov_rad=1.4))
    c["m05_dof"] = _case([(blob, tc.I4)], [point], GUT, [tmc.FLOOR], frame=dict(dof_mode=1, focus_dist=2.9, aperture=0.004))
    veil = lc.blob(opacity=-1.2, n=16, log_scale=-1.7, seed=5)
    for tag, lim in (("0", 0.0), ("05", 0.5), ("1", 1.0)):
        c["m06_threshold_" + tag] = _case([(veil, tc.I4)], [point], GUT, [tmc.FLOOR], mesh_min_T=lim)
    c["m07_fixture"] = _case([(blob, tc.I4)], [sun, spot, far], GS,
                             [tmc.FLOOR, tmc.fixture(tc.trs((0.3, 0.3, 0.3), (0, 1, 0), 25.0, (-0.8, -0.32, 0.3)))])
    c["m08_headlight"] = _case([(blob, tc.I4)], [], GUT, [tmc.FLOOR])
    c["m08_shadows_off"] = _case([(blob, tc.I4)], [point], GS, [tmc.FLOOR], light=dict(shadows_mode=0))
    stack = lc.blob(n=60, centre=(0.0, 0.45, 0.0), radius=0.5, opacity=-2.2, seed=21, log_scale=-1.8)
    for k in (4, 18, 32):
        c[f"m09_spp_{k}"] = _case([(stack, tc.I4)], [point], GS, [tmc.FLOOR], light=dict(particle_shadow_transmittance_threshold=0.05),
                                  trace=dict(samples_per_pass=k))
    deep = lc.join(lc.floor(n_side=62, half=1.3, seed=15, y=-0.3), lc.blob(n=253, seed=16, radius=0.35, log_scale=-3.3))
    deep["scale"][:62 * 62] += np.log(np.float32(0.14))
    c["m12_deep"] = _case([(deep, tc.I4)], [point], GUT, [tmc.FLOOR, WALL_FRONT], W=33, H=25)
    return c


def restate_with(c, gbuffer, mesh, inst, rows=None):
    """np_hybrid_mesh.frame of the case on a G-buffer (image as stored in float, depth, ids, normal) and mesh hit records"""
    L = c["light"]
    kw = lc._trace_kw(c)
    image, depth, ids, normal = gbuffer
    return nhm.frame(image, depth, ids, normal, mesh, c["meshes"], [m["materials"] for m in c["meshes"]], inst, c["V"], c["P"], c["W"], c["H"],
                     c["eye"], c["lights"], c["materials"], mesh_min_T=c["mesh_min_T"], shadows=L.get("shadows_mode", 0),
                     offset=L.get("particle_shadow_offset", 0.2), threshold=L.get("particle_shadow_transmittance_threshold", 0.8),
                     strength=L.get("particle_shadow_color_strength", 0.0), rows=rows, **kw)


def mesh_hits64(c):
    """the primary mesh rays of the case in float64 (np_mesh_rays), reshaped [H,W]: what the depth pre-pass finds"""
    import np_mesh_rays as nr
    from np_trace import rays
    kw = lc._trace_kw(c)
    W, H = c["W"], c["H"]
    O, D, OK = rays(np.asarray(c["V"], np.float64), np.asarray(c["P"], np.float64), W, H, kw["fisheye"], kw["fov_rad"], kw["dof"])
    ok = OK.reshape(-1)
    n = int(ok.sum())
    mr = nr.trace(c["meshes"], O.reshape(-1, 3)[ok], D.reshape(-1, 3)[ok], np.full(n, 0.001, np.float32), np.full(n, 10000.0, np.float32))
    mesh = {}
    for k in ("hit", "t", "b1", "b2", "pos", "nrm", "inst", "mat", "prim", "fragile"):
        v = mr[k]
        full = np.zeros((W * H,) + v.shape[1:], v.dtype)
        if k == "t":
            full[:] = np.inf
        full[ok] = v
        mesh[k] = full.reshape((H, W) + v.shape[1:])
    mesh["ok"], mesh["triangles"] = OK, mr["triangles"]
    return mesh


def oracle_gbuffer_cut(ob, case, plane, tol):
    """the CPU oracle's raster frame of the case against the depth plane [H,W]: (image float32, picked depth, ids, integrated normal,
    near [H,W] bool).  The oracle has no depth test, so the cut frame is assembled as test_lighting_cpu.oracle_gbuffer assembles one
    against a level: the sorted stream filtered to the splats whose key depth is <= the level.  Here every pixel has its own level; the
    filtered stream depends only on HOW MANY splats pass, so the pixels are grouped by that count and the frame is rendered once per
    distinct count.  near: some splat's key depth lies within tol [H,W] (np_hybrid_mesh.depth_plane's bound on the fp32 plane's
    error) plus two fp32 steps of the pixel's level: a device plane could keep or cut it (fragile)."""
    import occluder_levels as ol
    f = dict(tc.FRAME_DEFAULTS, **{k: v for k, v in case["frame"].items() if k in tc.FRAME_DEFAULTS})
    gut = case["frame"]["pipeline"] == GUT
    kw = dict(camera_model=f["camera_model"], fov_rad=f["fov_rad"] or None, dof_mode=f["dof_mode"], focus_dist=f["focus_dist"],
              aperture=f["aperture"], frame_sample_id=f["frame_sample_id"], kernel_degree=f["kernel_degree"],
              kernel_min_response=f["kernel_min_response"], alpha_clamp=f["alpha_clamp"], pipeline_3dgut=1 if gut else 0)
    inst = ob.make_instances([(ob.PreparedSet(a), M) for a, M in case["sets"]])
    V, P, eye, W, H = case["V"], case["P"], case["eye"], case["W"], case["H"]
    fr = ob.make_frame(V, P, eye, W, H, **kw)
    ftb = ob.make_frame(V, P, eye, W, H, front_to_back=1, **kw)
    keys, order = ob.sort_stable(*ob.key_cull(fr, inst))
    z = ol.depths_of_btf_keys(keys)                       # far to near: descending
    level = np.asarray(plane, np.float64).astype(np.float32)
    asc = z[::-1].astype(np.float32)                      # ascending
    count = np.searchsorted(asc, level.reshape(-1), side="right").reshape(H, W)   # splats with z <= level
    near = np.zeros((H, W), bool)
    if z.size:
        for k in (np.clip(count - 1, 0, z.size - 1), np.clip(count, 0, z.size - 1)):
            near |= np.abs(asc[k].astype(np.float64) - level) <= np.asarray(tol) + 2.0 * np.spacing(level)
    img, depth = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
    ids, nrm = np.zeros((H, W), np.uint32), np.zeros((H, W, 4), np.float32)
    for n in np.unique(count):
        keep = order[z.size - int(n):].copy()            # the n nearest of the far-to-near stream
        m = count == n
        if gut:
            d1, i1, n1 = ob.render_surface_gut(fr, inst, keep[::-1].copy(), 0.7, normals=True)
            c1 = ob.render_gut(ftb, inst, keep)[0]
        else:
            d1, i1, n1 = ob.render_surface(fr, inst, keep[::-1].copy(), 0.7, normals=True)
            c1 = ob.render(ftb, inst, order=keep)[0]
        img[m], depth[m], ids[m], nrm[m] = c1[m], d1[m], i1[m], n1[m]
    return img, depth, ids, nrm, near
