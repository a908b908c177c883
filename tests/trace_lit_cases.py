"""The scenes of the lit traced-frame tests (test_trace_lit_cpu.py, test_gpu_trace_lit.py), numpy only.  The pattern: a "floor" sheet
of flat opaque splats, "blob" occluders between light and floor, frames of 48 x 40 pixels (3 x 3 tiles, partial on both axes; one
case is 33 x 25).  A case
= dict(sets=[(arrays, M)], V, P, eye, W, H, frame, trace, light={MgsTraceLightParams overrides}, lights=[np_lighting light dicts],
materials=[one np_lighting material dict per instance]); restate(name) runs the float64 restatement once per process."""
import functools

import numpy as np

import np_lighting as nl
import np_trace_lit as ntl
import trace_cases as tc

SHADED = dict(ambient=(0.15, 0.15, 0.15), diffuse=(0.8, 0.8, 0.8), specular=(0.0, 0.0, 0.0), emission=(0.0, 0.0, 0.0), shininess=0.0)


def floor(n_side=14, half=1.3, y=-0.5, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.linspace(-half, half, n_side)
    xs, zs = np.meshgrid(g, g)
    n = xs.size
    pos = np.stack([xs.ravel(), np.full(n, y), zs.ravel()], 1) + rng.uniform(-0.03, 0.03, (n, 3))
    scale = np.tile(np.log([0.16, 0.02, 0.16]), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 3))
    rot = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)) + rng.uniform(-0.02, 0.02, (n, 4))
    return dict(positions=pos.astype(np.float32), f_dc=rng.uniform(0.2, 1.5, (n, 3)).astype(np.float32),
                f_rest=(rng.standard_normal((n, 45)) * 0.05).astype(np.float32), opacity=np.full(n, 4.0, np.float32),
                scale=scale.astype(np.float32), rotation=rot.astype(np.float32))


def blob(n=24, centre=(0.0, 0.15, 0.0), radius=0.22, opacity=4.0, seed=12, log_scale=-2.2):
    a = tc.cloud(n, seed, half=radius, log_scale=log_scale)
    a["positions"] = (a["positions"] + np.asarray(centre, np.float32)).astype(np.float32)
    a["opacity"] = np.full(n, opacity, np.float32)
    return a


def join(*sets):
    return {k: np.concatenate([s[k] for s in sets]) for k in sets[0]}


def _case(sets, lights, materials=None, light=None, trace=None, frame=None, eye=(0.0, 1.3, 2.6), target=(0.0, -0.35, 0.0), W=48, H=40):
    c = tc._case(sets, eye, target, W=W, H=H, frame=dict(frame or {}, lighting_mode=1), trace=trace)
    c.update(lights=lights, materials=materials or [SHADED] * len(sets), light=dict(dict(shadows_mode=1), **(light or {})))
    return c


def fins():
    """two thin vertical sheets either side of the view axis, seen edge-on through a 2-degree lens: their max-density-plane normals
    face the camera from opposite sides (+x and -x), so on the rays between them the integrated normal nearly cancels and
    surfaceFinalFiltering's -rayDirection fallback (length <= 0.2) is taken"""
    a = blob(n=2, radius=0.0)
    a["positions"][:] = ((-0.02, 0.0, 0.0), (0.02, 0.0, -0.3))
    a["scale"][:] = np.log((0.02, 0.5, 0.5))
    a["rotation"][:] = (1.0, 0.0, 0.0, 0.0)
    a["opacity"][:] = (0.0, 1.0)
    a["f_dc"][:] = ((1.0, 0.2, 0.2), (0.2, 0.2, 1.0))
    return a


def _trace_kw(c):
    f, t = dict(tc.FRAME_DEFAULTS, **{k: v for k, v in c["frame"].items() if k in tc.FRAME_DEFAULTS}), dict(tc.TRACE_DEFAULTS, **c["trace"])
    dof = (f["focus_dist"], f["aperture"], f["frame_sample_id"]) if f["dof_mode"] else None
    return dict(samples_per_pass=t["samples_per_pass"], max_passes=t["max_passes"], min_transmittance=t["min_transmittance"],
                adaptive_clamping=bool(t["kernel_adaptive_clamping"]), depth_iso_threshold=t["depth_iso_threshold"],
                kernel_degree=f["kernel_degree"], kernel_min_response=f["kernel_min_response"], alpha_clamp=f["alpha_clamp"],
                alpha_cull=f["alpha_cull_threshold"], sh_degree=f["sh_degree"], fisheye=f["camera_model"] == 1, fov_rad=f["fov_rad"], dof=dof,
                thin=f["thin_particle_threshold"], normal_method=f["normal_method"])


@functools.lru_cache(maxsize=None)
def cases():
    scene = join(floor(), blob())
    point = nl.default_light(position=(0.3, 1.6, 0.2), range=10.0, intensity=4.0)
    sun = nl.default_light(type=nl.LIGHT_DIRECTIONAL, direction=(-0.3, -1.0, -0.2), intensity=1.0)
    spot = nl.default_light(type=nl.LIGHT_SPOT, position=(-0.2, 1.4, 0.1), direction=(0.1, -1.0, 0.0), range=10.0, intensity=5.0,
                            inner_cone_deg=14.0, outer_cone_deg=24.0)  # the cone's edge crosses the floor ~0.85 from its axis
    c = {}
    c["l01_point"] = _case([(scene, tc.I4)], [point])
    c["l02_directional"] = _case([(scene, tc.I4)], [sun])
    c["l03_spot"] = _case([(scene, tc.I4)], [spot])
    c["l04_range"] = _case([(scene, tc.I4)], [nl.default_light(position=(0.9, 0.4, 0.0), range=1.4, intensity=2.0, attenuation_mode=1)])
    c["l05_three"] = _case([(scene, tc.I4)], [point, dict(sun, intensity=0.5), spot])
    c["l06_headlight"] = _case([(scene, tc.I4)], [])
    thin = join(floor(), blob(opacity=-2.6, n=12, log_scale=-1.9))
    for tag, st in (("s0", 0.0), ("s05", 0.5), ("s1", 1.0)):  # T stays inside (threshold, 1); s05 and s1 evaluate SH in the shadow walk
        c["l07_translucent_" + tag] = _case([(thin, tc.I4)], [point], light=dict(particle_shadow_transmittance_threshold=0.3, particle_shadow_color_strength=st))
    # more occluders on a shadow ray than slots: a tall stack of faint splats between light and floor, a low threshold
    stack = join(floor(), blob(n=60, centre=(0.0, 0.45, 0.0), radius=0.5, opacity=-2.2, seed=21, log_scale=-1.8))
    for k in (4, 1, 18, 32):
        c[f"l08_kcut_{k}"] = _case([(stack, tc.I4)], [point], light=dict(particle_shadow_transmittance_threshold=0.05), trace=dict(samples_per_pass=k))
    veil = floor(n_side=5, half=0.8, y=-0.36, seed=8)  # stacked layers: a faint sheet 0.14 above the opaque one, inside the default offset
    veil["opacity"][:] = -1.0                            # of 0.2 (a smaller floor: a ray that starts ON the surface is fragile more often)
    veil["scale"][:, [0, 2]] += np.float32(0.8)
    layers = join(floor(n_side=9, half=0.8), veil)
    c["l09_offset_0"] = _case([(layers, tc.I4)], [point], light=dict(particle_shadow_offset=0.0))
    c["l09_offset_02"] = _case([(layers, tc.I4)], [point], light=dict(particle_shadow_offset=0.2))
    c["l10_behind_light"] = _case([(join(floor(), blob(centre=(0.0, 1.3, 0.0))), tc.I4)], [nl.default_light(position=(0.0, 0.7, 0.0), range=10.0, intensity=2.0)])
    c["l11_materials"] = _case([(floor(), tc.I4), (blob(), tc.trs((1.2, 1.2, 1.2), (0, 1, 0), 30.0, (0.2, 0.0, 0.0))), (blob(seed=11), tc.trs((-1.0, 1.0, 1.0), (0, 1, 0), 0.0, (-0.7, 0.0, 0.3)))],
                               [point], materials=[dict(SHADED, specular=(0.5, 0.5, 0.5), shininess=64.0), nl.default_material(),
                                                   dict(SHADED, diffuse=(0.0, 0.0, 0.0), ambient=(0.6, 0.6, 0.6))])
    # a cloud too thin to reach the iso threshold around a small floor: its pixels are discarded
    c["l12_thin_cloud"] = _case([(join(floor(n_side=6, half=0.5), blob(n=30, centre=(0.0, 0.0, 0.0), radius=1.2, opacity=-3.5, seed=31, log_scale=-2.0)), tc.I4)], [point])
    c["l13_shadows_off"] = _case([(scene, tc.I4)], [point], light=dict(shadows_mode=0))
    c["l14_fisheye_dof"] = _case([(scene, tc.I4)], [point], frame=dict(camera_model=1, fov_rad=1.4, dof_mode=1, focus_dist=2.9, aperture=0.004))
    deep = join(floor(n_side=62, half=1.3, seed=15), blob(n=253, seed=16, radius=0.35, log_scale=-3.3))
    deep["scale"][:62 * 62] += np.log(np.float32(0.14))  # 4097 leaves: the shadow rays walk five levels
    c["l15_deep"] = _case([(deep, tc.I4)], [point], W=33, H=25)
    c["l17_fallback_normal"] = _case([(fins(), tc.I4)], [nl.default_light(position=(0.5, 0.5, 3.0), range=20.0, intensity=3.0, attenuation_mode=0)],
                                     eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0))
    c["l17_fallback_normal"]["P"] = tc.persp(2.0, 48 / 40)
    return c


@functools.lru_cache(maxsize=None)
def restate(name):
    """the restatement of a case from its arrays alone; computed once and shared: do not modify the result"""
    return restate_with(cases()[name], [(ntl.prepare_set(a), M) for a, M in cases()[name]["sets"]])


def restate_with(c, inst):
    L = c["light"]
    return ntl.lit(inst, c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"], shadows=L.get("shadows_mode", 0),
                   offset=L.get("particle_shadow_offset", 0.2), threshold=L.get("particle_shadow_transmittance_threshold", 0.8),
                   strength=L.get("particle_shadow_color_strength", 0.0), **_trace_kw(c))
