"""Independent restatement of the reference's deferred lighting pass and depth consolidation, in numpy.

Written from shaders/deferred_shading.comp.slang:38-167, shaders/wavefront.h.slang:104-280,388-403 and
shaders/depth_consolidate.frag.slang in their own order of operations, vectorised over the pixels.  float64 by default; `dtype`
switches every arithmetic operation to another format (the CPU test measures float32 against float64 to set the GPU bar).

light_frame() returns the lit image, the consolidated depth and a per-pixel AMBIGUITY MASK: the pixels whose outcome hangs on a
comparison the shader makes and whose operands are within a relative 1e-5 of each other —
  normal.w against 0.001                    (lit or passed through),
  distance against a light's range          (point / spot lights with attenuation mode 0, 2 or 3: the contribution is discontinuous
                                             at the range; mode 1 falls to zero there and is not),
  picked depth against 0.0001 and against D (consolidated depth).
`alt` is the lit image with every such near-threshold comparison decided the other way: inside the mask a pixel may be either.

Conventions: matrices are 4x4 numpy arrays in math (row, col) convention, as capi.set_camera takes them; images are [H, W, ...] with
row 0 = NDC y -1; lights and materials are dicts with the field names of MgsLight / MgsMaterial.
"""
from collections import namedtuple

import numpy as np

REL = 1e-5
INVALID_ID = 0xFFFFFFFF
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = 0, 1, 2

Result = namedtuple("Result", "lit consolidated mask mask_color mask_depth alt shaded")


def default_light(**kw):
    """shaderio::LightSource defaults (wavefront.h:81-93)"""
    d = dict(type=LIGHT_POINT, color=(1.0, 1.0, 1.0), intensity=1.0, position=(0.0, 0.0, 0.0), range=10.0,
             direction=(0.0, 0.0, -1.0), inner_cone_deg=30.0, outer_cone_deg=45.0, attenuation_mode=2)
    d.update(kw)
    return d


def default_material(**kw):
    """the splat sets' default (splat_set_vk.cpp:128-135): fully emissive"""
    d = dict(ambient=(0.0, 0.0, 0.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0), emission=(1.0, 1.0, 1.0), shininess=0.0)
    d.update(kw)
    return d


def need_shading(m):
    """updateMaterialNeedsShading (wavefront.h:55-59), in fp32 like the host code that derives it"""
    ln = lambda v: float(np.sqrt(np.sum(np.asarray(v, np.float32) ** 2, dtype=np.float32)))
    return ln(m["diffuse"]) > 0.001 or ln(m["ambient"]) > 0.001 or ln(m["specular"]) > 0.001


def headlight(camera_pos):
    """createHeadlight (wavefront.h.slang:104-119)"""
    return default_light(type=LIGHT_POINT, position=tuple(camera_pos), range=1e10, attenuation_mode=0, inner_cone_deg=0.0, outer_cone_deg=0.0)


def inverse_f32(m):
    """the inverses are computed in double and rounded once to fp32 (their rounding is parity unpinned)"""
    return np.linalg.inv(np.asarray(m, np.float32).astype(np.float64)).astype(np.float32)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _near(a, b):
    return np.abs(a - b) <= REL * np.abs(b)


def consolidate_depth(picked, occ_depth=None):
    """depth_consolidate.frag.slang: comparisons of fp32 values, hence exact; D = 1.0 (the depth clear) where nothing is bound.
    Returns (depth, ambiguity mask)."""
    p = np.asarray(picked, np.float32)
    D = np.ones_like(p) if occ_depth is None else np.asarray(occ_depth, np.float32)
    out = np.where((p > np.float32(0.0001)) & (p < D), p, D).astype(np.float32)
    mask = _near(p.astype(np.float64), 0.0001) | _near(p.astype(np.float64), D.astype(np.float64))
    return out, mask


def _attenuation(mode, distance, rng, one):
    if mode == 1:
        return one - (distance / rng)
    if mode == 2:
        return one / (one + distance * distance)
    if mode == 3:
        return one / (distance * distance + distance.dtype.type(0.01))
    return np.ones_like(distance)


def _shade_direct(light, world_pos, n, mat, view_dir, radiance, dt, flip):
    """wavefrontComputeShadingDirectOnly (:233-280), inShadow false, transmittance 1.  Returns the range-ambiguity mask."""
    one, zero = dt(1.0), dt(0.0)
    amb = np.zeros(world_pos.shape[:-1], bool)
    radiance += mat["ambient"]  # once per light
    color = np.asarray(light["color"], np.float32).astype(dt)
    inten = dt(np.float32(light["intensity"]))
    ltype = int(light["type"])
    direction = np.asarray(light["direction"], np.float32).astype(dt)
    if ltype == LIGHT_DIRECTIONAL:
        L = np.broadcast_to(-_normalize(direction), world_pos.shape)
        ndotl = np.maximum(_dot(n, L), zero)
        light_diffuse = (color * inten)[None, :] * ndotl[:, None]
    elif ltype in (LIGHT_POINT, LIGHT_SPOT):
        to_light = np.asarray(light["position"], np.float32).astype(dt) - world_pos
        distance = np.sqrt(_dot(to_light, to_light))
        L = _normalize(to_light)
        rng = dt(np.float32(light["range"]))
        mode = int(light["attenuation_mode"])
        outside = distance > rng
        if mode != 1:
            amb = _near(distance, rng)
            if flip:
                outside = outside ^ amb
        att = _attenuation(mode, distance, rng, one)
        ndotl = np.maximum(_dot(n, L), zero)
        if ltype == LIGHT_POINT:
            light_diffuse = ((color * inten)[None, :] * att[:, None]) * ndotl[:, None]
        else:
            spot_dir = _normalize(direction)
            theta = _dot(L, np.broadcast_to(-spot_dir, L.shape))
            rad = lambda deg: dt(np.float32(deg)) * dt(np.pi / 180.0)
            inner_cos, outer_cos = np.cos(rad(light["inner_cone_deg"])), np.cos(rad(light["outer_cone_deg"]))
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.clip((theta - outer_cos) / (inner_cos - outer_cos), zero, one)
            spot = t * t * (dt(3.0) - dt(2.0) * t)
            light_diffuse = (((color * inten)[None, :] * att[:, None]) * spot[:, None]) * ndotl[:, None]
            light_diffuse = np.where((theta < outer_cos)[:, None], zero, light_diffuse)  # continuous: smoothstep is 0 there
        light_diffuse = np.where(outside[:, None], zero, light_diffuse)
    else:
        L = _normalize(np.asarray(light["position"], np.float32).astype(dt) - world_pos)
        light_diffuse = np.zeros_like(world_pos)
    frag_diffuse = mat["diffuse"] * light_diffuse
    # wavefrontComputeSpecular (:388-403)
    k_pi = dt(3.14159265)
    k_sh = np.maximum(mat["shininess"], dt(4.0))
    k_energy = (dt(2.0) + k_sh) / (dt(2.0) * k_pi)
    V = _normalize(-view_dir)
    I = -L
    R = I - dt(2.0) * _dot(n, I)[:, None] * n
    specular = k_energy * np.power(np.maximum(_dot(V, R), zero), k_sh)
    spec = ((mat["specular"] * specular[:, None]) * color[None, :]) * inten
    radiance += frag_diffuse + spec
    return amb


def light_frame(image, depth, ids, normal, view, proj, camera_pos, lights, materials, inst_prefix, occ_depth=None, dtype=np.float64):
    """image float[H,W,4] (the frame as stored in its target format), depth float32[H,W], ids uint32[H,W] (global, instances
    concatenated: inst_prefix[k] = first id of instance k), normal float32[H,W,4]; lights: list of light dicts (empty: headlight);
    materials: one material dict per instance."""
    dt = np.dtype(dtype).type
    H, W = depth.shape
    img = np.asarray(image, np.float32)
    nrm = np.asarray(normal, np.float32)
    w = nrm[..., 3]
    thr = dt(np.float32(0.001)) if dt is np.float32 else dt(0.001)
    shaded = ~(w.astype(dt) < thr)
    mask_w = _near(w.astype(np.float64), 0.001)
    cons, mask_depth = consolidate_depth(depth, occ_depth)

    def run(flip):
        out = img.astype(dt).copy()
        sel = (shaded ^ mask_w) if flip else shaded
        ys, xs = np.nonzero(sel)
        if ys.size == 0:
            return out, np.zeros((H, W), bool)
        n = _normalize(nrm[ys, xs, :3].astype(dt))
        # reconstructWorldPos (:39-50)
        ndc_x = (xs.astype(dt) + dt(0.5)) / dt(W) * dt(2.0) - dt(1.0)
        ndc_y = (ys.astype(dt) + dt(0.5)) / dt(H) * dt(2.0) - dt(1.0)
        clip = np.stack([ndc_x, ndc_y, np.asarray(depth, np.float32)[ys, xs].astype(dt), np.ones(ys.size, dt)], -1)
        pinv, vinv = inverse_f32(proj).astype(dt), inverse_f32(view).astype(dt)
        mulv = lambda v, M: ((v[:, 0:1] * M[:, 0] + v[:, 1:2] * M[:, 1]) + v[:, 2:3] * M[:, 2]) + v[:, 3:4] * M[:, 3]  # mul(v, M) of the shaders == M v
        with np.errstate(divide="ignore", invalid="ignore"):
            vp = mulv(clip, pinv)
            vp = vp / vp[:, 3:4]
            world = mulv(vp, vinv)[:, :3]
            cam = np.asarray(camera_pos, np.float32).astype(dt)
            base = out[ys, xs, :3].copy()
            pid = np.asarray(ids, np.uint32)[ys, xs]
            valid = pid != INVALID_ID
            prefix = np.asarray(inst_prefix, np.int64)
            owner = np.clip(np.searchsorted(prefix, pid.astype(np.int64), side="right") - 1, 0, len(materials) - 1)
            tab = lambda k: np.array([np.asarray(m[k], np.float32) for m in materials], np.float32).astype(dt)[owner]
            v3 = lambda k, d: np.where(valid[:, None], base * tab(k), np.asarray(d, dt) if not isinstance(d, str) else base)
            mat = dict(ambient=v3("ambient", [0.1, 0.1, 0.1]), diffuse=v3("diffuse", "base"), specular=v3("specular", [0.0, 0.0, 0.0]),
                       emission=v3("emission", [0.0, 0.0, 0.0]))
            mat["shininess"] = np.where(valid, np.array([np.float32(m["shininess"]) for m in materials], np.float32).astype(dt)[owner], dt(32.0))
            needs = np.where(valid, np.array([need_shading(m) for m in materials], bool)[owner], True)
            view_dir = _normalize(world - cam)
            color = mat["emission"].copy()
            lit_part = color.copy()
            amb = np.zeros(ys.size, bool)
            for L in (lights if len(lights) else [headlight(np.asarray(camera_pos, np.float32))]):
                amb |= _shade_direct(L, world, n, mat, view_dir, lit_part, dt, flip)
            color = np.where(needs[:, None], lit_part, color)
        out[ys, xs, :3] = color
        out[ys, xs, 3] = dt(1.0)
        m = np.zeros((H, W), bool)
        m[ys, xs] = amb & needs
        return out, m

    lit, mask_range = run(False)
    mask_color = mask_w | mask_range
    alt = lit
    if mask_color.any():
        alt, mr2 = run(True)
        mask_color = mask_color | mr2
    return Result(lit, cons, mask_color | mask_depth, mask_color, mask_depth, alt, shaded)


def to_target(img, target):
    """round a float image to the target format the way the library's kernels store it: 'f32', 'f16' (round to nearest even) or
    'u8' (linear UNORM: clamp, * 255 + 0.5, truncate); returned in the format's own dtype"""
    if target == "f32":
        return np.asarray(img).astype(np.float32)
    if target == "f16":
        with np.errstate(over="ignore"):
            return np.asarray(img).astype(np.float16)
    x = np.clip(np.nan_to_num(np.asarray(img, np.float64), nan=0.0), 0.0, 1.0)
    return np.floor(x.astype(np.float32) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def from_target(img):
    """the float value a stored pixel reads back as"""
    a = np.asarray(img)
    return (a.astype(np.float32) / np.float32(255.0)) if a.dtype == np.uint8 else a.astype(np.float32)
