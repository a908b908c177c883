"""child process of test_gpu_radiance.py: every frame and ray batch of one storage format in a fresh interpreter.
usage: _child_radiance.py FORMAT OUT.npz   (FORMAT: f32, f16 or u8; SH and rgba are committed in it alike)
Every frame is rendered with MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED into an RGBA32F target; what is kept of it is the pixel under every
splat ("<key>/px" [n,4], the splats in the caller's global order) and the alpha of every pixel of radiance_cases.border_mask()
("<key>/border").  key = <scene>/<pose>/<site>/<frame sh_degree>[/<variant>].  A ray batch keeps radiance, transmittance and hit count."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import vk_gaussian_splatting_amd as mgs  # noqa: E402
from vk_gaussian_splatting_amd import capi, multigpu  # noqa: E402
import radiance_cases as rc  # noqa: E402

fmt, out = sys.argv[1], sys.argv[2]
SITES = ("raster", "gut_packed", "gut_tile", "trace", "shade_hit")
res = {}
border = rc.border_mask()


def build(kind, pose):
    sc = rc.scene(kind, pose)
    scene = mgs.Scene(0)
    for arrays, M in sc["sets"]:
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), M)
    scene.commit(rc.FORMATS[fmt], rc.FORMATS[fmt])
    return scene, sc


def params(sc, sh_degree, flags=4, **over):
    p = capi.default_params(rc.W, rc.H)
    capi.set_camera(p, sc["V"], sc["P"], sc["eye"])
    p.target_format, p.sh_degree, p.debug_flags = capi.TARGET_RGBA32F, sh_degree, flags
    for k, v in over.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def frame(scene, site, p):
    """one frame of a site -> the image [H,W,4] float32"""
    if site in ("raster", "gut_packed", "gut_tile"):
        if site != "raster":
            p.pipeline = capi.PIPELINE_3DGUT
            p.surface_outputs = 1 if site == "gut_tile" else 0
        o = scene.render(p, want_stats=True)
        assert o.error_flags == 0, (site, o.error_flags)
    else:
        t = capi.default_trace_params(trace_strategy=capi.TRACE_STRATEGY_STOCHASTIC_ANYHIT if site == "shade_hit" else capi.TRACE_STRATEGY_FULL_ANYHIT)
        scene.render_traced(p, t, want_stats=True)
    img = scene.download_frame(p)
    assert img.dtype == np.float32 and img.shape == (rc.H, rc.W, 4)
    return img


def keep(key, img, read):
    res[key + "/px"] = img[read[:, 1], read[:, 0]].copy()
    res[key + "/border"] = img[..., 3][border].copy()


for pose in rc.POSE_NAMES:
    scene, sc = build("four", pose)
    read = rc.geometry("four", pose)["read"]
    for site in SITES:
        for deg in range(4):
            keep(f"four/{pose}/{site}/{deg}", frame(scene, site, params(sc, deg)), read)
        if pose == rc.EXTRAS_POSE:
            keep(f"four/{pose}/{site}/3/sh_only", frame(scene, site, params(sc, 3, flags=4 | 2)), read)
    if pose == rc.EXTRAS_POSE:
        # the rasteriser's other instantiations: surface outputs, a bound all-far occluder (with and without them), two strips
        keep(f"four/{pose}/raster/3/surface", frame(scene, "raster", params(sc, 3, surface_outputs=1)), read)
        scene.upload_occluder(np.ones((rc.H, rc.W), np.float32))
        keep(f"four/{pose}/raster/3/occluder", frame(scene, "raster", params(sc, 3)), read)
        keep(f"four/{pose}/raster/3/occluder_surface", frame(scene, "raster", params(sc, 3, surface_outputs=1)), read)
        scene.clear_occluder()
        asm = np.zeros((rc.H, rc.W, 4), np.float32)
        for r in range(2):
            b, e = multigpu.strip_rows(rc.H, 2, r)
            part = frame(scene, "raster", params(sc, 3, strip_row_begin=b, strip_row_end=e))
            asm[16 * b:min(16 * e, rc.H)] = part[16 * b:min(16 * e, rc.H)]
        keep(f"four/{pose}/raster/3/strips", asm, read)
        # the ray queries
        r = rc.rays()
        batch = capi.make_rays(r["origin"], r["direction"])
        for deg, flags, tag in ((0, 4, "0"), (1, 4, "1"), (2, 4, "2"), (3, 4, "3"), (3, 6, "3/sh_only")):
            got, o = scene.trace_rays(batch, params(sc, deg, flags=flags), want_stats=True)
            assert o.invalid_rays == 0
            res[f"rays/{tag}/radiance"], res[f"rays/{tag}/transmittance"], res[f"rays/{tag}/hits"] = got["radiance"], got["transmittance"], got["hit_count"]
    scene.close()

scene, sc = build("twenty", rc.TWENTY_POSE)
read = rc.geometry("twenty", rc.TWENTY_POSE)["read"]
for site in ("raster", "gut_packed", "gut_tile", "trace"):
    for deg in range(4):
        keep(f"twenty/{rc.TWENTY_POSE}/{site}/{deg}", frame(scene, site, params(sc, deg)), read)
scene.close()
np.savez(out, **res)
print("child ok")
