"""GPU parity tests (-m gpu) of the 3DGUT raster pipeline: unscented-transform projection +
per-pixel particle response, HIP (k_project_gut.hip, k_composite_gut.hip) through the C ABI against the CPU oracle (orc_render_gut_order, restated from
threedgut_raster.{mesh,frag}.slang and cross-checked by an independent float64 restatement in the CPU tests).
Bar: >= 50 dB PSNR and a per-channel absolute tolerance; strips bit-identical to the full frame."""
import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth

pytestmark = pytest.mark.gpu
PSNR_MIN = 50.0
ABS_TOL = 3.0e-2  # one threshold fragment (alpha <= 1/255, response <= 0.0113, quad edge) may flip per pixel


@pytest.fixture(scope="module")
def scene_gut():
    sc = synth.make_scene(60000, seed=21)
    ss = mgs.SplatSet.from_arrays(**sc)
    scene = mgs.Scene(0)
    scene.add_instance(ss)
    scene.commit()
    yield scene, sc
    scene.close()


def setup(pose, W, H, **kw):
    eye = synth.orbit_pose(pose)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H, flip_y=kw.pop("flip", False))
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    p.pipeline = capi.PIPELINE_3DGUT
    for k, v in kw.items():
        setattr(p, k, v)
    return p, V, P, eye


def oracle_frame(ob, scene, sc, p, V, P, eye, W, H, transforms=(None,), **fkw):
    n = sc["positions"].shape[0]
    perm = scene.storage_order(0, n)
    ps_p = ob.PreparedSet({k: v[perm] for k, v in sc.items()})
    inst_p = ob.make_instances([(ps_p, m) for m in transforms])
    # the dist stage of a 3DGUT frame: CAMERA_TYPE selects the cull (dist.comp.slang:64-91), frameInfo.focal is the fisheye focal
    cull_kw = dict(camera_model=fkw.get("camera_model", 0), pipeline_3dgut=1)
    ok, oi = ob.key_cull(ob.make_frame(V, P, eye, W, H, **cull_kw), inst_p)
    oks, ois = ob.sort_stable(ok, oi)
    order = ((ois // n) * n + perm[ois % n]).astype(np.uint32)  # ties in the library's storage order
    inst = ob.make_instances([(ob.PreparedSet(sc), m) for m in transforms])
    fr = ob.make_frame(V, P, eye, W, H, target_fp16=1, **fkw)
    return ob.render_gut(fr, inst, order)


@pytest.mark.parametrize("name,kw,fkw", [
    ("pinhole conic (defaults)", {}, {}),
    ("pinhole eigen", dict(extent_method=capi.EXTENT_EIGEN), dict(extent_method=0)),
    ("conic + mip antialiasing, y flip", dict(ms_antialiasing=1, flip=True), dict(ms_antialiasing=1)),
    ("fisheye", dict(camera_model=capi.CAMERA_FISHEYE), dict(camera_model=1)),
    ("sh degree 1, opacity gaussian disabled", dict(sh_degree=1, debug_flags=4), dict(sh_degree=1, debug_flags=4)),
])
def test_gut_frame_matches_oracle(scene_gut, ob, name, kw, fkw):
    scene, sc = scene_gut
    W, H = 640, 480
    p, V, P, eye = setup(9, W, H, **dict(kw))
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p).astype(np.float32)
    oimg, st = oracle_frame(ob, scene, sc, p, V, P, eye, W, H, **fkw)
    psnr = ob.psnr_rgb(img, oimg)
    err = np.abs(img[..., :3] - oimg[..., :3])
    print(f"3DGUT {name}: PSNR {psnr:.2f} dB, max abs {err.max():.4f}, 99.99th pct {np.percentile(err, 99.99):.5f}, "
          f"sorted {out.sorted_count} oracle quads {st['quads']} fragments {st['fragments']}")
    assert out.error_flags == 0 and out.frustum_count == st["visible"]
    # the oracle counts every emitted quad; the build drops the ones that cover no pixel centre or lie off screen before the sort
    assert int(st["quads"]) * 0.85 <= int(out.sorted_count) <= int(st["quads"]) + 3
    if kw.get("debug_flags", 0) & 4:
        # opacity gaussian disabled: every accepted fragment is opaque, so a fragment on an acceptance threshold (response >
        # 0.0113, alpha > 1/255, quad edge) that falls on the other side changes the whole pixel — the stochastic tests' bar
        same = np.all(err <= 2e-3, axis=-1).mean()
        assert psnr >= PSNR_MIN and same >= 0.999, (psnr, same)
    else:
        assert psnr >= PSNR_MIN and err.max() <= ABS_TOL


def test_gut_two_instances_and_strips(ob):
    sc = synth.make_scene(20000, seed=5)
    ss = mgs.SplatSet.from_arrays(**sc)
    scene = mgs.Scene(0)
    M1, _ = mgs.compute_transform([0.8, 1.2, 1.0], [10.0, 35.0, -5.0], [1.0, 0.1, -0.5])
    scene.add_instance(ss)
    scene.add_instance(ss, M1)
    scene.commit()
    W, H = 800, 450
    p, V, P, eye = setup(3, W, H)
    out = scene.render(p, want_stats=True)
    full16 = scene.download_frame(p).view(np.uint16).copy()
    img = full16.view(np.float16).astype(np.float32)
    oimg, st = oracle_frame(ob, scene, sc, p, V, P, eye, W, H, transforms=(None, M1))
    psnr = ob.psnr_rgb(img, oimg)
    print(f"3DGUT two instances: PSNR {psnr:.2f} dB, max abs {np.abs(img[..., :3] - oimg[..., :3]).max():.4f}")
    assert out.error_flags == 0 and psnr >= PSNR_MIN
    # determinism + strips == full frame (the multi-GPU partition applies to this pipeline unchanged)
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), full16)
    for b, e in ((0, 7), (7, 20), (20, 29)):
        p.strip_row_begin, p.strip_row_end = b, e
        scene.render(p)
        part = scene.download_frame(p).view(np.uint16)
        y0, y1 = b * 16, min(e * 16, H)
        assert np.array_equal(part[y0:y1], full16[y0:y1]), (b, e)
    p.strip_row_begin, p.strip_row_end = 0, 0
    # the 3DGS pipeline on the same scene object still renders its own frame (separate record buffers)
    p.pipeline = capi.PIPELINE_3DGS
    o3 = scene.render(p, want_stats=True)
    assert o3.error_flags == 0
    p.pipeline = capi.PIPELINE_3DGUT
    scene.close()


@pytest.mark.parametrize("pipeline,expected", [(capi.PIPELINE_3DGS, "expected_rgba16f.npy"), (capi.PIPELINE_3DGUT, "expected_3dgut_rgba16f.npy")])
def test_vulkan_reproducible_fixture_on_the_gpu(ob, pipeline, expected):
    """the committed .ply + .vkgs project (tests/golden/vkrepro — the inputs a Vulkan box can hand to the reference) through
    the product's loader and both pipelines, against the committed expected frames"""
    import os
    from conftest import GOLDEN
    from vk_gaussian_splatting_amd import project
    d = os.path.join(GOLDEN, "vkrepro")
    pr = project.load_project(os.path.join(d, "repro.vkgs"))
    scene = pr.build_scene(0)
    want = np.load(os.path.join(d, expected)).astype(np.float32)
    H, W = want.shape[:2]
    p = pr.frame_params(W, H)
    p.pipeline = pipeline
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p).astype(np.float32)
    psnr = ob.psnr_rgb(img, want)
    print(f"vkrepro pipeline {pipeline}: PSNR {psnr:.2f} dB")
    assert out.error_flags == 0 and psnr >= PSNR_MIN and np.abs(img[..., :3] - want[..., :3]).max() <= ABS_TOL
    scene.close()


@pytest.mark.parametrize("case", ["u8_storage", "fisheye150_3dgut", "msaa_3dgs", "two_instances_trs"])
def test_vulkan_reproducible_cases_on_the_gpu(ob, case):
    """tests/golden/vkrepro/<case>/repro.vkgs through the product (project reader, loader, commit formats, instances, camera
    model, pipeline) against the committed expected frame of the case"""
    import json
    import os
    from conftest import GOLDEN
    from vk_gaussian_splatting_amd import project
    d = os.path.join(GOLDEN, "vkrepro", case)
    pr = project.load_project(os.path.join(d, "repro.vkgs"))
    cj = json.load(open(os.path.join(d, "camera.json")))
    scene = pr.build_scene(0)
    want = np.load(os.path.join(d, "expected_rgba16f.npy")).astype(np.float32)
    H, W = want.shape[:2]
    p = pr.frame_params(W, H)
    p.ms_antialiasing = int(cj["frame"]["msAntialiasing"])  # a UI setting of the reference: not part of the project file
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p).astype(np.float32)
    psnr = ob.psnr_rgb(img, want)
    print(f"vkrepro case {case}: PSNR {psnr:.2f} dB, sorted {out.sorted_count}")
    assert out.error_flags == 0 and psnr >= PSNR_MIN and np.abs(img[..., :3] - want[..., :3]).max() <= ABS_TOL
    scene.close()


def test_gut_surface_outputs_match_oracle(scene_gut, ob):
    """NEED_SURFACE_INFO in the 3DGUT pipeline (threedgut_raster.frag.slang:127-131,195-228): picked depth, the splat that set
    it, the integrated normal; the frame itself is unchanged by the side outputs.  The pick is a threshold test on T: >= 99.5 %
    of the pixels must pick the same splat."""
    scene, sc = scene_gut
    W, H = 640, 400
    p, V, P, eye = setup(4, W, H)
    scene.render(p)
    plain = scene.download_frame(p).copy()
    p.surface_outputs = 1
    p.depth_iso_threshold = 0.6
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    # the side outputs run in the compositor's XT variant (another instantiation: the compiler contracts its arithmetic
    # differently), so the frame may differ from the plain one in the last bits of fp16 — not more
    dframe = np.abs(scene.download_frame(p).astype(np.float32) - plain.astype(np.float32)).max()
    assert dframe <= 5e-3, dframe
    depth, ids, nrm = scene.download_surface(p, normals=True)
    n = sc["positions"].shape[0]
    perm = scene.storage_order(0, n)
    ps_p = ob.PreparedSet({k: v[perm] for k, v in sc.items()})
    inst_p = ob.make_instances([(ps_p, None)])
    ok, oi = ob.key_cull(ob.make_frame(V, P, eye, W, H), inst_p)
    _, ois = ob.sort_stable(ok, oi)
    order = perm[ois].astype(np.uint32)     # caller ids, far to near, ties in storage order
    inst = ob.make_instances([(ob.PreparedSet(sc), None)])
    od, oid, on = ob.render_surface_gut(ob.make_frame(V, P, eye, W, H), inst, order[::-1].copy(), 0.6, normals=True)
    same = ids == oid
    err = np.abs(nrm - on)
    print(f"3DGUT surface outputs: frame vs plain max abs {dframe:.2e}, same pick {same.mean():.5f}, normal max abs {err.max():.4f} mean {err.mean():.2e}, "
          f"covered {(ids != 0xFFFFFFFF).mean():.3f}")
    assert same.mean() >= 0.995
    assert np.allclose(depth[same], od[same], rtol=2e-6, atol=2e-7)
    assert (ids != 0xFFFFFFFF).any() and ((depth == 0) == (ids == 0xFFFFFFFF)).all()
    assert err.max() < 3e-2 and err.mean() < 3e-5 and np.quantile(err, 0.9999) < 3e-4
    img = scene.download_frame(p).astype(np.float32)
    assert np.allclose(nrm[..., 3], img[..., 3], atol=1e-3)
    # strips reproduce the side outputs of the full frame
    p.strip_row_begin, p.strip_row_end = 5, 14
    scene.render(p)
    d2, i2 = scene.download_surface(p)
    assert np.array_equal(i2[80:224], ids[80:224]) and np.array_equal(d2[80:224], depth[80:224])


@pytest.mark.parametrize("thin", [1e-6, 0.02])
def test_gut_iso_surface_normals_match_oracle(scene_gut, ob, thin):
    """NORMAL_METHOD_ISO_SURFACE (shaderio.h:126-128; threedgrt.h.slang:330-335 -> computeEllipsoidNormal :423-497): the fragment's
    normal is the normal of the 3-sigma kernel ellipsoid where the pixel's ray enters it, per pixel; picks and depth are those of
    the max-density method, the integrated normal differs from it.  thin = 0.02 makes many particles flat (one small axis ->
    the axis normal) or degenerate (two -> minus the ray)."""
    scene, sc = scene_gut
    W, H = 480, 320
    p, V, P, eye = setup(4, W, H)
    p.surface_outputs = 1
    p.depth_iso_threshold = 0.6
    p.thin_particle_threshold = thin
    scene.render(p)
    d0, i0, n0 = scene.download_surface(p, normals=True)
    p.normal_method = capi.NORMAL_ISO_SURFACE
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    depth, ids, nrm = scene.download_surface(p, normals=True)
    assert np.array_equal(ids, i0) and np.array_equal(depth, d0)   # the normal method does not touch the pick
    assert np.abs(nrm[..., :3] - n0[..., :3]).max() > 0.05         # ... but it is another normal
    n = sc["positions"].shape[0]
    perm = scene.storage_order(0, n)
    ps_p = ob.PreparedSet({k: v[perm] for k, v in sc.items()})
    inst_p = ob.make_instances([(ps_p, None)])
    ok, oi = ob.key_cull(ob.make_frame(V, P, eye, W, H), inst_p)
    _, ois = ob.sort_stable(ok, oi)
    order = perm[ois].astype(np.uint32)
    inst = ob.make_instances([(ob.PreparedSet(sc), None)])
    od, oid, on = ob.render_surface_gut(ob.make_frame(V, P, eye, W, H, normal_method=1), inst, order[::-1].copy(), 0.6,
                                        thin_particle_threshold=thin, normals=True)
    err = np.abs(nrm - on)
    print(f"3DGUT iso-surface normals (thin {thin}): max abs {err.max():.4f} mean {err.mean():.2e} q99.99 {np.quantile(err, 0.9999):.2e}, "
          f"vs max-density method max {np.abs(nrm[..., :3] - n0[..., :3]).max():.3f}")
    assert (ids == oid).mean() >= 0.995
    # max / mean as for the max-density normals (test_gut_surface_outputs_match_oracle: a fragment at the acceptance threshold may
    # be in on one side and out on the other).  The tail is wider here: the oracle follows the shader's b^2 - 4ac, whose
    # cancellation in fp32 moves a single fragment's normal by up to 5e-3 against float64
    # (test_gut_iso_surface_normal_against_the_quadric_gradient); the kernel's closest-approach form does not have it
    assert err.max() < 3e-2 and err.mean() < 3e-5 and np.quantile(err, 0.9999) < 5e-3
    # the integrated normal of a covered pixel is (nearly) a unit vector scaled by the coverage
    cov = nrm[..., 3]
    m = cov > 0.9
    assert m.any() and np.all(np.linalg.norm(nrm[m][:, :3], axis=1) <= cov[m] + 1e-3)
    p.normal_method = 7
    with pytest.raises(Exception):
        scene.render(p)


@pytest.mark.parametrize("pipeline", [capi.PIPELINE_3DGUT, capi.PIPELINE_3DGS])
@pytest.mark.parametrize("fov,eye", [(100.0, None), (150.0, (0.45, 0.15, 0.3)), (170.0, (0.0, 0.2, -0.4))])
def test_fisheye_dist_stage_cull_bit_exact(scene_gut, ob, pipeline, fov, eye):
    """CAMERA_TYPE == CAMERA_FISHEYE in the dist stage (dist.comp.slang:75-90): survivors are chosen by projectPointFisheye's
    validity (cone of maxAngle + image rectangle with the 0.1 margin) and the z test, not by the NDC box.  Wide fields of view
    and cameras inside the cloud, where the two culls differ by thousands of splats: keys and ids bit-exact vs the oracle
    (which shares the fixed-polynomial atan2), the frame >= 50 dB.  On a 3DGS pipeline frameInfo.focal stays the pinhole focal
    (gaussian_splatting.cpp:1239-1251) and the raster is the pinhole one: only the sorted set changes."""
    scene, sc = scene_gut
    n = sc["positions"].shape[0]
    W, H = 640, 480
    e = np.asarray(eye if eye is not None else synth.orbit_pose(7), np.float32)
    ctr = [0, 0, 0] if eye is None else [e[0] + 0.3, e[1] - 0.1, e[2] + 1.0]
    V, P = mgs.camera_lookat_perspective(e, ctr, [0, 1, 0], fov, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, e)
    p.pipeline, p.camera_model = pipeline, capi.CAMERA_FISHEYE
    gut = pipeline == capi.PIPELINE_3DGUT
    perm = scene.storage_order(0, n)
    inst_p = ob.make_instances([(ob.PreparedSet({k: v[perm] for k, v in sc.items()}), None)])
    fish = ob.make_frame(V, P, e, W, H, camera_model=1, pipeline_3dgut=int(gut))
    ok, oi = ob.key_cull(fish, inst_p)
    oks, ois = ob.sort_stable(ok, oi)
    so = scene.sort_keys(p)
    gk, gi = scene.sort_download(so.count)
    assert so.count == oks.size and np.array_equal(gk, oks) and np.array_equal(gi, perm[ois])
    # the pinhole box keeps a different set
    pk, pi = ob.key_cull(ob.make_frame(V, P, e, W, H), inst_p)
    only_fish, only_pin = np.setdiff1d(oi, pi).size, np.setdiff1d(pi, oi).size
    print(f"fisheye cull fov {fov} pipeline {pipeline}: {oi.size} survivors, {only_fish} not in the pinhole set, {only_pin} only in it")
    assert only_fish + only_pin > 100
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0 and out.frustum_count == oks.size
    img = scene.download_frame(p).astype(np.float32)
    inst = ob.make_instances([(ob.PreparedSet(sc), None)])
    order = perm[ois].astype(np.uint32)
    if gut:
        oimg, st = ob.render_gut(ob.make_frame(V, P, e, W, H, target_fp16=1, camera_model=1, pipeline_3dgut=1), inst, order)
    else:
        oimg, st = ob.render(ob.make_frame(V, P, e, W, H, target_fp16=1, camera_model=1), inst, order=order)
    psnr = ob.psnr_rgb(img, oimg)
    print(f"  frame PSNR {psnr:.2f} dB, sorted {out.sorted_count}, oracle quads {st['quads']}")
    assert psnr >= PSNR_MIN
    # strips == full frame with the fisheye cull (partition culling must stay conservative for it)
    full16 = scene.download_frame(p).view(np.uint16).copy()
    for b, en in ((0, 9), (9, 30)):
        p.strip_row_begin, p.strip_row_end = b, en
        scene.render(p)
        part = scene.download_frame(p).view(np.uint16)
        assert np.array_equal(part[b * 16:min(en * 16, H)], full16[b * 16:min(en * 16, H)]), (b, en)
