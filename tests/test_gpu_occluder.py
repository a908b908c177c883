"""GPU tests (-m gpu) of the occluder: splats depth-tested against the caller's depth image, the caller's colour behind
them (mgs_frame_set_occluder).  Correctness is always against the CPU oracle: the oracle has no depth test, so the
expected frame is assembled per depth LEVEL from oracle renders of the filtered draw order (occluder_levels.py); the
library is compared with itself only where the subject is plumbing (strips, graph replay, binding)."""
import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth
import occluder_levels as ol

pytestmark = pytest.mark.gpu

PSNR_MIN = 55.0   # the bars of tests/test_gpu_parity.py for frames against the oracle
ABS_TOL = 2.5e-2
GUT_PSNR_MIN = 50.0   # ... and of tests/test_gpu_gut.py
GUT_ABS_TOL = 3.0e-2
N = 60000


@pytest.fixture(scope="module")
def scene_occ():
    sc = synth.make_scene(N, seed=21)
    ss = mgs.SplatSet.from_arrays(**sc)
    scene = mgs.Scene(0)
    scene.add_instance(ss)
    scene.commit()
    yield scene, sc
    scene.close()


def camera(i, W, H):
    eye = synth.orbit_pose(i)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    return p, V, P, eye


def sorted_stream(ob, scene, sets, V, P, eye, W, H, **fkw):
    """the oracle's sorted stream far to near (ties in the library's storage order): (caller's ids, ndc z of each entry)"""
    insts = [(sc, scene.storage_order(i, sc["positions"].shape[0]), m) for i, (sc, m) in enumerate(sets)]
    oks, ois, _, _ = ob.storage_sorted_stream(ob.make_frame(V, P, eye, W, H, **fkw), insts)
    return ois, ol.depths_of_btf_keys(oks)


def check_frame(ob, img, exp, what, psnr_min=PSNR_MIN, abs_tol=ABS_TOL, alpha_rel=False):
    img = img.astype(np.float32)
    pr = ob.psnr_rgb(img, exp)
    e_rgb = float(np.abs(img[..., :3] - exp[..., :3]).max())
    ea = np.abs(img[..., 3] - exp[..., 3])
    if alpha_rel:  # MGS_ALPHA_SUM: the sum is unbounded (test_alpha_sum_mode_and_fp32_target's bar)
        ea = ea / np.maximum(exp[..., 3], 1.0)
    print(f"occluder {what}: PSNR {pr:.2f} dB, max abs rgb {e_rgb:.5f}, alpha {float(ea.max()):.5f}")
    assert pr >= psnr_min, (what, pr)
    assert e_rgb <= abs_tol, (what, e_rgb)
    assert float(ea.max()) <= (2e-2 if alpha_rel else abs_tol), (what, float(ea.max()))


class OracleCache:
    """oracle renders of a filtered order, shared by the cases of one (pose, size)"""

    def __init__(self, ob, inst, V, P, eye, W, H, render="render", **fkw):
        self.ob, self.inst, self.cam, self.fkw, self.fn, self.memo = ob, inst, (V, P, eye, W, H), fkw, getattr(ob, render), {}

    def _run(self, order, **kw):
        key = (order.tobytes(), tuple(sorted(kw.items())))
        if key not in self.memo:
            fr = self.ob.make_frame(*self.cam, **dict(self.fkw, **kw))
            self.memo[key] = self.fn(fr, self.inst, order)[0] if self.fn is not self.ob.render else self.fn(fr, self.inst, order=order)[0]
        return self.memo[key]

    def btf(self, fp16):
        return lambda o: self._run(o, target_fp16=fp16)

    def ftb(self):
        return lambda o: self._run(o, front_to_back=1)


# ---- 1. level images that align with nothing --------------------------------------------------------------------------
@pytest.mark.parametrize("pose,W,H", [(3, 640, 480), (30, 333, 217)])
def test_level_images_match_the_oracle(scene_occ, ob, pose, W, H):
    scene, sc = scene_occ
    p, V, P, eye = camera(pose, W, H)
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)  # asserts the gaps, "everything hidden" and "nothing hidden" on the CPU
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H)
    images = {"checkerboard": ol.checkerboard(W, H, levels), "diagonal": ol.diagonal(W, H, levels[2], levels[4])}
    bg = ol.random_background(W, H, seed=pose)
    for name, depth in images.items():
        for back in (None, bg):
            for fmt, fp16 in ((capi.TARGET_RGBA32F, 0), (capi.TARGET_RGBA16F, 1)):
                p.target_format = fmt
                scene.upload_occluder(depth, back)
                out = scene.render(p, want_stats=True)
                img = scene.download_frame(p)
                assert out.error_flags == 0
                exp = ol.expected_frame(oc.btf(fp16), oc.ftb(), order, z, depth, back)
                check_frame(ob, img, exp, f"{name} {W}x{H} bg={back is not None} fp16={fp16}")
    scene.clear_occluder()


# ---- 2. alpha sum, raster knobs, storage formats ----------------------------------------------------------------------
def test_alpha_sum_with_background_alpha(scene_occ, ob):
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(12, W, H)
    p.alpha_mode, p.target_format = capi.ALPHA_SUM, capi.TARGET_RGBA32F
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    depth = ol.checkerboard(W, H, levels)
    bg = ol.random_background(W, H, seed=2)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H)
    scene.upload_occluder(depth, bg)
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p)
    scene.clear_occluder()
    assert out.error_flags == 0
    exp = ol.expected_frame(oc.btf(0), oc.ftb(), order, z, depth, bg, alpha_sum=True)
    check_frame(ob, img, exp, "alpha sum", psnr_min=PSNR_MIN, alpha_rel=True)
    hidden = depth == 0.0
    assert np.array_equal(img[hidden], bg[hidden])  # nothing passed: the geometry itself, its alpha included


@pytest.mark.parametrize("kw", [dict(ms_antialiasing=1), dict(debug_flags=4)])
def test_raster_knobs_with_an_occluder(scene_occ, ob, kw):
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(20, W, H)
    for k, v in kw.items():
        setattr(p, k, v)
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    depth = ol.checkerboard(W, H, levels)
    bg = ol.random_background(W, H, seed=3)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H, **kw)
    scene.upload_occluder(depth, bg)
    scene.render(p)
    img = scene.download_frame(p).astype(np.float32)
    scene.clear_occluder()
    exp = ol.expected_frame(oc.btf(1), oc.ftb(), order, z, depth, bg)
    if kw.get("debug_flags", 0) & 4:
        # every accepted fragment is opaque: one on a discard threshold that falls on the other side changes the whole pixel —
        # the bar of the same knob in tests/test_gpu_parity.py::test_raster_knobs_match_oracle (45 dB)
        same = np.all(np.abs(img - exp) <= ABS_TOL, axis=-1).mean()
        pr = ob.psnr_rgb(img, exp)
        print(f"occluder opacity gaussian disabled: PSNR {pr:.2f} dB, {same:.5f} of the pixels within {ABS_TOL}")
        assert pr >= 45.0, pr
    else:
        check_frame(ob, img, exp, str(kw))


@pytest.mark.parametrize("shf,rgbaf", [(capi.FORMAT_FLOAT16, capi.FORMAT_FLOAT16), (capi.FORMAT_UINT8, capi.FORMAT_UINT8)])
def test_storage_formats_with_an_occluder(ob, shf, rgbaf):
    sc = synth.make_scene(20000, seed=8)
    scene = mgs.Scene(0)
    scene.add_instance(mgs.SplatSet.from_arrays(**sc))
    scene.commit(shf, rgbaf)
    W, H = 320, 240
    p, V, P, eye = camera(7, W, H)
    perm = scene.storage_order(0, 20000)
    oks, order, _, _ = ob.storage_sorted_stream(ob.make_frame(V, P, eye, W, H), [(sc, perm, None)], shf, rgbaf)
    z = ol.depths_of_btf_keys(oks)
    levels = ol.pick_levels(z)
    depth = ol.checkerboard(W, H, levels)
    bg = ol.random_background(W, H, seed=4)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc, shf, rgbaf), None)]), V, P, eye, W, H)
    scene.upload_occluder(depth, bg)
    scene.render(p)
    img = scene.download_frame(p)
    exp = ol.expected_frame(oc.btf(1), oc.ftb(), order, z, depth, bg)
    check_frame(ob, img, exp, f"storage sh {shf} rgba {rgbaf}")  # the oracle quantises the same way: the fp32 bar holds
    scene.close()


# ---- 3. surface outputs -----------------------------------------------------------------------------------------------
def test_surface_outputs_with_an_occluder(scene_occ, ob):
    scene, sc = scene_occ
    W, H = 640, 360
    p, V, P, eye = camera(11, W, H)
    p.surface_outputs, p.depth_iso_threshold = 1, 0.7
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    dimg = ol.checkerboard(W, H, levels)
    scene.upload_occluder(dimg)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    depth, ids, nrm = scene.download_surface(p, normals=True)
    scene.clear_occluder()
    inst = ob.make_instances([(ob.PreparedSet(sc), None)])
    odepth, oids, onrm = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint32), np.zeros((H, W, 4), np.float32)
    for L in levels:
        keep = order[z <= L]
        d, i, n = ob.render_surface(ob.make_frame(V, P, eye, W, H), inst, keep[::-1].copy(), 0.7, normals=True)
        m = dimg == L
        odepth[m], oids[m], onrm[m] = d[m], i[m], n[m]
    same = ids == oids
    print(f"occluder surface outputs: {same.mean():.5f} same picks")
    assert same.mean() >= 0.995, same.mean()  # the bars of test_surface_side_outputs_match_oracle / test_integrated_normal_matches_oracle
    assert np.allclose(depth[same], odepth[same], rtol=1e-6, atol=1e-7)
    hidden = dimg == 0.0
    assert (ids[hidden] == 0xFFFFFFFF).all() and (depth[hidden] == 0).all() and (nrm[hidden] == 0).all()
    err = np.abs(nrm - onrm)
    assert err.max() < 2e-2 and err.mean() < 2e-5 and np.quantile(err, 0.9999) < 2e-4, (err.max(), err.mean())
    # a picked splat never lies behind the pixel's depth
    zid = np.full(N, np.inf, np.float32)
    zid[order] = z
    picked = ids != 0xFFFFFFFF
    assert (zid[ids[picked]] <= dimg[picked]).all()


# ---- 4. 3DGUT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,fkw", [("pinhole", {}, {}), ("fisheye", dict(camera_model=capi.CAMERA_FISHEYE), dict(camera_model=1))])
def test_gut_with_an_occluder(scene_occ, ob, name, kw, fkw):
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(9, W, H)
    p.pipeline = capi.PIPELINE_3DGUT
    for k, v in kw.items():
        setattr(p, k, v)
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H, pipeline_3dgut=1, **fkw)
    levels = ol.pick_levels(z)
    depth = ol.checkerboard(W, H, [levels[0], levels[2], levels[4]])
    bg = ol.random_background(W, H, seed=5)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H, render="render_gut", **fkw)
    scene.upload_occluder(depth, bg)
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p)
    scene.clear_occluder()
    assert out.error_flags == 0
    exp = ol.expected_frame(oc.btf(1), oc.ftb(), order, z, depth, bg)
    check_frame(ob, img, exp, f"3DGUT {name}", psnr_min=GUT_PSNR_MIN, abs_tol=GUT_ABS_TOL)


# ---- 5. two instances, unified order ----------------------------------------------------------------------------------
def test_two_instances_with_an_occluder(ob):
    sc = synth.make_scene(20000, seed=42)
    M1, _ = capi.compute_transform([0.8, 0.8, 0.8], [0.0, 35.0, 10.0], [0.6, 0.1, -0.4])
    scene = mgs.Scene(0)
    ss = mgs.SplatSet.from_arrays(**sc)
    scene.add_instance(ss)
    scene.add_instance(ss, M1)
    scene.commit()
    W, H = 333, 217
    p, V, P, eye = camera(14, W, H)
    order, z = sorted_stream(ob, scene, [(sc, None), (sc, M1)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    depth = ol.checkerboard(W, H, levels)
    bg = ol.random_background(W, H, seed=6)
    ps = ob.PreparedSet(sc)
    oc = OracleCache(ob, ob.make_instances([(ps, None), (ps, M1)]), V, P, eye, W, H)
    scene.upload_occluder(depth, bg)
    out = scene.render(p, want_stats=True)
    img = scene.download_frame(p)
    assert out.error_flags == 0
    exp = ol.expected_frame(oc.btf(1), oc.ftb(), order, z, depth, bg)
    check_frame(ob, img, exp, "two instances")
    scene.close()


# ---- 6. CPU-async order: per-fragment test only, no early stop --------------------------------------------------------
def test_cpu_async_sort_with_an_occluder(scene_occ, ob):
    """the cross-check of the early stop: the same level image under an order that is NOT monotone in ndc z.  The bar is
    test_cpu_async_sort_mode's (std::sort is not stable: the tie order may differ from the oracle's run)."""
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(6, W, H)
    gorder, gz = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    # depth of every splat by id: the oracle's keys of the same frame made without the dist-stage cull (the CPU order draws
    # every splat and culls at raster)
    ok, oi = ob.key_cull(ob.make_frame(V, P, eye, W, H, frustum_culling=2), ob.make_instances([(ob.PreparedSet(sc), None)]))
    assert oi.size == N
    zid = np.zeros(N, np.float32)
    zid[oi] = ol.depths_of_btf_keys(ok)
    # the levels lie in gaps of ALL the depths drawn, not only of the dist-stage survivors'
    inside = zid[(zid > 0.0) & (zid <= 1.0)]
    levels = ol.pick_levels(inside)
    ol.assert_levels_in_gaps(zid[np.isfinite(zid)], levels)
    assert np.isin(gz, inside).all()
    fwd = -np.array([V[2, 0], V[2, 1], V[2, 2]], np.float32)
    _, oidx, _, _ = ob.cpu_sort(fwd, eye, [(sc["positions"], None)])
    depth = ol.checkerboard(W, H, levels)
    bg = ol.random_background(W, H, seed=7)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H, frustum_culling=2)
    exp = ol.expected_frame(oc.btf(1), oc.ftb(), oidx, zid[oidx], depth, bg)
    scene.upload_occluder(depth, bg)
    p.sort_mode, p.cpu_sort_blocking = capi.SORT_CPU_ASYNC, 1
    scene.render(p)
    img = scene.download_frame(p).astype(np.float32)
    pr = ob.psnr_rgb(img, exp)
    print(f"occluder CPU-async order: PSNR {pr:.2f} dB")
    assert pr >= 45.0
    # ... and the GPU-sorted frame (early stop on) of the same images agrees with the same oracle frames
    p.sort_mode = capi.SORT_GPU_RADIX
    scene.render(p)
    img2 = scene.download_frame(p)
    scene.clear_occluder()
    oc2 = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H)
    check_frame(ob, img2, ol.expected_frame(oc2.btf(1), oc2.ftb(), gorder, gz, depth, bg), "GPU order, same images")


# ---- 7. identities (plumbing) -----------------------------------------------------------------------------------------
def test_trivial_depths_are_identities(scene_occ):
    scene, sc = scene_occ
    for W, H in ((640, 480), (333, 217)):
        for fmt in (capi.TARGET_RGBA16F, capi.TARGET_RGBA32F, capi.TARGET_RGBA8):
            p, V, P, eye = camera(3, W, H)
            p.target_format = fmt
            scene.clear_occluder()
            scene.render(p)
            plain = scene.download_frame(p).copy()
            scene.upload_occluder(np.ones((H, W), np.float32))
            out = scene.render(p, want_stats=True)
            assert out.error_flags == 0
            assert np.array_equal(scene.download_frame(p).view(np.uint8), plain.view(np.uint8)), (W, H, fmt)
            scene.upload_occluder(np.zeros((H, W), np.float32))
            out = scene.render(p, want_stats=True)
            assert out.error_flags == 0 and not scene.download_frame(p).any()
            bg = ol.random_background(W, H, seed=9)
            scene.upload_occluder(np.zeros((H, W), np.float32), bg)
            out = scene.render(p, want_stats=True)
            got = scene.download_frame(p)
            assert out.error_flags == 0
            if fmt == capi.TARGET_RGBA32F:
                assert np.array_equal(got[..., :3], bg[..., :3]) and not got[..., 3].any()
            elif fmt == capi.TARGET_RGBA16F:
                assert np.array_equal(got[..., :3], bg[..., :3].astype(np.float16)) and not got[..., 3].any()
            # a NaN depth passes nothing
            scene.upload_occluder(np.full((H, W), np.nan, np.float32))
            scene.render(p)
            assert not scene.download_frame(p).any()
    scene.clear_occluder()


def _wall(scene, ob, sc, p, V, P, eye, W, H):
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    return ol.checkerboard(W, H, levels), ol.random_background(W, H, seed=10)


def test_strips_and_graph_replay_with_an_occluder(scene_occ, ob):
    scene, sc = scene_occ
    W, H = 333, 217
    for mode in (dict(), dict(alpha_mode=capi.ALPHA_SUM), dict(surface_outputs=1), dict(pipeline=capi.PIPELINE_3DGUT)):
        p, V, P, eye = camera(17, W, H)
        for k, v in mode.items():
            setattr(p, k, v)
        depth, bg = _wall(scene, ob, sc, p, V, P, eye, W, H)
        scene.upload_occluder(depth, bg)
        scene.render(p)
        full = scene.download_frame(p).view(np.uint16).copy()
        # plain launches (timed frames are not replayed from a graph) == the replayed graph
        p.collect_timings = 1
        scene.render(p)
        assert np.array_equal(scene.download_frame(p).view(np.uint16), full), mode
        p.collect_timings = 0
        rows = (H + 15) // 16
        got = np.zeros_like(full)
        for r0, r1 in ((0, 3), (3, 4), (4, rows)):  # three uneven strips
            p.strip_row_begin, p.strip_row_end = r0, r1
            scene.render(p)
            s = scene.download_frame(p).view(np.uint16)
            got[r0 * 16:min(r1 * 16, H)] = s[r0 * 16:min(r1 * 16, H)]
        assert np.array_equal(got, full), mode
    scene.clear_occluder()


def test_bind_rebind_unbind_and_contexts(scene_occ, ob):
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(25, W, H)
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    oc = OracleCache(ob, ob.make_instances([(ob.PreparedSet(sc), None)]), V, P, eye, W, H)
    ctx = scene.frame_context()
    ctx.render(p)
    ctx_plain = ctx.download_frame(p).copy()
    d1, d2 = ol.checkerboard(W, H, levels), ol.diagonal(W, H, levels[1], levels[3])
    bg = ol.random_background(W, H, seed=11)
    frames = []
    for _ in range(2):  # twice: the second round replays the captured graphs
        scene.upload_occluder(d1, bg)
        scene.render(p)
        a = scene.download_frame(p).copy()
        scene.upload_occluder(d2)
        scene.render(p)
        b = scene.download_frame(p).copy()
        scene.clear_occluder()
        scene.render(p)
        c = scene.download_frame(p).copy()
        frames.append((a, b, c))
    for x, y in zip(frames[0], frames[1]):
        assert np.array_equal(x.view(np.uint16), y.view(np.uint16))
    a, b, c = frames[0]
    check_frame(ob, a, ol.expected_frame(oc.btf(1), oc.ftb(), order, z, d1, bg), "bound")
    check_frame(ob, b, ol.expected_frame(oc.btf(1), oc.ftb(), order, z, d2, None), "re-bound")
    check_frame(ob, c, ol.expected_frame(oc.btf(1), oc.ftb(), order, z, np.ones((H, W), np.float32), None), "unbound")
    assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)
    assert np.array_equal(c.view(np.uint16), ctx_plain.view(np.uint16))
    # a second context with nothing bound is unaffected by the scene's binding; its own binding is its own
    scene.upload_occluder(d1, bg)
    ctx.render(p)
    assert np.array_equal(ctx.download_frame(p).view(np.uint16), ctx_plain.view(np.uint16))
    ctx.upload_occluder(d2)
    ctx.render(p)
    assert np.array_equal(ctx.download_frame(p).view(np.uint16), b.view(np.uint16))
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), a.view(np.uint16))
    ctx.close()
    scene.clear_occluder()


def test_caller_owned_images_are_read_every_frame(scene_occ, ob):
    """device images bound once; their contents rewritten between frames without re-binding"""
    import torch
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(25, W, H)
    order, z = sorted_stream(ob, scene, [(sc, None)], V, P, eye, W, H)
    levels = ol.pick_levels(z)
    d1, d2 = ol.checkerboard(W, H, levels), ol.diagonal(W, H, levels[1], levels[3])
    bg = ol.random_background(W, H, seed=12)
    td, tc = torch.from_numpy(d1).cuda(), torch.from_numpy(bg).cuda()
    torch.cuda.synchronize()
    scene.set_occluder(td.data_ptr(), tc.data_ptr(), W, H)
    scene.render(p)
    a = scene.download_frame(p).copy()
    scene.upload_occluder(d1, bg)
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), a.view(np.uint16))
    scene.set_occluder(td.data_ptr(), tc.data_ptr(), W, H)
    scene.sync()
    td.copy_(torch.from_numpy(d2).cuda())
    torch.cuda.synchronize()
    scene.render(p)
    b = scene.download_frame(p).copy()
    scene.upload_occluder(d2, bg)
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), b.view(np.uint16))
    assert not np.array_equal(a, b)
    scene.clear_occluder()
    scene.sync()


# ---- 8. errors --------------------------------------------------------------------------------------------------------
def test_occluder_errors(scene_occ):
    scene, sc = scene_occ
    W, H = 320, 240
    p, V, P, eye = camera(4, W, H)
    scene.upload_occluder(np.ones((H // 2, W), np.float32))
    with pytest.raises(mgs.MgsError) as e:
        scene.render(p)
    assert e.value.code == -1 and "occluder" in str(e.value)  # MGS_ERR_INVALID_ARG
    scene.upload_occluder(np.ones((H, W), np.float32))
    p.sort_mode = capi.SORT_STOCHASTIC
    with pytest.raises(mgs.MgsError) as e:
        scene.render(p)
    assert e.value.code == -8  # MGS_ERR_UNSUPPORTED
    p.sort_mode = capi.SORT_GPU_RADIX
    with pytest.raises(mgs.MgsError):
        scene.set_occluder(1 << 20, 0, 0, H)
    with pytest.raises(ValueError):
        scene.upload_occluder(np.ones((H, W, 2), np.float32))
    lib = capi.load_library()
    assert lib.mgs_frame_set_occluder(None, None, None, W, H) == -1
    assert lib.mgs_frame_upload_occluder(None, None, None, W, H) == -1
    # the handle still renders, and stochastic frames work again once nothing is bound
    scene.clear_occluder()
    p.sort_mode = capi.SORT_STOCHASTIC
    scene.render(p)
    p.sort_mode = capi.SORT_GPU_RADIX
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
