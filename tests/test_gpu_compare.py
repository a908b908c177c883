"""GPU tests (-m gpu) of the image comparison (mgs_compare_*, k_compare.hip).

Metrics and split view are checked against the independent float64 restatement of the reference's shaders (np_compare.py) applied
to the images the library itself holds (its own downloaded frames, or an uploaded capture).  The bars come from the CPU test
(test_compare_cpu.py::test_bars_from_the_reference_alone), see compare_cases.py:
  - fixed sums: equal to the restatement's except on boundary pixels, |difference| <= the number of boundary pixels of the pair;
  - exact sums: within 4 x the recorded float32-vs-float64 difference (plus the separable-vs-2-D difference in reference mode);
  - mse / psnr / flip: the host formula applied to the returned fixed sums, exactly; two calls return the same bits.
Measured on an MI355X (the print lines of these tests): see DESIGN.md 3.9.
Where the subject is plumbing the library is compared with itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth
import compare_cases as cc
import lighting_cases as lc
import np_compare as npc

pytestmark = pytest.mark.gpu

TARGETS = {"f32": capi.TARGET_RGBA32F, "f16": capi.TARGET_RGBA16F, "u8": capi.TARGET_RGBA8}
ERR_STATE = -6


def make_scene(sh_format=capi.FORMAT_FLOAT32):
    scene = mgs.Scene(0)
    for arrays, m in lc.scene_sets():
        scene.add_instance(mgs.SplatSet.from_arrays(**arrays), m)
    scene.commit(sh_format, capi.FORMAT_FLOAT32)
    return scene


@pytest.fixture(scope="module")
def scene():
    s = make_scene()
    yield s
    s.close()


@pytest.fixture(scope="module")
def scene_u8():
    s = make_scene(capi.FORMAT_UINT8)
    yield s
    s.close()


def params(W, H, pose=11, target="f16", gut=0):
    eye = synth.orbit_pose(pose)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    p.target_format, p.pipeline = TARGETS[target], gut
    return p


def as_float(img):
    """a downloaded frame as the kernels read it"""
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255.0)
    return img.astype(np.float32)


def frame(s, p):
    out = s.render(p, want_stats=True)
    assert out.error_flags == 0
    return as_float(s.download_frame(p))


def bits(m):
    return (m.mse_fixed, m.flip_fixed) + tuple(np.float64(v).tobytes() for v in (m.mse, m.psnr, m.flip, m.mse_exact, m.psnr_exact, m.flip_exact))


def check_metrics(name, s, cap, cur, modes=(0, 1, 2), exact=False):
    """the handle holds `cap` as its capture and `cur` as its last frame.  exact: an fp16 / u8 pair of equal sizes that must have
    no MSE boundary pixel, so that mse_fixed equals the restatement's exactly"""
    n = cap.shape[0] * cap.shape[1]
    sampled = cap.shape[:2] != cur.shape[:2]
    for mode in modes:
        m = s.compare_metrics(mode)
        again = s.compare_metrics(mode)
        assert bits(m) == bits(again), (name, mode, "two calls differ")
        r = npc.metrics(cap, cur, mode, cc.PPD, np.float64)
        nb_mse = cc.boundary_count(r["mse_units"], cc.recorded("mse", sampled))
        d_mse = abs(int(m.mse_fixed) - r["mse_fixed"])
        rel_mse = abs(m.mse_exact - r["mse_exact"]) / r["mse_exact"]
        line = (f"compare {name} mode {mode}: mse_fixed {m.mse_fixed} (restatement {r['mse_fixed']}, {nb_mse} boundary pixels), mse_exact rel "
                f"{rel_mse:.3e} (bar {cc.gpu_bar(None, sampled):.2e}), psnr {m.psnr:.2f} exact {m.psnr_exact:.2f}")
        if mode:
            nb_flip = cc.boundary_count(r["flip_units"], cc.flip_bar(mode))
            d_flip = abs(int(m.flip_fixed) - r["flip_fixed"])
            gsum = m.flip_exact ** 3 * n
            tol = cc.gpu_bar(mode) * r["flip_powered_sum"]  # a relative bar on the sum
            line += (f", flip_fixed {m.flip_fixed} (restatement {r['flip_fixed']}, {nb_flip} boundary), powered sum {gsum:.9e} vs {r['flip_powered_sum']:.9e} "
                     f"(|d| {abs(gsum - r['flip_powered_sum']):.3e}, allowed {tol:.3e}), flip {m.flip:.5f} exact {m.flip_exact:.5f}")
        print(line + f", {m.elapsed_ms:.3f} ms")
        assert d_mse <= nb_mse, (name, mode, d_mse, nb_mse)
        if exact:
            assert nb_mse == 0 and d_mse == 0, (name, mode, nb_mse, d_mse)
        assert rel_mse <= cc.gpu_bar(None, sampled), (name, mode, rel_mse)
        if mode:
            assert d_flip <= nb_flip, (name, mode, d_flip, nb_flip)
            assert abs(gsum - r["flip_powered_sum"]) <= tol, (name, mode)
        else:
            assert m.flip_fixed == 0 and m.flip == 0.0 and m.flip_exact == 0.0
        mse, psnr, flip = npc.collect(m.mse_fixed, m.flip_fixed)
        assert np.float32(m.mse) == mse and np.float32(m.flip) == flip, (name, mode)
        # float log10 is the C library's: the host formula holds for numpy's float32 log10 or for the correctly rounded one
        import math
        rounded = min(np.float32(10.0) * np.float32(math.log10(float(np.float32(1.0) / mse))), np.float32(99.99)) if mse >= np.float32(1e-10) else np.float32(99.99)
        assert np.float32(m.psnr) in (psnr, np.float32(rounded)), (name, mode, m.psnr, psnr, rounded)


# ---- 1. metrics against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(160, 120), (320, 240), (200, 160)])
def test_synthetic_perturbation_of_a_frame(scene, W, H):
    p = params(W, H)
    cur = frame(scene, p)
    cap = cc.perturb(cur, seed=5)  # noise and a step on the library's own fp16 frame (clipped to [0.1, 0.9])
    scene.compare_capture_upload(cap)
    check_metrics(f"perturbed_{W}x{H}", scene, cap, cur, exact=(W, H) != (200, 160))  # seed 5 at 200 x 160: two boundary pixels
    scene.compare_release()


def test_capture_of_another_size(scene):
    small = frame(scene, params(160, 120))
    cap = cc.perturb(small, seed=6)
    scene.compare_capture_upload(cap)
    cur = frame(scene, params(320, 240))
    check_metrics("capture160x120_current320x240", scene, cap, cur)
    scene.compare_release()


def test_full_hd_mse_and_flip_approx(scene):
    p = params(1920, 1080)
    cur = frame(scene, p)
    cap = cc.perturb(cur, seed=7)
    scene.compare_capture_upload(cap)
    check_metrics("perturbed_1920x1080", scene, cap, cur, modes=(0, 1))
    m = scene.compare_metrics(capi.FLIP_REFERENCE)  # runs; its value is checked at the sizes the brute-force restatement reaches
    print(f"compare perturbed_1920x1080 mode 2: flip {m.flip:.5f} exact {m.flip_exact:.5f}, {m.elapsed_ms:.3f} ms")
    assert 0.0 < m.flip_exact < 1.0
    scene.compare_release()


@pytest.mark.parametrize("target", ["f16", "u8", "f32"])
def test_fp32_against_uint8_sh_storage(scene, scene_u8, target):
    p = params(320, 240, target=target)
    cap = frame(scene, p)
    cur = frame(scene_u8, p)
    scene_u8.compare_capture_upload(cap)
    check_metrics(f"storage_{target}", scene_u8, cap, cur, exact=target != "f32")
    scene_u8.compare_release()


def test_two_poses_and_two_pipelines_captured_on_the_device(scene):
    p = params(320, 240, pose=11)
    cap = frame(scene, p)
    scene.compare_capture()
    cur = frame(scene, params(320, 240, pose=12))
    check_metrics("two_poses", scene, cap, cur, modes=(0, 1))
    cur = frame(scene, params(320, 240, pose=11, gut=1))
    check_metrics("3dgs_vs_3dgut", scene, cap, cur, exact=True)
    scene.compare_release()


# ---- 2. the split view ---------------------------------------------------------------------------------------------------------
def test_composite_against_the_restatement(scene):
    p = params(200, 160)
    cur = frame(scene, p)
    cap = cc.perturb(cur, seed=8)
    scene.compare_capture_upload(cap)
    bar = cc.GPU_MARGIN * cc.F32_VS_F64_COMPOSITE
    for mode in range(6):
        got = scene.compare_composite(split=0.4, left=mode, right=mode)
        ref = npc.composite(cap, cur, 0.4, mode, mode, 5.0, 0, 0, np.float64)
        assert got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        print(f"composite mode {mode}: max error {err:.3e} (bar {bar:.1e})")
        assert np.array_equal(got[:, 78:83], ref[:, 78:83].astype(np.float32))  # int(0.4f * 200) = 80: the divider, exact
        if mode < 2:
            assert np.array_equal(got, ref.astype(np.float32))
        assert err <= bar, mode
    got = scene.compare_composite(split=0.5, left=capi.SHOW_CAPTURE, right="diff-red-gray")
    ref = npc.composite(cap, cur, 0.5, 0, 3)
    assert np.array_equal(got[:, :98], cap[:, :98]) and np.abs(got - ref).max() <= bar
    # another output size: both sides sampled (clamp-to-edge, the documented rule; the reference's sampler is unpinned)
    for mode in (0, 1, 3, 5):
        got = scene.compare_composite(split=0.3, left=mode, right=mode, width=300, height=200)
        ref = npc.composite(cap, cur, 0.3, mode, mode, 5.0, 300, 200, np.float64)
        inner = float(np.abs(got - ref)[2:-2, 2:-2].max())
        edge = float(np.abs(got - ref).max())
        print(f"composite 300x200 mode {mode}: max error {inner:.3e} inside, {edge:.3e} with the edge (clamp rule), bar {bar:.1e}")
        assert got.shape == (200, 300, 4) and inner <= bar and edge <= bar, mode
    scene.compare_release()


# ---- 3. plumbing: the library against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["f16", "f32", "u8"])
def test_a_frame_against_its_own_capture(scene, target):
    p = params(320, 240, target=target)
    scene.render(p)
    scene.compare_capture()
    for mode in (0, 1, 2):
        m = scene.compare_metrics(mode)
        assert m.mse_fixed == 0 and m.flip_fixed == 0 and m.psnr == np.float32(99.99) and m.flip == 0.0
        assert m.mse_exact == 0.0 and m.flip_exact == 0.0 and m.psnr_exact == np.inf
    scene.compare_release()


def test_state_errors_and_a_context_owns_its_capture(scene):
    p = params(320, 240)
    ctx = scene.frame_context()
    try:
        for call in (ctx.compare_capture, ctx.compare_metrics, ctx.compare_composite):
            with pytest.raises(mgs.MgsError) as e:  # no frame on this handle yet
                call()
            assert e.value.code == ERR_STATE
        scene.render(p)
        scene.compare_capture()
        ctx.render(p)
        with pytest.raises(mgs.MgsError) as e:  # the scene's capture is not the context's
            ctx.compare_metrics()
        assert e.value.code == ERR_STATE and "no capture" in str(e.value)
        ctx.compare_capture()
        ctx.render(params(320, 240, pose=12))
        assert ctx.compare_metrics(0).mse_fixed > 0 and scene.compare_metrics(0).mse_fixed == 0
        q = params(320, 240)
        q.strip_row_begin, q.strip_row_end = 3, 9
        scene.render(q)
        for call in (scene.compare_capture, scene.compare_metrics, scene.compare_composite):
            with pytest.raises(mgs.MgsError) as e:  # strip-only: the buffer holds only some rows
                call()
            assert e.value.code == ERR_STATE and "strip" in str(e.value)
        scene.render(p)
        scene.compare_release()
        with pytest.raises(mgs.MgsError) as e:
            scene.compare_metrics()
        assert e.value.code == ERR_STATE
    finally:
        ctx.close()
        scene.compare_release()


def test_a_held_capture_changes_no_frame(scene):
    p = params(320, 240, pose=12)
    scene.compare_release()
    scene.render(p)
    before = scene.download_frame(p).copy()
    scene.compare_capture()
    scene.render(params(320, 240, pose=11))
    scene.render(p)
    assert np.array_equal(scene.download_frame(p).view(np.uint16), before.view(np.uint16))
    scene.compare_release()


def test_destroying_a_handle_frees_its_compare_state(scene):
    """a frame context that captured, measured (reference mode: 17 planes) and composited at 1920 x 1080 holds about 210 MB of
    compare state; destroying it must give all of it back"""
    import torch
    p = params(1920, 1080)

    def once():
        ctx = scene.frame_context()
        try:
            ctx.render(p)
            ctx.compare_capture()
            ctx.compare_metrics(capi.FLIP_REFERENCE)
            ctx.compare_composite(left=capi.SHOW_CAPTURE, right=capi.SHOW_FLIP)
            _, working = ctx.memory_usage()
        finally:
            ctx.close()
        return working
    once()  # whatever the runtime keeps after a first use is kept now
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(6):
        working = once()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    print(f"compare state: a context's working set {working / 2**20:.0f} MiB; free memory moved by {(free0 - free1) / 2**20:.1f} MiB over six contexts")
    assert working >= 200 * 2**20  # the working set counts the compare buffers
    assert free0 - free1 < 64 * 2**20, "destroying a handle leaks its compare buffers"


def test_the_vkrepro_tool_device_path_equals_its_host_value():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import compare_vkrepro as cv
    want, got = cc.synthetic_pair("s320")
    got = got.copy()
    got[10:20, 10:20, :3] = -0.01  # an fp target may hold slightly negative colours
    host, mse = cv.psnr_rgb(want, got)
    dev = cv.device_psnr(want, got)
    print(f"compare_vkrepro --device: {dev:.6f} dB, host {host:.6f} dB")
    assert abs(dev - host) <= 1e-5 * host


def test_graph_replay_and_gathered_frames():
    here = os.path.dirname(os.path.abspath(__file__))
    fake = os.path.join(here, "helpers", "libfakerccl.so")
    assert os.path.exists(fake), "tests/helpers/libfakerccl.so is built by build()"
    out = {}
    for mode, extra in (("graph", {}), ("plain", {"MGS_GRAPH": "0"})):
        r = subprocess.run([sys.executable, os.path.join(here, "_child_compare.py")], env=dict(os.environ, MGS_RCCL_LIB=fake, **extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith("METRICS")]
        assert len(lines) == 9
        per = {}
        for l in lines:
            per.setdefault(l[2], set()).add(" ".join(l[3:]))
        assert all(len(v) == 1 for v in per.values()), "first frame, replayed frame and gathered frame give different metrics"
        out[mode] = per
    assert out["graph"] == out["plain"]
