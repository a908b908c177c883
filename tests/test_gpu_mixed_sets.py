"""GPU parity tests (-m gpu) of scenes made of several DIFFERENT splat sets (tests/mixed_scene.py) against the CPU oracle.

Every other GPU test renders one SplatSet added again and again, which the library de-duplicates to one device set: per-set
and per-instance code (partition prefixes, instance lookup in the compositor and the 3DGUT kernels, SH of each set's own
degree, each set's storage order, the id mapping back to the caller) cannot be told from a one-set version there.  The
oracle follows each instance's own set in its own storage order (ob.storage_sorted_stream).  Bars are the suite's:
integer streams bit-exact, frames at PSNR_MIN / ABS_TOL of test_gpu_parity.py (3DGUT: test_gpu_gut.py's)."""
import numpy as np
import pytest

from mixed_scene import MixedScene, check_projected_records, distinct_sets, mixed_layout, projective
import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, multigpu, synth

pytestmark = pytest.mark.gpu

PSNR_MIN = 55.0       # dB, as test_gpu_parity.py
ABS_TOL = 2.5e-2
GUT_PSNR_MIN = 50.0   # as test_gpu_gut.py
GUT_ABS_TOL = 3.0e-2
B = 1                 # the one-splat degree-0 instance of mixed_layout()


@pytest.fixture(scope="module")
def sets():
    return distinct_sets()


@pytest.fixture(scope="module")
def mixed(sets):
    m = MixedScene(sets, mixed_layout())
    yield m
    m.close()


def camera(pose, W, H, inside=False):
    if inside:   # inside the instances' clouds, looking across them
        eye, ctr = np.array([0.3, 0.1, 0.2], np.float32), [1.2, 0.0, 1.0]
    else:
        eye, ctr = synth.orbit_pose(pose), [0, 0, 0]
    V, P = mgs.camera_lookat_perspective(eye, ctr, [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    return p, V, P, eye


def frame_vs_oracle(ob, m, p, V, P, eye, W, H, label, **fkw):
    """render p, compare with the oracle's frame in the oracle's own sorted order; returns (img, oimg, stream)"""
    gut = p.pipeline == capi.PIPELINE_3DGUT
    out = m.scene.render(p, want_stats=True)
    img = m.scene.download_frame(p).astype(np.float32)
    stream = m.oracle_stream(ob, ob.make_frame(V, P, eye, W, H, pipeline_3dgut=int(gut)))
    fr = ob.make_frame(V, P, eye, W, H, target_fp16=1, sh_degree=p.sh_degree, **fkw)
    oimg, st = (ob.render_gut if gut else ob.render)(fr, stream[3], order=stream[2])
    psnr = ob.psnr_rgb(img, oimg)
    err = np.abs(img[..., :3] - oimg[..., :3]).max()
    print(f"{label}: PSNR {psnr:.2f} dB, max abs {err:.4f}, frustum {out.frustum_count} (oracle {st['visible']})")
    assert out.error_flags == 0 and out.frustum_count == st["visible"]
    assert psnr >= (GUT_PSNR_MIN if gut else PSNR_MIN) and err <= (GUT_ABS_TOL if gut else ABS_TOL)
    return img, oimg, stream


def test_mixed_scene_layout(mixed):
    """the scene really holds five different device sets: counts, SH degrees and storage orders differ"""
    assert mixed.counts == [6921, 1, 2048, 2049, 6921, 30000]
    assert mixed.scene.splat_count == 47940
    assert np.array_equal(mixed.perms[0], mixed.perms[4])                     # A twice: one set, one order
    assert not np.array_equal(mixed.perms[5][:6921], mixed.perms[0])          # E has its own order
    for k, deg in enumerate([3, 0, 1, 2, 3, 3]):
        n = mixed.counts[k]
        sh = mixed.scene.download_set(k, 3, 45 * n)
        assert np.array_equal(sh[3 * ((deg + 1) ** 2 - 1) * n:], np.zeros(sh.size - 3 * ((deg + 1) ** 2 - 1) * n, np.float32))


@pytest.mark.parametrize("pose", [3, 21, 46, "inside"])
def test_sorted_stream_bit_exact(mixed, ob, pose):
    """(key, id) stream of the mixed scene == the oracle's stable sort with ties in the library's storage order, ids in the
    caller's space of every instance; frustum_count == the oracle's visible count"""
    W, H = 640, 480
    p, V, P, eye = camera(pose if pose != "inside" else 0, W, H, inside=pose == "inside")
    oks, ois, _, _ = mixed.oracle_stream(ob, ob.make_frame(V, P, eye, W, H))
    so = mixed.scene.sort_keys(p)
    gk, gi = mixed.scene.sort_download(so.count)
    per = np.bincount(mixed.instance_of(ois), minlength=6)
    print(f"pose {pose}: {so.count} sorted, per instance {per.tolist()}")
    assert so.count == oks.size
    assert np.array_equal(gk, oks) and np.array_equal(gi, ois)
    assert (per[[0, 2, 3, 4, 5]] > 0).all()           # every multi-splat instance is in the stream
    out = mixed.scene.render(p, want_stats=True)
    assert out.error_flags == 0 and out.frustum_count == oks.size


def test_projected_records_per_instance(sets, ob):
    """download_projected of every sorted splat against orc_project, worst splat reported per instance (fresh scene: the
    default bin size of the rectangles)"""
    m = MixedScene(sets, mixed_layout())
    W, H = 640, 480
    p, V, P, eye = camera(3, W, H)
    out = m.scene.render(p, want_stats=True)
    _, gi = m.scene.sort_download(out.sorted_count)
    keys, ois, sids, inst_s = m.oracle_stream(ob, ob.make_frame(V, P, eye, W, H))
    # the frame sorts the stream's survivors that cover a pixel: align each frame id with its oracle storage id
    where = {int(c): j for j, c in enumerate(ois)}
    j = np.array([where[int(g)] for g in gi])
    rec, rect = m.scene.download_projected(gi)
    k = m.instance_of(gi)
    assert np.array_equal(m.instance_of(ois[j]), k) and set(np.unique(k)) >= {0, 1, 2, 3, 4, 5}
    check_projected_records(ob, ob.make_frame(V, P, eye, W, H), inst_s, sids[j], k, rec, rect, W, H, "mixed pose 3")
    m.close()


@pytest.mark.parametrize("sh_degree", [3, 2, 1, 0])
def test_frames_sh_per_set(mixed, ob, sh_degree):
    """frames at frame SH degree 3..0 over sets of degree 3, 0 (no SH buffer), 1 and 2.  The per-set 48-element SH record is
    zero padded, so a kernel that reads MORE coefficients than its set holds is hidden by the padding; what this covers is a
    set degree BELOW the frame degree (min(set, frame)), the degree-0 set without SH buffer (sh == nullptr) and each set's
    own buffers.  At degree 3 the pixels of the one-splat degree-0 instance are compared on their own as well."""
    W, H = 640, 480
    p, V, P, eye = camera(3, W, H)
    p.sh_degree = sh_degree
    img, oimg, stream = frame_vs_oracle(ob, mixed, p, V, P, eye, W, H, f"mixed sh_degree {sh_degree}")
    if sh_degree == 3:
        assert (mixed.instance_of(stream[1]) == B).any(), "the degree-0 instance must be in the frame"
        q = ob.project(ob.make_frame(V, P, eye, W, H), stream[3], B, 0)
        cx, cy = q.center_px
        r = 0.5 * max(np.hypot(*q.basis1), np.hypot(*q.basis2))
        assert q.valid and r >= 15.0 and 0 <= cx < W and 0 <= cy < H
        y0, y1, x0, x1 = int(max(0, cy - r)), int(min(H, cy + r)), int(max(0, cx - r)), int(min(W, cx + r))
        wi, wo = img[y0:y1, x0:x1], oimg[y0:y1, x0:x1]
        psnr, err = ob.psnr_rgb(wi, wo), np.abs(wi[..., :3] - wo[..., :3]).max()
        print(f"  degree-0 splat window {x1 - x0}x{y1 - y0}: PSNR {psnr:.2f} dB, max abs {err:.4f}")
        assert psnr >= PSNR_MIN and err <= ABS_TOL


@pytest.mark.parametrize("fmt", [capi.FORMAT_FLOAT16, capi.FORMAT_UINT8])
def test_storage_formats_per_set(sets, ob, fmt):
    """commit(fmt, fmt) of the mixed scene: every instance's download_set bit-exact against its own set quantised the same
    way; the degree-0 set has no SH (an empty download that writes nothing); the frame against the same-quantisation oracle"""
    m = MixedScene(sets, mixed_layout(), fmt, fmt)
    for i, (name, _) in enumerate(m.layout):
        ps = ob.PreparedSet(sets[name], sh_format=fmt, rgba_format=fmt)
        n = ps.count
        assert np.array_equal(m.scene.download_set(i, 0, 3 * n), ps.positions), i
        assert np.array_equal(m.scene.download_set(i, 1, 6 * n), ps.cov6), i
        assert np.array_equal(m.scene.download_set(i, 2, 4 * n), ps.rgba), i
        assert np.array_equal(m.scene.download_set(i, 3, ps.sh_stride * n), ps.sh[: ps.sh_stride * n]), i
    assert ob.PreparedSet(sets["B"]).sh_stride == 0
    assert m.scene.download_set(B, 3, 0).size == 0
    assert not m.scene.download_set(B, 3, 48).any()     # nothing written for a set without SH
    W, H = 480, 360
    p, V, P, eye = camera(7, W, H)
    frame_vs_oracle(ob, m, p, V, P, eye, W, H, f"mixed storage format {fmt}")
    m.close()


@pytest.mark.parametrize("count", [16, 17, 24])
def test_more_than_16_instances(sets, ob, count):
    """16 instances fill the compositor's inline table; 17 and 24 take the instTable binary search of the compositor and the
    3DGUT kernels, over unevenly spaced global offsets (A, B, C, D cycling, E as instance 16)"""
    names = ["A", "B", "C", "D"]
    layout = []
    for k in range(count):
        M, _ = mgs.compute_transform([0.5 + 0.01 * k] * 3, [7.0 * k, 13.0 * k, 0.0],
                                     [(k % 8) * 1.6 - 5.6, 0.3 * (k % 3), (k // 8) * 1.8 - 3.6])
        layout.append(("E" if k == 16 else names[k % 4], projective(M) if k == 5 else M))
    m = MixedScene(sets, layout)
    W, H = 480, 270
    eye = np.array([7.0, 4.0, 8.0], np.float32)
    V, P = mgs.camera_lookat_perspective(eye, [0, 0, 0], [0, 1, 0], 60.0, 0.1, 2000.0, W, H)
    p = capi.default_params(W, H)
    capi.set_camera(p, V, P, eye)
    oks, ois, _, _ = m.oracle_stream(ob, ob.make_frame(V, P, eye, W, H))
    so = m.scene.sort_keys(p)
    gk, gi = m.scene.sort_download(so.count)
    assert so.count == oks.size and np.array_equal(gk, oks) and np.array_equal(gi, ois)
    present = np.unique(m.instance_of(ois))
    print(f"{count} instances: {so.count} sorted, {present.size} instances in the stream")
    assert present.size >= count - 2 and present.max() == count - 1
    frame_vs_oracle(ob, m, p, V, P, eye, W, H, f"{count} instances 3DGS")
    p.pipeline = capi.PIPELINE_3DGUT
    frame_vs_oracle(ob, m, p, V, P, eye, W, H, f"{count} instances 3DGUT")
    m.close()


def test_surface_outputs_in_the_callers_id_space(mixed, ob):
    """picked depth, the picking splat's id in the CALLER's id space of its own instance and set, the integrated normal,
    against the oracle (bars of test_surface_side_outputs_match_oracle / test_integrated_normal_matches_oracle); the share of
    matching picks is checked per instance too, so that a small instance whose ids come back in another set's storage order
    cannot hide under the whole frame's share"""
    W, H = 640, 360
    p, V, P, eye = camera(11, W, H)
    mixed.scene.render(p)
    plain = mixed.scene.download_frame(p).copy()
    p.surface_outputs, p.depth_iso_threshold, p.quantize_normals = 1, 0.7, 1
    out = mixed.scene.render(p, want_stats=True)
    assert out.error_flags == 0
    assert np.array_equal(mixed.scene.download_frame(p).view(np.uint16), plain.view(np.uint16))
    depth, ids, nrm = mixed.scene.download_surface(p, normals=True)
    _, _, sids, inst_s = mixed.oracle_stream(ob, ob.make_frame(V, P, eye, W, H))
    od, osid, on = ob.render_surface(ob.make_frame(V, P, eye, W, H), inst_s, sids[::-1].copy(), 0.7, normals=True)
    oid = osid.copy()
    hit = osid != 0xFFFFFFFF
    oid[hit] = ob.caller_ids(osid[hit], mixed.counts, mixed.perms)
    same = ids == oid
    err = np.abs(nrm - on)
    print(f"mixed surface outputs: same pick {same.mean():.5f}, normal max abs {err.max():.4f} mean {err.mean():.2e}")
    assert same.mean() >= 0.995
    assert np.allclose(depth[same], od[same], rtol=1e-6, atol=1e-7)
    assert (ids != 0xFFFFFFFF).any() and ((depth == 0) == (ids == 0xFFFFFFFF)).all()
    k = np.where(hit, mixed.instance_of(np.where(hit, oid, 0)), -1)
    for q in range(6):
        mk = k == q
        print(f"  instance {q}: {int(mk.sum())} picked pixels, same {same[mk].mean() if mk.any() else 1.0:.5f}")
        if mk.sum() >= 200:
            assert same[mk].mean() >= 0.99, q
    assert (k == B).sum() >= 200 and (k == 2).sum() >= 200 and (k == 5).sum() >= 200
    assert err.max() < 2e-2 and err.mean() < 2e-5 and np.quantile(err, 0.9999) < 2e-4, (err.max(), err.mean())
    p.surface_outputs = 0


def test_transforms_edited_between_frames(sets, ob):
    """set_transform takes instance 2 (set C) through identity -> affine -> projective -> identity: each frame is bit-identical
    to the first frame of a freshly created and committed scene with the same transforms (identity / affine shortcut flags,
    the graph cache, the previous frame's partition order, the bin history) and within the oracle's bar"""
    W, H = 480, 360
    p, V, P, eye = camera(5, W, H)
    Maff, _ = mgs.compute_transform([0.8, 1.1, 0.9], [15.0, -30.0, 10.0], [0.6, -0.2, 0.9])
    seq = [np.eye(4, dtype=np.float32), Maff, projective(Maff, 2.0e-3, 1.0e-3), np.eye(4, dtype=np.float32)]
    m = MixedScene(sets, mixed_layout())
    for step, M in enumerate(seq):
        m.set_transform(2, M)
        m.scene.render(p)
        got = m.scene.download_frame(p).view(np.uint16).copy()
        f = MixedScene(sets, m.layout)
        f.scene.render(p)
        fresh = f.scene.download_frame(p).view(np.uint16).copy()
        f.close()
        assert np.array_equal(got, fresh), f"step {step}: the edited scene's frame differs from a fresh scene's"
        frame_vs_oracle(ob, m, p, V, P, eye, W, H, f"transform step {step}")
    m.close()


def test_strips_and_frame_contexts(mixed):
    """G = 3 tile-row strips reassemble the mixed scene's frame bit for bit; a frame context renders the same frame"""
    W, H = 640, 360
    p, *_ = camera(23, W, H)
    mixed.scene.render(p)
    full = mixed.scene.download_frame(p).view(np.uint16).copy()
    asm = np.zeros_like(full)
    G = 3
    for r in range(G):
        b, e = multigpu.strip_rows(H, G, r)
        p.strip_row_begin, p.strip_row_end = b, e
        mixed.scene.render(p)
        part = mixed.scene.download_frame(p).view(np.uint16)
        y0, y1 = b * 16, min(e * 16, H)
        asm[y0:y1] = part[y0:y1]
    assert np.array_equal(asm, full)
    p.strip_row_begin = p.strip_row_end = 0
    ctx = mixed.scene.frame_context()
    ctx.render(p)
    assert np.array_equal(ctx.download_frame(p).view(np.uint16), full)
    ctx.close()
