"""GPU tests (-m gpu) of the 3DGUT kernels below the frame: the emitted set, the per-particle records of k_project_gut.hip
(mgs_frame_download_projected_gut) with their bin rectangles, the exact per-pixel fragment counts and nearest-fragment ids of every
k_composite_gut instantiation the count mode reaches, and the packed compositor k_composite_gut2 through colours that name the
particle — all against the float64 restatement tests/np_gut.py on the cases of tests/gut_cases.py (tests/test_gut_cpu.py holds the
oracle to the same restatement and measures the yardsticks of the bars used here).

The blend with the opacity gaussian on is held to the float64 interval of np_gut.GutFragments.blend; the bin rectangles are checked
once more with 32x16-px bins in a child process (tests/_child_gut_rects.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi
import fragment_cases as fc
import gut_cases as gc
import np_gut as ng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(name, sh_format=0):
        key = name.split("+")[0]
        if key == "strip":
            key = "cloud"
        key = (key, sh_format)
        if key not in made:
            scene, sets = mgs.Scene(0), {}
            for arrays, m in gc.case(name)["sets"]:
                if id(arrays) not in sets:
                    sets[id(arrays)] = mgs.SplatSet.from_arrays(**arrays)
                scene.add_instance(sets[id(arrays)], m)
            scene.commit(sh_format, 0)   # (the colour plane stays fp32: it holds the opacity, which the cases' thresholds are about)
            made[key] = scene
        return made[key]

    yield get
    for s in made.values():
        s.close()


def frame_params(name, **kw):
    c = gc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.pipeline, p.target_format, p.sh_degree = capi.PIPELINE_3DGUT, capi.TARGET_RGBA32F, 0
    for k, v in dict(c["params"], **kw).items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def strip_rows(name):
    c = gc.case(name)
    r0, r1 = c["st"]["strip"] if c["st"]["strip"] is not None else (0, (c["H"] + 15) // 16)
    return slice(r0 * 16, min(r1 * 16, c["H"]))


@pytest.mark.parametrize("name", gc.CASES)
def test_emitted_set_records_and_rectangles(scenes, name):
    c, scene = gc.case(name), scenes(name)
    prs = gc.projected(name)
    emits, reason, fragile, rect_fragile = (gc.stack(prs, k) for k in ("emits", "reason", "fragile", "rect_fragile"))
    assert fragile[emits].mean() <= gc.FRAGILE_CAP
    pr = {k: gc.stack(prs, k) for k in ("cx", "cy", "half1", "half2", "box", "B", "ro", "opacity", "window")}
    dist = reason == ng.REJECTIONS.index("dist")
    dist_open = int((gc.stack([p["margins"] for p in prs], "dist") < gc.DELTA).sum())
    # the default frame (256x128-px bins) and the count mode's (128x64-px bins: several bins on these frames)
    for mode, bin_px in ((dict(), (256, 128)), (dict(alpha_mode=capi.ALPHA_SUM, debug_flags=4), (128, 64))):
        p = frame_params(name, **mode)
        out = scene.render(p, want_stats=True)
        assert out.error_flags == 0
        assert abs(int(out.frustum_count) - int((~dist).sum())) <= dist_open
        _, ids = scene.sort_download(out.sorted_count)
        ids = ids[:out.sorted_count].astype(np.int64)
        assert np.unique(ids).size == ids.size
        got = np.zeros(emits.size, bool)
        got[ids] = True
        differ = (got != emits) & ~fragile
        assert not differ.any(), [(int(i), "emitted" if got[i] else "dropped", ng.REJECTIONS[reason[i]] if reason[i] >= 0 else "emits") for i in np.flatnonzero(differ)[:8]]
        idx = np.flatnonzero(got & emits & ~fragile)
        rec, rect = scene.download_projected_gut(idx)
        dev, worst = ng.record_deviation(pr, idx, rec)
        print(f"\n3DGUT kernel vs float64, {name}, bins {bin_px} ({idx.size} particles of {ids.size} sorted): "
              + ", ".join(f"{k} {dev[k]:.2e} / {gc.BAR_FACTOR * gc.ORACLE_DEV[name][k]:.1e} (#{worst[k]})" for k in ng.FIELDS))
        over = {k: (dev[k], worst[k]) for k in ng.FIELDS if dev[k] > gc.BAR_FACTOR * gc.ORACLE_DEV[name][k]}
        assert not over, over
        assert np.all(rec[:, 20:23] == 0.0)
        w = pr["window"][idx]
        want = np.stack([w[:, 0] // bin_px[0], w[:, 1] // bin_px[1], w[:, 2] // bin_px[0], w[:, 3] // bin_px[1]], 1)
        sure = ~rect_fragile[idx]
        bad = (fc.unpack_rects(rect) != want).any(1) & sure
        assert not bad.any(), [(int(idx[i]), fc.unpack_rects(rect)[i].tolist(), want[i].tolist()) for i in np.flatnonzero(bad)[:8]]
        assert sure.mean() >= 0.95


def check_counts(name, ref, alpha, what, ids=None):
    rows = strip_rows(name)
    cap = gc.BORDERLINE_CAP.get(name.split("+")[0], gc.BORDERLINE_CAP["default"])
    assert ref.borderline.mean() <= cap
    got = np.rint(alpha).astype(np.int64)
    assert np.array_equal(got[rows].astype(np.float32), alpha[rows]), "the alpha plane of the count mode is not integral"
    off = np.abs(got - ref.count) > np.where(ref.borderline, ref.borderline_count, 0)
    off[:rows.start], off[rows.stop:] = False, False
    print(f"3DGUT counts, {name}, {what}: {int(ref.count.sum())} fragments, {int(ref.borderline.sum())} borderline pixels, {int((got != ref.count)[rows].sum())} pixels differ")
    assert not off.any(), ng.describe(ref, got, ref.count, off)
    if ids is not None:
        got_id = np.where(ids == 0xFFFFFFFF, -1, ids.astype(np.int64))
        bad = (got_id != ref.nearest_id) & ~ref.nearest_open & ~ref.borderline
        bad[:rows.start], bad[rows.stop:] = False, False
        assert not bad.any(), ng.describe(ref, got_id, ref.nearest_id, bad)


COUNT_VARIANTS = {
    "plain": dict(),                                                             # XT 0
    "surface": dict(surface_outputs=1),                                          # XT 2
    "iso_surface": dict(surface_outputs=1, normal_method=capi.NORMAL_ISO_SURFACE),   # XT 3
}


@pytest.mark.parametrize("name", gc.CASES)
@pytest.mark.parametrize("variant", list(COUNT_VARIANTS))
def test_fragment_counts(scenes, name, variant):
    scene, kw = scenes(name), COUNT_VARIANTS[variant]
    p = frame_params(name, alpha_mode=capi.ALPHA_SUM, debug_flags=4, **kw)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    alpha = np.ascontiguousarray(scene.download_frame(p)[..., 3])
    ids = scene.download_surface(p)[1] if kw else None   # every fragment is opaque: the picked splat is the nearest fragment's
    check_counts(name, gc.reference_fragments(name), alpha, variant, ids)


@pytest.mark.parametrize("name", ["cloud", "inside+eigen", "fisheye150"])
@pytest.mark.parametrize("degree", [0, 1, 3, 4, 5, 8])
def test_fragment_counts_of_every_kernel_degree(scenes, name, degree):
    scene = scenes(name)
    p = frame_params(name, alpha_mode=capi.ALPHA_SUM, debug_flags=4, kernel_degree=degree)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    check_counts(name, gc.reference_fragments(name, degree), np.ascontiguousarray(scene.download_frame(p)[..., 3]), f"degree {degree}")


OCC_VARIANTS = dict(COUNT_VARIANTS, lens=dict(dof_mode=capi.DOF_FIXED_FOCUS, aperture=0.0, focus_dist=1.0),   # XT 1
                    **{f"degree {d}": dict(kernel_degree=d) for d in (0, 1, 3, 4, 5, 8)})


@pytest.mark.parametrize("name", ["cloud", "trs"])
@pytest.mark.parametrize("kind", ["plane", "step"])
@pytest.mark.parametrize("sort_mode", [capi.SORT_GPU_RADIX, capi.SORT_CPU_ASYNC], ids=["stop", "walk"])
@pytest.mark.parametrize("variant", list(OCC_VARIANTS))
def test_fragment_counts_behind_an_occluder(scenes, name, kind, sort_mode, variant):
    """every variant of the count mode with OCC (XT 1: plain and the zero-aperture lens; XT 2: surface outputs and the kernel degrees;
    XT 3): a particle leaves a fragment only where its key depth is <= the occluder's.  "stop": lists sorted by the key end at the first
    record behind it (occStop 1); "walk": the CPU sorter orders by plane distance, so every record is tested (occStop 0)."""
    scene = scenes(name)
    kw = OCC_VARIANTS[variant]
    surf = "surface_outputs" in kw
    scene.upload_occluder(gc.occluder_depth(name, kind))
    try:
        p = frame_params(name, alpha_mode=capi.ALPHA_SUM, debug_flags=4, sort_mode=sort_mode, **kw)
        for _ in range(3 if sort_mode == capi.SORT_CPU_ASYNC else 1):   # the asynchronous sorter's order arrives a frame late
            out = scene.render(p, want_stats=True)
        assert out.error_flags == 0
        alpha = np.ascontiguousarray(scene.download_frame(p)[..., 3])
        ids = scene.download_surface(p)[1] if surf and sort_mode == capi.SORT_GPU_RADIX else None   # (the nearest by the KEY's depth)
    finally:
        scene.clear_occluder()
    degree = kw.get("kernel_degree", 2)
    ref = gc.reference_fragments(name, degree, kind)
    assert 0.2 * ref.count.sum() < gc.reference_fragments(name, degree).count.sum() - ref.count.sum(), "the occluder hides next to nothing"
    check_counts(name, ref, alpha, f"occluder {kind}, {variant}, sort {sort_mode}", ids)


def test_strips_cut_inside_bins_equal_the_full_frames_rows(scenes):
    scene = scenes("cloud")
    p = frame_params("cloud", alpha_mode=capi.ALPHA_SUM, debug_flags=4)
    scene.render(p)
    full = np.ascontiguousarray(scene.download_frame(p)[..., 3]).copy()
    for r0, r1 in ((0, 3), (3, 5), (5, 9), (2, 5)):   # 64-px bins are four tile rows: every strip ends inside one
        p.strip_row_begin, p.strip_row_end = r0, r1
        scene.render(p)
        part = scene.download_frame(p)[..., 3]
        assert np.array_equal(part[r0 * 16:min(r1 * 16, 136)], full[r0 * 16:min(r1 * 16, 136)]), (r0, r1)


@pytest.mark.parametrize("sh_format", [0, 1, 2])
def test_fragment_counts_with_every_sh_storage_format(scenes, sh_format):
    """SHF 0 / 1 / 2 of k_composite_gut (XT 2): the sets hold SH of degree 1, all zero, and the frame asks for degree 1"""
    scene = scenes("cloud", sh_format)
    p = frame_params("cloud", alpha_mode=capi.ALPHA_SUM, debug_flags=4, surface_outputs=1, sh_degree=1)
    assert scene.render(p, want_stats=True).error_flags == 0
    check_counts("cloud", gc.reference_fragments("cloud"), np.ascontiguousarray(scene.download_frame(p)[..., 3]), f"sh format {sh_format}",
                 scene.download_surface(p)[1])


@pytest.mark.parametrize("name,sh_format", [(n, 0) for n in ["cloud", "trs", "inside", "fisheye175", "shapes+eigen"]] + [("cloud", 1), ("cloud", 2), ("trs", 2)])
@pytest.mark.parametrize("lens", [False, True])
def test_packed_compositor_shows_the_nearest_fragment(scenes, name, sh_format, lens):
    """k_composite_gut2 (the default 3DGUT frame) cannot count, but with the opacity gaussian disabled every fragment is opaque: the pixel
    is the colour of the nearest fragment's particle — which names the particle — with alpha 1, or 0 where there is none.  lens: depth of
    field with aperture 0 selects XT 1; gutLensSample scales the lens offset by sqrt(rand * aperture) = 0, so the origin does not move
    and the direction is normalize(d * focus_dist), d again up to rounding: the same picture."""
    c, scene = gc.case(name), scenes(name, sh_format)
    kw = dict(dof_mode=capi.DOF_FIXED_FOCUS, aperture=0.0, focus_dist=1.0) if lens else {}
    # SHF 0 / 1 / 2 of k_composite_gut2: the sets' SH (degree 1) is all zero and is read with sh_degree = 1.  fp32 and fp16 keep the zeros,
    # so the colour is the particle's exactly; the uint8 storage dequantises a zero to 1/255, a radiance of at most 0.17 colour steps
    p = frame_params(name, debug_flags=4, sh_degree=1, **kw)
    out = scene.render(p, want_stats=True)
    assert out.error_flags == 0
    img = scene.download_frame(p).astype(np.float32)
    ref = gc.reference_fragments(name)
    n0 = c["sets"][0][0]["positions"].shape[0]
    want = np.where(ref.nearest_id >= 0, ref.nearest_id % n0, -1)   # the instances of a set share its colours
    got = gc.decode_colour(img[..., :3], 0.25 if sh_format == 2 else 1e-3)
    settled = ~ref.nearest_open & ~ref.borderline
    bad = (got != want) & settled
    print(f"3DGUT packed compositor, {name}, lens {lens}: {int(settled.sum())} settled pixels of {settled.size}, {int((got != want).sum())} differ in all")
    assert not bad.any(), ng.describe(ref, got, want, bad)
    assert np.array_equal(img[..., 3][settled], (want >= 0).astype(np.float32)[settled])
    assert np.all(img[settled & (want < 0)] == 0.0)


@pytest.mark.parametrize("name", gc.GAUSS_CASES)
@pytest.mark.parametrize("compositor", ["packed", "tile"])
def test_blend_with_the_gaussian_on_lies_in_the_float64_interval(scenes, name, compositor):
    """the real blend (alpha clamp, response * opacity, front-to-back weights, the T >= 1e-4 saturation test) of k_composite_gut2 (the
    default frame) and of k_composite_gut (XT 2: the same frame with the surface outputs on), RGBA32F: every channel of every non-fragile
    pixel within the float64 interval between "every borderline fragment in" and "out", widened by BAR_FACTOR times the oracle frame's
    own distance from it (gut_cases.GAUSS_DEV, measured by test_gut_cpu.py)."""
    scene = scenes(name)
    p = frame_params(name, **(dict(surface_outputs=1) if compositor == "tile" else {}))
    assert scene.render(p, want_stats=True).error_flags == 0
    img = scene.download_frame(p).astype(np.float64)
    lo, hi, fragile = gc.reference_blend(name)
    assert fragile.mean() <= gc.GAUSS_FRAGILE_CAP
    d = gc.interval_distance(img, lo, hi, fragile)
    print(f"3DGUT blend, {name}, {compositor}: distance from the interval {d:.2e}, tolerance {gc.BAR_FACTOR * gc.GAUSS_DEV[name]:.1e}")
    assert d <= gc.BAR_FACTOR * gc.GAUSS_DEV[name]


RECT_CHILD_CASES = ["shapes", "cloud+eigen", "trs", "inside"]


def test_bin_rectangles_with_32x16_px_bins():
    """the same frames in a process whose bins are forced to 32x16 px (MGS_BIN_SHIFT=1,0: 7 x 9 bins on 200x136): the rectangles rebuilt
    from the ride codes, and those kept by id, equal the bin rectangle of the restatement's pixel window — the boxes of `shapes` that end
    on tile and region edges end on bin edges here"""
    import tempfile
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_gut_rects.py")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rects.npz")
        e = {k: v for k, v in os.environ.items() if k not in ("MGS_DIRECT_BIN", "MGS_BIN_SHIFT", "MGS_DB_TRANSPOSE", "MGS_RECT_RIDE", "MGS_RIDE_SPLIT")}
        e["MGS_BIN_SHIFT"] = "1,0"
        r = subprocess.run([sys.executable, child, out] + RECT_CHILD_CASES, env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
        res = dict(np.load(out))
    for name in RECT_CHILD_CASES:
        prs = gc.projected(name)
        emits, fragile, rect_fragile, w = (gc.stack(prs, k) for k in ("emits", "fragile", "rect_fragile", "window"))
        ids, rect = res[name + "/ids"].astype(np.int64), fc.unpack_rects(res[name + "/rect"])
        got = np.zeros(emits.size, bool)
        got[ids] = True
        assert not ((got != emits) & ~fragile).any()
        sure = emits[ids] & ~rect_fragile[ids]
        want = np.stack([w[ids, 0] // 32, w[ids, 1] // 16, w[ids, 2] // 32, w[ids, 3] // 16], 1)
        bad = (rect != want).any(1) & sure
        print(f"3DGUT rectangles with 32x16-px bins, {name}: {int(sure.sum())} of {ids.size} compared, {np.unique(rect, axis=0).shape[0]} different rectangles")
        assert not bad.any(), [(int(ids[i]), rect[i].tolist(), want[i].tolist()) for i in np.flatnonzero(bad)[:8]]
        assert sure.mean() >= 0.95 and np.unique(rect, axis=0).shape[0] >= 20
