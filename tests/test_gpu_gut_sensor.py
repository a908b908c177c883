"""GPU tests (-m gpu) of the sensor models (mgs_frame_set_sensor): k_project_gut<true>, the sensor's rays in both 3DGUT compositors and
in mgs_trace_generate_rays, and the binding rules, against the float64 restatement tests/np_gut_sensor.py on the cases of
tests/gut_sensor_cases.py.  Every frame is rendered once, in one child process (tests/_child_gut_sensor.py); the tests compare what it
left.  tests/test_gut_sensor_cpu.py asserts the cases' premises and measures the bars' yardsticks without a device."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fragment_cases as fc
import gut_cases as gc
import gut_sensor_cases as sc
import np_gut as ng
import np_gut_sensor as ns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_gut_sensor.py")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "sensor.npz")
        e = {k: v for k, v in os.environ.items() if not k.startswith("MGS_") or k in ("MGS_LIB", "MGS_RCCL_LIB")}
        r = subprocess.run([sys.executable, child, out], env=e, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
        return dict(np.load(out))


@pytest.mark.parametrize("name", sc.CASES)
def test_records(frames, name):
    """the emitted set and the records of k_project_gut<true> against the restatement; bars as test_gpu_gut_records.py (BAR_FACTOR times
    the oracle's measured deviation on the scene the case is built from); rectangles of non-fragile particles exact"""
    prs = sc.projected(name)
    emits, reason, fragile, rect_fragile = (gc.stack(prs, k) for k in ("emits", "reason", "fragile", "rect_fragile"))
    pr = {k: gc.stack(prs, k) for k in ("cx", "cy", "half1", "half2", "box", "B", "ro", "opacity", "window")}
    ids = frames[name + "/ids"].astype(np.int64)
    assert np.unique(ids).size == ids.size
    got = np.zeros(emits.size, bool)
    got[ids] = True
    differ = (got != emits) & ~fragile
    assert not differ.any(), [(int(i), "emitted" if got[i] else "dropped", ng.REJECTIONS[reason[i]] if reason[i] >= 0 else "emits") for i in np.flatnonzero(differ)[:8]]
    keep = got[ids] & emits[ids] & ~fragile[ids]
    idx, rec, rect = ids[keep], frames[name + "/rec"][keep], frames[name + "/rect"][keep]
    dev, worst = ng.record_deviation(pr, idx, rec)
    bars = {k: gc.BAR_FACTOR * gc.ORACLE_DEV[sc.RECORD_BASE[name]][k] for k in ng.FIELDS}
    print(f"\nsensor records vs float64, {name} ({idx.size} particles of {ids.size} sorted): " + ", ".join(f"{k} {dev[k]:.2e} / {bars[k]:.1e} (#{worst[k]})" for k in ng.FIELDS))
    over = {k: (dev[k], worst[k]) for k in ng.FIELDS if dev[k] > bars[k]}
    assert not over, over
    w = pr["window"][idx]
    want = np.stack([w[:, 0] // 256, w[:, 1] // 128, w[:, 2] // 256, w[:, 3] // 128], 1)
    sure = ~rect_fragile[idx]
    bad = (fc.unpack_rects(rect) != want).any(1) & sure
    assert not bad.any() and sure.mean() >= 0.95


@pytest.mark.parametrize("name", sc.CASES)
def test_fragment_counts(frames, name):
    """exact per-pixel counts of the tile compositor (plain and with the surface outputs) through the additive-alpha count mode; the packed
    compositor (k_composite_gut2 cannot count) and a MGS_SORT_STOCHASTIC frame with every fragment opaque show the nearest fragment's
    particle, alpha = "a fragment".  A stochastic frame cannot be counted either: MGS_SORT_STOCHASTIC forces the coverage alpha mode
    (its pixel's alpha is "a fragment was accepted"), so MGS_ALPHA_SUM has no effect on it; with the opacity gaussian off every fragment
    is accepted and the pixel is the nearest fragment, which is what is compared."""
    c, ref = sc.case(name), sc.reference_fragments(name)
    assert ref.borderline.mean() <= gc.BORDERLINE_CAP["default"]
    for what in ("count_plain", "count_surface"):
        alpha = frames[name + "/" + what]
        got = np.rint(alpha).astype(np.int64)
        assert np.array_equal(got.astype(np.float32), alpha), "the alpha plane of the count mode is not integral"
        off = np.abs(got - ref.count) > np.where(ref.borderline, ref.borderline_count, 0)
        print(f"sensor counts, {name}, {what}: {int(ref.count.sum())} fragments, {int(ref.borderline.sum())} borderline pixels, {int((got != ref.count).sum())} pixels differ")
        assert not off.any(), ng.describe(ref, got, ref.count, off)
    settled = ~ref.nearest_open & ~ref.borderline
    sid = frames[name + "/count_surface_ids"]
    got_id = np.where(sid == 0xFFFFFFFF, -1, sid.astype(np.int64))
    bad = (got_id != ref.nearest_id) & settled
    assert not bad.any(), ng.describe(ref, got_id, ref.nearest_id, bad)
    n0 = c["sets"][0][0]["positions"].shape[0]
    want = np.where(ref.nearest_id >= 0, ref.nearest_id % n0, -1)
    for what in ("opaque_packed", "opaque_stochastic"):
        img = frames[name + "/" + what]
        got = gc.decode_colour(img[..., :3], 1e-3)
        bad = (got != want) & settled & (want >= 0)
        assert not bad.any(), (what, ng.describe(ref, got, want, bad))
    img = frames[name + "/opaque_packed"]
    assert np.array_equal(img[..., 3][settled], (want >= 0).astype(np.float32)[settled]) and np.all(img[settled & (want < 0)] == 0.0)
    # a pixel without a ray holds no fragment in any of them
    noray = ~ref.rays[1] & (ref.rays[2] > sc.DELTA)
    if noray.any():
        assert not frames[name + "/count_plain"][noray].any() and not frames[name + "/opaque_packed"][noray].any()


@pytest.mark.parametrize("name", sc.CASES)
@pytest.mark.parametrize("compositor", ["packed", "tile"])
def test_blend_lies_in_the_float64_interval(frames, name, compositor):
    """as test_blend_with_the_gaussian_on_lies_in_the_float64_interval.  Tolerance: BAR_FACTOR x gut_sensor_cases.GAUSS_DEV, the distance
    of the whole restatement's numpy float32 run from its float64 interval on this case"""
    img = frames[name + "/blend_" + compositor].astype(np.float64)
    lo, hi, fragile = sc.reference_blend(name)
    assert fragile.mean() <= gc.GAUSS_FRAGILE_CAP
    d = gc.interval_distance(img, lo, hi, fragile)
    tol = gc.BAR_FACTOR * sc.GAUSS_DEV[name]
    print(f"sensor blend, {name}, {compositor}: distance from the interval {d:.2e}, tolerance {tol:.1e}")
    assert d <= tol


@pytest.mark.parametrize("name", sc.CASES)
def test_rays(frames, name):
    """the rays mgs_trace_generate_rays writes with the sensor bound: the float64 projection of each lands on its pixel's centre within
    BAR_FACTOR x the residual of the float32 numpy run of the same fixed-count Newton; the pixels without a ray are the restatement's
    outside the fragile mask; the origin is the camera's"""
    c = sc.case(name)
    rays = frames[name + "/rays"]
    _, ok, edge, _ = sc.rays(name)
    sure = edge > sc.DELTA
    has = rays[..., 3] <= rays[..., 7]          # a pixel without a ray gets the invalid window (1, 0)
    assert np.array_equal(has[sure], ok[sure])
    both = has & ok & sure
    assert np.all(rays[..., 3][both] == np.float32(0.001)) and np.all(rays[..., 7][both] == np.float32(10000.0))
    eye = np.linalg.inv(np.asarray(c["cam"][0], np.float64))[:3, 3]
    assert np.abs(rays[..., 0:3] - eye).max() <= 1e-6
    assert np.abs(np.linalg.norm(rays[..., 4:7].astype(np.float64), axis=-1) - 1.0)[both].max() <= 1e-6
    res = float(np.where(both, sc.ray_residual(name, rays[..., 4:7]), 0.0).max())
    print(f"sensor rays, {name}: {int(both.sum())} rays, residual {res:.2e} px, bar {gc.BAR_FACTOR * sc.RAY_RESIDUAL[name]:.1e}")
    assert res <= gc.BAR_FACTOR * sc.RAY_RESIDUAL[name]


def test_binding_rules(frames):
    r = {k[6:]: v for k, v in frames.items() if k.startswith("rules/")}
    same = lambda a, b: np.array_equal(r[a].view(np.uint32), r[b].view(np.uint32))   # noqa: E731  (bit for bit)
    assert same("plain", "plain2") and same("mild", "mild2")
    assert not same("plain", "mild") and not same("mild", "strong")          # binding and rebinding change the replayed frame
    assert same("ctx_plain", "plain") and same("ctx_mild", "mild")           # a context has its own binding ...
    assert same("strong_again", "strong") and same("after_refusals", "strong")   # ... and leaves the scene's alone; so does a refusal
    assert same("restored", "plain") and same("restored_last", "plain")      # unbinding restores the no-sensor frame
    for what in ("3dgs", "lit", "meshes", "traced", "traced_lit", "hybrid"):
        assert bool(r["refuse_" + what]), what
    assert r["works_after_unbinding"].all(), r["works_after_unbinding"]
