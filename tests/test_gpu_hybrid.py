"""GPU tests (-m gpu) of hybrid frames (mgs_render_hybrid) against the float64 restatement np_hybrid.py fed the GPU's own raster
G-buffer: one child process renders every case of hybrid_cases.py and the further checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hybrid_cases as hc
import lighting_cases
import np_lighting as nl
import np_trace
import np_trace_lit as ntl
from oracle import binding as ob

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("image", "depth", "id", "normal")


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hybrid") / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_hybrid.py"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _gbuffer(child, tag):
    return tuple(child[f"{tag}_u_{k}"] for k in KEYS)


def _against_restatement(child, tag, case, inst=None):
    """every assertion of a frame against np_hybrid fed the unlit frame's G-buffer; returns (psnr, worst non-fragile error, fragile share)"""
    for k in KEYS[1:]:
        assert child[f"{tag}_u_{k}"].tobytes() == child[f"{tag}_h_{k}"].tobytes(), f"the hybrid frame changed the raster pass's {k}"
    g = _gbuffer(child, tag)
    stored = nl.from_target(g[0])
    r = hc.restate_with(case, (stored,) + g[1:], inst or hc.prepared(case))
    ok, st = ~r["fragile"], r["state"]
    got = child[f"{tag}_h_image"]
    img = nl.from_target(got).astype(np.float64)
    assert np.array_equal(child[f"{tag}_shadow_hits"][ok], r["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
    assert not got[ok & (st == 1)].any(), "a discarded pixel is not (0,0,0,0)"
    # (state 2, a valid surface without a picked id, occurs in no raster frame of these scenes: for it this assertion is vacuous on
    # the GPU, and neither the -1 marker of k_hybrid_surface nor the leave-alone branch of k_trace_light runs; that rule is covered
    # by the restatement alone, test_hybrid_cpu.py::test_invalid_id_passes_through_and_thresholds, on an edited G-buffer)
    keep = (st == 0) | (st == 2)
    assert got[keep].tobytes() == g[0][keep].tobytes(), "a pixel outside the field of view or without a picked id changed"
    psnr = np_trace.psnr_rgb(img, r["image"])
    with np.errstate(invalid="ignore"):
        worst = np.abs(img[..., :3] - r["image"][..., :3])[ok].max()
    share = r["fragile"].mean()
    print(f"{tag}: PSNR {psnr:.2f} dB, worst non-fragile pixel error {worst:.3e}, fragile {share:.4f}, light_ms {float(child[f'{tag}_light_ms']):.3f}")
    assert share <= hc.FRAGILE_CAP
    lo, hi = int(r["rays"][ok].sum()), int(r["rays"][ok].sum() + 64 * (~ok).sum())
    assert lo <= int(child[f"{tag}_shadow_rays"]) <= hi
    if ok.all():
        assert int(child[f"{tag}_shadow_rays"]) == int(r["rays"].sum())
    assert int(child[f"{tag}_shadow_accepted"]) == int(child[f"{tag}_shadow_hits"].sum())
    assert int(child[f"{tag}_error_flags"]) == 0
    assert int(child[f"{tag}_sorted"]) == int(child[f"{tag}_u_sorted"]) > 0  # `out` is filled as mgs_render fills it
    return psnr, worst, r


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_case_against_restatement(child, name):
    psnr, _, r = _against_restatement(child, name, hc.cases()[name])
    assert psnr >= 50.0
    if name == "h11_thin_cloud":
        assert (r["state"] == 1).all() and not child[f"{name}_h_image"].any()
    else:
        assert (r["state"] == 3).sum() >= 300


def test_shadows_off_equals_the_deferred_raster_pass(child):
    """h09 (pinhole, shadows off, every light in range): the hybrid frame's rgb against mgs_render with lighting_mode = 1 within the
    deferred pass's own bar; the two differ only in the rounding of the view direction and of the position"""
    c = hc.cases()["h09_shadows_off"]
    r = hc.restate_with(c, _gbuffer(child, "h09_shadows_off"), hc.prepared(c))
    s = r["surface"]
    a, b = child["h09_shadows_off_h_image"], child["h09_deferred_image"]
    ok, _ = lighting_cases.pixel_ok(a[s][:, :3], b[s][:, :3].astype(np.float64), "f32", lighting_cases.GPU_BAR)
    print(f"hybrid vs deferred pass: worst |difference| {np.abs(a[s][:, :3].astype(np.float64) - b[s][:, :3]).max():.3e} over {int(s.sum())} pixels")
    assert s.sum() > 1000 and ok.all()


# What the fp32 lit value of a pixel may differ from its float64 restatement by, relative to the value: the position the light
# vector is formed from carries 2 d_pos <= 2e-5 (np_hybrid, hybrid_cases: d_pos <= 9.5e-6) over a light distance of ~2, i.e. 1e-5
# in the attenuation and in n.l; the ~50 fp32 operations of the shading chain add 50 x 2^-24 = 3e-6; the ramp of the shadow's
# transmittance divides T's 1e-6 by 1 - threshold = 0.7.  Sum 1.5e-5, doubled for contraction in the compiled kernel, rounded up.
TARGET_WINDOW = 4e-5
# share of the non-fragile pixels whose four channels have ONE possible stored value inside that window (measured: f16 0.788,
# u8 0.982; a pixel counts only when all four channels are sure, and an f16 unit is 5e-4 to 1e-3 of the value)
SURE_FLOOR = dict(f16=0.75, u8=0.97)


def _ordered(stored):
    """stored values as numbers that order like them (f16: its float value; u8: the integer)"""
    return stored.astype(np.float64)


@pytest.mark.parametrize("tag", ["f16", "u8"])
def test_target_formats_bit_for_bit(child, tag):
    """An RGBA16F / RGBA8 frame equals the converted RGBA32F lit values computed from the G-buffer of a frame of that format.  The
    device rounds ITS fp32 lit value once; the float64 restatement of that value is known to TARGET_WINDOW (relative: a value that
    is exactly 0 stays 0), so per channel the stored value must lie between the conversions of the window's two ends — which are
    the same stored value or neighbours — on EVERY non-fragile pixel, and equal them bit for bit where they coincide.  On top:
    the frame against the converted restatement at the bar of the frames (50 dB), and every check of a case."""
    c = hc.cases()["h07_translucent_s1"]
    g = _gbuffer(child, "target_" + tag)
    assert g[0].dtype == (np.float16 if tag == "f16" else np.uint8)
    r = hc.restate_with(c, (nl.from_target(g[0]),) + g[1:], hc.prepared(c))
    got = child[f"target_{tag}_h_image"]
    ok = ~r["fragile"]
    e = r["image"]
    a, b = e * (1.0 - TARGET_WINDOW), e * (1.0 + TARGET_WINDOW)
    lo, hi = nl.to_target(np.minimum(a, b), tag), nl.to_target(np.maximum(a, b), tag)
    assert got.dtype == lo.dtype
    nxt = np.minimum(lo.astype(np.int64) + 1, 255) if tag == "u8" else np.nextafter(lo, np.float16(np.inf))
    assert (_ordered(hi) <= _ordered(nxt))[ok].all()  # the two ends are one stored value or neighbours
    inside = (_ordered(lo) <= _ordered(got)) & (_ordered(got) <= _ordered(hi))
    assert inside[ok].all(), f"{int((~inside[ok]).sum())} channel values outside the conversions of the window's ends"
    sure = (lo == hi).all(-1) & ok
    share = sure.sum() / ok.sum()
    print(f"target {tag}: {share:.4f} of the non-fragile pixels have one possible stored value")
    assert share >= SURE_FLOOR[tag] and got[sure].tobytes() == lo[sure].tobytes()
    psnr_stored = np_trace.psnr_rgb(nl.from_target(got).astype(np.float64), nl.from_target(nl.to_target(e, tag)).astype(np.float64))
    print(f"target {tag}: PSNR against the converted restatement {psnr_stored:.2f} dB")
    assert psnr_stored >= 50.0
    _against_restatement(child, "target_" + tag, c)


@pytest.mark.parametrize("tag", ["f16", "u8"])
def test_quantised_storage_against_restatement(child, tag):
    c = hc.cases()["h07_translucent_s1"]
    arrays, M = c["sets"][0]
    inst = [(ntl.prepare_set(arrays, rgba=child[f"store_{tag}_rgba"], sh=child[f"store_{tag}_sh"]), M)]
    psnr, _, _ = _against_restatement(child, "store_" + tag, c, inst)
    assert psnr >= 50.0


def test_temporal_accumulation_after_the_light_pass(child):
    singles, acc = child["dof_singles"].astype(np.float32), child["dof_accumulated"].astype(np.float32)
    assert not np.array_equal(singles[0], singles[2])
    main = np.zeros_like(singles[0])
    for k in range(3):
        main = ob.post_accumulate(main, singles[k], k)
        err = float(np.abs(acc[k] - main).max())
        print(f"temporal accumulation of hybrid frames, sample {k}: worst error {err:.3e}")
        assert err <= 1e-3, k  # the bar of the lit traced frames


def test_determinism_strips_context(child):
    assert child["same_twice"]
    assert all(child[f"strip_{r}"] for r in range(3))
    assert child["context_same"] and child["context_rebuilt"] == 0


def test_other_paths_untouched_and_the_hierarchy_is_shared(child):
    assert child["traced_lit_same_after"] and child["raster_same_after"]
    assert child["traced_lit_rebuilt_after_hybrid"] == 0
    assert child["hit_counts_refused"]


def test_working_bytes_count_the_scratch(child):
    # across the first hybrid frame of a handle that has rendered the unlit frame: ray parameter, radiance, shadow hits and the
    # normalised normal (the hierarchy is the scene's and counts into scene_bytes)
    assert int(child["working_bytes_growth"]) >= 48 * 40 * (4 + 16 + 4 + 16)
    assert int(child["working_bytes_after_traced_lit"]) >= 48 * 40 * 16  # ... of which a lit traced frame allocates all but the last


def test_bound_occluder_is_refused(child):
    msg = str(child["occluder_refusal"])
    assert msg.startswith("-8 ") and "mgs_frame_set_occluder(handle, NULL, NULL, 0, 0)" in msg  # MGS_ERR_UNSUPPORTED
    assert child["same_after_refusal"]
