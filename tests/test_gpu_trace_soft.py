"""GPU tests (-m gpu) of soft shadows (MGS_SHADOWS_SOFT) in lit traced frames and hybrid frames against the float64 restatement
np_trace_soft.py: one child process renders every case of trace_soft_cases.py and the further checks.  The bars are
test_gpu_trace_lit.py's and test_gpu_hybrid.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import np_lighting as nl
import np_trace
import trace_soft_cases as sc
from oracle import binding as ob

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_ARG, STATE, UNSUPPORTED = -1, -6, -8


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("trace_soft") / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_trace_soft.py"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", sc.traced())
def test_case_against_restatement(child, name):
    r = sc.restate(name, 0)
    ok = ~r["fragile"]
    img = child[f"{name}_image"].astype(np.float64)
    assert np.array_equal(child[f"{name}_hits"][ok], r["base"]["hits"][ok])
    assert np.array_equal(child[f"{name}_id"][ok].astype(np.int64), r["base"]["id"][ok])
    assert np.array_equal(child[f"{name}_shadow_hits"][ok], r["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
    none = ok & ~r["surface"]  # discarded pixels are exactly (0,0,0,0); outside the fisheye circle the frame stays (0,0,0,1)
    assert np.array_equal(img[none], r["image"][none]) and not img[none][:, :3].any(), "a discarded pixel is not (0,0,0,0)"
    psnr = np_trace.psnr_rgb(img, r["image"])
    worst = np.abs(img[..., :3] - r["image"][..., :3])[ok].max()
    print(f"{name}: PSNR {psnr:.2f} dB, worst non-fragile pixel error {worst:.3e}, fragile {r['fragile'].mean():.4f}, "
          f"light_ms {float(child[f'{name}_light_ms']):.3f}")
    assert psnr >= 50.0
    lo, hi = int(r["rays"][ok].sum()), int(r["rays"][ok].sum() + 64 * (~ok).sum())
    assert lo <= int(child[f"{name}_shadow_rays"]) <= hi
    assert int(child[f"{name}_shadow_accepted"]) == int(child[f"{name}_shadow_hits"].sum())


@pytest.mark.parametrize("name", sc.meshed())
def test_mesh_case_against_restatement(child, name):
    """a lit frame with trace meshes: both loops over the lights of a pixel draw from one state.  test_gpu_trace_mesh.py's bars"""
    for sid, img_key, sh_key in ((0, f"{name}_image", f"{name}_shadow_hits"), (1, f"{name}_sample1_image", f"{name}_sample1_shadow_hits")):
        r = sc.restate_mesh(name, sid)
        ok = ~r["fragile"]
        img = child[img_key].astype(np.float64)
        assert np.array_equal(child[sh_key][ok], r["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
        both, fresh = r["both_loops"] & ok, r["mesh_loop_fresh"] & ok
        assert both.sum() >= 50 and fresh.sum() >= 50, "the case must run both loops on some pixels and the mesh loop alone on others"
        psnr = np_trace.psnr_rgb(img, r["image"])
        worst = np.abs(img[..., :3] - r["image"][..., :3])[ok].max()
        worst_both = np.abs(img[..., :3] - r["image"][..., :3])[both].max()
        print(f"{name} sample {sid}: PSNR {psnr:.2f} dB, worst non-fragile pixel error {worst:.3e} (pixels with both loops: {int(both.sum())}, worst "
              f"{worst_both:.3e}; mesh loop from the fresh seed: {int(fresh.sum())}), fragile {r['fragile'].mean():.4f}")
        assert psnr >= 50.0 and r["fragile"].mean() <= sc.FRAGILE_CAP
        if sid == 0:
            assert np.array_equal(child[f"{name}_hits"][ok], r["hits"][ok])
            lo, hi = int(r["shadow_rays"][ok].sum()), int(r["shadow_rays"][ok].sum() + 64 * (~ok).sum())
            assert lo <= int(child[f"{name}_shadow_rays"]) <= hi
    assert child["s06_same_twice"] and child["s06_zero_radii_is_hard"] and all(child[f"s06_strip_{k}"] for k in range(3))


@pytest.mark.parametrize("name", sc.hybrids())
def test_hybrid_case_against_restatement(child, name):
    g = tuple(child[f"{name}_u_{k}"] for k in ("image", "depth", "id", "normal"))
    r = sc.restate_hybrid(name, (nl.from_target(g[0]),) + g[1:], 0)
    ok, st = ~r["fragile"], r["state"]
    got = child[f"{name}_image"]
    img = nl.from_target(got).astype(np.float64)
    assert np.array_equal(child[f"{name}_shadow_hits"][ok], r["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
    assert not got[ok & (st == 1)].any(), "a discarded pixel is not (0,0,0,0)"
    keep = (st == 0) | (st == 2)
    assert got[keep].tobytes() == g[0][keep].tobytes()
    psnr = np_trace.psnr_rgb(img, r["image"])
    with np.errstate(invalid="ignore"):
        worst = np.abs(img[..., :3] - r["image"][..., :3])[ok].max()
    print(f"{name}: PSNR {psnr:.2f} dB, worst non-fragile pixel error {worst:.3e}, fragile {r['fragile'].mean():.4f}")
    assert psnr >= 50.0 and r["fragile"].mean() <= sc.FRAGILE_CAP and (st == 3).sum() >= 300
    lo, hi = int(r["rays"][ok].sum()), int(r["rays"][ok].sum() + 64 * (~ok).sum())
    assert lo <= int(child[f"{name}_shadow_rays"]) <= hi
    assert child[f"{name}_zero_radii_is_hard"]


def test_zero_radii_and_directional_lights_are_the_hard_frame(child):
    assert child["zero_radii_is_hard"] and child["directional_is_hard"]


def test_determinism_and_sample_ids(child):
    assert child["same_twice"] and child["second_rebuilt"] == 0
    r0, r1 = sc.restate("s01_penumbra", 0), sc.restate("s01_penumbra", 1)
    ok = ~r0["fragile"] & ~r1["fragile"]
    pen = ok & (np.abs(r0["shadow_T"] - r1["shadow_T"]).max((2, 3)) > 1e-3) & (np.abs(r0["image"] - r1["image"]).max(-1) > 1e-4)
    a, b = child["s01_samples"][0], child["s01_samples"][1]
    differ = (a != b).any(-1)
    print(f"penumbra pixels whose restated frames differ between sample ids 0 and 1: {int(pen.sum())}; device pixels that differ: {int(differ.sum())}")
    assert pen.sum() >= 20 and differ[pen].all()
    no_ray = ok & (r0["rays"] == 0)
    assert no_ray.any() and a[no_ray].tobytes() == b[no_ray].tobytes()
    assert np.array_equal(child["s01_sample1_shadow_hits"][ok], r1["shadow_hits"][ok])
    # the lens's state is its own: a second sample of the depth-of-field case against its restatement
    r = sc.restate("s05_fisheye_dof", 1)
    psnr = np_trace.psnr_rgb(child["s05_sample1_image"].astype(np.float64), r["image"])
    print(f"s05_fisheye_dof sample 1: PSNR {psnr:.2f} dB")
    assert psnr >= 50.0


def test_strips_and_context(child):
    assert all(child[f"strip_{r}"] for r in range(3))
    assert child["context_same"] and child["context_rebuilt"] == 0


def test_temporal_accumulation_of_soft_frames(child):
    singles, acc = child["s01_samples"].astype(np.float32), child["accumulated"].astype(np.float32)
    main = np.zeros_like(singles[0])
    for k in range(3):
        main = ob.post_accumulate(main, singles[k], k)
        err = float(np.abs(acc[k] - main).max())
        print(f"temporal accumulation of soft frames, sample {k}: worst error {err:.3e}")
        assert err <= 1e-3, k  # the bar of the lit frames (test_gpu_trace_lit.py)


def test_mean_of_sixteen_samples(child):
    rs = [sc.restate("s01_penumbra", k) for k in range(16)]
    want = np.mean([r["image"] for r in rs], 0)
    got = child["s01_samples"].astype(np.float64).mean(0)
    psnr = np_trace.psnr_rgb(got, want)
    print(f"mean of 16 sample ids: PSNR {psnr:.2f} dB")
    assert psnr >= 50.0


def test_radii_interface(child):
    assert child["count_mismatch_code"] == INVALID_ARG and child["negative_code"] == INVALID_ARG and child["nan_code"] == INVALID_ARG
    assert child["context_setter_code"] == STATE
    assert child["same_after_refusals"] and child["radius_one_differs"]
    assert child["set_lights_resets"] and child["null_restores"]


def test_entry_points_that_stay_without_soft_shadows(child):
    assert child["indirect_code"] == UNSUPPORTED and child["shade_points_code"] == UNSUPPORTED
    assert child["same_after_all"]


def test_other_paths_untouched_by_soft_frames(child):
    assert child["hard_same_after"] and child["unlit_same_after"] and child["raster_same_after"]
