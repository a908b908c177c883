"""GPU tests (-m gpu) of lit traced frames (mgs_render_traced_lit) against the float64 restatement np_trace_lit.py: one child process
renders every case of trace_lit_cases.py and the further checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import np_lighting as nl
import np_trace
import np_trace_lit as ntl
import trace_lit_cases as lc
from oracle import binding as ob

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("trace_lit") / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_trace_lit.py"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", sorted(lc.cases()))
def test_case_against_restatement(child, name):
    r = lc.restate(name)
    ok = ~r["fragile"]
    img = child[f"{name}_image"].astype(np.float64)
    assert np.array_equal(child[f"{name}_hits"][ok], r["base"]["hits"][ok])
    assert np.array_equal(child[f"{name}_id"][ok].astype(np.int64), r["base"]["id"][ok])
    assert np.array_equal(child[f"{name}_shadow_hits"][ok], r["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
    none = ok & ~r["surface"]  # discarded pixels are exactly (0,0,0,0); outside the fisheye circle the frame stays (0,0,0,1)
    assert np.array_equal(img[none], r["image"][none]) and not img[none][:, :3].any(), "a discarded pixel is not (0,0,0,0)"
    assert not img[none & (r["base"]["image"][..., 3] != 1.0)].any()
    psnr = np_trace.psnr_rgb(img, r["image"])
    worst = np.abs(img[..., :3] - r["image"][..., :3])[ok].max()
    print(f"{name}: PSNR {psnr:.2f} dB, worst non-fragile pixel error {worst:.3e}, light_ms {float(child[f'{name}_light_ms']):.3f}")
    assert psnr >= 50.0
    lo, hi = int(r["rays"][ok].sum()), int(r["rays"][ok].sum() + 64 * (~ok).sum())
    assert lo <= int(child[f"{name}_shadow_rays"]) <= hi
    if ok.all():
        assert int(child[f"{name}_shadow_rays"]) == int(r["rays"].sum())
    assert int(child[f"{name}_shadow_accepted"]) == int(child[f"{name}_shadow_hits"].sum())


def test_temporal_accumulation_after_the_light_pass(child):
    singles, acc = child["dof_singles"].astype(np.float32), child["dof_accumulated"].astype(np.float32)
    assert not np.array_equal(singles[0], singles[2])
    main = np.zeros_like(singles[0])
    for k in range(3):
        main = ob.post_accumulate(main, singles[k], k)
        err = float(np.abs(acc[k] - main).max())
        print(f"temporal accumulation of lit frames, sample {k}: worst error {err:.3e}")
        assert err <= 1e-3, k  # the bar of the unlit traced frames (test_gpu_trace.py)


def test_target_formats_bit_for_bit(child):
    f32 = child["l07_translucent_s1_image"]
    assert child["target_f16"].tobytes() == nl.to_target(f32, "f16").tobytes()
    assert child["target_u8"].tobytes() == nl.to_target(f32, "u8").tobytes()


@pytest.mark.parametrize("tag", ["f16", "u8"])
def test_quantised_storage_against_restatement(child, tag):
    """fp16 / uint8 SH and colour storage: the restatement is fed what mgs_scene_download_set returns (the SH branch of the shadow
    walk runs: colour strength 1)"""
    c = lc.cases()["l07_translucent_s1"]
    arrays, M = c["sets"][0]
    r = lc.restate_with(c, [(ntl.prepare_set(arrays, rgba=child[f"store_{tag}_rgba"], sh=child[f"store_{tag}_sh"]), M)])
    ok = ~r["fragile"]
    img = child[f"store_{tag}_image"].astype(np.float64)
    assert np.array_equal(child[f"store_{tag}_hits"][ok], r["base"]["hits"][ok])
    assert np.array_equal(child[f"store_{tag}_shadow_hits"][ok], r["shadow_hits"][ok])
    psnr = np_trace.psnr_rgb(img, r["image"])
    print(f"{tag} storage: PSNR {psnr:.2f} dB, worst non-fragile pixel error {np.abs(img[..., :3] - r['image'][..., :3])[ok].max():.3e}")
    assert psnr >= 50.0 and ok.mean() >= 0.95


def test_shadow_hits_belong_to_the_last_lit_frame(child):
    assert child["stale_shadow_hits_refused"]


def test_determinism_strips_context(child):
    assert child["same_twice"] and child["second_rebuilt"] == 0
    assert all(child[f"strip_{r}"] for r in range(3))
    assert child["context_same"] and child["context_rebuilt"] == 0


def test_lights_and_materials_change_the_frame_without_a_rebuild(child):
    assert child["light_changed_frame"] and child["light_changed_rebuilt"] == 0
    assert child["material_changed_frame"] and child["material_changed_rebuilt"] == 0
    assert child["working_bytes"] >= 48 * 40 * (4 + 16 + 4)


def test_other_paths_untouched_by_a_lit_frame(child):
    assert child["unlit_same_after"] and child["raster_same_after"]


def test_default_materials_no_shadows_equal_the_unlit_frame(child):
    surf = lc.restate("l13_shadows_off")["surface"] & ~lc.restate("l13_shadows_off")["fragile"]
    a, b = child["unlit_equal_image_lit"], child["unlit_equal_image_unlit"]
    assert a[surf].tobytes() == b[surf].tobytes()
