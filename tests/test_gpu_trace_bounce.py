"""Indirect traced frames (mgs_render_traced_indirect) on the device, one child process per group.

cases     every case of trace_bounce_cases.py against the float64 restatement (np_trace_bounce.py), RGBA32F, with the bars of
          test_gpu_trace_mesh.py: on non-fragile pixels hit counts, picked ids and shadow hit counts (summed over all bounces) are
          equal; surface depth within depth_tol; PSNR >= 50 dB; worst non-fragile channel <= 1e-3; the statistics (rays and mesh hits
          per bounce, accepted hits) between the non-fragile sums and those plus what the fragile pixels may add.
identical every bounce material illum 0 (never set, or set so), or every mesh instance invisible: image, side outputs, hit counts
          and shadow hits byte-identical to mgs_render_traced_lit on the same handle; with the mirrors set the image differs.
unmoved   mgs_render, mgs_render_traced, mgs_render_traced_lit byte-identical before and after; strips; a frame context; target
          formats; the running mean.
lifecycle working_bytes growth, error codes, bounce materials do not rebuild the hierarchy, refusals leave the handle usable."""
import os
import subprocess
import sys

import numpy as np
import pytest

import np_lighting as nl
import np_trace as nt
import np_trace_bounce as ntb
import trace_bounce_cases as tbc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    got = {}

    def run(mode):
        if mode not in got:
            out = str(tmp_path_factory.mktemp(mode) / "out.npz")
            r = subprocess.run([sys.executable, os.path.join(HERE, "_child_trace_bounce.py"), mode, out], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
            got[mode] = np.load(out)
        return got[mode]
    return run


@pytest.mark.parametrize("name", list(tbc.cases()))
def test_case_against_the_float64_restatement(child, name):
    against_restatement(child("cases"), name, tbc.restate(name), tbc.cases()[name])


@pytest.mark.parametrize("fmt", ["f16", "u8"])
def test_quantised_splat_storage_stays_within_the_bars(child, fmt):
    """b1 with fp16 / uint8 colour and SH storage (k_trace_bounce<1, .> and <2, .>), against the restatement of the arrays as the
    device holds them"""
    r, case = child("storage"), tbc.cases()["b1"]
    inst = [(ntb.ntl.prepare_set(a, rgba=r[f"b1_{fmt}_rgba_{k}"], sh=r[f"b1_{fmt}_sh_{k}"]), M) for k, (a, M) in enumerate(case["sets"])]
    against_restatement(r, f"b1_{fmt}", tbc.restate_with(case, inst), case)


@pytest.mark.parametrize("fmt", ["f16", "u8"])
@pytest.mark.parametrize("name", [n for n in tbc.STORAGE_CASES if n != "b1"])
def test_quantised_splat_storage_at_the_k_buffer_ends(child, name, fmt):
    """the same with samples_per_pass 4 and 32 (k_trace_bounce<1 | 2, 4> and <1 | 2, 32>)"""
    r, case = child("storage"), tbc.cases()[name]
    inst = [(ntb.ntl.prepare_set(a, rgba=r[f"{name}_{fmt}_rgba_{k}"], sh=r[f"{name}_{fmt}_sh_{k}"]), M) for k, (a, M) in enumerate(case["sets"])]
    against_restatement(r, f"{name}_{fmt}", tbc.restate_with(case, inst), case)


def test_bare_mirror_adds_specular_times_the_ray_query_of_the_reflected_ray(child):
    """Ties the bounce walk to mgs_trace_rays.  On a mirror pixel with no particle hit in front (T = 1), whose bounce ray meets no
    mesh and whose splat material is emission (1, 1, 1) alone, one bounce adds specular x the radiance the ray query integrates on
    reflect(rayDir, normal) from the downloaded hit record in (0.001, 10000).  The bar: a handful of fp32 products per channel with
    values below 4, 16 ulps of 4 = 1e-5 (test_gpu_trace_mesh.py's)."""
    r, case = child("bare"), tbc.cases()["bare"]
    h = r["mesh"]
    spec = np.array([np.float32(case["meshes"][0]["materials"][int(m)]["specular"]) for m in np.where(h["hit"] == 1, h["material_id"], 0).reshape(-1)],
                    np.float64).reshape(h.shape + (3,))
    bare = (h["hit"] == 1) & (r["hits"] == 0)
    assert bare.sum() > 200
    gain = r["indirect"][..., :3].astype(np.float64) - r["lit"][..., :3].astype(np.float64)
    want = spec * r["walk"]["radiance"].astype(np.float64)
    err = np.abs(gain - want)[bare]
    print(f"bare mirror: {int(bare.sum())} pixels, {int((want[bare] > 0).any(-1).sum())} see the blob, worst {err.max():.2e}")
    assert (want[bare] > 0.01).any(-1).sum() > 20        # the reflection of the blob is in the frame
    assert err.max() <= 1e-5


def against_restatement(r, name, ref, case):
    img, want = r[name + "_image"].astype(np.float64), ref["image"]
    nf, fr = ~ref["fragile"] & ref["ok"], ref["fragile"] & ref["ok"]
    print(f"{name}: fragile {fr.mean():.4f}")
    assert np.array_equal(r[name + "_hits"][nf], ref["hits"][nf])
    assert np.array_equal(r[name + "_id"].astype(np.int64)[nf], ref["id"][nf])
    assert np.array_equal(r[name + "_shadow_hits"][nf], ref["shadow_hits"][nf])
    h, m = r[name + "_mesh"], ref["mesh"]       # the primary hit
    assert np.array_equal((h["hit"] == 1)[nf], m["hit"][nf]) and np.array_equal(h["primitive_id"][nf], m["prim"][nf])
    derr = np.abs(r[name + "_depth"].astype(np.float64) - ref["depth"])
    assert (derr[nf] <= ref["depth_tol"][nf] + 1e-7).all(), float((derr - ref["depth_tol"])[nf].max())
    psnr = nt.psnr_rgb(img, want)
    worst = np.abs(img - want)[nf].max()
    print(f"{name}: PSNR {psnr:.1f} dB, worst non-fragile channel {worst:.2e}, rays {r[name + '_rays'][:case['max_bounces']].tolist()}")
    assert psnr >= 50.0 and worst <= 1e-3
    assert (img[nf & ref["composited"], 3] == 1.0).all()
    # statistics: a non-fragile pixel's path is the restatement's; a fragile one may be live or not at any bounce
    nb = case["max_bounces"]
    rays, hits = r[name + "_rays"], r[name + "_mesh_hits"]
    assert (rays[nb:] == 0).all() and (hits[nb:] == 0).all()
    for b in range(nb):
        lo = int((ref["live"][b] & nf).sum())
        assert lo <= rays[b] <= lo + fr.sum(), (b, lo, int(rays[b]))
        assert hits[b] <= rays[b]
    if fr.sum() == 0:
        assert np.array_equal(rays[:nb], ref["rays"]) and np.array_equal(hits[:nb], ref["mesh_hits"])
        assert int(r[name + "_particle_hits"]) == ref["particle_hits"] and int(r[name + "_accepted"]) == ref["hits"][ref["ok"]].sum()
    assert int(r[name + "_accepted"]) >= ref["hits"][nf].sum() and int(r[name + "_shadow_accepted"]) >= ref["shadow_hits"][nf].sum()


def test_sixteen_rounds_differ_from_three_and_from_one(child):
    r = child("cases")
    a, b, c = (r[f"b2_{n}_image"] for n in (1, 3, 16))
    assert a.tobytes() != b.tobytes() and b.tobytes() != c.tobytes()
    assert r["b2_16_rays"][15] > 0
    assert r["b4_far_rays"].sum() == 0 and r["b4_head_rays"][0] > 0


@pytest.mark.parametrize("name", ["b1", "b3"])
def test_illum_zero_is_the_lit_frame_byte_for_byte(child, name):
    r = child("identical")
    assert r[name + "_none"] and r[name + "_zero"] and r[name + "_invisible"]
    assert r[name + "_zero_rays"].sum() == 0
    assert r[name + "_differs"]


def test_other_entry_points_strips_contexts_formats_accumulation(child):
    r = child("unmoved")
    assert r["others"] and r["strip"] and r["context"]
    full = r["full"]
    assert r["target_f16"].tobytes() == nl.to_target(full, "f16").tobytes() and r["target_u8"].tobytes() == nl.to_target(full, "u8").tobytes()
    assert np.array_equal(r["accum0"], full) and np.array_equal(r["accum1"], full)    # the mean of two equal samples


def test_lifecycle(child):
    r = child("lifecycle")
    assert int(r["growth"]) == 64 * int(r["pixels"]) + 264      # the documented state (64 B a pixel) and the counter block
    assert int(r["rebuilt_after_materials"]) == 0
    assert int(r["code_setting_off"]) == -6 and int(r["code_direct"]) == -1
    assert int(r["code_bounces_0"]) == -1 and int(r["code_bounces_17"]) == -1
    assert int(r["code_context_materials"]) == -6 and int(r["code_bad_ior"]) == -1 and int(r["code_no_instance"]) == -1
    assert r["usable"]
