"""mgs_render_traced with the stochastic trace strategies on the device against the float64 restatement (np_trace_stochastic.py),
one child process per case.  Pass-stochastic frames are compared per pixel (the device makes the restatement's draws); any-hit frames
structurally per pixel and, like the pass-stochastic ones, in distribution: the mean of N samples against the restatement's exact
outcome distribution within Bernstein's bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import np_trace
import np_trace_stochastic as nts
import trace_cases as tc
import trace_stochastic_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN = [n for n in sorted(sc.cases()) if sc.cases()[n]["sets"] and n not in ("g_ties", "h_ring")]


def run_child(tmp_path, *args):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_trace_stochastic.py"), args[0], out, *args[1:]], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def device_ray_hits(name, got):
    """the restatement's per-ray part, fed what the device holds when the case commits quantised colours and SH"""
    case = sc.cases()[name]
    if case["commit"] != "u8":
        return sc.ray_hits(name)
    sets = [(np_trace.prepare_set(a, rgba=got[f"rgba_{k}"], sh=got[f"sh_{k}"]), M) for k, (a, M) in enumerate(case["sets"])]
    return sc.ray_hits_with(case, sets)


@pytest.mark.parametrize("name", PLAIN)
def test_pass_stochastic_matches_restatement(name, tmp_path):
    got = run_child(tmp_path, "case", name)
    R = device_ray_hits(name, got)
    for sid in sc.SAMPLE_IDS:
        ref = sc.pass_sample(name, sid, R=R)
        g = {k: got[f"pass{sid}_{k}"] for k in ("image", "hits", "depth", "id", "normal")}
        ok = ~ref["fragile"]
        assert ref["fragile"].mean() <= 0.02
        psnr = np_trace.psnr_rgb(g["image"], ref["image"])
        print(f"{name} sample {sid}: PSNR {psnr:.2f} dB, worst non-fragile error {np.abs(g['image'] - ref['image'])[ok].max(initial=0.0):.3e}, "
              f"hit counts differ on {(g['hits'][ok] != ref['hits'][ok]).sum()}, ids on {(g['id'].astype(np.int64)[ok] != ref['id'][ok]).sum()} pixels")
        assert set(np.unique(g["image"][..., 3])) <= {0.0, 1.0}
        assert np.array_equal(g["hits"][ok], ref["hits"][ok])
        assert np.array_equal(g["id"].astype(np.int64)[ok], ref["id"][ok])
        assert (np.abs(g["depth"].astype(np.float64) - ref["depth"]) - ref["depth_tol"])[ok].max(initial=0.0) <= 0.0
        assert np.abs(g["normal"].astype(np.float64) - ref["normal"])[ok].max(initial=0.0) <= 2e-3
        assert psnr >= 50.0
        assert int(got[f"pass{sid}_accepted_hits"]) == int(g["hits"].sum())
    assert got["pass0_image"].tobytes() != got["pass5_image"].tobytes()


@pytest.mark.parametrize("name", PLAIN)
def test_anyhit_structure(name, tmp_path):
    got = run_child(tmp_path, "case", name)
    R = device_ray_hits(name, got)
    img, hits, ids = got["any_image"].astype(np.float64), got["any_hits"], got["any_id"].astype(np.int64)
    assert set(np.unique(img[..., 3])) <= {0.0, 1.0} and set(np.unique(hits)) <= {0, 1}
    traced = R["OK"]
    assert np.array_equal(hits[traced], img[..., 3][traced].astype(np.int64)) and not hits[~traced].any()
    assert int(got["any_max_passes_used"]) == 1 and int(got["any_accepted_hits"]) == int(hits.sum())
    assert hits.sum() > 20
    worst = 0.0
    for y, x in zip(*np.nonzero(hits)):
        e = [h for h in R["hits"][y][x] if h["acc"] and h["gid"] == ids[y, x]]
        if R["fragile"][y, x]:
            continue
        assert len(e) == 1, (y, x, ids[y, x])
        e = e[0]
        worst = max(worst, np.abs(img[y, x, :3] - e["col"]).max())
        assert np.abs(img[y, x, :3] - e["col"]).max() <= 1e-4
        z, tol = nts.depth_and_tol(R, y, x, e["t"], e["d_t"])
        assert abs(float(got["any_depth"][y, x]) - z) <= tol
        assert np.abs(got["any_normal"][y, x, :3] - e["nrm"]).max() <= 2e-3 and got["any_normal"][y, x, 3] == 1.0
    print(f"{name}: {int(hits.sum())} kept hits, worst radiance error {worst:.3e}")
    none = (hits == 0) & traced
    assert not img[none].any() and (ids[none] == np_trace.INVALID).all() and not got["any_normal"][none].any() and not got["any_depth"][none].any()


@pytest.mark.parametrize("name", PLAIN + ["g_ties", "h_ring"])
def test_anyhit_without_gaussian_opacity_is_the_nearest_accepted_hit(name, tmp_path):
    """MGS_DEBUG_OPACITY_GAUSSIAN_DISABLED: every accepted hit has alpha 1 and is always kept, so the frame is strategy 0's of the same
    case with that flag: the NEAREST accepted hit, per pixel, whatever the traversal cut (every case: instances under a transform,
    fisheye rays, quantised storage, candidates that are not accepted in front of the first accepted one)"""
    got = run_child(tmp_path, "case", name)
    case = sc.cases()[name]
    case = dict(case, frame=dict(case["frame"], debug_flags=case["frame"].get("debug_flags", 0) | 4))
    sets = sc.prepared(case)
    if case["commit"] == "u8":
        sets = [(np_trace.prepare_set(a, rgba=got[f"rgba_{k}"], sh=got[f"sh_{k}"]), M) for k, (a, M) in enumerate(case["sets"])]
    ref = tc.restate_with(case, sets)
    ok = ~ref["fragile"]
    g = {k: got[f"anyopaque_{k}"] for k in ("image", "hits", "depth", "id", "normal")}
    err = np.abs(g["image"].astype(np.float64) - ref["image"])[ok].max(initial=0.0)
    print(f"{name}: fragile {ref['fragile'].mean():.4f}, {int((ref['hits'] > 0).sum())} rays with a hit, worst non-fragile pixel error {err:.3e}")
    assert ref["fragile"].mean() <= 0.02 and (ref["hits"][ok] > 0).sum() > 20
    assert np.array_equal(g["id"].astype(np.int64)[ok], ref["id"][ok]) and np.array_equal(g["hits"][ok], ref["hits"][ok])
    assert (np.abs(g["depth"].astype(np.float64) - ref["depth"]) - ref["depth_tol"])[ok].max(initial=0.0) <= 0.0
    assert np.abs(g["normal"].astype(np.float64) - ref["normal"])[ok].max(initial=0.0) <= 2e-3
    assert np_trace.psnr_rgb(g["image"], ref["image"]) >= 50.0
    if name in ("g_ties", "h_ring"):   # the flag is the case's own: the plain any-hit frame is the same frame
        assert all(got[f"any_{k}"].tobytes() == g[k].tobytes() for k in g)
    if name == "g_ties":
        # some compared ray's nearest accepted hit is a particle with a bit-identical copy at caller index + 160 (the id equality above
        # then says that the lower copy was picked)
        assert (ok & (ref["id"] < 40)).sum() > 5
    elif name == "h_ring":
        # eight different particles with bit-identical t on the central ray: the lowest caller's id wins although another is stored first
        order = got["storage_order_0"]
        ring_in_storage = order[np.isin(order, np.arange(tc.RING))]
        assert ring_in_storage[0] != 0 and ok[12, 16] and int(got["any_id"][12, 16]) == 0


def test_mechanics(tmp_path):
    r = run_child(tmp_path, "mechanics")
    assert r["first_rebuilt"] == 1 and r["switch_rebuilt"] == 0 and r["explicit_0_equals_null"]
    for s in (1, 2):
        assert r[f"s{s}_same_twice"] and r[f"s{s}_other_sample_differs"] and r[f"s{s}_strip"] and r[f"s{s}_two_strips"] and r[f"s{s}_context"], s
        assert r[f"s{s}_accepted_equals_sum"], s
    assert r["s2_max_passes_used"] == 1


def test_empty_scene_and_fisheye_border(tmp_path):
    e = run_child(tmp_path, "case", "f_empty")
    for k in ("pass0", "any"):
        assert not e[f"{k}_image"].any() and not e[f"{k}_hits"].any()
    f = run_child(tmp_path, "case", "d_fisheye_k04")
    outside = ~sc.ray_hits("d_fisheye_k04")["OK"]
    assert outside.any()
    for k in ("pass0", "any"):
        assert (f[f"{k}_image"][outside] == (0, 0, 0, 1)).all()


def test_both_strategies_converge_to_the_blend(tmp_path):
    """N samples accumulated by the library against the restatement's exact outcome distribution: Bernstein's inequality with L = 20
    (failure probability <= 2 e^-20 per comparison), per pixel and channel and for the frame-wide average; 1e-4 is slack for the fp32
    running mean"""
    r = run_child(tmp_path, "stat")
    R, case = sc.ray_hits(sc.STAT_CASE), sc.cases()[sc.STAT_CASE]
    ok = ~R["fragile"]
    for s, dist in ((1, nts.pass_distribution(R, samples_per_pass=case["trace"]["samples_per_pass"], min_transmittance=0.0)), (2, nts.anyhit_distribution(R))):
        mu, var, rng = nts.moments(dist)
        a, b, ra, rb = nts.bernstein_ok(r[f"mean_{s}"].astype(np.float64), mu, var, rng, ok, sc.N_STAT)
        print(f"strategy {s}: {sc.N_STAT} samples in {float(r[f'seconds_{s}']):.2f} s; worst |mean - mu| / bound per pixel {ra:.3f}, frame-wide {rb:.3f}")
        assert a and b
