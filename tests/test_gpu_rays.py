"""Ray queries (mgs_trace_rays_device, mgs_trace_rays, mgs_trace_generate_rays) on the device, one child process per group.

a. Tied to the traced frames bit for bit: the rays mgs_trace_generate_rays writes, traced as a batch, give the frame mgs_render_traced
   makes of the same parameters.
b. Arbitrary rays against the float64 restatement (np_trace_rays.py) under the bars test_gpu_trace.py holds strategy 0 to.
c. Reorder changes nothing but time.
d. Sizes and edges.   e. The reorder buffers in working_bytes.   f. One hierarchy for every traced entry point of a handle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_cases as rc
from test_gpu_trace import compare

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EMPTY_ID = 0xFFFFFFFF


def run_child(tmp_path, mode):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_rays.py"), mode, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_empty(res):
    assert not bits(res["radiance"]).any() and (res["transmittance"] == 1.0).all() and not bits(res["t_iso"]).any()
    assert (res["id"] == EMPTY_ID).all() and not res["hit_count"].any() and not res["passes"].any() and not bits(res["normal"]).any()


@pytest.fixture(scope="module")
def tied(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("tied"), "tied")


@pytest.mark.parametrize("spp", [4, 18, 32])   # one per K-buffer size
@pytest.mark.parametrize("cam", ["pinhole", "fisheye", "dof"])
def test_generated_rays_give_the_traced_frame_bit_for_bit(tied, cam, spp):
    """k_rays_generate restates primaryRay with the roundings k_trace's code has (k_trace_rays.hip: primaryRayAsTraced), so the rays are
    the bits the frame kernel traces, and the same walk gives the same pixel"""
    tag = f"{cam}_{spp}"
    res, img = tied[tag + "_result"].reshape(24, 40), tied[tag + "_image"]
    rays = tied[cam + "_rays"].reshape(24, 40)
    outside = rays["t_min"] > rays["t_max"]                 # fisheye pixels outside the image circle
    assert outside.any() == (cam == "fisheye") and (~outside).sum() > 500
    assert int(tied[tag + "_invalid_rays"]) == int(outside.sum())
    if outside.any():
        assert (rays["t_min"][outside] == 1.0).all() and (rays["t_max"][outside] == 0.0).all()
        assert_empty(res[outside])
        assert (img[outside] == np.array([0, 0, 0, 1], np.float32)).all()
    ok = ~outside
    assert (rays["t_min"][ok] == np.float32(0.001)).all() and (rays["t_max"][ok] == np.float32(10000.0)).all()
    assert np.array_equal(bits(res["radiance"])[ok], bits(img[..., :3])[ok]) and img[..., :3].any()
    assert np.array_equal(bits(np.float32(1.0) - res["transmittance"])[ok], bits(img[..., 3])[ok])
    assert np.array_equal(res["hit_count"][ok], tied[tag + "_hits"][ok]) and res["hit_count"].max() > 3
    assert np.array_equal(res["id"][ok], tied[tag + "_id"][ok]) and (res["id"][ok] != EMPTY_ID).any()
    assert np.array_equal(bits(res["normal"])[ok], bits(tied[tag + "_normal"])[ok])
    assert ((res["t_iso"] > 0) == (res["id"] != EMPTY_ID)).all()
    assert int(res["passes"].max()) == int(tied[f"{tag}_rays_max_passes_used"]) == int(tied[f"{tag}_frame_max_passes_used"])
    for k in ("node_visits", "candidate_tests", "accepted_hits"):
        assert int(tied[f"{tag}_rays_{k}"]) == int(tied[f"{tag}_frame_{k}"]) > 0, k
    assert int(tied[tag + "_rays_accepted_hits"]) == int(res["hit_count"].sum())


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("batch"), "batch")


def test_arbitrary_rays_match_the_restatement(batch):
    """About 4 000 rays of ray_cases.py: origins inside, outside and far outside the scene box, unit and non-unit directions,
    axis-parallel ones, windows that start inside the scene or cut it in half.  The restatement's fragile share of this batch is
    0.0185 (SEED 7; test_rays_cpu.py holds it to the 0.02 of the frames' cases).  On the other rays: hit counts and picked ids are
    equal and the radiance meets the 50 dB of test_gpu_trace.compare; t_iso follows within the restatement's fp32 tolerance and lies
    inside the ray's window; transmittance and normals as the frames' alpha and normals."""
    ref = rc.restate()
    got = batch["caller_0"]
    _, _, tmin, tmax = rc.batch()
    assert ref["fragile"].mean() <= 0.02                       # the cap test_gpu_trace.py applies to its cases (a literal there too)
    # test_gpu_trace's bars, on the batch as a one-row image
    ref_img = dict(image=np.concatenate([ref["radiance"], (1.0 - ref["transmittance"])[:, None]], 1)[None], hits=ref["hits"][None],
                   id=ref["id"][None], fragile=ref["fragile"][None])
    got_img = np.concatenate([got["radiance"], (np.float32(1.0) - got["transmittance"])[:, None]], 1)[None]
    compare(got_img, got["hit_count"][None].astype(np.int64), ref_img, got["id"][None], "ray batch")
    ok = ~ref["fragile"]
    assert (np.abs(got["transmittance"].astype(np.float64) - ref["transmittance"]) - ref["transmittance_tol"])[ok].max() <= 0.0
    assert np.abs(got["normal"].astype(np.float64) - ref["normal"])[ok].max() <= 2e-3          # test_gpu_trace's bar of the side output
    assert np.array_equal(got["passes"][ok], ref["passes"][ok])
    excess = np.abs(got["t_iso"].astype(np.float64) - ref["t_iso"]) - ref["t_iso_tol"]
    print(f"ray batch: t_iso worst error {np.abs(got['t_iso'].astype(np.float64) - ref['t_iso'])[ok].max():.3e}, largest tolerance "
          f"{ref['t_iso_tol'][ok].max():.3e}")
    assert excess[ok].max() <= 0.0
    # every picked hit lies in its ray's window, fragile or not
    picked = got["id"] != EMPTY_ID
    assert picked.sum() > 1000
    assert (got["t_iso"][picked] > np.maximum(tmin, 0)[picked]).all() and (got["t_iso"][picked] <= tmax[picked]).all()
    # invalid rays: the empty result, counted
    bad = np.array(rc.INVALID_AT)
    assert_empty(got[bad])
    assert int(batch["caller_0_invalid_rays"]) == len(bad)
    assert int(batch["caller_0_accepted_hits"]) == int(got["hit_count"].sum()) and int(batch["caller_0_max_passes_used"]) == int(got["passes"].max())


def test_reorder_changes_nothing_but_time(batch):
    base = batch["caller_0"]
    for name in ("caller_1", "reversed_0", "reversed_1", "shuffled_0", "shuffled_1"):
        assert batch[name].tobytes() == base.tobytes(), name
        for k in ("node_visits", "candidate_tests", "accepted_hits", "max_passes_used", "invalid_rays"):
            assert int(batch[f"{name}_{k}"]) == int(batch[f"caller_0_{k}"]), (name, k)
    assert float(batch["caller_0_reorder_ms"]) == 0.0       # no reorder, no events read (times themselves are not asserted)


def test_entry_points_share_one_hierarchy(tmp_path):
    """Every traced entry point derives the hierarchy's proxy from the same four parameters, so one handle that goes through
    mgs_render_traced, mgs_trace_rays_device, mgs_render_traced_lit, mgs_render_hybrid and mgs_render_traced again builds the
    hierarchy once, and the last frame is the first"""
    r = run_child(tmp_path, "shared")
    assert int(r["first_rebuilt"]) == 1
    assert int(r["query_rebuilt"]) == 0 and int(r["lit_rebuilt"]) == 0 and int(r["last_rebuilt"]) == 0
    assert np.array_equal(r["query_hits"], r["first_hits"]) and r["first_hits"].max() > 3
    assert r["last_image"].tobytes() == r["first_image"].tobytes() and r["first_image"].any()
    assert np.array_equal(r["last_hits"], r["first_hits"])


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("edges"), "edges")


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257])
def test_counts_around_wave_and_workgroup(edges, count):
    for reorder in (0, 1):
        assert edges[f"count_{count}_{reorder}_equal"], reorder       # the first `count` results of the 257-ray batch, bit for bit
        assert edges[f"count_{count}_{reorder}_sentinel"], reorder    # nothing behind the result array is touched
        assert edges[f"count_{count}_{reorder}_hits"], reorder


def test_invalid_batch_empty_scene_host_variant_context_and_memory(edges):
    for reorder in (0, 1):
        assert_empty(edges[f"invalid_{reorder}"])
        assert int(edges[f"invalid_{reorder}_invalid_rays"]) == 300
        assert [int(edges[f"invalid_{reorder}_{k}"]) for k in ("node_visits", "candidate_tests", "accepted_hits", "max_passes_used")] == [0] * 4
        # a scene without instances: valid rays, nothing to hit (a pass is not even started)
        assert_empty(edges[f"empty_{reorder}"])
        assert edges[f"empty_{reorder}_stats"].tolist() == [0] * 5
    assert edges["host_equal"] and edges["host_hits"] and edges["host_reordered_equal"] and int(edges["host_empty"]) == 0
    assert edges["context_equal"] and edges["frame_unchanged"]
    assert edges["nosurf_same"] and edges["nosurf_empty"]          # surface_outputs gates t_iso, id and the normals, nothing else
    m0, m1, m2 = (int(v) for v in edges["working_bytes"])
    assert m1 - m0 >= 2 * 4 * 3000 and m2 == m1
