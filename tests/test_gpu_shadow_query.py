"""Shadow and light queries (mgs_trace_shadow_rays, mgs_shade_points and their _device variants) on the device against the float64
restatement np_shadow_query.py, one child process per group.  Hits are exact on non-fragile items; the transmittance bar is
gut_cases.BAR_FACTOR times shadow_query_cases.TWIN_DEV (test_gpu_trace_lit.py has no separable bar for the shadow term); colours meet
the lit frames' 50 dB."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gut_cases as gc
import np_shadow_query as nsq
import np_trace
import np_trace_lit as ntl
import shadow_query_cases as sq

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INT_STATS = ("node_visits", "candidate_tests", "accepted_hits", "max_passes_used", "invalid_rays")
LSTATS = ("shadow_rays", "shadow_node_visits", "shadow_candidate_tests", "shadow_accepted_hits")


def run_child(tmp_path, mode):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_shadow_query.py"), mode, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.fixture(scope="module")
def rays(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("sq_rays"), "rays")


@pytest.fixture(scope="module")
def points(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("sq_points"), "points")


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("sq_edges"), "edges")


def check_rays(got, ref, name, what):
    ok = ref["valid"] & ~ref["fragile"]
    assert ref["fragile"].mean() <= 0.02
    assert np.array_equal(got["hits"][ok].astype(np.int64), ref["hits"][ok]), f"{what}: hits differ on non-fragile rays"
    dev = float(np.abs(got["transmittance"].astype(np.float64) - ref["transmittance"])[ok].max())
    bar = gc.BAR_FACTOR * sq.TWIN_DEV[name]
    print(f"{what}: transmittance worst error {dev:.3e}, bar {bar:.1e}, {int(ref['hits'][ok].sum())} hits")
    assert dev <= bar
    bad = ~ref["valid"]
    assert (got["transmittance"][bad] == 1.0).all() and not got["hits"][bad].any()


@pytest.mark.parametrize("name", sorted(sq.RAY_CONFIGS))
def test_shadow_rays_against_the_restatement(rays, name):
    ref = sq.restate_rays(name)
    got = rays[f"{name}_0"]
    check_rays(got, ref, name, name)
    assert int(rays[f"{name}_0_invalid_rays"]) == int((~ref["valid"]).sum())
    assert int(rays[f"{name}_0_accepted_hits"]) == int(got["hits"].sum()) > 0 and int(rays[f"{name}_0_max_passes_used"]) == 1


@pytest.mark.parametrize("name", sorted(sq.RAY_CONFIGS))
def test_reorder_and_the_host_variant_change_nothing(rays, name):
    base = rays[f"{name}_0"]
    assert rays[f"{name}_1"].tobytes() == base.tobytes() and rays[f"{name}_host"].tobytes() == base.tobytes()
    for k in INT_STATS:
        assert int(rays[f"{name}_1_{k}"]) == int(rays[f"{name}_0_{k}"]), k
    assert int(rays[f"{name}_host_accepted_hits"]) == int(base["hits"].sum())
    assert float(rays[f"{name}_0_reorder_ms"]) == 0.0 and float(rays[f"{name}_1_reorder_ms"]) > 0.0  # the key and the sort ran


@pytest.mark.parametrize("tag", ["f16", "u8"])
def test_quantised_storage_with_the_tint_on(rays, tag):
    """the SH branch of the walk in every storage format: the restatement is fed what mgs_scene_download_set returns"""
    inst = [(ntl.prepare_set(a, rgba=rays[f"store_{tag}_rgba_{k}"], sh=rays[f"store_{tag}_sh_{k}"]), M) for k, (a, M) in enumerate(sq.scene(sq.MAIN))]
    ref = sq.restate_rays_with("thr0_tint", nsq.per_inst(inst, float(np.float32(sq.KMR)), float(np.float32(sq.ACULL)), True))
    check_rays(rays[f"store_{tag}"], ref, "thr0_tint", f"{tag} storage")
    assert rays[f"store_{tag}"].tobytes() != rays["thr0_tint_0"].tobytes()


@pytest.mark.parametrize("name", sorted(sq.POINT_CONFIGS))
def test_shade_points_against_the_restatement(points, name):
    ref = sq.restate_points(name)
    got = points[f"{name}_0"]
    ok = ref["valid"] & ~ref["fragile"]
    assert np.array_equal(got["shadow_hits"][ok].astype(np.int64), ref["shadow_hits"][ok])
    psnr = np_trace.psnr_rgb(got["color"][ok][None], ref["color"][ok][None])
    worst = float(np.abs(got["color"].astype(np.float64) - ref["color"])[ok].max())
    print(f"{name}: PSNR {psnr:.2f} dB, worst non-fragile colour error {worst:.3e}, light_ms unasserted")
    assert psnr >= 50.0  # the lit frames' colour bar (test_gpu_trace_lit.py)
    bad = ~ref["valid"]
    assert not got["color"][bad].any() and not got["shadow_hits"][bad].any() and int(points[f"{name}_0_invalid"]) == int(bad.sum())
    # a point's ray count hangs on needShading and the lights' range decisions alone: the batch holds no point within the margin of a
    # range (test_shadow_query_cpu.py holds it to that), so the count is exact whatever happens inside the shadow walks
    assert not ref["range_fragile"].any()
    assert int(points[f"{name}_0_shadow_rays"]) == int(ref["rays"].sum())
    assert int(points[f"{name}_0_shadow_accepted_hits"]) == int(got["shadow_hits"].sum())
    pts = sq.point_batch()
    emissive = ref["valid"] & (pts["material"] == 0)  # the default material: emission only, bit for bit the radiance
    assert got["color"][emissive].tobytes() == pts["radiance"][emissive].tobytes()


@pytest.mark.parametrize("name", sorted(sq.POINT_CONFIGS))
def test_points_reorder_and_host_variant(points, name):
    base = points[f"{name}_0"]
    assert points[f"{name}_1"].tobytes() == base.tobytes()
    for k in LSTATS:
        assert int(points[f"{name}_1_{k}"]) == int(points[f"{name}_0_{k}"]), k
    assert points[f"{name}_host_refused"]
    keep = np.setdiff1d(np.arange(sq.N), [sq.INVALID_AT[4]])
    assert points[f"{name}_host"][keep].tobytes() == base[keep].tobytes()
    assert int(points[f"{name}_host_invalid"]) == int(points[f"{name}_0_invalid"]) - 1
    if name == "no_shadows":
        assert int(points["no_shadows_built_a_hierarchy"]) == 1  # pure shading built none: the first shadow ray does
        assert int(points["no_shadows_0_shadow_rays"]) == 0


def test_empty_scene_and_empty_batches(edges):
    valid = sq.restate_rays("default")["valid"]
    for reorder in (0, 1):
        got = edges[f"empty_{reorder}"]
        assert (got["transmittance"] == 1.0).all() and not got["hits"].any()
        assert edges[f"empty_{reorder}_stats"].tolist() == [0, 0, 0, 0, int((~valid).sum()), 0]
    assert not edges["empty_points"]["shadow_hits"].any() and edges["empty_points"]["color"].any()
    assert int(edges["zero_rays"]) == 0 and int(edges["zero_points"]) == 0


def test_a_query_leaves_the_frame_and_ignores_bindings(edges):
    assert edges["frame_unchanged"] and edges["bound_equal"] and edges["bound_points_any"]
    assert int(edges["first_rebuilt"]) == 0  # the lit frame built the hierarchy the query shares
    assert int(edges["working_bytes"]) >= sq.N * 8  # a reordered batch's keys and indices belong to the handle


def test_a_moved_instance_rebuilds_the_hierarchy(edges):
    assert int(edges["moved_rebuilt"]) == 1
    whole, moved = edges["whole"], edges["moved"]
    assert moved.tobytes() != whole.tobytes() and (moved["transmittance"].sum() > whole["transmittance"].sum())  # an occluder left
