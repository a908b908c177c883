"""Mesh ray queries (mgs_trace_mesh_rays, mgs_trace_mesh_rays_device) on the device, one child process per group.

a. Closest mode against the float64 brute force (np_mesh_rays.py) under the bars of mesh_ray_cases.py; occlusion mode against closest.
b. The watertight case: exact t and id, no tolerance and no mask.
c. Host = device, reorder changes nothing (integer statistics included), a frame context = the scene handle.
d. Lifecycle: rebuilds, visibility without a rebuild, an empty scene, meshes without splats, scene_bytes.
e. The pick image against the mesh rasteriser.   f. Frames, shadow queries and mesh passes are not disturbed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ray_cases as mrc
import np_mesh_rays as nr
from vk_gaussian_splatting_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
STATS = ("triangles", "leaves", "nodes", "node_visits", "triangle_tests", "hits", "invalid_rays", "bvh_rebuilt")


def run_child(tmp_path, mode):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_mesh_rays.py"), mode, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def split(rays):
    return rays["origin"], rays["direction"], rays["t_min"], rays["t_max"]


def assert_miss(h):
    assert np.isposinf(h["t"]).all() and (h["instance_id"] == NONE).all() and (h["primitive_id"] == NONE).all() and (h["material_id"] == NONE).all()
    assert not h["hit"].any() and not h["position"].any() and not h["normal"].any() and not h["b1"].any() and not h["b2"].any()
    assert not h["reserved"].any()


def against_reference(h, ref, name):
    """closest-mode hits against np_mesh_rays.trace: the issue's rules for non-fragile and fragile rays"""
    ok = ~ref["fragile"]
    hit = h["hit"] == 1
    assert np.array_equal(hit[ok], ref["hit"][ok]), name
    assert np.array_equal(h["primitive_id"][ok], ref["prim"][ok]) and np.array_equal(h["instance_id"][ok], ref["inst"][ok]), name
    assert np.array_equal(h["material_id"][ok], ref["mat"][ok]), name
    got = dict(hit=hit, t=h["t"], b1=h["b1"], b2=h["b2"], pos=h["position"], nrm=h["normal"])
    e = nr.errors(got, ref, ok)
    print(f"{name}: errors {e}, bars t {mrc.GPU_T_BAR:.1e} bary {mrc.GPU_BARY_BAR:.1e} pos {mrc.GPU_POS_BAR:.1e} nrm {mrc.GPU_NRM_BAR:.1e}")
    assert e["t"] <= mrc.GPU_T_BAR and e["bary"] <= mrc.GPU_BARY_BAR and e["pos"] <= mrc.GPU_POS_BAR and e["nrm"] <= mrc.GPU_NRM_BAR, name
    fr = ref["fragile"]
    if fr.any():  # one of the reference's two nearest candidates (NONE = a miss, where the reference has fewer), or a miss at a window end
        assert ((h["primitive_id"][fr] == ref["prim"][fr]) | (h["primitive_id"][fr] == ref["prim2"][fr]) | (~hit[fr] & ref["window_end"][fr])).all(), name
    assert_miss(h[~hit])
    assert (h["t"][hit] > np.maximum(ref_window(ref)[0], 0)[hit]).all() and (h["t"][hit] < ref_window(ref)[1][hit]).all()


def ref_window(ref):
    return ref["_tmin"], ref["_tmax"]


def reference(name, rays, meshes=None):
    O, D, tmin, tmax = split(rays)
    ref = dict(mrc.reference(name, (O, D, tmin, tmax)) if meshes is None else nr.trace(meshes, O, D, tmin, tmax))
    ref["_tmin"], ref["_tmax"] = tmin, tmax
    return ref


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("cases"), "cases")


@pytest.mark.parametrize("name", list(mrc.batches()))
def test_closest_hits_match_the_reference(cases, name):
    rays, h = cases[name + "_rays"], cases[name + "_closest_0"]
    ref = reference(name, rays)
    assert ref["fragile"].mean() <= mrc.FRAGILE_CAP
    against_reference(h, ref, name)
    st = dict(zip(STATS, cases[name + "_closest_0_stats"].tolist()))
    assert st["triangles"] == ref["triangles"] and st["leaves"] == ref["leaves"] and st["hits"] == int((h["hit"] == 1).sum())
    assert st["invalid_rays"] == int((~ref["valid"]).sum()) and cases[name + "_closest_0_sentinel"]
    assert_miss(h[~ref["valid"]])
    if rays.shape[0] > 1:
        assert st["hits"] > 0 and st["node_visits"] > 0 and st["triangle_tests"] > 0


@pytest.mark.parametrize("name", list(mrc.batches()))
def test_occlusion_equals_closest_hit_flag(cases, name):
    ref = reference(name, cases[name + "_rays"])
    ok = ~ref["fragile"]
    occ, close = cases[name + "_occlusion_0"], cases[name + "_closest_0"]
    assert np.array_equal(occ["hit"][ok], close["hit"][ok]) and np.array_equal(occ["hit"][ok] == 1, ref["hit"][ok])
    blank = occ.copy()
    blank["hit"] = 0
    assert_miss(blank)                                              # nothing but the flag is reported
    so, sc = cases[name + "_occlusion_0_stats"], cases[name + "_closest_0_stats"]
    assert so[5] == int((occ["hit"] == 1).sum()) and so[4] <= sc[4] and cases[name + "_occlusion_0_sentinel"]   # stops early: no more tests


@pytest.mark.parametrize("name", list(mrc.batches()))
def test_host_reorder_and_context_change_nothing(cases, name):
    base = cases[name + "_closest_0"]
    for other in ("_closest_1", "_host", "_context"):
        assert cases[name + other].tobytes() == base.tobytes(), other
    assert cases[name + "_occlusion_1"].tobytes() == cases[name + "_occlusion_0"].tobytes()
    for tag in ("closest", "occlusion"):
        a, b = cases[f"{name}_{tag}_0_stats"], cases[f"{name}_{tag}_1_stats"]
        assert np.array_equal(a[:7], b[:7]), tag                    # every integer statistic
    assert np.array_equal(cases[name + "_host_stats"][:7], cases[name + "_closest_0_stats"][:7])


@pytest.fixture(scope="module")
def watertight(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("wt"), "watertight")


@pytest.mark.parametrize("tag,shift", [("identity", None), ("translated", mrc.WT_SHIFT)])
def test_watertight_grid_is_exact(watertight, tag, shift):
    """axis-parallel rays at shared vertices, edge midpoints and along shared edges of an integer grid: every quantity is exact in
    fp32, so every ray hits, t is exact and the id is the lowest among the triangles whose closed set holds the point"""
    _, _, _, _, t, prim = mrc.watertight_rays(shift)
    for reorder in (0, 1):
        h = watertight[f"{tag}_{reorder}"]
        assert (h["hit"] == 1).all() and np.array_equal(h["t"], t) and np.array_equal(h["primitive_id"], prim), reorder
    assert (watertight[tag + "_occlusion"]["hit"] == 1).all()


@pytest.fixture(scope="module")
def life(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("life"), "lifecycle")


def test_lifecycle_rebuilds_visibility_empty_scene_and_memory(life):
    meshes = mrc.scenes()["mid"]
    O, D, tmin, tmax = mrc.rays_of("mid_257")
    rays = capi.make_rays(O, D, tmin, tmax)
    assert life["rebuilt"].tolist() == [1, 0] and life["second"].tobytes() == life["first"].tobytes()
    against_reference(life["first"], reference(None, rays, meshes[:3]), "meshes without splats")
    assert int(life["hidden_rebuilt"]) == 0 and life["hidden"].tobytes() != life["first"].tobytes()
    against_reference(life["hidden"], reference(None, rays, meshes[:2] + [dict(meshes[2], visible=False)]), "hidden box")
    assert int(life["moved_rebuilt"]) == 1
    moved = [meshes[0], dict(meshes[1], transform=mrc.SHIFTED), meshes[2]]
    against_reference(life["moved"], reference(None, rays, moved), "moved instance")
    assert int(life["added_rebuilt"]) == 1 and int(life["added_triangles"]) == sum(len(m["indices"]) for m in meshes)
    against_reference(life["added"], reference(None, rays, moved + [dict(meshes[3], visible=True)]), "added instance")
    # no mesh at all: every ray misses (the invalid ones too), nothing was built
    assert_miss(life["empty_hits"])
    st = dict(zip(STATS, life["empty_stats"].tolist()))
    assert st["triangles"] == st["leaves"] == st["nodes"] == st["node_visits"] == st["triangle_tests"] == st["hits"] == 0
    m0, m1, m2, m3 = life["scene_bytes"].tolist()
    assert m2 - m1 == int(life["bvh_bytes_expected"]) > 0 and m3 == m2 and m1 > m0


def test_pick_image_equals_the_rasterisers_primitive_ids(life):
    """two independent implementations: the closest-hit primitive id of the generated pinhole primary rays against
    mgs_meshes_download(which = 2) of mgs_meshes_render, on every pixel the reference marks comparable"""
    comparable, ref_prim = mrc.raster_mask(mc.fixture_meshes(capi.Mesh.load_obj(mc.FIXTURE).view()))
    assert 1 - comparable.mean() <= mrc.RASTER_EXCLUDED_CAP
    pick = life["pick"]["primitive_id"].reshape(mrc.RH, mrc.RW)
    raster = life["raster_prim"]
    assert (raster != NONE).mean() > 0.1
    assert np.array_equal(pick[comparable], raster[comparable])
    assert np.array_equal(pick[comparable], ref_prim[comparable])


def test_mesh_queries_disturb_nothing_they_do_not_own(life):
    assert bool(life["frame_held"]) and bool(life["mesh_images_held"]) and bool(life["unchanged"]) and int(life["mixed_hits"]) > 0
