"""GPU tests (-m gpu) of the mesh pass (mgs_meshes_render, k_mesh.hip).

The pass is checked against the independent numpy restatement (np_mesh.py, float64).  Where coverage is decided on exactly
representable inputs (the fill-rule case) the primitive-id image must be equal in every pixel.  Elsewhere at most
mesh_cases.COVERAGE_CAP = 0.5 % of the covered pixels may differ in their primitive, each of them a boundary pixel, and on the others
depth and colour stay within 4 x the float32-vs-float64 difference of the restatement itself
(tests/test_mesh_cpu.py::test_cap_and_tolerance_from_the_reference_alone).  Plumbing is compared bit for bit with the library itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi
import mesh_cases as mc
import np_lighting as nl
import np_mesh as nm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def to_capi_mesh(m):
    mats = [capi.make_material(**mm) for mm in (m.get("materials") or [])]
    return mgs.Mesh.from_arrays(m["positions"], m["indices"], m["normals"], m.get("material_ids"), mats or None)


def make_scene(meshes):
    scene = mgs.Scene(0)
    keep = [to_capi_mesh(m) for m in meshes]
    for m, cm in zip(meshes, keep):
        scene.add_mesh_instance(cm, m.get("transform"))
    return scene, keep


def params(cam, w, h, lighting=0, **kw):
    V, P, eye = cam
    p = capi.default_params(w, h)
    capi.set_camera(p, V, P, eye)
    p.lighting_mode = lighting
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check(name, got, ref):
    share, on_boundary, dd, dc = mc.compare(got, ref, name)
    print(f"mesh {name}: {share:.5f} of the covered pixels differ in their primitive (cap {mc.COVERAGE_CAP}), all on boundaries: {on_boundary}; "
          f"depth {dd:.3e} (bar {mc.GPU_DEPTH_BAR:.1e}), colour {dc:.3e} (bar {mc.GPU_COLOR_BAR:.1e})")
    assert share <= mc.COVERAGE_CAP and on_boundary, (name, share)
    assert dd <= mc.GPU_DEPTH_BAR and dc <= mc.GPU_COLOR_BAR, (name, dd, dc)
    none = ref.prim == nm.NONE
    assert (got[0][none & (got[2] == nm.NONE)] == 1.0).all() and (got[1][none & (got[2] == nm.NONE)] == 0.0).all()
    assert (got[1][got[2] != nm.NONE][:, 3] == 1.0).all()


@pytest.fixture(scope="module")
def fixture_view():
    return mgs.Mesh.load_obj(mc.FIXTURE).view()


# ---- 1. exact fill rule: no tolerance, no cap -------------------------------------------------------------------------------
def test_fill_rule_exact():
    m = mc.fill_mesh()
    cam = (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), np.zeros(3, np.float32))
    scene, keep = make_scene([m])
    p = params(cam, mc.FW, mc.FH)
    out = scene.render_meshes(p, want_stats=True)
    depth, color, prim = scene.download_meshes()
    ref = nm.render([m], *cam, mc.FW, mc.FH, 0, [], np.float64)
    assert np.array_equal(prim, ref.prim)
    assert np.array_equal(depth, ref.depth)
    ids = set(np.unique(prim).tolist())
    assert 4 not in ids and 6 not in ids and 7 not in ids and {0, 1, 2, 3, 5, 8, 9, nm.NONE} <= ids  # zero area, equal depth, depth 1.0
    assert out.triangles_in == 10 and out.fragments == ref.fragments
    scene.close()


# ---- 2. watertight grid ---------------------------------------------------------------------------------------------------------
def test_watertight_grid_and_second_instance():
    m = mc.grid_mesh()
    cam = mc.grid_camera()
    scene, keep = make_scene([m])
    p = params(cam, mc.W, mc.H)
    scene.render_meshes(p)
    depth, color, prim = scene.download_meshes()
    assert (prim != nm.NONE).all()
    check("grid", (depth, color, prim), nm.render([m], *cam, mc.W, mc.H, 0, [], np.float64))
    scene.add_mesh_instance(keep[0], None)  # the same triangles again, later in primitive order: LESS keeps the first
    out = scene.render_meshes(p, want_stats=True)
    d2, c2, p2 = scene.download_meshes()
    assert np.array_equal(p2, prim) and np.array_equal(d2, depth)
    assert out.fragments == 2 * mc.W * mc.H  # every pixel exactly once per instance
    scene.close()


# ---- 3. both coverage paths -----------------------------------------------------------------------------------------------------
def test_both_coverage_paths_against_the_restatement():
    meshes, cam = mc.both_paths_meshes()
    scene, keep = make_scene(meshes)
    p = params(cam, mc.W, mc.H, lighting=1)
    out = scene.render_meshes(p, want_stats=True)
    got = scene.download_meshes()
    ref = nm.render(meshes, *cam, mc.W, mc.H, 1, [], np.float64)
    check("both_paths", got, ref)
    assert out.triangles_in == ref.triangles_in == 1 + 2 + 20000
    print(f"fragments {out.fragments} (restatement {ref.fragments}), rasterised {out.triangles_rasterised}, {out.elapsed_ms:.3f} ms")
    assert out.fragments == ref.fragments and out.flags == 0  # covered pixels plus overdraw as the restatement counts it
    assert {0, 1, 2} <= set(np.unique(got[2]).tolist()) and (got[2] >= 3).any() and (got[2] != nm.NONE).any()
    scene.close()


# ---- 4. shading ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shading_unlit", "shading_headlight", "shading_mixed"])
def test_shading_against_the_restatement(fixture_view, name):
    meshes, cam, w, h, mode, lights = mc.cases(fixture_view)[name]
    scene, keep = make_scene(meshes)
    scene.set_lights([capi.make_light(**l) for l in lights])
    p = params(cam, w, h, lighting=mode)
    scene.render_meshes(p)
    got = scene.download_meshes()
    ref = nm.render(meshes, *cam, w, h, mode, lights, np.float64)
    check(name, got, ref)
    # a purely emissive material is unchanged by lights
    T = fixture_view["indices"].shape[0]
    glow = (fixture_view["material_ids"] == 1)[got[2][got[2] != nm.NONE] % T]
    px = got[1][got[2] != nm.NONE][glow]
    assert glow.any() and (px[:, :3] == np.float32([0.2, 0.9, 0.4])).all()
    scene.close()


# ---- 5. plumbing, bit for bit -------------------------------------------------------------------------------------------------
def test_plumbing_bit_for_bit(fixture_view):
    meshes, cam, w, h, mode, lights = mc.cases(fixture_view)["shading_headlight"]
    scene, keep = make_scene(meshes)
    p = params(cam, w, 96, lighting=1)
    scene.render_meshes(p)
    full = [a.copy() for a in scene.download_meshes()]
    scene.render_meshes(p)
    again = scene.download_meshes()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(full, again))
    # strips: tile rows [0, 2), [2, 5), [5, 6) of the 96-row frame, each on a handle of its own, assembled
    asm = [np.zeros_like(a) for a in full]
    for r0, r1 in ((0, 2), (2, 5), (5, 6)):
        ctx = scene.frame_context()
        q = params(cam, w, 96, lighting=1, strip_row_begin=r0, strip_row_end=r1)
        ctx.render_meshes(q)
        for a, b in zip(asm, ctx.download_meshes()):
            a[r0 * 16:r1 * 16] = b[r0 * 16:r1 * 16]
        ctx.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(full, asm))
    # a frame context gives the scene handle's images; it may not edit
    ctx = scene.frame_context()
    ctx.render_meshes(p)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(full, ctx.download_meshes()))
    with pytest.raises(mgs.MgsError) as e:
        ctx.set_mesh_visible(0, 0)
    assert e.value.code == capi.ERR_STATE
    ctx.close()
    # set_transform takes effect on the next pass
    scene.set_mesh_transform(1, mc.MOVED)
    scene.render_meshes(p)
    moved = scene.download_meshes()
    assert not np.array_equal(moved[2], full[2])
    meshes2 = [meshes[0], dict(meshes[1], transform=mc.MOVED)]
    check("moved", moved, nm.render(meshes2, *cam, w, 96, 1, [], np.float64))
    # nothing visible: the cleared images
    scene.set_mesh_visible(0, 0)
    scene.set_mesh_visible(1, 0)
    out = scene.render_meshes(p, want_stats=True)
    d, c, i = scene.download_meshes()
    assert (d == 1.0).all() and (c == 0.0).all() and (i == nm.NONE).all() and out.triangles_in == 0 and out.fragments == 0
    sb, _ = scene.memory_usage()
    assert sb >= fixture_view["positions"].nbytes * 2 + fixture_view["indices"].nbytes
    scene.close()


# ---- 6. end to end, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"])
def test_mesh_pass_then_splats_equals_uploaded_occluder(tmp_path, graph):
    out = str(tmp_path / "frames.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_mesh.py"), "frame", out], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MGS_GRAPH=graph))
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    d = np.load(out)
    for alpha in (0, 1):
        for lighting in (0, 1):
            key = f"a{alpha}_l{lighting}"
            assert np.array_equal(d["with_" + key], d["ref_" + key]), key
            assert d["with_" + key].any()
    for key in ("a0_l1", "a1_l1"):
        cons, _ = nl.consolidate_depth(d["picked_" + key], d["mdepth_" + key])
        assert np.array_equal(d["cons_" + key], cons) and (d["mdepth_" + key] < 1.0).any()


def test_gathered_two_ranks_with_mesh_pass(tmp_path):
    so = os.path.join(os.path.dirname(HERE), "tests", "helpers", "libfakerccl.so")
    assert os.path.exists(so), "tests/helpers/libfakerccl.so not built (__graft_entry__.build() makes it)"
    idfile = str(tmp_path / "uid")
    env = dict(os.environ, MGS_RCCL_LIB=so, MGS_FAKE_RCCL_TIMEOUT="45")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_child_mesh.py"), "gather", "-", str(r), "2", idfile], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "CHILD_DONE" in o, o[-2000:]
        assert f"GATHERED_EQUALS_FULL rank {r}: True" in o, o[-2000:]


# ---- 7. the work list of the large triangles, exceeded ----------------------------------------------------------------------------
def _worklist_child(tmp_path, capacity):
    out = str(tmp_path / f"wl_{capacity}.npz")
    env = dict(os.environ)
    env.pop("MGS_MESH_WORK_ITEMS", None)
    if capacity:
        env["MGS_MESH_WORK_ITEMS"] = str(capacity)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_mesh_worklist.py"), out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def worklist_reference(tmp_path_factory):
    meshes, cam = mc.worklist_meshes()
    return _worklist_child(tmp_path_factory.mktemp("wl"), 0), nm.render(meshes, *cam, mc.W, mc.H, 0, [], np.float64)


def test_worklist_scene_against_the_restatement(worklist_reference):
    d, ref = worklist_reference
    check("worklist", (d["depth0"], d["color0"], d["prim0"]), ref)
    assert int(d["stats0"][2]) == ref.fragments and int(d["stats0"][3]) == 0  # the default capacity holds the scene's chunks
    first = 3 + 20000  # the two grids' triangles are seen
    assert np.isin(d["prim0"], np.arange(first, first + 2 * 512)).sum() > 1000


@pytest.mark.parametrize("capacity", [1, 37, 250])
def test_full_worklist_gives_the_same_images(tmp_path, worklist_reference, capacity):
    """a list that is exceeded (at once, by the first wave; after a few waves; by the last ones) is slow, never wrong: every image
    and every counter equals the pass with room, bit for bit, on the first pass and on the one after it"""
    full, _ = worklist_reference
    d = _worklist_child(tmp_path, capacity)
    for rep in (0, 1):
        for k in ("depth", "color", "prim"):
            assert np.array_equal(d[f"{k}{rep}"].view(np.uint32), full[f"{k}0"].view(np.uint32)), (k, rep)
        assert np.array_equal(d[f"stats{rep}"][:3], full["stats0"][:3]), (d[f"stats{rep}"], full["stats0"])
        assert int(d[f"stats{rep}"][3]) == capi.MESH_WORK_LIST_FULL


# ---- 8. the project file's meshes ------------------------------------------------------------------------------------------------
def test_project_adds_its_mesh_instances(tmp_path):
    import json
    import warnings
    from vk_gaussian_splatting_amd import project
    data = {"version": 4, "renderer": {}, "splatSets": [], "splats": [],
            "meshAssets": [{"id": 3, "path": os.path.relpath(mc.FIXTURE, tmp_path)}, {"id": 4, "path": "missing.obj"}],
            "meshInstances": {"items": [
                {"meshAssetId": 3, "position": [-0.9, 0.1, 0.2], "rotation": [0, 0, 0], "scale": [1.6, 0.6, 1.1], "materials": [{"diffuse": [0.1, 0.2, 0.9]}]},
                {"meshAssetId": 9}, {"meshAssetId": 4},
                {"meshAssetId": 3, "position": [1.3, 0.0, -0.6], "rotation": [0, 40, 0], "scale": [1, 1, 1]}]}}
    path = tmp_path / "p.vkgs"
    path.write_text(json.dumps(data))
    pr = project.load_project(str(path))
    scene = mgs.Scene(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ids = pr.add_meshes(scene)
        views, placed = pr.resolve_meshes()
    assert ids == [0, 1] and len(placed) == 2
    cam = mc.camera()
    p = params(cam, mc.W, mc.H, lighting=1)
    out = scene.render_meshes(p, want_stats=True)
    v = views[3]
    meshes = [dict(positions=v["positions"], indices=v["indices"], normals=v["normals"], material_ids=v["material_ids"], materials=v["materials"],
                   transform=M, visible=True) for _, M in placed]
    assert v["materials"][0]["diffuse"] == pytest.approx((0.1, 0.2, 0.9))
    ref = nm.render(meshes, *cam, mc.W, mc.H, 1, [], np.float64)
    check("project", scene.download_meshes(), ref)
    assert out.triangles_in == 2 * v["indices"].shape[0] and (ref.prim != nm.NONE).sum() > 500
    scene.close()
