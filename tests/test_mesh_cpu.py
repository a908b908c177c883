"""CPU tests of the mesh feature: the header / library / ctypes agreement, the OBJ subset on the fixture, argument validation that
needs no device, and the coverage cap and tolerances of the GPU tests, established on the numpy restatement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vk_gaussian_splatting_amd import capi
import mesh_cases as mc
import np_mesh as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mgs_mesh_from_arrays", "mgs_mesh_load_obj", "mgs_mesh_view", "mgs_mesh_destroy", "mgs_mesh_instance_add",
                "mgs_mesh_instance_set_transform", "mgs_mesh_instance_set_visible", "mgs_meshes_render", "mgs_meshes_download"]


def test_header_library_and_ctypes_agree():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define\s+MGS_HAS_MESHES\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr) and re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    lib = capi.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS, name
    # MgsMeshView: 5 pointers, 2 x u64, u32 (+ padding); MgsMeshOut: 3 x u64, f32, u32
    assert C.sizeof(capi.MeshView) == 64 and C.sizeof(capi.MeshOut) == 32
    assert "PARITY UNPINNED" in hdr[hdr.index("MGS_HAS_MESHES)"):]


@pytest.fixture(scope="module")
def fixture_view():
    return capi.Mesh.load_obj(mc.FIXTURE).view()


def _parse_fixture():
    """an independent reading of the fixture: (positions, faces as lists of (v, n or None), material name per face, shape per face)"""
    pos, nrm, faces, cur, shape = [], [], [], None, 0
    for ln in open(mc.FIXTURE):
        t = ln.split()
        if not t or t[0].startswith("#"):
            continue
        if t[0] == "v":
            pos.append([float(x) for x in t[1:4]])
        elif t[0] == "vn":
            nrm.append([float(x) for x in t[1:4]])
        elif t[0] in ("o", "g"):
            shape += 1 if (faces and faces[-1][2] == shape) else 0
        elif t[0] == "usemtl":
            cur = t[1]
        elif t[0] == "f":
            cs = []
            for c in t[1:]:
                p = c.split("/")
                vi = int(p[0])
                ni = int(p[2]) if len(p) > 2 and p[2] else None
                cs.append((vi - 1 if vi > 0 else len(pos) + vi, None if ni is None else (ni - 1 if ni > 0 else len(nrm) + ni)))
            faces.append((cs, cur, shape))
    return np.array(pos, np.float32), np.array(nrm, np.float32), faces


def test_obj_subset_on_the_fixture(fixture_view):
    v = fixture_view
    pos, nrm, faces = _parse_fixture()
    names = ["red", "glow"]
    corners, mids, shapes = [], [], []
    for cs, mat, shape in faces:
        for k in range(1, len(cs) - 1):  # fan from the first corner
            corners += [cs[0], cs[k], cs[k + 1]]
            mids.append(names.index(mat) if mat in names else 0)
            shapes.append(shape)
    assert len(faces) == 21 and any(len(f[0]) == 5 for f in faces) and any(len(f[0]) == 4 for f in faces) and any(len(f[0]) == 3 for f in faces)
    assert v["indices"].shape == (len(mids), 3) and np.array_equal(v["indices"].reshape(-1), np.arange(3 * len(mids)))  # de-indexed
    assert np.array_equal(v["positions"], pos[[c[0] for c in corners]])
    assert np.array_equal(v["material_ids"], np.array(mids, np.uint32))
    assert len(v["materials"]) == 2
    assert v["materials"][0]["diffuse"] == pytest.approx((0.8, 0.3, 0.25)) and v["materials"][0]["shininess"] == 24.0
    assert v["materials"][1]["emission"] == pytest.approx((0.2, 0.9, 0.4)) and v["materials"][1]["diffuse"] == (0.0, 0.0, 0.0) and v["materials"][1]["shininess"] == 1.0
    # generated normals: obj_loader.cpp:98-151 restated literally — per shape, arrays that persist across shapes
    gen, visited = np.zeros((pos.shape[0], 3), np.float32), np.zeros(pos.shape[0], bool)
    expect = np.zeros((len(corners), 3), np.float32)
    for s in sorted(set(shapes)):  # a shape's corners are emitted right after its faces went into the running normals (:156-187)
        ts = [t for t in range(len(mids)) if shapes[t] == s]
        nm.generate_normals(pos, np.array([[corners[3 * t + k][0] for k in range(3)] for t in ts]), gen, visited)
        for t in ts:
            for k in range(3):
                c = corners[3 * t + k]
                expect[3 * t + k] = nrm[c[1]] if c[1] is not None else gen[c[0]]
    assert any(c[1] is None for c in corners) and any(c[1] is not None for c in corners)
    assert np.array_equal(v["normals"].view(np.uint32), expect.view(np.uint32))


def test_obj_errors(tmp_path):
    with pytest.raises(capi.MgsError) as e:
        capi.Mesh.load_obj(str(tmp_path / "missing.obj"))
    assert e.value.code == capi.ERR_IO
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n")
    with pytest.raises(capi.MgsError) as e:
        capi.Mesh.load_obj(str(bad))
    assert e.value.code == capi.ERR_FORMAT
    plain = tmp_path / "plain.obj"
    plain.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    v = capi.Mesh.load_obj(str(plain)).view()
    assert len(v["materials"]) == 1 and v["materials"][0] == dict(ambient=pytest.approx((0.1,) * 3), diffuse=pytest.approx((0.7,) * 3),
                                                                  specular=(1.0, 1.0, 1.0), emission=(0.0, 0.0, 0.0), shininess=32.0)
    assert np.array_equal(v["material_ids"], [0])


def test_from_arrays_validation_and_generated_normals():
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    for kw in (dict(positions=pos, indices=[0, 1, 2, 3]), dict(positions=pos, indices=[0, 1, 4]), dict(positions=np.zeros((0, 3)), indices=[0, 1, 2])):
        with pytest.raises(capi.MgsError) as e:
            capi.Mesh.from_arrays(**kw)
        assert e.value.code == capi.ERR_INVALID_ARG
    idx = [[0, 1, 2], [1, 3, 2], [2, 3, 0]]
    v = capi.Mesh.from_arrays(pos, idx, material_ids=[0, 7, 1], materials=[capi.make_material(), capi.make_material(shininess=3.0)]).view()
    assert np.array_equal(v["normals"].view(np.uint32), nm.generate_normals(pos, idx).view(np.uint32))
    assert np.array_equal(v["material_ids"], [0, 0, 1])  # ids >= material_count become 0


def test_cap_and_tolerance_from_the_reference_alone(fixture_view):
    worst_d, worst_c = 0.0, 0.0
    for name, (meshes, (V, P, eye), w, h, mode, lights) in mc.cases(fixture_view).items():
        r64 = nm.render(meshes, V, P, eye, w, h, mode, lights, np.float64)
        r32 = nm.render(meshes, V, P, eye, w, h, mode, lights, np.float32)
        share, on_boundary, dd, dc = mc.compare((r32.depth, r32.color, r32.prim), r64, name)
        print(f"mesh {name}: covered {(r64.prim != nm.NONE).mean():.3f}, fragments {r64.fragments}, f32 vs f64 coverage differs on {share:.5f} of the covered "
              f"pixels, depth {dd:.3e}, colour {dc:.3e}")
        assert (r64.prim != nm.NONE).any() or name == "none", name
        assert share <= mc.COVERAGE_CAP / 4 and on_boundary, (name, share, on_boundary)
        worst_d, worst_c = max(worst_d, dd), max(worst_c, dc)
    assert mc.DEPTH_F32_VS_F64 / 2 <= worst_d <= mc.DEPTH_F32_VS_F64, worst_d
    assert mc.COLOR_F32_VS_F64 / 2 <= worst_c <= mc.COLOR_F32_VS_F64, worst_c


def test_project_mesh_sections(tmp_path):
    import json
    from vk_gaussian_splatting_amd import project
    data = {"version": 4, "renderer": {}, "splatSets": [], "splats": [],
            "meshAssets": [{"id": 3, "path": os.path.relpath(mc.FIXTURE, tmp_path)}, {"id": 4, "path": "missing.obj"}],
            "meshInstances": {"nextNamingNumber": 2, "items": [
                {"meshAssetId": 3, "name": "a", "position": [1, 2, 3], "rotation": [0, 90, 0], "scale": [1, 2, 1], "materials": [{"diffuse": [0.1, 0.2, 0.3]}]},
                {"meshAssetId": 9, "name": "dangling"}]}}
    path = tmp_path / "p.vkgs"
    path.write_text(json.dumps(data))
    pr = project.load_project(str(path))
    assert pr.mesh_assets == {3: os.path.normpath(mc.FIXTURE), 4: os.path.normpath(str(tmp_path / "missing.obj"))}
    assert len(pr.mesh_instances) == 2 and pr.mesh_instances[0]["scale"] == (1, 2, 1) and pr.mesh_instances[0]["materials"][0]["diffuse"] == [0.1, 0.2, 0.3]
    out = tmp_path / "q.vkgs"
    project.save_project(pr, str(out))
    back = json.loads(out.read_text())
    assert back["meshAssets"] == data["meshAssets"] and back["meshInstances"] == data["meshInstances"]  # written back unchanged


def _project_v2(tmp_path):
    return {"version": 4, "renderer": {}, "splatSets": [], "splats": [],
            "meshAssets": [{"id": 3, "path": os.path.relpath(mc.FIXTURE, tmp_path)}, {"id": 4, "path": "missing.obj"}],
            "meshInstances": {"nextNamingNumber": 2, "items": [
                {"meshAssetId": 3, "name": "a", "position": [1, 2, 3], "rotation": [0, 90, 0], "scale": [1, 2, 1], "materials": [{"diffuse": [0.1, 0.2, 0.3]}]},
                {"meshAssetId": 9, "name": "dangling"},
                {"meshAssetId": 4, "name": "of the missing file"},
                {"meshAssetId": 3, "name": "b", "materials": [{}, {"shininess": 5.0, "emission": [0.5, 0.25, 0.0]}, {"shininess": 99.0}]}]}}


def test_project_resolves_assets_instances_and_material_overrides(tmp_path):
    import json
    from vk_gaussian_splatting_amd import project
    path = tmp_path / "p.vkgs"
    path.write_text(json.dumps(_project_v2(tmp_path)))
    pr = project.load_project(str(path))
    with pytest.warns(UserWarning, match="missing.obj"):  # a mesh file that cannot be loaded is skipped with a warning
        views, placed = pr.resolve_meshes()
    assert set(views) == {3}
    assert [a for a, _ in placed] == [3, 3]  # the instance of an unknown asset and the one of the missing file are skipped
    Ma, _ = capi.compute_transform((1, 2, 1), (0, 90, 0), (1, 2, 3))
    Mb, _ = capi.compute_transform((1, 1, 1), (0, 0, 0), (0, 0, 0))
    assert np.array_equal(placed[0][1], Ma) and np.array_equal(placed[1][1], Mb) and not np.array_equal(Ma, Mb)
    # overrides go to the MESH's materials, in order, field by field; entries beyond the mesh's materials are ignored
    plain = capi.Mesh.load_obj(mc.FIXTURE).view()["materials"]
    m0, m1 = views[3]["materials"]
    assert m0["diffuse"] == pytest.approx((0.1, 0.2, 0.3)) and m0["shininess"] == 24.0 and m0["ambient"] == plain[0]["ambient"]
    assert m1["shininess"] == 5.0 and m1["emission"] == (0.5, 0.25, 0.0) and m1["diffuse"] == plain[1]["diffuse"]
    assert len(views[3]["materials"]) == 2


@pytest.mark.parametrize("version", [0, 1])
def test_project_legacy_meshes_section(tmp_path, version):
    """vkgs_project_reader.cpp:476-553: a list (version 0) or {"items": [...]} (version 1); every entry is a mesh of its own"""
    import json
    from vk_gaussian_splatting_amd import project
    items = [{"path": os.path.relpath(mc.FIXTURE, tmp_path), "name": "a", "position": [0, 1, 0], "rotation": [0, 0, 0], "scale": [2, 2, 2],
              "materials": [{"shininess": 5.0}]},
             {"path": ""},
             {"path": "missing.obj"},
             {"path": os.path.relpath(mc.FIXTURE, tmp_path)}]
    data = {"version": version, "renderer": {}, "splats": [], "meshes": items if version == 0 else {"nextNamingNumber": 7, "items": items}}
    path = tmp_path / "legacy.vkgs"
    path.write_text(json.dumps(data))
    pr = project.load_project(str(path))
    assert sorted(pr.mesh_assets) == [0, 2, 3] and [i["asset"] for i in pr.mesh_instances] == [0, 2, 3]  # the entry without a path is skipped
    assert pr.mesh_instances[0]["scale"] == (2, 2, 2) and pr.mesh_instances[2]["scale"] == (1.0, 1.0, 1.0)
    with pytest.warns(UserWarning, match="missing.obj"):
        views, placed = pr.resolve_meshes()
    assert [a for a, _ in placed] == [0, 3]
    assert views[0]["materials"][0]["shininess"] == 5.0 and views[3]["materials"][0]["shininess"] == 24.0  # not shared between entries
    out = tmp_path / "back.vkgs"
    project.save_project(pr, str(out))
    assert json.loads(out.read_text())["meshes"] == data["meshes"]  # written back unchanged
