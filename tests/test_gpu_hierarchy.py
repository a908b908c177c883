"""The two device-built hierarchies, downloaded (mgs_debug_download_hierarchy) and held to np_hierarchy.py's float64 statement of what
they must contain; one child process per tree.

Hard, no tolerance: the leaf ids are exactly the valid set, each once; the tree's shape; every upper node bit for bit the min / max of
its children, no NaN, the .w words; every splat leaf box contains the float64 ellipsoid box on all six faces; every triangle leaf box
strictly contains its record's vertices; the records' vertices bit for bit the fp32 vertex stage; rebuilds are byte-identical; the
hook's lifecycle.  Bounded by derivation: a face lies at most 32 * 2^-24 * (h + the sum of the centre's absolute terms) outside the
exact box; the leaves' float64 Morton codes do not decrease but for pairs with a leaf within 2^-10 of a cell boundary.
Printed per group and kernel degree: the worst containment margin in ulps of h and the worst excess over the tightness bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hierarchy_cases as hc
import np_hierarchy as nh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_ARG, STATE = -1, -6


def run_child(tmp_path, mode):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_hierarchy.py"), mode, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.fixture(scope="module")
def splats(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("splats"), "splats")


@pytest.fixture(scope="module")
def meshes(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("meshes"), "meshes")


def info_of(d, tag):
    a = d[tag + "_info"]
    return dict(levels=int(a[0]), total_nodes=int(a[1]), leaves=int(a[2]), primitives=int(a[3]), level_offset=a[4:15].astype(np.uint32),
                level_count=a[15:26].astype(np.uint32), box_lo=d[tag + "_frame"][:3], box_inv_ext=d[tag + "_frame"][3:])


def splat_planes(d, tag, sets):
    return [(hc.storage_planes(a, d[f"{tag}_order_{k}"].astype(np.int64), d[f"{tag}_density_{k}"]), M) for k, (a, M) in enumerate(sets)]


def check_splat_tree(d, tag, ref, total):
    """every assertion on one downloaded splat hierarchy -> (containment dict, excused pairs, pairs)"""
    info, nodes = info_of(d, tag), d[tag + "_nodes"]
    valid = np.nonzero(ref["valid"])[0]
    nh.check_nodes(info, nodes, valid.size)
    assert info["primitives"] == total
    assert d[tag + "_out"][:2].tolist() == [info["leaves"], info["total_nodes"]]
    ids = nodes[:valid.size, 3].astype(np.int64)
    assert np.array_equal(np.sort(ids), valid), "the leaves are not exactly the valid splats, each once"
    m = nh.splat_containment(nodes, ref)
    excused, pairs = nh.check_order(ref["c"][ids], info["box_lo"], info["box_inv_ext"], ids)
    return m, excused, pairs


@pytest.mark.parametrize("name", list(hc.splat_groups()))
def test_splat_leaves_contain_the_float64_ellipsoid_boxes(splats, name):
    sets = hc.splat_groups()[name]
    pls = splat_planes(splats, name, sets)
    total = sum(a["positions"].shape[0] for a, _ in sets)
    cull = splats[name + "_cull"]
    failures = []
    for degree, adaptive in hc.PROXIES:
        ref = nh.scene_splats(pls, degree, hc.KMR, adaptive, cull)
        m, excused, pairs = check_splat_tree(splats, f"{name}_{degree}_{adaptive}", ref, total)
        if name == "f_nonfinite":
            where = np.argsort(splats[name + "_order_0"])          # caller's index -> storage index
            assert not ref["valid"][where[:hc.F_BAD]].any() and ref["valid"][where[hc.F_HUGE]] and ref["valid"].sum() == total - hc.F_BAD - 2
        if name == "e_thresholds":
            at = int(np.argsort(splats[name + "_order_0"])[hc.E_CULL_FROM])
            assert not ref["valid"][at] and 10 < ref["valid"][np.argsort(splats[name + "_order_0"])[:80]].sum() < 70   # at: no leaf; below and above
        with np.errstate(divide="ignore", invalid="ignore"):
            ulps, ratio = m["margin"] / (2 * nh.EPS * m["h"]), m["margin"] / m["bound"]
        print(f"{name} degree {degree} adaptive {adaptive}: {m['ids'].size} leaves, worst containment margin {ulps.min():.2f} ulps of h, "
              f"worst excess / bound {ratio.max():.3f}, {excused} of {pairs} pairs excused")
        if not (m["margin"] >= 0).all():
            failures.append(f"containment: degree {degree} adaptive {adaptive}: {(m['margin'] < 0).any(1).mean():.1%} of the boxes, worst {ulps.min():.1f} ulps of h")
        if not (m["margin"] <= m["bound"]).all():
            failures.append(f"tightness: degree {degree} adaptive {adaptive}: worst excess / bound {ratio.max():.3f}")
        assert excused <= hc.EXCUSED_CAP * pairs
        if name == "h_two_instances":   # the case bites: along level 0 the owner of the leaf changes at least every other step
            owner = m["ids"] >= total // 2
            assert (owner[1:] != owner[:-1]).sum() >= owner.size // 2
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", hc.COUNTS)
def test_splat_tree_shape_at_every_leaf_count(splats, n):
    sets = hc.count_scene(n)
    ref = nh.scene_splats(splat_planes(splats, f"count_{n}", sets), 2, hc.KMR, 1, hc.CULL)
    assert ref["valid"].sum() == n
    m, _, _ = check_splat_tree(splats, f"count_{n}", ref, sets[0][0]["positions"].shape[0])
    assert (m["margin"] >= 0).all() and (m["margin"] <= m["bound"]).all()


def test_splat_hierarchy_determinism_and_lifecycle(splats):
    assert bool(splats["rebuilt_twice"]) and bool(splats["same_after_rebuild"]) and bool(splats["context_equal"])
    assert int(splats["err_before"]) == STATE and int(splats["err_capacity"]) == INVALID_ARG and int(splats["err_which"]) == INVALID_ARG
    assert bool(splats["usable_after_refusal"]) and bool(splats["memory_unchanged"]) and int(splats["rebuilt_after_download"]) == 0


def check_mesh_tree(d, tag, ms):
    ref = nh.scene_triangles(ms)
    info, nodes, tris = info_of(d, tag), d[tag + "_nodes"], d[tag + "_tris"]
    valid = np.nonzero(ref["valid"])[0]
    nl = valid.size
    nh.check_nodes(info, nodes, nl)
    assert info["primitives"] == ref["valid"].size and d[tag + "_out"][:3].tolist() == [nl, info["total_nodes"], ref["valid"].size]
    if nl == 0:
        return ref, valid
    tris = tris.reshape(nl, 3, 4)
    prim = tris[:, 0, 3].astype(np.int64)
    assert np.array_equal(nodes[:nl, 3], np.arange(nl, dtype=np.uint32)) and np.array_equal(np.sort(prim), valid)
    assert np.array_equal(tris[:, 1, 3], ref["inst"][prim]) and np.array_equal(tris[:, 2, 3], ref["mat"][prim])
    # the record's vertices: bit for bit the fp32 vertex stage, and within its bound of the float64 transform
    assert np.ascontiguousarray(tris[:, :, :3]).tobytes() == ref["tri32"][prim].view(np.uint32).tobytes()
    v = nh.f64(tris[:, :, :3])
    assert (np.abs(v - ref["tri64"][prim]) <= ref["bound"][prim]).all()
    # strict containment of the record's vertices, on every axis
    lo, hi = nh.f64(nodes[:nl, 0:3]), nh.f64(nodes[:nl, 4:7])
    assert (lo < v.min(1)).all() and (hi > v.max(1)).all(), "a leaf box does not strictly contain its triangle"
    excused, pairs = nh.check_order(v.mean(1), info["box_lo"], info["box_inv_ext"])
    print(f"mesh {tag}: {nl} leaves, {excused} of {pairs} pairs excused")
    assert excused <= hc.EXCUSED_CAP * pairs
    return ref, valid


@pytest.mark.parametrize("n", hc.COUNTS)
def test_triangle_tree_shape_at_every_leaf_count(meshes, n):
    _, valid = check_mesh_tree(meshes, f"count_{n}", hc.count_mesh(n))
    assert valid.size == n


def test_triangle_content(meshes):
    ms, names = hc.mesh_content()
    ref, valid = check_mesh_tree(meshes, "content", ms)
    first = np.cumsum([0] + [len(m["indices"]) for m in ms])
    deg, hid = names.index("degenerate"), names.index("hidden")
    assert ref["valid"][first[deg]:first[deg + 1]].tolist() == hc.MESH_VALID["degenerate"]
    assert ref["valid"][first[hid]:first[hid + 1]].all()          # visibility is not part of the build
    assert set(ref["mat"][valid].tolist()) == {0, 1, 2, 3}


def test_triangle_hierarchy_determinism_and_lifecycle(meshes):
    assert bool(meshes["rebuilt_twice"]) and bool(meshes["same_after_rebuild"]) and bool(meshes["context_equal"])
    assert int(meshes["err_before"]) == STATE and int(meshes["err_capacity"]) == INVALID_ARG and int(meshes["err_capacity_nodes"]) == INVALID_ARG
    assert bool(meshes["usable_after_refusal"]) and bool(meshes["memory_unchanged"]) and int(meshes["rebuilt_after_download"]) == 0
