"""CPU tests of hybrid frames with meshes (mgs_frame_set_hybrid_meshes): the header, the export and the binding, the refusals that need no
device; the float64 restatement np_hybrid_mesh.py on the CPU oracle's raster G-buffer; the restatement's own rules on an edited G-buffer.

The CPU oracle has no depth test against an occluder.  The cut G-buffer is assembled from it as test_lighting_cpu.py assembles one
against a level: the sorted stream filtered to the splats whose key depth is <= the pixel's plane value, rendered once per distinct
number of splats that pass (hybrid_mesh_cases.oracle_gbuffer_cut).  The plane is the float64 one made from np_mesh_rays' hits."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import hybrid_cases as hc
import hybrid_mesh_cases as hmc
import np_hybrid_mesh as nhm
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_export_and_binding():
    h = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_HYBRID_MESHES 1", h)
    assert re.search(r"int mgs_frame_set_hybrid_meshes\(MgsScene scene_or_context, const MgsTraceMeshParams\* params", h)
    lib = capi.load_library()
    for name in ("mgs_frame_set_hybrid_meshes", "mgs_debug_download_hybrid_depth"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mgs_frame_set_hybrid_meshes.restype is C.c_int
    assert list(lib.mgs_frame_set_hybrid_meshes.argtypes) == [C.c_void_p, C.POINTER(capi.TraceMeshParams)]
    assert callable(capi.Scene.set_hybrid_meshes) and callable(capi.Scene.hybrid_mesh_depth)
    assert C.sizeof(capi.TraceMeshParams) == 16   # reused as it is: ABI 5.1


def test_refusals_without_a_device():
    lib = capi.load_library()
    err = lambda: lib.mgs_last_error().decode()
    good = capi.TraceMeshParams()
    lib.mgs_trace_mesh_params_default(C.byref(good))
    good.enabled = 1
    for field, value in (("enabled", 2), ("enabled", -1), ("min_mesh_composite_transmittance", -0.1), ("min_mesh_composite_transmittance", 1.5),
                         ("min_mesh_composite_transmittance", float("nan"))):
        bad = capi.TraceMeshParams.from_buffer_copy(good)
        setattr(bad, field, value)
        assert lib.mgs_frame_set_hybrid_meshes(None, C.byref(bad)) == -1 and "null scene" not in err(), field
    for k in range(2):
        bad = capi.TraceMeshParams.from_buffer_copy(good)
        bad.reserved[k] = 1
        assert lib.mgs_frame_set_hybrid_meshes(None, C.byref(bad)) == -1 and "reserved" in err()
    assert lib.mgs_frame_set_hybrid_meshes(None, C.byref(good)) == -1 and "null scene" in err()
    assert lib.mgs_frame_set_hybrid_meshes(None, None) == -1 and "null scene" in err()   # NULL = off: valid
    assert lib.mgs_debug_download_hybrid_depth(None, None, 0) == -1


@functools.lru_cache(maxsize=None)
def _oracle_frame(name):
    from oracle import binding as ob
    c = hmc.cases()[name]
    mesh = hmc.mesh_hits64(c)
    plane, tol = nhm.depth_plane(mesh, c["V"], c["P"])
    *g, near = hmc.oracle_gbuffer_cut(ob, c, plane, tol)
    g = tuple(g)
    r = hmc.restate_with(c, g, mesh, hc.prepared(c))
    r["fragile"] = r["fragile"] | (near & mesh["hit"])   # a splat at the plane: the device's fp32 plane could cut it or keep it
    r["uncut"] = hc.oracle_gbuffer(ob, c)
    return c, g, mesh, r


@pytest.mark.parametrize("name", sorted(hmc.cases()))
def test_restatement_on_the_oracle_gbuffer(name):
    c, g, mesh, r = _oracle_frame(name)
    share = r["fragile"].mean()
    st = r["state"]
    print(f"{name}: fragile {share:.4f}, lit {int((st == 3).sum())}, settled {int((st == 4).sum())}, discarded {int((st == 1).sum())}, "
          f"composited {int(r['composited'].sum())}, mesh rays {int(r['mesh_rays'].sum())}, occluded {int(r['occluded'].sum())}")
    assert share <= hmc.FRAGILE_CAP
    assert np.isfinite(r["image"]).all()
    assert (r["image"][r["composited"], 3] == 1.0).all()
    hit = mesh["hit"]
    if c["mesh_min_T"] >= 1.0:
        assert not r["composited"].any()
    elif c["mesh_min_T"] == 0.0:
        assert (r["composited"] == (hit & (r["T"] > 0.0) & (st != 0))).all()
    if c["light"].get("shadows_mode", 0) == 0 or not c["lights"]:
        assert r["mesh_rays"].sum() == 0 and r["shadow_rays"].sum() == 0
    # the cut: where no mesh is hit the G-buffer is the uncut one; a pick that survives lies in front of the plane
    u = r["uncut"]
    for a_, b_ in zip(g, u):
        assert a_[~hit].tobytes() == b_[~hit].tobytes()
    ok = ~r["fragile"]
    assert not (ok & (st == 4)).any(), "a surface behind the mesh survived the depth test on a non-fragile pixel"
    if name.startswith("m06"):   # the veil's large splats reach under the floor: some are cut
        assert (hit & (g[2] != u[2])).sum() < 200
    elif name in ("m02_wall", "m12_deep"):
        cut = hit & (g[2] != u[2])
        behind = ok & (st == 1) & r["composited"] & (u[2] != 0xFFFFFFFF)
        print(f"{name}: {int(cut.sum())} pixels whose pick the plane changed, {int(behind.sum())} discarded behind the mesh and composited at T = 1")
        assert cut.sum() >= 20 and behind.sum() >= 20
    else:
        assert all(a_.tobytes() == b_.tobytes() for a_, b_ in zip(g, u)), "the floor under the splats must occlude nothing"


def test_the_plane_is_one_on_misses_and_the_hit_depth_elsewhere():
    c = hmc.cases()["m01_3dgs_floor"]
    mesh = hmc.mesh_hits64(c)
    plane, tol = nhm.depth_plane(mesh, c["V"], c["P"])
    assert (plane[~mesh["hit"]] == 1.0).all() and mesh["hit"].sum() > 500
    assert ((plane[mesh["hit"]] > 0.0) & (plane[mesh["hit"]] < 1.0)).all() and (tol[mesh["hit"]] < 1e-5).all()


def test_rules_on_an_edited_gbuffer():
    """a settled pixel behind the mesh, a discarded pixel, and the threshold at exactly T"""
    c, g, mesh, r = _oracle_frame("m03_3dgut")
    img, depth, ids, nrm = (a.copy() for a in g)
    lit = np.argwhere((r["state"] == 3) & mesh["hit"] & ~r["fragile"])
    assert len(lit) >= 3
    (ya, xa), (yb, xb), (yc, xc) = lit[0], lit[1], lit[2]
    m2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in mesh.items()}
    m2["t"][ya, xa] = 0.5 * r["t"][ya, xa]          # a: the mesh in front of the surface
    nrm[yb, xb] = 0.0                                # b: no normal: discarded
    img[yc, xc, 3] = np.float32(0.75)                # c: T = 0.25 exactly
    c2 = dict(c, mesh_min_T=0.25)
    r2 = hmc.restate_with(c2, (img, depth, ids, nrm), m2, hc.prepared(c))
    # a: settled: the raster colour unlit, T its own; T = 1 - alpha > 0.25 or not decides the composite
    assert r2["state"][ya, xa] == 4 and not r2["fragile"][ya, xa]
    Ta = float(np.float32(1.0) - img[ya, xa, 3])
    assert r2["T"][ya, xa] == Ta
    if Ta > 0.25:
        assert r2["composited"][ya, xa] and r2["image"][ya, xa, 3] == 1.0 and (r2["image"][ya, xa, :3] >= img[ya, xa, :3] - 1e-12).all()
    else:
        assert not r2["composited"][ya, xa] and np.array_equal(r2["image"][ya, xa], img[ya, xa].astype(np.float64))
    # b: discarded: radiance 0 and T = 1, so the mesh alone at full weight
    assert r2["state"][yb, xb] == 1 and r2["T"][yb, xb] == 1.0 and r2["composited"][yb, xb] and r2["image"][yb, xb, 3] == 1.0
    # c: T > threshold fails at equality, and is fragile there
    assert not r2["composited"][yc, xc] and r2["fragile"][yc, xc] and r2["image"][yc, xc, 3] == 0.75
    # everything else is untouched by the edits
    same = np.ones(r["state"].shape, bool)
    for y, x in ((ya, xa), (yb, xb), (yc, xc)):
        same[y, x] = False
    keep = same & ((r["T"] > 0.25) | ~mesh["hit"])
    assert np.array_equal(r2["image"][keep], r["image"][keep])
