"""Mesh hits in the traced frames without a device: the header's section and macro, the binding's struct and argtypes, the argument
checks of mgs_frame_set_trace_meshes that run before the handle is looked at, and the committed cases' meshes."""
import ctypes as C
import os
import re

import numpy as np

import mesh_ray_cases as mrc
import np_mesh_rays as nr
import np_trace as nt
import np_trace_lit as ntl
import np_trace_mesh as ntm
import trace_cases as tc
import trace_lit_cases as tlc
import trace_mesh_cases as tmc
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgs_trace_mesh_params_default", "mgs_frame_set_trace_meshes", "mgs_trace_download_mesh_hits", "mgs_trace_mesh_stats")


def test_header_section_struct_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_TRACE_MESHES 1", hdr)
    assert hdr.index("MGS_HAS_MESH_RAY_QUERY): the caller's rays") < hdr.index("#define MGS_HAS_TRACE_MESHES 1") < hdr.index("runtime image comparison")
    body = hdr.split("typedef struct MgsTraceMeshParams {")[1].split("} MgsTraceMeshParams;")[0]
    assert [m for m in re.findall(r"(\w+)(?:\[\d\])?;", body)] == ["enabled", "min_mesh_composite_transmittance", "reserved"]
    lib = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\(" % name, hdr), name
    T = capi.TraceMeshParams
    assert C.sizeof(T) == 16 and (T.enabled.offset, T.min_mesh_composite_transmittance.offset, T.reserved.offset) == (0, 4, 8)
    assert C.sizeof(capi.TraceParams) == 32 and C.sizeof(capi.MeshRayOut) == 72 and C.sizeof(capi.MeshHit) == 64
    assert lib.mgs_frame_set_trace_meshes.argtypes[1]._type_ is T and lib.mgs_trace_mesh_stats.argtypes[1]._type_ is capi.MeshRayOut
    assert lib.mgs_trace_download_mesh_hits.argtypes[2] is C.c_size_t
    q = T(7, 0.5, (C.c_uint32 * 2)(1, 1))
    lib.mgs_trace_mesh_params_default(C.byref(q))
    assert (q.enabled, q.min_mesh_composite_transmittance, list(q.reserved)) == (0, 0.0, [0, 0])


def test_argument_checks_need_no_device():
    """the range checks run before the handle is looked at: a null handle is only reported when they pass"""
    lib = capi.load_library()
    T = capi.TraceMeshParams
    for bad in (T(2, 0.0), T(-1, 0.0), T(1, -0.01), T(1, 1.01), T(1, float("nan")), T(1, 0.0, (C.c_uint32 * 2)(0, 1)), T(0, 0.0, (C.c_uint32 * 2)(3, 0))):
        assert lib.mgs_frame_set_trace_meshes(None, C.byref(bad)) == -1 and "null scene" not in lib.mgs_last_error().decode()
    for good in (T(1, 0.0), T(1, 1.0), T(0, 0.5)):
        assert lib.mgs_frame_set_trace_meshes(None, C.byref(good)) == -1 and "null scene" in lib.mgs_last_error().decode()
    assert lib.mgs_frame_set_trace_meshes(None, None) == -1 and "null scene" in lib.mgs_last_error().decode()      # NULL = off: valid
    assert lib.mgs_trace_download_mesh_hits(None, None, 0) == -1 and lib.mgs_trace_mesh_stats(None, None, None) == -1


def _same(a, b, keys):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def test_walk_copy_equals_np_trace_without_meshes():
    for name in list(tc.cases())[:2]:
        c = tc.cases()[name]
        inst = [(nt.prepare_set(a), np.eye(4) if M is None else M) for a, M in c["sets"]]
        kw = tlc._trace_kw(c)
        a, b = nt.trace(inst, c["V"], c["P"], c["W"], c["H"], **kw), ntm.walk(inst, c["V"], c["P"], c["W"], c["H"], **kw)
        assert _same(a, b, a.keys()) and a["hits"].any(), name


def test_frame_without_meshes_equals_np_trace_lit_on_l01_point():
    c = dict(tlc.cases()["l01_point"], meshes=[], mesh_min_T=0.0)
    c["sets"] = [(a, np.eye(4) if M is None else M) for a, M in c["sets"]]
    got, ref = tmc.restate_with(c, [(ntl.prepare_set(a), M) for a, M in c["sets"]]), tlc.restate("l01_point")
    assert _same(got, ref, ("image", "shadow_hits", "fragile")) and np.array_equal(got["shadow_rays"], ref["rays"])
    assert np.array_equal(got["splat_lit"], ref["surface"]) and ref["shadow_hits"].any() and not got["mesh_rays"].any()


def test_every_case_keeps_its_fragile_share_under_the_cap():
    for name in tmc.cases():
        r = tmc.restate(name)
        share = r["fragile"][r["ok"]].mean()
        print(f"{name}: fragile {share:.4f}, mesh on {r['mesh']['hit'].mean():.3f}, composited {r['composited'].mean():.3f}")
        assert share <= mrc.FRAGILE_CAP, name
        assert tmc.cases()[name]["W"] <= 48 and tmc.cases()[name]["H"] <= 40


def _without_meshes(name):
    c = dict(tmc.cases()[name], meshes=[])
    return tmc.restate_with(c, [(ntl.prepare_set(a), M) for a, M in c["sets"]])


def test_each_case_does_what_it_is_for():
    R = tmc.restate
    # u1: splats behind the quad are cut (fewer hits than without the mesh), splats in front weight it by T, on non-fragile pixels
    u1, bare = R("u1"), _without_meshes("u1")
    nf = ~u1["fragile"] & ~bare["fragile"]
    assert (nf & u1["composited"] & (u1["hits"] < bare["hits"])).sum() > 50
    assert (nf & u1["composited"] & (u1["T"] < 0.9)).sum() > 20 and (nf & u1["composited"] & (u1["T"] == 1.0)).sum() > 20
    # u2: no splat set, the meshes alone
    assert not tmc.cases()["u2"]["sets"] and R("u2")["composited"].sum() > 100 and not R("u2")["hits"].any()
    # u3: the threshold removes the mesh under the dense blob and keeps it under the thin one
    u3 = R("u3")
    hit, nf = u3["mesh"]["hit"], ~u3["fragile"]
    assert (nf & hit & ~u3["composited"]).sum() > 50 and (nf & u3["composited"] & (u3["hits"] > 0) & (u3["T"] > 0.5)).sum() > 50
    # u4: the invisible instance is never hit, both transformed ones are
    inst = R("u4")["mesh"]["inst"][R("u4")["mesh"]["hit"]]
    assert set(np.unique(inst)) == {1, 2} and np.linalg.det(mrc.MIRRORED[:3, :3]) < 0
    # u5: fisheye pixels outside the circle, and a lens that moves the rays
    assert (~R("u5")["ok"]).sum() > 20 and tmc.cases()["u5"]["frame"]["dof_mode"] == 1
    # l1: the blob's shadow darkens mesh pixels (against the frame without shadow rays)
    def unshadowed(name):
        c = dict(tmc.cases()[name], light=dict(shadows_mode=0))
        return tmc.restate_with(c, [(ntl.prepare_set(a), M) for a, M in c["sets"]])
    l1, l1u = R("l1"), unshadowed("l1")
    nf = ~l1["fragile"]
    assert (nf & l1["composited"] & ~l1["splat_lit"] & (l1["image"][..., :3].sum(-1) < l1u["image"][..., :3].sum(-1) - 1e-2)).sum() > 30
    # l2: the mesh box's shadow darkens splat pixels
    l2, l2u = R("l2"), unshadowed("l2")
    nf = ~l2["fragile"]
    dark = nf & l2["splat_lit"] & (l2["occluded"] > 0)
    assert dark.sum() > 10 and (l2["image"][dark, :3].sum(-1) < l2u["image"][dark, :3].sum(-1) - 1e-3).all()
    # l3: meshes occlude mesh pixels
    l3 = R("l3")
    assert (~l3["fragile"] & l3["composited"] & (l3["occluded"] > 0)).sum() > 10
    # l4: the range skips the light on some mesh pixels and not on others; the headlight variant has no lights; both materials show
    l4 = R("l4_spot")
    nf = ~l4["fragile"] & l4["composited"]
    assert (nf & l4["range_skipped"]).sum() > 100 and (nf & ~l4["range_skipped"] & (l4["mesh_rays"] > 0)).sum() > 100
    assert not tmc.cases()["l4_headlight"]["lights"] and not R("l4_headlight")["mesh_rays"].any()
    assert set(np.unique(l4["mesh"]["mat"][l4["mesh"]["hit"]])) == {0, 1}
    # l5: a lit splat surface in front of the mesh with T left for it, and a discarded cloud: picked nowhere, the mesh at full weight
    l5 = R("l5")
    nf = ~l5["fragile"] & l5["composited"]
    assert (nf & l5["splat_lit"] & (l5["T"] > 0.05)).sum() > 20
    assert (nf & ~l5["splat_lit"] & (l5["hits"] > 0) & (l5["image"][..., 3] == 1.0)).sum() > 20
    # l6: the three K-buffer sizes, a specular material
    assert [tmc.cases()[f"l6_{k}"]["trace"]["samples_per_pass"] for k in (4, 18, 32)] == [4, 18, 32]
    assert tmc.cases()["l6_4"]["meshes"][0]["materials"][0]["shininess"] == 64.0
