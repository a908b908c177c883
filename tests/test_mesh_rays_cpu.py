"""Mesh ray queries without a device: the float64 brute force against hand-computed hits, the fragile cap of the committed cases,
the float32 restatement of the kernel's arithmetic against float64 (which sets the GPU test's bars), the watertight case on the
restatement, the rasteriser comparison's excluded share, and the host-side argument checks of the two entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ray_cases as mrc
import np_mesh_rays as nr
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_macro_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_MESH_RAY_QUERY 1", hdr)
    lib = capi.load_library()
    for name in ("mgs_mesh_ray_params_default", "mgs_trace_mesh_rays", "mgs_trace_mesh_rays_device"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(capi.MeshHit) == 64 == capi.MESH_HIT_DTYPE.itemsize and C.sizeof(capi.MeshRayParams) == 16
    q = capi.MeshRayParams(7, 7, (C.c_uint32 * 2)(1, 1))
    lib.mgs_mesh_ray_params_default(C.byref(q))
    assert (q.mode, q.reorder, list(q.reserved)) == (0, 0, [0, 0])


def test_reference_on_two_hand_computed_triangles():
    """triangle 0 in the plane z = 0, triangle 1 (material 1) in the plane z = -1 behind it, under a translation by (1, 0, 0)"""
    M = np.eye(4, dtype=np.float32)
    M[0, 3] = 1.0
    mesh = dict(positions=np.float32([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, -1], [4, 0, -1], [0, 4, -1]]), indices=[[0, 1, 2], [3, 4, 5]],
                normals=np.float32([[0, 0, 1]] * 3 + [[0, 1, 0]] * 3), material_ids=[0, 1], transform=M, visible=True)
    O = np.float32([[1.5, 0.5, 3], [1.5, 0.5, 3], [3.5, 0.5, 3], [1.5, 0.5, 3], [1.5, 0.5, 3], [9, 9, 3], [1.5, 0.5, -3]])
    D = np.float32([[0, 0, -1], [0, 0, -2], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 1]])
    tmin = np.float32([0, 0, 0, 3.5, 0, 0, 0])
    tmax = np.float32([100, 100, 100, 100, 3.0, 100, 100])
    for fn in (nr.trace, nr.trace_f32):
        r = fn([mesh], O, D, tmin, tmax)
        assert r["hit"].tolist() == [True, True, True, True, False, False, True]
        assert r["prim"].tolist() == [0, 0, 1, 1, nr.NONE, nr.NONE, 1]           # ray 3 starts behind triangle 0; ray 4's window ends AT it (open)
        assert np.allclose(r["t"][[0, 1, 2, 3, 6]], [3.0, 1.5, 4.0, 4.0, 2.0], rtol=0, atol=1e-6)
        assert r["mat"].tolist()[:4] == [0, 0, 1, 1] and r["inst"].tolist()[:4] == [0] * 4
        assert np.allclose([r["b1"][0], r["b2"][0]], [0.25, 0.25], atol=1e-6)  # local point (0.5, 0.5, 0)
        assert np.allclose(r["pos"][0], [1.5, 0.5, 0.0], atol=1e-6) and np.allclose(r["nrm"][0], [0, 0, 1], atol=1e-6)
        assert np.allclose(r["nrm"][2], [0, 1, 0], atol=1e-6)                    # the vertex normals, not the face's; not flipped
    hidden = nr.trace([dict(mesh, visible=False)], O, D, tmin, tmax)
    assert not hidden["hit"].any() and hidden["triangles"] == 2


@pytest.fixture(scope="module")
def measured():
    out = {}
    for name in mrc.batches():
        rays = mrc.rays_of(name)
        ref = mrc.reference(name)
        f32 = nr.trace_f32(mrc.scenes()[mrc.batches()[name][0]], *rays)
        out[name] = (rays, ref, f32)
    return out


def test_fragile_share_of_every_case_is_under_the_cap(measured):
    sizes = {n: measured[n][0][0].shape[0] for n in measured}
    assert sizes == {"tiny_1": 1, "tiny_255": 255, "mid_256": 256, "mid_257": 257, "big_4000": 4000}
    for name, (rays, ref, _) in measured.items():
        share = ref["fragile"].mean()
        print(f"{name}: fragile {share:.4f}, hits {ref['hit'].mean():.3f}, invalid {(~ref['valid']).sum()}")
        assert share <= mrc.FRAGILE_CAP, name
        if rays[0].shape[0] > 1:
            assert 0.15 < ref["hit"].mean() < 0.999, name          # the batch both hits and misses
    big = measured["big_4000"][1]
    assert (~big["valid"]).sum() > 6                                # the generated fisheye rays outside the image circle too
    tri, prim, inst, mat, vis, valid, _, _ = nr.world_triangles(mrc.scenes()["big"])
    assert (~valid).sum() >= 2 and [len(m["indices"]) for m in mrc.scenes()["big"]] == [512, 513, 10, 64]
    assert [len(m["indices"]) for m in mrc.scenes()["tiny"]] == [1, 7, 8, 9] and [len(m["indices"]) for m in mrc.scenes()["mid"]][:2] == [64, 65]


def test_f32_restatement_agrees_and_sets_the_bars(measured):
    worst = dict(t=0.0, bary=0.0, pos=0.0, nrm=0.0)
    for name, (_, ref, f32) in measured.items():
        ok = ~ref["fragile"]
        assert np.array_equal(f32["hit"][ok], ref["hit"][ok]), name
        assert np.array_equal(f32["prim"][ok], ref["prim"][ok]) and np.array_equal(f32["inst"][ok], ref["inst"][ok]), name
        assert np.array_equal(f32["mat"][ok], ref["mat"][ok]), name
        assert f32["leaf_ok"].all(), name       # no accepted hit is refused by its own leaf box under slabHit (window and cut = its t)
        e = nr.errors(f32, ref, ok)
        print(name, {k: f"{v:.3e}" for k, v in e.items()})
        worst = {k: max(worst[k], e[k]) for k in worst}
    print("worst", {k: f"{v:.3e}" for k, v in worst.items()})
    for got, const in ((worst["t"], mrc.T_F32_VS_F64), (worst["bary"], mrc.BARY_F32_VS_F64), (worst["pos"], mrc.POS_F32_VS_F64),
                       (worst["nrm"], mrc.NRM_F32_VS_F64)):
        assert abs(got - const) <= 0.02 * const, (got, const)      # the constants ARE the measurement


@pytest.mark.parametrize("shift", [None, mrc.WT_SHIFT], ids=["identity", "translated"])
def test_watertight_case_is_exact_on_the_restatement(shift):
    O, D, tmin, tmax, t, prim = mrc.watertight_rays(shift)
    got = nr.trace_f32([mrc.watertight_mesh(shift)], O, D, tmin, tmax)
    assert got["hit"].all() and np.array_equal(got["t"], t) and np.array_equal(got["prim"], prim)
    assert O.shape[0] > 300


def test_rasteriser_comparison_leaves_out_at_most_the_cap():
    view = capi.Mesh.load_obj(mc.FIXTURE).view()
    comparable, prim = mrc.raster_mask(mc.fixture_meshes(view))
    print(f"pick image: excluded {1 - comparable.mean():.4f}, covered {(prim != nr.NONE).mean():.3f}")
    assert 1 - comparable.mean() <= mrc.RASTER_EXCLUDED_CAP and (prim != nr.NONE).mean() > 0.1


def test_argument_checks_need_no_device():
    """every check below runs before the handle is looked at: a null handle is only reported when they pass"""
    lib = capi.load_library()
    rays = capi.make_rays(np.zeros((4, 3)), np.tile([0, 0, 1.0], (4, 1)))
    hits = np.zeros(4, capi.MESH_HIT_DTYPE)
    rp, hp = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)

    def call(fn, q, r=rp, h=hp, n=4):
        return fn(None, r, n, C.byref(q) if q is not None else None, h, None), lib.mgs_last_error().decode()

    for fn in (lib.mgs_trace_mesh_rays, lib.mgs_trace_mesh_rays_device):
        for bad in (capi.MeshRayParams(2, 0), capi.MeshRayParams(-1, 0), capi.MeshRayParams(0, 2), capi.MeshRayParams(0, 0, (C.c_uint32 * 2)(0, 1)),
                    capi.MeshRayParams(1, 1, (C.c_uint32 * 2)(5, 0))):
            rc, msg = call(fn, bad)
            assert rc == -1 and "null scene" not in msg, msg                      # MGS_ERR_INVALID_ARG
        rc, msg = call(fn, None, r=None)
        assert rc == -1 and "null rays or hits" in msg
        rc, msg = call(fn, None, h=None)
        assert rc == -1 and "null rays or hits" in msg
        rc, msg = call(fn, None, n=1 << 31)
        assert rc != 0 and rc != -1 and "2^31 - 1" in msg                         # MGS_ERR_UNSUPPORTED
        rc, msg = call(fn, capi.MeshRayParams(1, 1))
        assert rc == -1 and "null scene" in msg                                   # everything else passed
    rc, msg = call(lib.mgs_trace_mesh_rays_device, None, r=C.c_void_p(rp.value + 4))
    assert rc == -1 and "16-byte aligned" in msg
    rc, msg = call(lib.mgs_trace_mesh_rays, None, r=C.c_void_p(rp.value + 4))     # host arrays are staged: no alignment asked
    assert "null scene" in msg
    assert call(lib.mgs_trace_mesh_rays, None, n=0)[1].count("null scene") == 1  # count 0 still needs a handle
