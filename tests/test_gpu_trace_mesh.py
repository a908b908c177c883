"""Traced frames with mesh hits (mgs_frame_set_trace_meshes) on the device, one child process per group.

cases     every case of trace_mesh_cases.py against the float64 restatement (np_trace_mesh.py), RGBA32F: on non-fragile pixels hit
          counts, picked ids, shadow hit counts and the mesh hit's ids are equal; t, position and normal within
          mesh_ray_cases.GPU_*_BAR; surface depth within depth_tol; discarded pixels without a mesh exactly 0; PSNR >= 50 dB;
          worst non-fragile channel <= 1e-3; the integer statistics between the non-fragile sums and those plus the fragile pixels'.

exact     the frame's hit records equal, byte for byte, the mesh ray query in closest mode on the generated rays with the window
          (0.001, 10000), pinhole (u1) and fisheye with depth of field (u5); the primary statistics equal the query's; the unlit
          composite equals the ray query cut at the mesh plus float(T) * (emission + ambient + diffuse), alpha 1 on the mesh.
lit       the mesh points' colour equals the light query (mgs_shade_points) at the hit records where no mesh occludes the light and
          the walk's T is 1: the splats' shadow on the mesh floor (l1); mesh on mesh (l3): the points the occlusion query reports
          occluded get the ambient term alone.
unmoved   setting off, or on with every instance invisible: byte-identical to the scene without meshes; strips, a frame context,
          target formats, mgs_render and the mesh query before and after.
lifecycle rebuilds, visibility, working_bytes, error codes.
The bars: sums of a handful of fp32 products per channel with values below 4: 16 ulps of 4 = 1e-5 (the composite adds in fp32 what
the test adds in float64 from fp32 inputs)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ray_cases as mrc
import np_lighting as nl
import np_mesh_rays as nr
import np_trace as nt
import np_trace_lit as ntl
import trace_mesh_cases as tmc
from vk_gaussian_splatting_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-5
UNSUPPORTED, STATE = -8, -6


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    got = {}

    def run(mode):
        if mode not in got:
            out = str(tmp_path_factory.mktemp(mode) / "out.npz")
            r = subprocess.run([sys.executable, os.path.join(HERE, "_child_trace_mesh.py"), mode, out], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
            got[mode] = np.load(out)
        return got[mode]
    return run


@pytest.mark.parametrize("name", list(tmc.cases()))
def test_case_against_the_float64_restatement(child, name):
    against_restatement(child("cases"), name, tmc.restate(name), tmc.cases()[name])


@pytest.mark.parametrize("fmt", ["f16", "u8"])
@pytest.mark.parametrize("name", ["u1", "l1"])
def test_quantised_splat_storage_stays_within_the_bars(child, name, fmt):
    """fp16 / uint8 colour and SH storage: the SHF != fp32 instantiations of k_trace<., ., true> in front of the composite, against the
    restatement of the arrays as the device holds them"""
    r, case = child("storage"), tmc.cases()[name]
    inst = [(ntl.prepare_set(a, rgba=r[f"{name}_{fmt}_rgba_{k}"], sh=r[f"{name}_{fmt}_sh_{k}"]), M) for k, (a, M) in enumerate(case["sets"])]
    against_restatement(r, f"{name}_{fmt}", tmc.restate_with(case, inst), case)


def against_restatement(r, name, ref, case):
    lit = "lights" in case
    img, want = r[name + "_image"].astype(np.float64), ref["image"]
    nf = ~ref["fragile"] & ref["ok"]
    fr = ref["fragile"] & ref["ok"]
    print(f"{name}: fragile {fr.mean():.4f}")
    # integers
    assert np.array_equal(r[name + "_hits"][nf], ref["hits"][nf])
    assert np.array_equal(r[name + "_id"].astype(np.int64)[nf], ref["id"][nf])      # (the side output is in the caller's ids)
    if lit:
        assert np.array_equal(r[name + "_shadow_hits"][nf], ref["shadow_hits"][nf])
    h, m = r[name + "_mesh"], ref["mesh"]
    hit = h["hit"] == 1
    assert np.array_equal(hit[nf], m["hit"][nf])
    for key, rk in (("instance_id", "inst"), ("primitive_id", "prim"), ("material_id", "mat")):
        assert np.array_equal(h[key][nf], m[rk][nf]), key
    got = dict(hit=hit.reshape(-1), t=h["t"].reshape(-1), b1=h["b1"].reshape(-1), b2=h["b2"].reshape(-1), pos=h["position"].reshape(-1, 3),
               nrm=h["normal"].reshape(-1, 3))
    flat = {k: (v if np.isscalar(v) else v.reshape((-1,) + v.shape[2:])) for k, v in m.items()}
    e = nr.errors(got, flat, nf.reshape(-1))
    print(f"{name}: mesh errors {e}")
    assert e["t"] <= mrc.GPU_T_BAR and e["pos"] <= mrc.GPU_POS_BAR and e["nrm"] <= mrc.GPU_NRM_BAR
    # depth
    derr = np.abs(r[name + "_depth"].astype(np.float64) - ref["depth"])
    assert (derr[nf] <= ref["depth_tol"][nf] + 1e-7).all(), float((derr - ref["depth_tol"])[nf].max())
    # the image
    empty = nf & ~m["hit"] & (want == 0).all(-1)
    assert (img[empty] == 0).all()
    psnr = nt.psnr_rgb(img, want)
    worst = np.abs(img - want)[nf].max()
    print(f"{name}: PSNR {psnr:.1f} dB, worst non-fragile channel {worst:.2e}")
    assert psnr >= 50.0 and worst <= 1e-3
    assert (img[nf & ref["composited"], 3] == 1.0).all()
    # statistics: between the non-fragile pixels' sums and those plus what the fragile pixels may add
    nl_ = max(len(case.get("lights", [])), 1)
    prim_hits = int(r[name + "_primary"][5])
    assert m["hit"][nf].sum() <= prim_hits <= m["hit"][nf].sum() + fr.sum()
    assert int(r[name + "_primary"][6]) == int((~ref["ok"]).sum()) and int(r[name + "_primary"][0]) == m["triangles"]
    acc = int(r[name + "_accepted"])
    assert ref["hits"][nf].sum() <= acc <= ref["hits"][nf].sum() + (ref["base"]["candidates"][fr] + 1).sum()
    if lit:
        occ = int(r[name + "_shadow"][5])
        assert ref["occluded"][nf].sum() <= occ <= ref["occluded"][nf].sum() + 2 * nl_ * fr.sum()
        rays = int(r[name + "_shadow_rays"])
        assert ref["shadow_rays"][nf].sum() <= rays <= ref["shadow_rays"][nf].sum() + 2 * nl_ * fr.sum()
    else:
        assert not r[name + "_shadow"].any()


def test_temporal_accumulation_of_mesh_frames(child):
    r = child("unmoved")
    singles, acc = r["dof_singles"].astype(np.float64), r["dof_accumulated"].astype(np.float64)
    assert np.abs(singles[0] - singles[1]).max() > 1e-3                       # the samples differ: the lens moves
    for k in range(3):
        assert np.abs(acc[k] - singles[:k + 1].mean(0)).max() <= 1e-3, k      # post_accumulate: the running mean


def mat_arrays():
    m = tmc.MATERIALS
    return {k: np.float64([x[k] for x in m]) for k in ("ambient", "diffuse", "emission")}


@pytest.mark.parametrize("name", ["u1", "u5"])
def test_hit_records_are_the_mesh_query_on_the_generated_rays(child, name):
    r = child("exact")
    mesh, query = r[name + "_mesh"], r[name + "_query"]
    assert mesh.tobytes() == query.tobytes()
    assert np.array_equal(r[name + "_primary"], r[name + "_query_stats"]) and not r[name + "_shadow"].any()
    hit = mesh["hit"] == 1
    assert 0.1 < hit.mean() < 0.9 and len(np.unique(mesh["material_id"][hit])) == 2
    if name == "u5":
        assert r[name + "_primary"][6] > 0          # fisheye pixels outside the image circle


@pytest.mark.parametrize("name", ["u1", "u5"])
def test_unlit_composite_is_the_cut_walk_plus_the_weighted_material(child, name):
    r = child("exact")
    case = tmc.cases()[name]
    mesh, walk, rays = r[name + "_mesh"], r[name + "_walk"], r[name + "_rays"]
    img = r[name + "_image"].reshape(-1, 4).astype(np.float64)
    valid = rays["t_min"] <= rays["t_max"]
    hit = mesh["hit"] == 1
    M = mat_arrays()
    T = walk["transmittance"].astype(np.float64)
    colour = (M["emission"] + M["ambient"] + M["diffuse"])[np.where(hit, mesh["material_id"], 0)]
    want = walk["radiance"].astype(np.float64) + np.where(hit[:, None], T[:, None] * colour, 0.0)
    alpha = np.where(hit, 1.0, 1.0 - T)
    err = np.abs(img[valid, :3] - want[valid]).max()
    print(f"{name}: worst channel error {err:.2e}, alpha {np.abs(img[valid, 3] - alpha[valid]).max():.2e}")
    assert err <= BAR and np.abs(img[valid, 3] - alpha[valid]).max() <= BAR
    assert np.array_equal(r[name + "_hits"].reshape(-1)[valid], walk["hit_count"][valid])
    # what the case is for: splats behind the mesh are cut (the frame without meshes has more of them), splats in front weight it
    off = r[name + "_off_image"].reshape(-1, 4)
    assert (np.abs(off[hit, :3] - img[hit, :3]).max(1) > 1e-3).any()
    assert ((T < 0.9) & hit).any() and ((T == 1.0) & hit).any()
    # surface depth: the iso pick's where there is one, else the mesh's, else 0
    depth, ids = r[name + "_depth"].reshape(-1), r[name + "_id"].reshape(-1)
    assert (depth[hit & valid] != 0).all() and (depth[~hit & (ids == 0xFFFFFFFF)] == 0).all()
    # the threshold 0.5 removes the mesh exactly where the walk's T is at or below it (pixels within 1e-6 of it left out)
    thr = r[name + "_thr_image"].reshape(-1, 4)
    gone, stays = hit & (T < 0.5 - 1e-6), hit & (T > 0.5 + 1e-6)
    assert np.abs(thr[gone, :3] - walk["radiance"][gone]).max(initial=0) <= BAR and np.abs(thr[stays] - img[stays]).max(initial=0) == 0
    if name == "u1":
        assert gone.any() and stays.any()


def test_splat_shadow_on_the_mesh_floor_is_the_light_query(child):
    r = child("lit")
    mesh, pts = r["l1_mesh"], r["l1_points"]
    img, plain = r["l1_image"].reshape(-1, 4), r["l1_noshadow_image"].reshape(-1, 4)
    hit = mesh["hit"] == 1
    bare = hit & (r["l1_hits"].reshape(-1) == 0)            # nothing in front: T = 1, base 0
    assert bare.sum() > 200
    err = np.abs(img[bare, :3].astype(np.float64) - pts["color"][bare]).max()
    print(f"l1: worst channel error against mgs_shade_points {err:.2e}")
    assert err <= BAR and (img[bare, 3] == 1.0).all()
    assert np.array_equal(r["l1_shadow_hits"].reshape(-1)[bare], pts["shadow_hits"][bare])
    darker = bare & (img[:, :3].sum(1) < plain[:, :3].sum(1) - 1e-3)
    assert darker.sum() > 10 and (pts["shadow_hits"][darker] > 0).all()      # the blob's shadow falls on the mesh
    assert not r["l1_shadow"][5]                                             # one floor: none of its occlusion rays is occluded
    assert (r["l1_off_image"].reshape(-1, 4)[bare] == 0).all()               # off: those pixels are empty


def test_mesh_shadows_on_meshes(child):
    r = child("lit")
    mesh, pts, occ = r["l3_mesh"], r["l3_points"], r["l3_occluded"] == 1
    img = r["l3_image"].reshape(-1, 4).astype(np.float64)
    hit = mesh["hit"] == 1
    M = mat_arrays()
    mid = np.where(hit, mesh["material_id"], 0)
    shaded = mid == 0                                        # material 1 is emission only: needShading 0
    lit_ok = hit & ~occ
    assert np.abs(img[lit_ok, :3] - pts["color"][lit_ok]).max() <= BAR
    shadowed = hit & occ & shaded
    assert shadowed.sum() > 10 and np.abs(img[shadowed, :3] - M["ambient"][0]).max() <= BAR      # ambient alone (inShadow)
    glow = hit & ~shaded
    assert glow.any() and np.abs(img[glow, :3] - M["emission"][1]).max() <= BAR
    assert (img[hit, 3] == 1.0).all() and (img[~hit] == 0).all()
    assert r["l3_shadow"][5] == (hit & shaded & occ).sum()   # rays occluded: one light, one ray per shaded mesh pixel


@pytest.mark.parametrize("name", ["u1", "l1"])
def test_nothing_else_moves(child, name):
    r = child("unmoved")
    for key in ("off_equal", "on_differs", "invisible_equal", "invisible_all_miss", "strips_equal", "context_equal"):
        assert bool(r[f"{name}_{key}"]), key
    on = r[name + "_on_image"]
    f16, u8 = r[name + "_target_f16"], r[name + "_target_u8"]
    assert np.array_equal(f16, on.astype(np.float16))
    assert u8.tobytes() == nl.to_target(on, "u8").tobytes() and f16.tobytes() == nl.to_target(on, "f16").tobytes()
    assert bool(r[name + "_target_f16_side_equal"]) and bool(r[name + "_target_u8_side_equal"])
    if name == "u1":
        assert bool(r["render_and_query_unmoved"])


def test_lifecycle_and_errors(child):
    r = child("lifecycle")
    assert r["rebuilt"].tolist() == [1, 0, 1, 0, 0] and bool(r["moved_changes"]) and bool(r["hidden_changes"])
    assert int(r["state_off"]) == STATE                                             # MGS_ERR_STATE
    # the documented per-pixel bytes: 64 + 4 + 4, an unlit frame's fp32 pixel and ray parameter 16 + 4; the two counter blocks, and
    # the leaf counter of the triangle hierarchy's build, which stays with the handle that ran it (as after a mesh query)
    assert int(r["working_bytes_growth"]) == 92 * int(r["pixels"]) + 64 + 4
    assert r["invalid_arg"].tolist() == [-1] * 4 and bool(r["still_on_after_refusals"])      # MGS_ERR_INVALID_ARG on a live handle
    assert r["unsupported"].tolist() == [UNSUPPORTED] * 3 and bool(r["strategy_runs_when_off"])
