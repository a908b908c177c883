"""GPU tests (-m gpu) of hybrid frames with meshes (mgs_frame_set_hybrid_meshes), one child process per group.

cases   every case of hybrid_mesh_cases.py:
        * the hit records of the depth pre-pass against np_mesh_rays in float64 (mesh_ray_cases.GPU_*_BAR), ids equal on non-fragile pixels;
        * the depth plane against float64 from the device's own hit records within np_hybrid_mesh.depth_plane's tolerance, exactly 1.0 on
          misses;
        * the raster step: image, picked depth, ids and normal that mgs_render (lighting 0, surface outputs 1) leaves on another handle
          with the downloaded plane bound through mgs_frame_upload_occluder.  The side outputs are compared byte for byte with the
          hybrid frame's; the unlit image is the restatement's input (the hybrid frame's own unlit pixel is overwritten by its light
          pass and cannot be downloaded), and byte for byte the hybrid frame's pixel wherever the hand-over leaves the pixel alone;
        * the final frame against np_hybrid_mesh fed that G-buffer and the device's hit records: PSNR >= 50 dB and 1e-3 on every
          non-fragile pixel (DESIGN 3.18's bars), alpha exactly 1 on composited pixels, shadow hits equal, the sums bounded.
props   the defining properties, the byte equalities, formats, accumulation, strips, a frame context and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hybrid_cases as hc
import hybrid_mesh_cases as hmc
import mesh_ray_cases as mrc
import np_hybrid_mesh as nhm
import np_lighting as nl
import np_mesh_rays as nr
import np_trace
from oracle import binding as ob

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("image", "depth", "id", "normal")
UNSUPPORTED, STATE = -8, -6


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    got = {}

    def run(mode):
        if mode not in got:
            out = str(tmp_path_factory.mktemp(mode) / "out.npz")
            r = subprocess.run([sys.executable, os.path.join(HERE, "_child_hybrid_mesh.py"), mode, out], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
            got[mode] = dict(np.load(out))
        return got[mode]
    return run


def against_restatement(r, tag, case):
    """every assertion of one frame; returns (psnr, worst non-fragile error, the restatement)"""
    rec = r[f"{tag}_mesh"]
    mesh = nhm.from_records(rec)
    # the depth plane from the device's own records
    plane, tol = nhm.depth_plane(mesh, case["V"], case["P"])
    got_plane = r[f"{tag}_plane"]
    assert (got_plane[~mesh["hit"]] == np.float32(1.0)).all(), "the plane is not exactly 1.0 on a miss"
    derr = np.abs(got_plane.astype(np.float64) - plane)[mesh["hit"]]
    print(f"{tag}: depth plane worst error {derr.max() if derr.size else 0.0:.3e} (tolerance up to {tol.max():.3e})")
    assert (derr <= tol[mesh["hit"]]).all()
    # the raster step: the side outputs of the frame rendered alone against the same plane
    for k in KEYS[1:]:
        assert r[f"{tag}_u_{k}"].tobytes() == r[f"{tag}_{k}"].tobytes(), f"the raster pass's {k} differs from mgs_render's against the same plane"
    g = tuple(r[f"{tag}_u_{k}"] for k in KEYS)
    ref = hmc.restate_with(case, (nl.from_target(g[0]),) + g[1:], mesh, hc.prepared(case))
    ok, st = ~ref["fragile"], ref["state"]
    got = r[f"{tag}_image"]
    img = nl.from_target(got).astype(np.float64)
    alone = ((st == 0) | (st == 2) | (st == 4)) & ~(ref["composited"] & mesh["hit"])
    assert got[alone & ok].tobytes() == g[0][alone & ok].tobytes(), "a pixel the hand-over settles is not the raster pass's pixel"
    assert not got[ok & (st == 1) & ~ref["composited"]].any(), "a discarded pixel without a composited mesh is not (0,0,0,0)"
    assert np.array_equal(r[f"{tag}_shadow_hits"][ok], ref["shadow_hits"][ok]), "shadow hit counts differ on non-fragile pixels"
    assert (img[ok & ref["composited"], 3] == 1.0).all(), "alpha is not exactly 1 on a composited mesh pixel"
    psnr = np_trace.psnr_rgb(img, ref["image"])
    worst = np.abs(img - ref["image"])[ok].max()
    share = ref["fragile"].mean()
    print(f"{tag}: PSNR {psnr:.2f} dB, worst non-fragile channel {worst:.3e}, fragile {share:.4f}, composited {int(ref['composited'].sum())}, "
          f"lit {int((st == 3).sum())}, settled {int((st == 4).sum())}, discarded {int((st == 1).sum())}, light_ms {float(r[f'{tag}_light_ms']):.3f}")
    assert share <= hmc.FRAGILE_CAP
    assert psnr >= 50.0 and worst <= 1e-3
    # the sums: between the non-fragile pixels' and those plus what the fragile pixels may add (two shading sites, every light)
    nlights, fr = max(len(case["lights"]), 1), int((~ok).sum())
    rays = int(r[f"{tag}_shadow_rays"])
    assert ref["shadow_rays"][ok].sum() <= rays <= ref["shadow_rays"][ok].sum() + 2 * nlights * fr
    occ = int(r[f"{tag}_shadow"][5])
    assert ref["occluded"][ok].sum() <= occ <= ref["occluded"][ok].sum() + 2 * nlights * fr
    assert int(r[f"{tag}_shadow_accepted"]) == int(r[f"{tag}_shadow_hits"].sum())
    assert int(r[f"{tag}_primary"][5]) == int(mesh["hit"].sum()) and int(r[f"{tag}_error_flags"]) == 0
    return psnr, worst, ref


@pytest.mark.parametrize("name", sorted(hmc.cases()))
def test_case_against_restatement(child, name):
    r, case = child("cases"), hmc.cases()[name]
    _, _, ref = against_restatement(r, name, case)
    # the hit records against the float64 mesh rays
    m = hmc.mesh_hits64(case)
    h = r[f"{name}_mesh"]
    nf = ~m["fragile"] & m["ok"]
    hit = h["hit"] == 1
    assert np.array_equal(hit[nf], m["hit"][nf])
    for key, rk in (("instance_id", "inst"), ("primitive_id", "prim"), ("material_id", "mat")):
        assert np.array_equal(h[key][nf & hit], m[rk][nf & hit]), key
    got = dict(hit=hit.reshape(-1), t=h["t"].reshape(-1), b1=h["b1"].reshape(-1), b2=h["b2"].reshape(-1), pos=h["position"].reshape(-1, 3),
               nrm=h["normal"].reshape(-1, 3))
    flat = {k: v.reshape((-1,) + v.shape[2:]) for k, v in m.items() if not np.isscalar(v)}
    e = nr.errors(got, flat, nf.reshape(-1))
    print(f"{name}: mesh errors {e}")
    assert e["t"] <= mrc.GPU_T_BAR and e["pos"] <= mrc.GPU_POS_BAR and e["nrm"] <= mrc.GPU_NRM_BAR
    assert int(r[f"{name}_primary"][6]) == int((~m["ok"]).sum()) and int(r[f"{name}_primary"][0]) == m["triangles"]
    if name.startswith("m06_threshold_1"):
        assert not ref["composited"].any()
    elif name == "m06_threshold_05":
        on = ref["composited"][hit]
        assert on.any() and not on.all()
    else:
        assert ref["composited"].sum() >= 200
    if name == "m02_wall":
        assert ((ref["state"] == 1) & ref["composited"]).sum() >= 20   # discarded behind the wall: the mesh at T = 1
        # the wall's shadow on the splats, apart from the depth cut: lit splat pixels whose light the MESH occludes (the restatement's
        # occlusion answer, held per pixel above) are darker than in the same frame, the setting on, without shadow rays
        shadowed = ~ref["fragile"] & (ref["state"] == 3) & (ref["occluded"] > 0)
        a, b = r["m02_wall_image"][..., :3].sum(-1), r["m02_wall_shadows_off_image"][..., :3].sum(-1)
        print(f"m02: {int(shadowed.sum())} lit splat pixels in the wall's shadow, {int((shadowed & (a < b)).sum())} of them darker than without shadow rays")
        assert shadowed.sum() >= 5 and (a < b)[shadowed].all()
    if name == "m04_fisheye":
        assert (~m["ok"]).sum() > 50


@pytest.mark.parametrize("tag", ["f16", "u8"])
def test_target_formats(child, tag):
    """T comes from the stored alpha of that format: the restatement is fed the frame of that format rendered alone against the plane.
    As hybrid_cases' format tests: the frame against the converted restatement at the bar of the frames"""
    r, case = child("props"), hmc.cases()["m06_threshold_0"]
    assert r[f"target_{tag}_u_image"].dtype == (np.float16 if tag == "f16" else np.uint8)
    rec = r[f"target_{tag}_mesh"]
    mesh = nhm.from_records(rec)
    g = tuple(r[f"target_{tag}_u_{k}"] for k in KEYS)
    for k in KEYS[1:]:
        assert g[KEYS.index(k)].tobytes() == r[f"target_{tag}_{k}"].tobytes()
    ref = hmc.restate_with(case, (nl.from_target(g[0]),) + g[1:], mesh, hc.prepared(case))
    got = r[f"target_{tag}_image"]
    ok = ~ref["fragile"]
    want = nl.from_target(nl.to_target(ref["image"], tag)).astype(np.float64)
    psnr = np_trace.psnr_rgb(nl.from_target(got).astype(np.float64), want)
    step = 2.0 ** -10 * np.maximum(np.abs(want), 2.0 ** -14) if tag == "f16" else 1.0 / 255.0   # one unit of the stored value
    err = np.abs(nl.from_target(got).astype(np.float64) - want)
    print(f"target {tag}: PSNR against the converted restatement {psnr:.2f} dB, worst error in stored units {(err / step)[ok].max():.2f}")
    assert psnr >= 50.0 and (err <= step * 1.001)[ok].all()
    assert (nl.from_target(got)[ok & ref["composited"], 3] == 1.0).all()


def test_splat_shadow_on_the_floor(child):
    r = child("props")
    c1 = hmc.cases()["m01_3dgs_floor"]
    mesh = nhm.from_records(r["m01_mesh"])
    floor = mesh["hit"] & (r["m01_id"] == 0xFFFFFFFF)
    a, b = r["m01_image"][..., :3].sum(-1), r["m01_shadows_off_image"][..., :3].sum(-1)
    darker = floor & (a < b - 0.05)
    print(f"m01: {int(darker.sum())} floor pixels darker with shadows on, of {int(floor.sum())}")
    assert darker.sum() >= 10 and c1["W"] == 48


def test_setting_off_invisible_and_rebuilds(child):
    r = child("props")
    assert r["m01_same_twice"] and r["off_after_on_same"] and r["invisible_same"] and r["invisible_hits_all_miss"]
    assert r["trace_meshes_ignored_when_on"] and r["moved_differs"]
    # (visibility is not part of the hierarchy's signature: the walk skips an invisible instance's triangles)
    assert int(r["rebuilt_unchanged"]) == 0 and int(r["rebuilt_moved"]) == 1
    assert int(r["mesh_hits_after_off"]) == STATE and int(r["plane_after_off"]) == STATE
    # hit record 64 B, its t 4 B, T 4 B, the plane 4 B a pixel
    assert int(r["working_bytes_growth"]) >= 48 * 40 * (64 + 4 + 4 + 4)


def test_refusals(child):
    r = child("props")
    assert int(r["occluder_on"]) == UNSUPPORTED and int(r["occluder_off"]) == UNSUPPORTED
    assert int(r["trace_meshes_off"]) == UNSUPPORTED and int(r["soft_on"]) == UNSUPPORTED


def test_temporal_accumulation_after_the_composite(child):
    r = child("props")
    singles, acc = r["dof_singles"].astype(np.float32), r["dof_accumulated"].astype(np.float32)
    assert not np.array_equal(singles[0], singles[2])
    main = np.zeros_like(singles[0])
    for k in range(3):
        main = ob.post_accumulate(main, singles[k], k)
        err = float(np.abs(acc[k] - main).max())
        print(f"temporal accumulation of hybrid frames with meshes, sample {k}: worst error {err:.3e}")
        assert err <= 1e-3, k


def test_strips_and_frame_context(child):
    r = child("props")
    assert r["strip_0"] and r["strip_1"]
    assert r["context_off_by_default"] and r["context_same"]


def test_render_tool_hybrid_meshes(tmp_path):
    """tools/mgs_render.py --pipeline hybrid --mesh ... --hybrid-meshes 1: the route renders (the pre-pass hits the mesh, mesh pixels are
    opaque, the threshold reaches the setting), and its argument checks refuse what the frame cannot do"""
    import re
    root = os.path.dirname(HERE)
    tool, obj = os.path.join(root, "tools", "mgs_render.py"), os.path.join(HERE, "golden", "meshes", "fixture.obj")
    out = str(tmp_path / "frame.npy")
    base = [sys.executable, tool, "syn:3000", out, "--size", "96", "64", "--pipeline", "hybrid", "--lighting", "1", "--shadows", "1"]
    r = subprocess.run(base + ["--mesh", obj, "--hybrid-meshes", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    m = re.search(r"depth pre-pass: (\d+) hits", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout
    img = np.load(out)
    assert img.shape == (64, 96, 4) and (img[..., 3] == 1.0).sum() >= int(m.group(1)) // 2 > 0
    r1 = subprocess.run(base + ["--mesh", obj, "--hybrid-meshes", "1", "--mesh-composite-threshold", "1.0"], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0 and not np.array_equal(np.load(out), img)   # threshold 1: no mesh pixel is composited
    for extra, word in ((["--hybrid-meshes", "1"], "--mesh"), (["--mesh", obj], "--hybrid-meshes 1"),
                        (["--mesh", obj, "--hybrid-meshes", "1", "--shadows", "2"], "hard shadows")):
        bad = subprocess.run(base[:-2] + extra if "--shadows" in extra else base + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and word in bad.stderr, bad.stderr[-800:]
