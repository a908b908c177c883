"""CPU tests of the soft-shadow restatement (np_trace_soft.py), its cases, and the interface's parts that need no device."""
import ast
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import np_trace_lit as ntl
import np_trace_soft as nts
import trace_lit_cases as lc
import trace_soft_cases as sc
from np_trace_stochastic import rand, xxhash32
from vk_gaussian_splatting_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_symbols():
    h = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define MGS_HAS_SOFT_SHADOWS 1", h) and "mgs_scene_set_light_radii" in h
    lib = capi.load_library()
    assert hasattr(lib, "mgs_scene_set_light_radii") and "mgs_scene_set_light_radii" in capi.EXPORTED_SYMBOLS
    assert lib.mgs_scene_set_light_radii(None, None, 0) == -1


_PROBE = """
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from vk_gaussian_splatting_amd import capi
lib = capi.load_library()
def params(**over):
    p = capi.default_params(48, 40)
    p.lighting_mode = 1
    for k, v in over.items():
        setattr(p, k, v)
    return p
def light(mode):
    return C.byref(capi.default_trace_light_params(shadows_mode=mode))
out = []
for mode in (2, 3):
    out.append((lib.mgs_render_traced_lit(None, C.byref(params()), None, light(mode), None, None), b"null scene" in lib.mgs_last_error()))
    for pipeline in (0, 1):
        out.append((lib.mgs_render_hybrid(None, C.byref(params(pipeline=pipeline)), None, light(mode), None, None), b"null scene" in lib.mgs_last_error()))
out.append((lib.mgs_render_traced_indirect(None, C.byref(params(lighting_mode=2)), None, light(2), None, None, None, None), b"null scene" in lib.mgs_last_error()))
print(out)
"""


def _probe(switch):
    """the outcomes of SOFT (and of the out-of-range mode 3) on a null handle in a fresh process: the switch is read once per process"""
    env = {k: v for k, v in os.environ.items() if k != "MGS_SOFT_SHADOWS"}
    if switch is not None:
        env["MGS_SOFT_SHADOWS"] = switch
    r = subprocess.run([sys.executable, "-c", _PROBE, ROOT], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return ast.literal_eval(r.stdout.strip().splitlines()[-1])


def test_soft_passes_the_range_checks_under_the_process_switch():
    """With MGS_SOFT_SHADOWS=1 MGS_SHADOWS_SOFT is in range for lit and hybrid frames: the call gets as far as the null handle.
    Without the switch (or with 0) it is MGS_ERR_UNSUPPORTED before the handle is looked at, as in every earlier build.  Mode 3 stays
    out of range and the indirect frame keeps refusing SOFT, either way."""
    reached, unsupported, bad = (-1, True), (-8, False), (-1, False)
    assert _probe("1") == [reached] * 3 + [bad] * 3 + [unsupported]
    for off in (None, "0"):
        assert _probe(off) == [unsupported] * 3 + [bad] * 3 + [unsupported]


def test_draws_are_two_per_light_with_a_disk():
    lights = [dict(type=1), dict(type=0), dict(type=2), dict(type=1)]
    s = xxhash32(5, 7, 3)
    want = s
    for _ in range(4):  # lights 0 and 2; light 3 has radius 0, light 1 is directional
        want, _ = rand(want)
    assert nts.skip_draws(s, lights, [0.5, 0.5, 1.0, 0.0]) == want and nts.skip_draws(s, lights, [0.0] * 4) == s


def test_sample_lies_on_the_disk_and_r_is_drawn_first():
    L = dict(type=1, position=(0.3, 1.6, 0.2), range=10.0)
    pos = np.array([0.1, -0.5, 0.4])
    seed = xxhash32(11, 13, 0)
    s1, u1 = rand(seed)
    s2, u2 = rand(s1)
    out_seed, ldir, ldist, inr, frag, eps = nts.sample_light(L, 0.6, pos, seed, 1e-6)
    lp = np.asarray(L["position"], np.float32).astype(np.float64)
    sp = pos + ldir * ldist
    n = (lp - pos) / np.linalg.norm(lp - pos)
    assert out_seed == s2 and inr and not frag and 0.0 < eps < 1e-4
    assert abs(np.dot(sp - lp, n)) < 1e-12 and abs(np.linalg.norm(sp - lp) - float(np.float32(0.6)) * 0.5 * np.sqrt(u1)) < 1e-12
    # culled by the sample's distance: the draws are consumed anyway
    out_seed, ldir, _, inr, _, _ = nts.sample_light(dict(L, range=0.5), 0.6, pos, seed, 1e-6)
    assert out_seed == s2 and not inr and ldir is None
    # the pole of Frisvad's basis is fragile
    assert nts.sample_light(dict(L, position=(0.1, -0.5, -3.0)), 0.6, pos, seed, 1e-6)[4]


def test_zero_radii_equal_the_hard_restatement_exactly():
    name = "s02_order"
    c = sc.cases()[name]
    z = sc.restate(name, 0, (0.0, 0.0, 0.0))
    h = ntl.lit(sc.prepared(name), c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"], c["materials"], shadows=1, **lc._trace_kw(c))
    for k in ("image", "shadow_hits", "shadow_T", "fragile", "surface", "rays", "fallback"):
        assert np.array_equal(z[k], h[k]), k


def test_penumbra_differs_between_sample_ids():
    r0, r1 = sc.restate("s01_penumbra", 0), sc.restate("s01_penumbra", 1)
    ok = ~r0["fragile"] & ~r1["fragile"]
    n = int((np.abs(r0["shadow_T"] - r1["shadow_T"]).max((2, 3))[ok] > 1e-3).sum())
    print(f"non-fragile pixels of s01_penumbra whose shadow_T differs between sample ids 0 and 1: {n}")
    assert n >= 20


@pytest.mark.parametrize("name", sc.traced())
def test_fragile_cap(name):
    r = sc.restate(name, 0)
    print(f"{name}: fragile {r['fragile'].mean():.4f}, lit pixels {int(r['surface'].sum())}, shadow rays {int(r['rays'].sum())}")
    assert r["fragile"].mean() <= sc.FRAGILE_CAP and r["surface"].sum() >= 300


@pytest.mark.parametrize("name", sc.meshed())
def test_mesh_case_runs_both_loops_and_continues_the_state(name):
    c = sc.cases()[name]
    r = sc.restate_mesh(name, 0)
    ok = ~r["fragile"]
    both, fresh = r["both_loops"] & ok, r["mesh_loop_fresh"] & ok
    print(f"{name}: fragile {r['fragile'].mean():.4f}, both loops {int(both.sum())}, mesh loop from the fresh seed {int(fresh.sum())}")
    assert r["fragile"].mean() <= sc.FRAGILE_CAP and both.sum() >= 50
    # the fresh seed in all three ways: nothing picked, and a pick whose instance has needShading 0 (the second instance)
    n0 = c["sets"][0][0]["positions"].shape[0]
    assert (fresh & (r["id"] == nts.INVALID)).sum() >= 50 and (fresh & (r["id"] != nts.INVALID) & (r["id"] >= n0)).sum() >= 20
    # two draws per light with a disk separate the loops: the state the mesh loop starts from on a both-loops pixel
    y, x = np.argwhere(both)[0]
    s0 = nts.seed_of(x, y, 0)
    assert nts.skip_draws(s0, c["lights"], c["radii"]) != s0
    # with all radii 0 the frame is np_trace_mesh's hard one, exactly
    import np_trace_mesh as ntm
    z = sc.restate_mesh(name, 0, (0.0,) * len(c["lights"]))
    h = ntm.frame(sc.prepared(name), c["meshes"], [m["materials"] for m in c["meshes"]], c["V"], c["P"], c["W"], c["H"], c["eye"], c["lights"],
                  c["materials"], lit=True, mesh_min_T=c["mesh_min_T"], **dict(sc._light_kw(c), shadows=1), **lc._trace_kw(c))
    for k in ("image", "shadow_hits", "fragile", "shadow_rays", "mesh_rays", "occluded"):
        assert np.array_equal(z[k], h[k]), k


def test_range_case_is_decided_by_the_sample():
    """s03: some non-fragile pixels are culled although the light's centre is in range, or lit although it is not"""
    c = sc.cases()["s03_range"]
    r, z = sc.restate("s03_range", 0), sc.restate("s03_range", 0, (0.0,))
    ok = ~r["fragile"] & ~z["fragile"]
    assert ((r["rays"] != z["rays"]) & ok).sum() >= 5 and len(c["lights"]) == 1


def test_project_and_lights_json_radius(tmp_path):
    from vk_gaussian_splatting_amd import project
    splats = {"splatSets": [{"id": 0, "path": "a.ply"}], "splats": [{"splatSetId": 0, "name": "a"}]}
    v5 = dict(splats, version=5, renderer={"lightingMode": 1, "shadowsMode": 2},
              lights={"assets": [{"id": 7, "type": 1, "range": 7.0, "proxyScale": 0.25}, {"id": 8, "type": 1}],
                      "instances": [{"assetId": 7, "translation": [1, 2, 3]}, {"assetId": 8, "translation": [0, 0, 0]}]})
    f = tmp_path / "v5.vkgs"
    f.write_text(json.dumps(v5))
    pr = project.load_project(str(f))
    assert [L["radius"] for L in pr.lights] == [0.25, 1.0] and pr.renderer["shadowsMode"] == 2
    v3 = dict(splats, version=3, lights={"assets": [{"id": 1, "type": 1, "radius": 4.0, "scale": 0.5}], "instances": [{"assetId": 1, "position": [0, 1, 0]}]})
    f.write_text(json.dumps(v3))
    L = project.load_project(str(f)).lights[0]
    assert L["range"] == 4.0 and L["radius"] == 0.5  # the old "radius" is the range, the old "scale" the proxyScale
    # a lights.json entry: MgsLight's fields and "radius", which stays beside the C struct
    cl = capi.make_light(**json.loads('{"type": 1, "position": [0, 2, 0], "radius": 0.4}'))
    assert cl.radius == 0.4 and list(cl.position) == [0, 2, 0] and not hasattr(capi.make_light(), "radius")
