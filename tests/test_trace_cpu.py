"""The traced pipeline without a device: the restatement's own consistency (np_trace.py), the share of fragile pixels of every case
the GPU test compares (so that it cannot hide behind the mask), and the argument checks of mgs_render_traced that run before the
handle is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_reference as npr
import np_trace
import trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(tc.cases())


def test_header_declares_trace():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define\s+MGS_HAS_TRACE\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr) and re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    for name in ("mgs_trace_params_default", "mgs_render_traced", "mgs_trace_download_hit_counts"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS, name
    body = hdr[hdr.index("MGS_HAS_TRACE)"):]
    assert "PARITY UNPINNED" in body and "1 - T" in body and "NOT the reference's 1.0" in body
    assert C.sizeof(capi.TraceParams) == 32 and C.sizeof(capi.TraceOut) == 56
    t = capi.default_trace_params()
    assert (t.samples_per_pass, t.max_passes, t.kernel_adaptive_clamping) == (18, 200, 1)
    assert abs(t.min_transmittance - 0.01) < 1e-7 and abs(t.depth_iso_threshold - 0.7) < 1e-7


@pytest.mark.parametrize("name", CASES)
def test_fragile_pixels_stay_rare(name):
    """at most 2 % of a frame may be set aside as fragile: the seeds of trace_cases.py are chosen so that this holds"""
    r = tc.restate(name)
    frac = float(r["fragile"].mean())
    print(f"{name}: fragile {frac:.4f}, hits max {int(r['hits'].max())}, candidates max {int(r['candidates'].max())}")
    assert frac <= 0.02


def test_cases_exercise_what_they_are_for():
    r = {n: tc.restate(n) for n in CASES}
    assert r["a_outside"]["hits"].max() > 4
    # many passes: a ray with more candidates than four slots; out of passes: more candidates than 3 x 2 AND transmittance left
    assert r["f_many_passes"]["candidates"].max() > 3 * 4
    g = r["g_out_of_passes"]
    assert ((g["candidates"] > 6) & (g["image"][..., 3] < 0.99)).any()
    assert r["m_empty"]["hits"].max() == 0 and not r["m_empty"]["image"].any()
    assert (r["h_fisheye"]["image"][0, 0] == (0, 0, 0, 1)).all()  # a corner pixel is outside the field of view
    assert np.abs(r["i_dof_0"]["image"] - r["i_dof_3"]["image"]).max() > 1e-4  # the two samples differ
    lcase = r["l_no_leaf"]
    assert not np.isin(lcase["id"], [5, 6]).any()
    assert (r["e_leaves_1"]["hits"] <= 1).all() and r["e_leaves_1"]["hits"].max() == 1
    # K-buffer sizes: some ray that is compared exactly has more candidates than the buffer the kernel holds them in
    for name, slots in (("n_spp_05", 18), ("n_spp_17", 18), ("n_spp_19", 32), ("n_spp_32", 32), ("n_spp_32_all_candidates", 32), ("n_spp_01", 4)):
        assert r[name]["candidates"][~r[name]["fragile"]].max() > slots, name
    # with min_transmittance 0 a ray ends when it has no candidate left: some ray accepts more hits than one pass holds
    assert r["n_spp_32_all_candidates"]["hits"][~r["n_spp_32_all_candidates"]["fragile"]].max() > 32
    # the set that is instanced twice is hit through both instances, and so are the mirrored and the sheared instance; the dead one never
    ids = r["r_five_instances"]["id"][~r["r_five_instances"]["fragile"]]
    for lo, hi in ((0, 220), (220, 420), (420, 640), (790, 990)):
        assert ((ids >= lo) & (ids < hi)).any(), (lo, hi)
    assert not ((ids >= 640) & (ids < 790)).any()
    assert not np.isin(r["o_dead_third"]["id"] % 3, [0])[r["o_dead_third"]["id"] != np_trace.INVALID].any()  # every third particle is dead
    # thresholds of the pick: 1.0 picks the first accepted hit wherever there is one, 0.0 picks nothing
    one, zero = r["v_iso_threshold_1"], r["v_iso_threshold_0"]
    assert np.array_equal(one["id"] != np_trace.INVALID, one["hits"] > 0) and (one["hits"] > 0).any()
    assert (zero["id"] == np_trace.INVALID).all() and not zero["depth"].any() and np.array_equal(zero["image"], one["image"])
    # the debug flags and the kernel degrees change the frame
    assert r["u_no_gaussian"]["hits"].max() == 1 and np.abs(r["u_sh_only"]["image"] - r["u_no_gaussian"]["image"]).max() > 1e-2
    degs = [r[f"j_degree_{d}"]["image"] for d in (1, 3, 4, 5, 8)]
    assert all(np.abs(a - b).max() > 1e-3 for a, b in zip(degs, degs[1:]))
    # normals: the iso-surface method and the thin-particle branches give other normals than the default
    case = tc.cases()["t_normal_thin"]
    s = np.exp(case["sets"][0][0]["scale"].astype(np.float64))
    n_small = (s < 0.06).sum(1)
    assert (n_small == 0).any() and (n_small == 1).any() and (n_small == 2).any()
    assert (np.abs(s / 0.06 - 1.0) > 0.1).all() and (np.abs(s / (0.02 * s.max(1, keepdims=True)) - 1.0) > 0.1).all()
    plain = tc.restate_with(dict(case, frame={}), [(np_trace.prepare_set(a), M) for a, M in case["sets"]])
    assert np.abs(r["t_normal_thin"]["normal"] - plain["normal"]).max() > 0.05
    assert np.abs(r["t_normal_thin_iso"]["normal"] - r["t_normal_thin"]["normal"]).max() > 0.05
    assert np.array_equal(r["t_normal_thin"]["image"], plain["image"])


def test_axis_parallel_rays_have_exact_zero_components():
    """q_axis_rays: column 16 has d.x == 0 and row 12 has d.y == 0 exactly (1 / d is infinite in the slab test), and the frame has a
    partial 8-pixel tile on both axes"""
    case = tc.cases()["q_axis_rays"]
    assert case["W"] % 8 and case["H"] % 8
    _, D, ok = np_trace.rays(case["V"], case["P"], case["W"], case["H"])
    assert ok.all() and (D[:, 16, 0] == 0.0).all() and (D[12, :, 1] == 0.0).all()
    assert (D[:, 15, 0] != 0.0).all() and (D[11, :, 1] != 0.0).all()
    r = tc.restate("q_axis_rays")
    assert r["hits"][:, 16][~r["fragile"][:, 16]].max() > 4 and r["hits"][12][~r["fragile"][12]].max() > 4


def test_exact_ties_are_ordered_by_the_callers_id_and_the_case_can_see_it():
    """s_ties_*: 40 particles are bit-identical copies of 40 others (other colour, other opacity) at distant caller indices.  The
    pair's order is (t, caller's global id); a pixel with such a pair is not fragile on its account; ordering the pair the other way
    round changes such a pixel's colour by more than 1e-3 and the picked id on 237 pixels.  A device that ordered them otherwise
    would fail test_gpu_trace.py on the picked ids of the non-fragile pixels (where a pair straddles the pick), on the 2e-3 bound of
    the integrated normal and, if the colours move enough, on the frame's 50 dB PSNR; there is no per-pixel bound on the image."""
    case = tc.cases()["s_ties_18"]
    sets = [(np_trace.prepare_set(a), M) for a, M in case["sets"]]
    ps = sets[0][0]
    assert np.array_equal(ps["shape"][300:], ps["shape"][:40]) and len(set(ps["shape"][:300])) == 300
    r = tc.restate("s_ties_18")
    seen = r["tie_pair"] & ~r["fragile"]
    assert seen.sum() > 20
    swapped = tc.restate_with(case, sets, reverse_ties=True)
    seen &= ~swapped["fragile"]
    diff = np.abs(swapped["image"] - r["image"])[..., :3].max(-1)
    print(f"s_ties_18: {int(seen.sum())} non-fragile pixels walk a duplicate pair; swapping the tie order moves them by up to {diff[seen].max():.3e}, "
          f"the picked id on {(swapped['id'] != r['id'])[seen].sum()} of them")
    assert (diff[seen] > 1e-3).any() and (swapped["id"] != r["id"])[seen].any()
    # fewer slots: pairs straddle pass boundaries; the copy of a hit that ended a pass is never a hit (t > tMin + epsT fails)
    r4 = tc.restate("s_ties_04")
    assert (r4["tie_pair"] & ~r4["fragile"]).any()
    ok = ~(r["fragile"] | r4["fragile"])
    assert (r4["hits"][ok] != r["hits"][ok]).any()
    # the copy of the hit in the last slot of a pass is lost, so the frame depends on K: running 32 samples per pass through a
    # smaller K-buffer shows here
    r32 = tc.restate("s_ties_32")
    ok = ~(r["fragile"] | r32["fragile"])
    assert (r32["hits"][ok] != r["hits"][ok]).any()
    r1 = tc.restate("s_ties_01")
    assert not r1["tie_pair"].any()          # at K = 1 the second copy is never a hit
    picked = r1["id"][~r1["fragile"]]
    assert not ((picked >= 300) & (picked != np_trace.INVALID)).any() and (picked < 40).any()


def test_declared_ties_of_different_particles_show_the_order_by_callers_id():
    """q_axis_ring_ties: eight DIFFERENT particles (identity quaternion, one centre z, one log-scale z) have bit-identical t on the
    central ray, whose direction is (0, 0, -1) exactly; they are listed in the reverse of their Morton order, so an order by storage
    id is the reverse of the order by the caller's id.  K = 5 is below the group's size: the K-th cut decides WHICH five are hits."""
    case = tc.cases()["q_axis_ring_ties"]
    a = case["sets"][0][0]
    g = np.arange(tc.RING)
    assert (a["rotation"][g] == (1, 0, 0, 0)).all() and len(set(a["positions"][g, 2])) == 1 and len(set(a["scale"][g, 2])) == 1
    assert len(set(a["positions"][g, 0])) == tc.RING and len(set(a["positions"][g, 1])) == tc.RING
    assert np.array_equal(case["sets"][0][1], tc.I4) and case["trace"]["samples_per_pass"] < tc.RING
    _, D, _ = np_trace.rays(case["V"], case["P"], case["W"], case["H"])
    assert tuple(D[12, 16]) == (0.0, 0.0, -1.0)
    r = tc.restate("q_axis_ring_ties")
    assert not r["fragile"][12, 16] and r["tie_pair"][12, 16] and r["candidates"][12, 16] == tc.RING
    assert r["hits"][12, 16] == 5 and r["id"][12, 16] < 5          # five of the eight are hits: the five lowest caller's ids
    sets = [(np_trace.prepare_set(a), tc.I4)]
    swapped = tc.restate_with(case, sets, reverse_ties=True)
    assert not swapped["fragile"][12, 16] and swapped["hits"][12, 16] == 5
    d_img = np.abs(swapped["image"][12, 16] - r["image"][12, 16]).max()
    d_nrm = np.abs(swapped["normal"][12, 16] - r["normal"][12, 16]).max()
    print(f"q_axis_ring_ties centre pixel: id {r['id'][12, 16]} -> {swapped['id'][12, 16]} with the tie order reversed, colour moves by {d_img:.3e}, "
          f"normal by {d_nrm:.3e}")
    assert swapped["id"][12, 16] != r["id"][12, 16] and swapped["id"][12, 16] >= 3 and d_img > 1e-2 and d_nrm > 2e-3
    # without the declaration the pixel is set aside, as every accidental tie is
    assert tc.restate_with(case, sets, exact_ties=())["fragile"][12, 16]


def test_quantised_sets_enter_the_restatement_as_the_device_holds_them():
    a = tc.cloud(50, 77, sh_coeffs=8)
    plain = np_trace.prepare_set(a)
    sh = np.round(plain["sh"] * 127.5) / 127.5
    rgba = np.round(plain["rgba"] * 255.0) / 255.0
    q = np_trace.prepare_set(a, rgba=rgba, sh=sh)
    assert np.array_equal(q["sh"], sh.astype(np.float32).astype(np.float64)) and np.array_equal(q["rgba"], rgba.astype(np.float32).astype(np.float64))
    assert q["degree"] == 2 and not q["sh"][:, 8:].any() and np.array_equal(q["pos"], plain["pos"])


def test_pass_walk_equals_one_sorted_walk_when_k_is_large():
    """with K larger than any ray's hit count the passes reduce to one sorted walk (non-fragile pixels)"""
    name = "e_leaves_64"
    case = dict(tc.cases()[name])
    sets = [(np_trace.prepare_set(a), M) for a, M in case["sets"]]
    one = tc.restate_with(case, sets, single_sorted_walk=True)
    assert one["candidates"].max() <= 64
    case["trace"] = dict(samples_per_pass=64)
    multi = tc.restate_with(case, sets)
    ok = ~(one["fragile"] | multi["fragile"])
    assert ok.mean() > 0.9
    assert np.array_equal(one["hits"][ok], multi["hits"][ok]) and np.array_equal(one["id"][ok], multi["id"][ok])
    assert np.abs(one["image"][ok] - multi["image"][ok]).max() <= 1e-14


def test_single_splat_alpha_equals_the_3dgut_response():
    """a single splat's alpha along the central ray == gut_opacity of tests/np_reference.py for the same ray and particle"""
    W = H = 33  # odd: pixel (16, 16) holds the central ray; np_reference generates the ray of SV_Position + 0.5, i.e. pixel + 1
    rng = np.random.Generator(np.random.PCG64(5))
    for trial in range(8):
        a = tc.cloud(1, 100 + trial, half=0.05, log_scale=-1.2)
        a["opacity"][:] = 1.0
        M = tc.trs((1.0, 1.0, 1.0), rng.standard_normal(3), 30.0 * trial, (0.02 * trial, 0.0, 0.0))
        V, P = tc.lookat((0.1, 0.2, 2.0), (0, 0, 0)), tc.persp(50.0, 1.0)
        ps = np_trace.prepare_set(a)
        r = np_trace.trace([(ps, M)], V, P, W, H, kernel_min_response=0.0113, alpha_cull=1.0 / 255.0)
        # the same particle: the restatement holds exp(scale) as the device's fp32 exponential, np_reference exponentiates in double
        g = npr.gut_project(a["positions"], np.log(ps["s"]), a["rotation"], ps["rgba"], M, V, P, W, H)
        # np_reference's fragment ray: inuv = ((px + 0.5) + 0.5) / size; the traced ray: (px + 0.5) / size
        want = npr.gut_opacity(g, 0, float(ps["rgba"][0, 3]), M, V, P, W, H, 16 - 0.5, 16 - 0.5)
        got = r["image"][16, 16, 3]
        assert want is not None and r["hits"][16, 16] == 1
        assert abs(got - want) <= 1e-12, (trial, got, want)


def test_argument_validation_needs_no_device():
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    p = capi.default_params(64, 48)

    def call(params, trace):
        return lib.mgs_render_traced(None, C.byref(params), C.byref(trace) if trace is not None else None, None)

    # valid parameters reach the handle check
    assert call(p, capi.default_trace_params()) == -1 and b"null scene" in lib.mgs_last_error()
    assert call(p, None) == -1 and b"null scene" in lib.mgs_last_error()
    assert lib.mgs_render_traced(None, None, None, None) == -1
    for bad in (dict(samples_per_pass=0), dict(samples_per_pass=33), dict(max_passes=0), dict(min_transmittance=1.0),
                dict(min_transmittance=-0.1), dict(kernel_adaptive_clamping=2), dict(depth_iso_threshold=1.5)):
        assert call(p, capi.default_trace_params(**bad)) == -1, bad
        assert b"null scene" not in lib.mgs_last_error(), bad
    for field, value, code in (("kernel_degree", 6, -1), ("kernel_min_response", 0.0, -1), ("camera_model", 2, -1), ("width", 0, -1),
                               ("target_format", 3, -1), ("normal_method", 2, -1), ("lighting_mode", 1, -8), ("sort_mode", 3, -8)):
        q = capi.default_params(64, 48)
        setattr(q, field, value)
        assert call(q, None) == code, field
        assert b"null scene" not in lib.mgs_last_error(), field
    assert lib.mgs_trace_download_hit_counts(None, None, 0) == -1
