"""The stochastic trace strategies without a device: header and binding, the argument checks that run before the handle is looked at,
and the float64 restatement's own consistency (np_trace_stochastic.py): its outcome distributions have the expectation of the trusted
strategy-0 restatement (np_trace.py), its fragile pixels stay rare, its own samples meet the statistical bounds the GPU test holds the
device to, and the cases reach every branch they are there for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_trace
import np_trace_stochastic as nts
import trace_cases as tc
import trace_stochastic_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WITH_SETS = [n for n in sorted(sc.cases()) if sc.cases()[n]["sets"]]
PLAIN = [n for n in WITH_SETS if n not in ("g_ties", "h_ring")]   # the cases of the per-pixel comparison of strategy 1


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define\s+MGS_HAS_TRACE_STRATEGIES\s+1\b", hdr)
    for name, v in (("FULL_ANYHIT", 0), ("PASS_STOCHASTIC", 1), ("STOCHASTIC_ANYHIT", 2)):
        assert re.search(r"MGS_TRACE_STRATEGY_%s\s*=\s*%d\b" % (name, v), hdr), name
    assert re.search(r"int32_t\s+trace_strategy;", hdr) and re.search(r"uint32_t\s+reserved\[2\];\s*\n\}\s*MgsTraceParams;", hdr)
    assert "the stochastic trace\n * strategies" not in hdr and "meshes in the traced scene, soft shadows, indirect lighting and bounces" in hdr
    from vk_gaussian_splatting_amd import capi
    assert (capi.TRACE_STRATEGY_FULL_ANYHIT, capi.TRACE_STRATEGY_PASS_STOCHASTIC, capi.TRACE_STRATEGY_STOCHASTIC_ANYHIT) == (0, 1, 2)
    assert C.sizeof(capi.TraceParams) == 32 and capi.TraceParams.trace_strategy.offset == 20
    assert capi.default_trace_params().trace_strategy == 0


def test_strategy_validation_needs_no_device():
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    p = capi.default_params(64, 48)
    for bad in (3, -1):
        t = capi.default_trace_params(trace_strategy=bad)
        assert lib.mgs_render_traced(None, C.byref(p), C.byref(t), None) == -1 and b"null scene" not in lib.mgs_last_error(), bad
    for s in (0, 1, 2):
        t = capi.default_trace_params(trace_strategy=s)
        assert lib.mgs_render_traced(None, C.byref(p), C.byref(t), None) == -1 and b"null scene" in lib.mgs_last_error(), s
    lit = capi.default_params(64, 48)
    lit.lighting_mode = 1
    for s in (1, 2):
        t = capi.default_trace_params(trace_strategy=s)
        assert lib.mgs_render_traced_lit(None, C.byref(lit), C.byref(t), None, None, None) == -8 and b"null scene" not in lib.mgs_last_error(), s
        assert lib.mgs_render_hybrid(None, C.byref(lit), C.byref(t), None, None, None) == -8 and b"null scene" not in lib.mgs_last_error(), s
    t = capi.default_trace_params()
    assert lib.mgs_render_traced_lit(None, C.byref(lit), C.byref(t), None, None, None) == -1 and b"null scene" in lib.mgs_last_error()
    assert lib.mgs_render_hybrid(None, C.byref(lit), C.byref(t), None, None, None) == -1 and b"null scene" in lib.mgs_last_error()


def _strategy0(name, **trace):
    case = sc.cases()[name]
    return tc.restate_with(dict(case, trace=dict(case["trace"], **trace)), sc.prepared(case))


@pytest.mark.parametrize("name", PLAIN)   # (the two tie cases disable the Gaussian opacity: T = 0 = min_transmittance is fragile there)
def test_expectation_of_both_strategies_is_the_blend(name):
    """sum of probability x outcome == the strategy-0 restatement at min_transmittance 0: a hit is kept with probability alpha_i
    prod_{j<i} (1 - alpha_j), a pass with probability opacity_k prod_{j<k} (1 - opacity_j), and those are the blend weights"""
    R = sc.ray_hits(name)
    one_pass = _strategy0(name, min_transmittance=0.0, samples_per_pass=10 ** 6, max_passes=10 ** 6)
    ok = ~(R["fragile"] | one_pass["fragile"])
    assert ok.mean() > 0.9
    assert max(len(h) for row in R["hits"] for h in row) == one_pass["candidates"].max() > 0
    mu_any = nts.moments(nts.anyhit_distribution(R))[0]
    mu_one = nts.moments(nts.pass_distribution(R, samples_per_pass=10 ** 6, max_passes=10 ** 6))[0]
    assert np.abs(mu_any - one_pass["image"])[ok].max() <= 1e-12
    assert np.abs(mu_one - one_pass["image"])[ok].max() <= 1e-12
    four = _strategy0(name, min_transmittance=0.0, samples_per_pass=4, max_passes=10 ** 6)
    ok4 = ~(R["fragile"] | four["fragile"])
    mu_four = nts.moments(nts.pass_distribution(R, samples_per_pass=4, max_passes=10 ** 6))[0]
    assert np.abs(mu_four - four["image"])[ok4].max() <= 1e-12
    if name == "a_faint_k04":
        assert (one_pass["candidates"][ok4] > 8).any()  # more than two passes of four on a compared ray


@pytest.mark.parametrize("name", PLAIN)
def test_fragile_pixels_stay_rare(name):
    for sid in sc.SAMPLE_IDS:
        r = sc.pass_sample(name, sid)
        print(f"{name} sample {sid}: fragile {r['fragile'].mean():.4f}, accepted at pass up to {r['accepted_pass'].max()}")
        assert r["fragile"].mean() <= 0.02
        a = nts.anyhit(sc.ray_hits(name), sid)
        assert a["fragile"].mean() <= 0.02


def test_own_samples_meet_the_statistical_bounds():
    """bounds (a) and (b) of the GPU convergence test hold for the restatement's own sampler (fewer samples: the bound follows N)"""
    R, N = sc.ray_hits(sc.STAT_CASE), 96
    case = sc.cases()[sc.STAT_CASE]
    ok = ~R["fragile"]
    for strategy in (1, 2):
        if strategy == 1:
            dist = nts.pass_distribution(R, samples_per_pass=case["trace"]["samples_per_pass"], min_transmittance=0.0)
            mean = np.mean([sc.pass_sample(sc.STAT_CASE, k, min_transmittance=0.0)["image"] for k in range(N)], 0)
        else:
            dist = nts.anyhit_distribution(R)
            mean = np.mean([nts.anyhit(R, k)["image"] for k in range(N)], 0)
        mu, var, rng = nts.moments(dist)
        a, b, ra, rb = nts.bernstein_ok(mean, mu, var, rng, ok, N, slack=0.0)
        print(f"strategy {strategy}: worst |mean - mu| / bound per pixel {ra:.3f}, frame-wide {rb:.3f}")
        assert a and b
        assert var[ok].max() > 1e-3   # there is noise to bound


def test_cases_exercise_what_they_are_for():
    first = later = never = fallback = fallback_rejected = not_nearest = False
    for name in PLAIN:
        R = sc.ray_hits(name)
        ncand = np.array([[len(h) for h in row] for row in R["hits"]])
        for sid in sc.SAMPLE_IDS:
            r = sc.pass_sample(name, sid)
            ok = ~r["fragile"]
            first |= bool((ok & (r["accepted_pass"] == 1)).any())
            later |= bool((ok & (r["accepted_pass"] > 1)).any())
            never |= bool((ok & (r["accepted_pass"] == 0) & (ncand > 0)).any())
            fallback |= bool((ok & r["fallback"]).any())
            fallback_rejected |= bool((ok & r["fallback_rejected"]).any())
            assert set(np.unique(r["image"][..., 3])) <= {0.0, 1.0}
            a = nts.anyhit(R, sid)
            not_nearest |= bool((~a["fragile"] & a["not_nearest"]).any())
    assert first and later and never and fallback and fallback_rejected and not_nearest
    fish = sc.pass_sample("d_fisheye_k04", 0)
    assert (fish["image"][0, 0] == (0, 0, 0, 1)).all()
    # K-buffer sizes 4 / 18 / 32 are all there, and a compared ray has more candidates than four slots
    assert {sc.frame_trace(sc.cases()[n])[1]["samples_per_pass"] for n in PLAIN} >= {4, 18, 32}
    # the duplicate pairs: with the Gaussian opacity disabled the nearest accepted hit of some compared ray is the lower copy of a pair
    g = tc.restate_with(sc.cases()["g_ties"], sc.prepared(sc.cases()["g_ties"]))
    assert ((g["id"] < 40) & ~g["fragile"]).sum() > 5 and not ((g["id"] >= 160) & (g["id"] != np_trace.INVALID) & ~g["fragile"]).any()
    h = tc.restate_with(sc.cases()["h_ring"], sc.prepared(sc.cases()["h_ring"]))
    assert not h["fragile"][12, 16] and h["id"][12, 16] == 0 and h["hits"][12, 16] == 1
