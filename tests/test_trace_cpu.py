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
