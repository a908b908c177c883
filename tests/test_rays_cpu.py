"""Ray queries (mgs_trace_rays) without a device: header, exports and binding, the argument checks that run before the handle is
looked at, and the float64 restatement for arbitrary rays (np_trace_rays.py) against the trusted restatement of the frames
(np_trace.py) and on the batch the GPU test uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_trace
import np_trace_rays
import ray_cases as rc
import trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_binding():
    hdr = open(os.path.join(ROOT, "include", "mgs.h")).read()
    assert re.search(r"#define\s+MGS_HAS_RAY_QUERY\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr) and re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    for name in ("mgs_trace_rays", "mgs_trace_rays_device", "mgs_trace_generate_rays", "mgs_ray_query_params_default"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(capi.Ray) == 32 and C.sizeof(capi.RayResult) == 48 and C.sizeof(capi.RayQueryParams) == 16
    assert C.sizeof(capi.RayQueryOut) == C.sizeof(capi.TraceOut) + 16
    assert capi.RAY_DTYPE.itemsize == 32 and capi.RAY_RESULT_DTYPE.itemsize == 48
    assert [capi.RAY_RESULT_DTYPE.fields[k][1] for k in ("transmittance", "t_iso", "id", "hit_count", "passes", "normal")] == [12, 16, 20, 24, 28, 32]
    assert (capi.RayResult.transmittance.offset, capi.RayResult.id.offset, capi.RayResult.normal.offset) == (12, 20, 32)
    q = capi.RayQueryParams(reorder=7)
    lib.mgs_ray_query_params_default(C.byref(q))
    assert q.reorder == 0
    # the scope text the other traced entry points pin stays word for word
    assert "meshes in the traced scene, soft shadows, indirect lighting and bounces" in hdr


def _call(lib, fn, p, t=None, q=None, rays=True, count=4):
    from vk_gaussian_splatting_amd import capi
    r = np.zeros(4, capi.RAY_DTYPE)
    res = np.zeros(4, capi.RAY_RESULT_DTYPE)
    rc_ = fn(None, r.ctypes.data_as(C.c_void_p) if rays else None, count, C.byref(p), C.byref(t) if t is not None else None,
             C.byref(q) if q is not None else None, res.ctypes.data_as(C.c_void_p), None)
    return rc_, lib.mgs_last_error()


@pytest.mark.parametrize("entry", ["mgs_trace_rays", "mgs_trace_rays_device"])
def test_argument_errors_need_no_device(entry):
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    fn = getattr(lib, entry)

    def params(**over):
        p = capi.default_params(64, 48)
        for k, v in over.items():
            setattr(p, k, v)
        return p

    range_errors = [dict(p=params(kernel_min_response=0.0)), dict(p=params(), t=capi.default_trace_params(samples_per_pass=0)),
                    dict(p=params(), t=capi.default_trace_params(samples_per_pass=33)), dict(p=params(), q=capi.RayQueryParams(reorder=2)),
                    dict(p=params(), rays=False)]
    for kw in range_errors:
        code, msg = _call(lib, fn, **kw)
        assert code == -1 and b"null scene" not in msg, (kw, msg)
    unsupported = [dict(p=params(), t=capi.default_trace_params(trace_strategy=1)), dict(p=params(), t=capi.default_trace_params(trace_strategy=2)),
                   dict(p=params(lighting_mode=1)), dict(p=params(sort_mode=capi.SORT_STOCHASTIC))]
    for kw in unsupported:
        code, msg = _call(lib, fn, **kw)
        assert code == -8 and b"null scene" not in msg, (kw, msg)
    # the camera, the frame size, the strip rows, the lens and the target are not range-checked: only the handle is missing
    free = params(width=0, height=-3, strip_row_begin=9, strip_row_end=2, camera_model=7, dof_mode=5, target_format=9, frame_sample_id=-1)
    free.view[0] = float("nan")
    code, msg = _call(lib, fn, free)
    assert code == -1 and b"null scene" in msg, msg
    # count == 0 with NULL arrays passes the checks as well
    code, msg = _call(lib, fn, params(), rays=False, count=0)
    assert code == -1 and b"null scene" in msg, msg
    # mgs_trace_generate_rays checks *params as mgs_render_traced does, before the handle
    assert lib.mgs_trace_generate_rays(None, C.byref(params(width=0)), None) == -1 and b"null scene" not in lib.mgs_last_error()
    assert lib.mgs_trace_generate_rays(None, C.byref(params(lighting_mode=1)), None) == -8


@pytest.mark.parametrize("name", ["b_inside", "c_two_instances"])
def test_restatement_reproduces_the_frames_restatement(name):
    """O, D from np_trace.rays and the primary rays' window, one image row per chunk: both are float64 restatements of the same
    arithmetic, so image, hits, ids, normals and the fragile mask are EQUAL"""
    case = tc.cases()[name]
    ref = tc.restate(name)
    W, H = case["W"], case["H"]
    O, D, ok = np_trace.rays(case["V"], case["P"], W, H)
    assert ok.all()
    t = dict(tc.TRACE_DEFAULTS, **case["trace"])
    got = np_trace_rays.trace_rays([(np_trace.prepare_set(a), M) for a, M in case["sets"]], O.reshape(-1, 3), D.reshape(-1, 3),
                                   np_trace.T_MIN, np_trace.T_MAX, samples_per_pass=t["samples_per_pass"], max_passes=t["max_passes"], chunk=W)
    assert np.array_equal(got["radiance"].reshape(H, W, 3), ref["image"][..., :3])
    assert np.array_equal(1.0 - got["transmittance"].reshape(H, W), ref["image"][..., 3])
    assert np.array_equal(got["hits"].reshape(H, W), ref["hits"]) and ref["hits"].max() > 3
    assert np.array_equal(got["id"].reshape(H, W), ref["id"]) and (ref["id"] != np_trace.INVALID).any()
    assert np.array_equal(got["normal"].reshape(H, W, 4), ref["normal"])
    assert np.array_equal(got["fragile"].reshape(H, W), ref["fragile"])
    assert np.array_equal(got["candidates"].reshape(H, W), ref["candidates"])
    assert got["valid"].all() and (got["passes"] >= 1).all()


def test_the_batch_of_the_gpu_test():
    """the fragile share of the restatement alone stays within the cap of the frames' cases (test_trace_cpu.py: 0.02), and the batch
    holds what it is there for: rays that hit, rays that miss, windows that cut hits away, non-unit and axis-parallel directions,
    several passes, invalid rays"""
    O, D, tmin, tmax = rc.batch()
    r = rc.restate()
    frac = float(r["fragile"].mean())
    print(f"ray batch: fragile {frac:.4f}, {int((r['hits'] > 0).sum())} rays with a hit, passes up to {r['passes'].max()}, "
          f"candidates up to {r['candidates'].max()}")
    assert frac <= 0.02
    assert sorted(np.nonzero(~r["valid"])[0].tolist()) == sorted(rc.INVALID_AT)
    bad = ~r["valid"]
    assert not r["radiance"][bad].any() and (r["transmittance"][bad] == 1.0).all() and not r["passes"][bad].any() and not r["hits"][bad].any()
    assert (r["hits"] > 0).sum() > 1500 and ((r["hits"] == 0) & r["valid"]).sum() > 300 and r["passes"].max() >= 3
    length = np.linalg.norm(D.astype(np.float64), axis=1)
    for want in (0.5, 3.0):
        assert ((np.abs(length - want) < 1e-3) & (r["hits"] > 0)).sum() > 100
    axis = ((D == 0).sum(1) == 2) & r["valid"]
    assert (axis & (r["hits"] > 0)).sum() > 50
    # a picked hit lies inside its ray's window
    picked = r["id"] != np_trace.INVALID
    assert picked.sum() > 1000
    assert (r["t_iso"][picked] > np.maximum(tmin, 0)[picked]).all() and (r["t_iso"][picked] < tmax[picked] + 1e-6).all()
    # the windows matter: the same rays with the primary window have more candidates (not always more accepted hits: a ray that
    # skips the near half of the scene keeps its transmittance for the far half)
    full = np_trace_rays.trace_rays(rc.prepared(), O[:400], D[:400], 0.001, 10000.0)
    cut = ((tmin[:400] > 0.001) | (tmax[:400] < 10000.0)) & r["valid"][:400]
    assert (full["candidates"][cut] >= r["candidates"][:400][cut]).all()
    assert (full["candidates"][cut] > r["candidates"][:400][cut]).sum() > 30


def test_scaling_a_direction_scales_t_and_nothing_else():
    """the property the header states: the ray is used as given, t is the parameter along the given direction"""
    O, D, tmin, tmax = (a[:256].astype(np.float64) for a in rc.batch())
    a = np_trace_rays.trace_rays(rc.prepared(), O, D, tmin, tmax)
    b = np_trace_rays.trace_rays(rc.prepared(), O, D * 4.0, tmin / 4.0, tmax / 4.0)
    ok = a["valid"] & ~(a["fragile"] | b["fragile"])
    assert ok.sum() > 200
    assert np.array_equal(a["hits"][ok], b["hits"][ok]) and np.array_equal(a["id"][ok], b["id"][ok])
    assert np.abs(a["radiance"] - b["radiance"])[ok].max() <= 1e-9
    assert np.abs(a["t_iso"] - 4.0 * b["t_iso"])[ok].max() <= 1e-9
