"""CPU tests of the sensor models (mgs_frame_set_sensor, MGS_HAS_SENSOR_MODEL): what the header and the library declare, every outcome
that needs no device, and the premises of the cases of tests/gut_sensor_cases.py from the float64 restatement tests/np_gut_sensor.py
alone — the inverse's round trip, the identity sensor against np_gut.project, the fragile caps, the branches each sensor exists for and
the float32 run of the restatement that the GPU tests' bars come from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from vk_gaussian_splatting_amd import capi
import gut_cases as gc
import gut_sensor_cases as sc
import np_gut
import np_gut_sensor as ns

INVALID_ARG, UNSUPPORTED = -1, -8


def header():
    return open(os.path.join(ROOT, "include", "mgs.h")).read()


def test_header_declares_the_sensor_model():
    hdr = header()
    assert re.search(r"#define\s+MGS_HAS_SENSOR_MODEL\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr) and re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_SENSOR_OPENCV_PINHOLE\s+0\b", hdr) and re.search(r"#define\s+MGS_SENSOR_OPENCV_FISHEYE\s+1\b", hdr)
    assert re.search(r"int\s+mgs_sensor_model_from_frame\(const MgsFrameParams\*", hdr) and re.search(r"int\s+mgs_frame_set_sensor\(MgsScene", hdr)
    body = hdr[hdr.index("(MGS_HAS_SENSOR_MODEL):"):hdr.index("typedef struct MgsSensorModel")]
    for words in ("PARITY UNPINNED", "threedgut_camera_projections.h.slang:85-186", "threedgut_camera_models.h.slang:25-61", "self-consistent",
                  "mgs_frame_set_sensor(handle, NULL)", "mgs_trace_generate_rays", "MGS_ERR_UNSUPPORTED", "(0.8, 1.2)"):
        assert words in body, words
    # the traced side's scope sentence stays as the other tests read it
    assert "meshes in the traced scene, soft shadows, indirect lighting and bounces" in hdr
    lib = capi.load_library()
    for name in ("mgs_sensor_model_from_frame", "mgs_frame_set_sensor"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert C.sizeof(capi.SensorModel) == 128 and C.sizeof(capi.FrameParams) == 288
    assert callable(capi.Scene.set_sensor)


@pytest.mark.parametrize("fisheye", [False, True])
def test_model_from_frame_is_the_frames_perfect_camera(fisheye):
    name = "identity_fisheye" if fisheye else "identity_pinhole"
    c = sc.case(name)
    V, P, eye = c["cam"]
    p = capi.default_params(c["W"], c["H"])
    capi.set_camera(p, V, P, eye)
    p.camera_model = 1 if fisheye else 0
    m = capi.sensor_model_from_frame(p)
    want = c["sensor"]
    assert (m.model, m.shutter) == (1 if fisheye else 0, 0) and not any(m.reserved)
    assert np.allclose(list(m.focal_length), want["focal_length"], rtol=1e-6) and list(m.principal_point) == [c["W"] / 2, c["H"] / 2]
    assert m.focal_length[1] < 0 if fisheye else m.focal_length[1] * P[1][1] > 0   # y follows proj[5]
    assert abs(m.max_angle - want["max_angle"]) <= 1e-6 * want["max_angle"]
    assert not any(list(m.radial) + list(m.tangential) + list(m.thin_prism) + list(m.fisheye_radial))
    lib = capi.load_library()
    assert lib.mgs_sensor_model_from_frame(None, C.byref(m)) == INVALID_ARG and lib.mgs_sensor_model_from_frame(C.byref(p), None) == INVALID_ARG


def test_ranges_are_checked_before_the_handle():
    lib = capi.load_library()
    err = lambda: lib.mgs_last_error().decode()   # noqa: E731
    p = capi.default_params(64, 48)
    good = capi.sensor_model_from_frame(p)

    def outcome(**fields):
        m = capi.SensorModel.from_buffer_copy(bytes(good))
        for k, v in fields.items():
            if k == "reserved":
                m.reserved[3] = v
            else:
                m.update(**{k: v})
        return lib.mgs_frame_set_sensor(None, C.byref(m)), err()

    for bad in (dict(model=2), dict(model=-1), dict(shutter=5), dict(shutter=-1), dict(focal_length=[0.0, 10.0]), dict(focal_length=[10.0, float("nan")]),
                dict(radial=[0, 0, float("inf"), 0, 0, 0]), dict(max_angle=-0.5), dict(thin_prism=[0, float("nan"), 0, 0]), dict(reserved=1)):
        rc, msg = outcome(**bad)
        assert rc == INVALID_ARG and "null scene" not in msg and "mgs_frame_set_sensor" in msg, (bad, rc, msg)
    for rolling in (1, 2, 3, 4):
        rc, msg = outcome(shutter=rolling)
        assert rc == UNSUPPORTED and "null scene" not in msg and "rolling" in msg
    # a model in range reaches the handle; so does unbinding
    rc, msg = outcome()
    assert rc == INVALID_ARG and "null scene" in msg
    assert lib.mgs_frame_set_sensor(None, None) == INVALID_ARG and "null scene" in err()


@pytest.mark.parametrize("name", sc.CASES)
def test_round_trip_of_the_inverse(name):
    """project(unproject(pixel centre)) within 1e-9 px on every pixel that has a ray; the directions are valid for the forward map"""
    c = sc.case(name)
    d, ok, edge, _ = sc.rays(name)
    px, valid = ns.forward_pixels(c["sensor"], d, c["W"], c["H"])
    yy, xx = np.mgrid[0:c["H"], 0:c["W"]]
    err = np.where(ok, np.maximum(np.abs(px[..., 0] - xx - 0.5), np.abs(px[..., 1] - yy - 0.5)), 0.0)
    print(f"{name}: {int(ok.sum())} of {ok.size} pixels have a ray, round trip {err.max():.2e} px")
    assert err.max() <= 1e-9 and valid[ok].all()


@pytest.mark.parametrize("name", ["identity_pinhole", "identity_fisheye"])
def test_identity_sensor_reproduces_the_perfect_camera(name):
    c = sc.case(name)
    V, P, _ = c["cam"]
    st = {k: v for k, v in c["st"].items() if k != "sensor"}
    for (arrays, m), pr in zip(c["sets"], sc.projected(name)):
        want = np_gut.project(arrays, m, V, P, c["W"], c["H"], st, sc.DELTA)
        for k in ("cx", "cy", "cov", "sigma", "emits", "reason", "n_valid"):
            assert np.array_equal(pr[k], want[k]), k


@pytest.mark.parametrize("name", sc.CASES)
def test_fragile_shares_stay_within_the_caps(name):
    prs = sc.projected(name)
    emits, fragile = gc.stack(prs, "emits"), gc.stack(prs, "fragile")
    lo, hi, gfragile = sc.reference_blend(name)
    ref = sc.reference_fragments(name)
    print(f"{name}: {int(emits.sum())} emitted, fragile {fragile[emits].mean():.4f}; blend fragile {gfragile.mean():.4f}; borderline pixels {ref.borderline.mean():.4f}")
    assert emits.sum() >= 200 and fragile[emits].mean() <= gc.FRAGILE_CAP
    assert gfragile.mean() <= gc.GAUSS_FRAGILE_CAP
    assert ref.borderline.mean() <= gc.BORDERLINE_CAP["default"]


def test_each_sensor_reaches_the_branch_it_exists_for():
    # strong: sigma points of emitted particles take the clipped fallback while the particle's mean does not; pixels without a ray
    pr = sc.projected("strong")[0]
    log = pr["sensor_log"]
    others = np.zeros(pr["emits"].size, bool)
    for slot in log[1:7]:
        others |= slot["fallback"]
    assert int((others & log[0]["ok"] & pr["emits"]).sum()) >= 5
    _, ok, edge, _ = sc.rays("strong")
    assert 0.05 < (~ok).mean() < 0.5 and ok[sc.H_PIN // 2, sc.W_PIN // 2] and not ok[0, 0]
    # mild: every coefficient is non-zero, the principal point is off centre, and the picture is not the identity's
    sn = sc.case("mild")["sensor"]
    assert all(np.all(sn[k] != 0) for k in ("radial", "tangential", "thin_prism"))
    assert np.all(np.abs(sn["principal_point"] - np.array([sc.W_PIN, sc.H_PIN]) / 2) >= 0.099 * np.array([sc.W_PIN, sc.H_PIN]))
    a, b = sc.projected("mild")[0], sc.projected("identity_pinhole")[0]
    assert np.abs(a["cx"] - b["cx"])[a["emits"] & b["emits"]].max() > 5.0
    # ocv_fisheye: the max_angle clamp is taken by sigma points, and cuts the corners (not the edges' midpoints) off the image
    pf = sc.projected("ocv_fisheye")[0]
    assert np.all(sc.case("ocv_fisheye")["sensor"]["fisheye_radial"] != 0)
    assert sum(int((~slot["ok"]).sum()) for slot in pf["sensor_log"][:7]) > 100
    _, okf, _, _ = sc.rays("ocv_fisheye")
    assert not okf[0, 0] and not okf[-1, -1] and okf[sc.H_FISH // 2, 1] and okf[1, sc.W_FISH // 2] and 0.02 < (~okf).mean() < 0.2
    # the identity sensors give every pixel a ray (the fisheye's image circle reaches the corners: computeMaxAngle)
    assert sc.rays("identity_pinhole")[1].all() and sc.rays("identity_fisheye")[1].all()


@pytest.mark.parametrize("name", sc.CASES)
def test_float32_run_of_the_restatement(name):
    """MEASURES what gut_sensor_cases.GAUSS_DEV and RAY_RESIDUAL record: the whole restatement in numpy float32 (front end, sensor, rays,
    response, blend) against its float64 run, under the float64 run's fragile mask alone, which is the mask the GPU test applies.  The
    has-ray sets of the two runs agree outside the fragile mask."""
    lo, hi, fragile = sc.reference_blend(name)
    lo32, hi32, _ = sc.float32_blend(name)
    assert lo32.dtype == np.float32 and all(pr[k].dtype == np.float32 for pr in sc.projected(name, "float32") for k in ("cx", "cov", "q1", "B", "ro", "opacity"))
    d = max(gc.interval_distance(lo32.astype(np.float64), lo, hi, fragile), gc.interval_distance(hi32.astype(np.float64), lo, hi, fragile))
    _, ok, edge, _ = sc.rays(name)
    _, ok32, _, _ = sc.rays(name, "float32")
    sure = edge > sc.DELTA
    assert not ((ok != ok32) & sure).any()
    res = float(np.where(ok & ok32 & sure, sc.ray_residual(name, sc.world_rays(name, "float32")), 0.0).max())
    print(f"{name}: float32 blend {d:.2e} from the float64 interval (recorded {sc.GAUSS_DEV[name]:.1e}); float32 ray residual {res:.2e} px "
          f"(recorded {sc.RAY_RESIDUAL[name]:.1e})")
    assert d <= sc.GAUSS_DEV[name] and res <= sc.RAY_RESIDUAL[name]
    assert d >= 0.25 * sc.GAUSS_DEV[name] and res >= 0.25 * sc.RAY_RESIDUAL[name], "the recorded figure is stale"
