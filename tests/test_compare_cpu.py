"""CPU tests (no GPU) of the image comparison: the header, the exports and the ctypes mirror; the numpy restatement
(np_compare.py) on hand-computed pixels and against the oracle's PSNR; and the bars the GPU test applies, measured from the
restatement alone (float32 against float64, two summation orders)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import compare_cases as cc
import np_compare as npc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs.h")
NEW = ["mgs_compare_capture", "mgs_compare_capture_upload", "mgs_compare_release", "mgs_compare_params_default", "mgs_compare_metrics",
       "mgs_compare_view_default", "mgs_compare_composite", "mgs_compare_download_composite"]


def test_header_declares_the_entry_points_and_keeps_both_abi_numbers():
    hdr = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr)
    assert re.search(r"#define\s+MGS_ABI_MINOR\s+1\b", hdr)
    assert re.search(r"#define\s+MGS_HAS_IMAGE_COMPARE\s+1\b", hdr)
    assert re.search(r"MGS_FLIP_DISABLED\s*=\s*0\s*,\s*MGS_FLIP_APPROX\s*=\s*1\s*,\s*MGS_FLIP_REFERENCE\s*=\s*2", hdr)
    assert "PARITY UNPINNED" in hdr.split("mgs_compare_metrics")[0].split("MgsCompareMetrics;")[-1] or "PARITY UNPINNED" in hdr.split("MgsCompareMetrics;")[1]
    from vk_gaussian_splatting_amd import capi
    lib = ctypes.CDLL(capi.lib_path())
    for name in NEW:
        assert hasattr(lib, name), f"{name} declared in mgs.h but not exported by libmgs.so"


def test_capi_mirrors_the_structures_and_defaults():
    import vk_gaussian_splatting_amd as mgs
    from vk_gaussian_splatting_amd import capi
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS
    assert ctypes.sizeof(capi.CompareParams) == 8 and ctypes.sizeof(capi.CompareMetrics) == 56 and ctypes.sizeof(capi.CompareView) == 24
    lib = capi.load_library()
    p = capi.CompareParams()
    lib.mgs_compare_params_default(ctypes.byref(p))
    assert p.flip_mode == capi.FLIP_REFERENCE == 2 and p.pixels_per_degree == 67.0
    v = capi.CompareView()
    lib.mgs_compare_view_default(ctypes.byref(v))
    assert (v.split_position, v.left, v.right, v.difference_amplify, v.width, v.height) == (0.5, 0, 1, 5.0, 0, 0)
    assert (mgs.FLIP_DISABLED, mgs.FLIP_APPROX, mgs.FLIP_REFERENCE) == (0, 1, 2) and mgs.SHOW_FLIP == 5
    for m in ("compare_capture", "compare_capture_upload", "compare_release", "compare_metrics", "compare_composite"):
        assert callable(getattr(mgs.Scene, m))


def test_null_handle_is_an_error_not_a_crash():
    from vk_gaussian_splatting_amd import capi
    lib = capi.load_library()
    m, v = capi.CompareMetrics(), capi.CompareView()
    img = np.zeros((2, 2, 4), np.float32)
    assert lib.mgs_compare_capture(None) == -1
    assert lib.mgs_compare_capture_upload(None, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2, 2) == -1
    assert lib.mgs_compare_release(None) == -1
    assert lib.mgs_compare_metrics(None, None, ctypes.byref(m)) == -1
    assert lib.mgs_compare_composite(None, ctypes.byref(v), None, None) == -1
    assert lib.mgs_compare_download_composite(None, img.ctypes.data_as(ctypes.c_void_p), img.nbytes) == -1
    assert b"null handle" in lib.mgs_last_error()
    lib.mgs_compare_params_default(None)
    lib.mgs_compare_view_default(None)


# ---- the restatement on hand-computed pixels ---------------------------------------------------------------------------------
def _img(rgb, H=2, W=2):
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rgb
    return a


def test_known_mse_of_a_2x2_pair():
    cap, cur = _img(0.5), _img(0.5)
    cur[0, 0, :3] = (0.75, 0.5, 0.25)  # squared error 0.0625 + 0 + 0.0625 on one of four pixels
    m = npc.metrics(cap, cur, flip_mode=0)
    assert m["mse_exact"] == 0.125 / 12.0
    assert m["mse_fixed"] == int(0.125 / 12.0 * 1e9)  # 10416666: one pixel adds uint(0.125 / 12 * 1e9), the others 0
    assert m["mse"] == np.float32(np.float32(10416666) / np.float32(1e9))
    assert abs(float(m["psnr"]) - 10.0 * math.log10(12.0 / 0.125)) < 1e-4
    same = npc.metrics(cap, cap, flip_mode=1)
    assert same["mse_fixed"] == 0 and same["psnr"] == np.float32(99.99) and same["flip"] == 0.0 and same["psnr_exact"] == math.inf


def test_constant_images_have_no_flip_feature_and_a_border_pixel_has_none_either():
    a = _img((0.2, 0.4, 0.6), 40, 40)
    # ppd 8: radii 8, 4, 2, 2, 2 fit a 40 x 40 image; the normalised mean of a constant is the constant up to rounding
    assert np.abs(npc.spatial_features(a, 8.0, np.float64)).max() < 1e-15
    assert np.abs(npc.sobel_feature(a, np.float64)).max() < 1e-15
    b = a.copy()
    b[20, 20, :3] = 0.9
    f = npc.spatial_features(b, 8.0, np.float64)
    assert f[:, 20, 20].all() and not f[:, 0, :].any() and not f[:, :, 39].any()  # the border returns its own luminance
    sigma, r = npc.sigma_radius(8.0, 0.5)
    assert r == 8 and not f[0, 7, 20] and f[0, 12, 20]  # within r of the border: 0, although the bright pixel is in reach
    assert [npc.sigma_radius(67.0, fr)[1] for fr in npc.FREQS] == [65, 33, 17, 9, 5]
    s = npc.sobel_feature(b, np.float64)
    assert s[20, 21] > 0 and s[20, 20] < 1e-15 and not s[0].any()
    # one pixel by hand: left neighbour of the bright pixel, gx = 2 * (L_bright - L_flat), gy = 0
    lum = lambda c: 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]
    assert abs(s[20, 19] - 2.0 * (lum((0.9,) * 3) - lum((0.2, 0.4, 0.6)))) < 1e-6


def test_composite_divider_and_one_pixel_of_each_mode():
    cap, cur = _img((0.2, 0.4, 0.6), 8, 20), _img((0.3, 0.4, 0.5), 8, 20)
    out = npc.composite(cap, cur, split=0.5, left=0, right=1)
    assert (out[:, 10] == 1).all()  # splitPos = int(0.5 * 20) = 10: white centre
    for x in (8, 9, 11, 12):
        assert (out[:, x] == np.array([0, 0, 0, 1])).all()
    assert np.array_equal(out[:, 7], cap[:, 7].astype(np.float64)) and np.array_equal(out[:, 13], cur[:, 13].astype(np.float64))
    f32 = lambda v: np.float64(np.float32(v))
    d = [abs(f32(0.2) - f32(0.3)), 0.0, abs(f32(0.6) - f32(0.5))]
    raw = npc.composite(cap, cur, left=2, right=2)[3, 3]
    assert np.allclose(raw, [min(5 * d[0], 1), 0, min(5 * d[2], 1), 1], atol=1e-12)
    inten = min((d[0] * 0.299 + d[2] * 0.114) * 5.0, 1.0)
    gray = f32(0.3) * 0.299 + f32(0.4) * 0.587 + f32(0.5) * 0.114
    assert np.allclose(npc.composite(cap, cur, left=3, right=3)[3, 3], [gray + (1 - gray) * inten, gray - gray * inten, gray - gray * inten, 1], atol=1e-12)
    assert np.allclose(npc.composite(cap, cur, left=4, right=4)[3, 3], [inten, 0, 0, 1], atol=1e-12)
    heat = npc.composite(cap, cur, left=5, right=5)[3, 3]
    assert heat[3] == 1 and (heat[:3] != 0).all()
    same = npc.composite(cap, cap, left=5, right=5)[3, 3]  # no error: Turbo at 0
    assert np.allclose(same[:3], [0.13572138, 0.09140261, 0.10667330], atol=1e-12)
    wide = npc.composite(cap, cur, split=0.25, left=0, right=1, width=40, height=16)  # sampled: constant images stay constant
    assert wide.shape == (16, 40, 4) and np.allclose(wide[5, 2], cap[0, 0]) and np.allclose(wide[5, 30], cur[0, 0]) and (wide[:, 10] == 1).all()


def test_mse_and_psnr_equal_the_oracles(ob):
    cap, cur = cc.synthetic_pair("s160")
    m = npc.metrics(cap, cur, flip_mode=0)
    want = float(ob.psnr_rgb(cur, cap))
    assert abs(m["psnr_exact"] - want) <= 1e-9 * want, (m["psnr_exact"], want)


# ---- the bars ------------------------------------------------------------------------------------------------------------------
def test_bars_from_the_reference_alone():
    worst = {"mse": 0.0, "mse_sampled": 0.0, "flip1": 0.0, "flip2": 0.0, "sep": 0.0}
    for name, capsz, cursz, modes in cc.SYNTH_CASES:
        cap, cur = cc.synthetic_pair(name)
        n = cap.shape[0] * cap.shape[1]
        sampled = capsz != cursz
        for key, (rel, u64, same) in cc.measure(cap, cur, modes).items():
            nb = cc.boundary_count(u64, cc.recorded(key, sampled))
            print(f"bars {name} {key}: float32 vs float64 per pixel {rel:.3e}, {nb} boundary pixels of {n}, fixed sums equal: {same}, mean units {u64.mean():.3f}")
            assert nb / n <= cc.MAX_BOUNDARY_SHARE, (name, key, nb)
            assert same or nb > 0, (name, key)  # without a boundary pixel the float32 sums (both orders) equal the float64 sum
            k = "mse_sampled" if (key == "mse" and sampled) else key
            worst[k] = max(worst[k], rel)
            if key == "mse":  # fp16 values: float32 sums equal float64 sums in both orders; at equal sizes no boundary pixel at all
                assert same and (sampled or nb == 0), (name, key, nb)
        if 2 in modes:
            a = npc.flip_reference_powered(cap, cur, cc.PPD, np.float32, 0, npc.blur_2d)
            b = npc.flip_reference_powered(cap, cur, cc.PPD, np.float32, 0, npc.blur_separable)
            worst["sep"] = max(worst["sep"], cc.rel_diff(b, a.astype(np.float64)))
    recorded = {"mse": cc.F32_VS_F64_MSE, "mse_sampled": cc.F32_VS_F64_MSE_SAMPLED, "flip1": cc.F32_VS_F64_FLIP_APPROX,
                "flip2": cc.F32_VS_F64_FLIP_REF, "sep": cc.SEP_VS_2D_FLIP_REF}
    print("bars measured", {k: f"{v:.3e}" for k, v in worst.items()}, "recorded", recorded)
    for k, v in worst.items():
        assert recorded[k] / 2 <= v <= recorded[k], (k, v, recorded[k])


def test_composite_bar_from_the_reference_alone():
    worst = 0.0
    for name in ("s200", "sdiff"):
        cap, cur = cc.synthetic_pair(name)
        for mode in range(6):
            a = npc.composite(cap, cur, 0.4, mode, mode, 5.0, 0, 0, np.float64)
            b = npc.composite(cap, cur, 0.4, mode, mode, 5.0, 0, 0, np.float32)
            worst = max(worst, float(np.abs(a - b).max()))
    print(f"composite float32 vs float64: {worst:.3e} (recorded {cc.F32_VS_F64_COMPOSITE:.1e})")
    assert cc.F32_VS_F64_COMPOSITE / 2 <= worst <= cc.F32_VS_F64_COMPOSITE
