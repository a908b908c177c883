"""CPU tests of the occluder feature (mgs_frame_set_occluder / mgs_frame_upload_occluder): the C ABI declares and exports
the entry points, the ctypes layer exposes them, and the level-picking helper of the GPU tests does what it says."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import occluder_levels as ol

HEADER = os.path.join(ROOT, "include", "mgs.h")
LIB = os.path.join(ROOT, "vk_gaussian_splatting_amd", "csrc", "libmgs.so")
NEW = ("mgs_frame_set_occluder", "mgs_frame_upload_occluder")


def test_header_declares_and_library_exports_the_occluder_entry_points():
    hdr = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*MgsScene\b" % name, hdr), name
    assert re.search(r"#define\s+MGS_ABI_VERSION\s+5\b", hdr)
    assert "UNPINNED" in hdr.upper()  # the compare operator's parity is stated
    lib = ctypes.CDLL(LIB)  # loads without a GPU
    declared = sorted(set(re.findall(r"\b(mgs_[a-z0-9_]+)\s*\(", hdr)))
    assert set(NEW) <= set(declared)
    for name in declared:  # ... and nothing that was exported went away
        assert hasattr(lib, name), f"{name} declared in mgs.h but not exported by libmgs.so"


def test_null_handle_is_an_error_not_a_crash():
    lib = ctypes.CDLL(LIB)
    for name in NEW:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        assert fn(None, None, None, 4, 4) == -1  # MGS_ERR_INVALID_ARG
    lib.mgs_last_error.restype = ctypes.c_char_p
    assert b"null handle" in lib.mgs_last_error()


def test_capi_exposes_the_occluder_entry_points():
    from vk_gaussian_splatting_amd import capi
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.load_library()
    for name in NEW:
        assert getattr(lib, name).restype is ctypes.c_int
    for method in ("set_occluder", "upload_occluder", "clear_occluder"):
        assert callable(getattr(capi.Scene, method))


def test_key_codec_round_trips_and_orders():
    v = np.array([-3.5, -0.0, 0.0, 1e-30, 0.25, 0.9970989, 1.0, 7.0], np.float32)
    k = ol.encode_key(v)
    assert np.array_equal(ol.decode_key(k).view(np.uint32), v.view(np.uint32))
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(ol.depths_of_btf_keys(ol.encode_key(-v)), v)
    one = np.float32(1.0)
    assert ol.ulp_distance(np.array([one]), np.array([np.nextafter(one, np.float32(2))]))[0] == 1


def test_level_picking_finds_gaps_and_refuses_bad_levels():
    rng = np.random.default_rng(5)
    # depths like the test scene's: dense between 0.9 and 0.997, irregular gaps
    z = (0.9 + 0.097 * rng.random(40000) ** 2).astype(np.float32)
    levels = ol.pick_levels(z)
    assert len(levels) == 5 and levels[0] == 0.0 and levels[-1] == 1.0
    assert all(a < b for a, b in zip(levels, levels[1:]))
    for L, q in zip(levels[1:4], (0.25, 0.5, 0.75)):
        frac = float((z <= L).mean())
        assert abs(frac - q) < 0.02, (q, frac)
        assert int(ol.ulp_distance(z, np.full(z.shape, L, np.float32)).min()) > ol.MIN_GAP_ULP
    # a level on a splat's depth, and one a few steps off it, are refused
    with pytest.raises(AssertionError):
        ol.assert_levels_in_gaps(z, [z[123]])
    near = np.nextafter(np.nextafter(z[77], np.float32(2)), np.float32(2))
    with pytest.raises(AssertionError):
        ol.assert_levels_in_gaps(z, [near])
    # "everything hidden" must be true of the inputs
    with pytest.raises(AssertionError):
        ol.pick_levels(np.concatenate([z, np.array([-0.01], np.float32)]))
    # no gap wide enough: consecutive floats
    dense = np.float32(0.95) + np.arange(2000, dtype=np.float32) * np.float32(2.0 ** -24)
    with pytest.raises(AssertionError):
        ol.pick_level(dense, 0.5)


def test_level_images_and_expected_frame_assembly():
    levels = [np.float32(x) for x in (0.0, 0.3, 0.5, 0.7, 1.0)]
    cb = ol.checkerboard(333, 217, levels)
    assert cb.shape == (217, 333) and cb.dtype == np.float32 and set(np.unique(cb)) == set(levels)
    assert cb[0, 36] != cb[0, 37] and cb[22, 0] != cb[23, 0]
    dg = ol.diagonal(64, 48, 0.25, 1.0)
    assert set(np.unique(dg)) == {np.float32(0.25), np.float32(1.0)}
    # a toy "oracle": each draw-order entry i adds colour i+1 to every pixel with alpha 0.5
    H, W = 4, 6
    order = np.array([2, 0, 1], np.uint32)          # far to near
    z = np.array([0.9, 0.5, 0.1], np.float32)       # depth of each entry of the order

    def btf(o):
        img = np.zeros((H, W, 4), np.float32)
        for i in o:
            img[..., :3] = img[..., :3] * 0.5 + 0.5 * (i + 1)
            img[..., 3] += 0.5
        return img

    def ftb(o):
        img = btf(o[::-1])
        img[..., 3] = 1.0 - 0.5 ** len(o)
        return img
    depth = np.full((H, W), 1.0, np.float32)
    depth[:, :2] = 0.0
    depth[:, 2:4] = 0.3
    bg = np.full((H, W, 4), 8.0, np.float32)
    e = ol.expected_frame(btf, ftb, order, z, depth, bg)
    assert np.allclose(e[0, 0], [8, 8, 8, 0])                                   # everything hidden: the background
    assert np.allclose(e[0, 2], [0.5 * 2 + 0.5 * 8, ] * 3 + [0.5])               # only the nearest entry (id 1)
    assert np.allclose(e[0, 5, 3], 1 - 0.125)
    es = ol.expected_frame(btf, ftb, order, z, depth, bg, alpha_sum=True)
    assert np.allclose(es[0, 5, 3], 1.5 + 8.0) and np.allclose(es[0, 0, 3], 8.0)
