"""Helpers of the occluder tests (tests/test_gpu_occluder.py, tests/test_occluder_cpu.py): depth images made of a few
LEVELS, and the expected frame assembled from the CPU oracle alone.

The oracle has no depth test.  For a depth image that takes a few distinct values L_k on pixel sets S_k the expected
frame is: for each level, the oracle's frame of the sorted stream filtered to the entries with z_i <= L_k (z_i decoded
from the oracle's own depth key), plus transmittance x background, copied on S_k.  Every level must lie in a GAP of the
decoded depths (no splat within MIN_GAP_ULP fp32 steps), so that a last-bit difference in how an implementation rounds
z cannot move a splat across a level."""
import numpy as np

MIN_GAP_ULP = 16


def decode_key(keys):
    """inverse of encodeMinMaxFp32 (dist.comp.slang:33-38): order-preserving u32 -> fp32"""
    k = np.ascontiguousarray(keys, np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return bits.view(np.float32)


def encode_key(values):
    b = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def depths_of_btf_keys(keys):
    """back-to-front keys hold -ndc.z"""
    return -decode_key(keys)


def ulp_distance(a, b):
    """fp32 steps between a and b (finite): the encoded keys are consecutive integers for consecutive floats"""
    return np.abs(encode_key(a).astype(np.int64) - encode_key(b).astype(np.int64))


def assert_levels_in_gaps(z, levels, min_gap=MIN_GAP_ULP):
    """every level has no depth of z within min_gap fp32 steps"""
    z = np.ascontiguousarray(z, np.float32)
    for L in levels:
        if z.size == 0:
            continue
        d = int(ulp_distance(z, np.full(z.shape, L, np.float32)).min())
        assert d > min_gap, f"level {float(L)!r} lies {d} ulp from a splat depth (needs > {min_gap})"


def pick_level(z, quantile, window=200, min_gap=MIN_GAP_ULP):
    """the midpoint of the widest gap between consecutive distinct depths within `window` entries of the quantile"""
    zs = np.unique(np.ascontiguousarray(z, np.float32))
    assert zs.size >= 2, "pick_level: needs two distinct depths"
    c = int(round(quantile * (zs.size - 1)))
    lo, hi = max(0, c - window), min(zs.size - 1, c + window)
    gaps = ulp_distance(zs[lo + 1:hi + 1], zs[lo:hi])
    j = lo + int(np.argmax(gaps))
    L = np.float32((np.float64(zs[j]) + np.float64(zs[j + 1])) * 0.5)
    assert_levels_in_gaps(zs, [L], min_gap)
    return L


def pick_levels(z):
    """0.0 (everything hidden), the gaps nearest the quartiles, 1.0 (nothing hidden) — asserted to be true of z"""
    z = np.ascontiguousarray(z, np.float32)
    assert not (z <= 0.0).any(), "a splat with ndc.z <= 0 would pass level 0.0: choose another pose"
    assert not (z > 1.0).any(), "the dist-stage cull keeps ndc.z <= 1"
    levels = [np.float32(0.0)] + [pick_level(z, q) for q in (0.25, 0.5, 0.75)] + [np.float32(1.0)]
    assert_levels_in_gaps(z, levels)
    return levels


def checkerboard(W, H, levels, bw=37, bh=23):
    """blocks of bw x bh pixels cycling through the levels: aligned with no tile, region or wave boundary"""
    yy, xx = np.mgrid[0:H, 0:W]
    idx = ((xx // bw) + 2 * (yy // bh)) % len(levels)
    return np.asarray(levels, np.float32)[idx]


def diagonal(W, H, near, far):
    """two levels split along the image diagonal"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(xx * H > yy * W, np.float32(near), np.float32(far)).astype(np.float32)


def random_background(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)


def expected_frame(render_btf, render_ftb, order_btf, z, depth, background=None, alpha_sum=False):
    """the frame assembled from the oracle: render_btf(order) -> image in draw order far to near (alpha = sum of alpha),
    render_ftb(order) -> image in draw order near to far (alpha = 1 - T); order_btf / z: the sorted stream far to near and
    its depths; depth: the level image; background: [H,W,4] or None"""
    H, W = depth.shape
    out = np.zeros((H, W, 4), np.float32)
    order_btf = np.ascontiguousarray(order_btf, np.uint32)
    for L in np.unique(depth):
        keep = order_btf[z <= L]
        img = render_btf(keep)
        fimg = render_ftb(keep[::-1].copy())
        T = 1.0 - fimg[..., 3]
        e = np.empty((H, W, 4), np.float32)
        e[..., :3] = img[..., :3]
        e[..., 3] = img[..., 3] if alpha_sum else fimg[..., 3]
        if background is not None:
            e[..., :3] += T[..., None] * background[..., :3]
            if alpha_sum:
                e[..., 3] += background[..., 3]
        m = depth == L
        out[m] = e[m]
    return out
