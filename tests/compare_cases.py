"""Image pairs and recorded bars of the image-compare tests (test_compare_cpu.py measures and pins the bars without a GPU,
test_gpu_compare.py applies them to the library).

Synthetic pairs: a smooth colour field (a function of the normalised coordinate, so that two sizes show the same picture) against
the same field with noise of bounded magnitude and a step on the right half, both rounded to fp16 values in [0.1, 0.9] as a
RGBA16F frame would hold them.  The noise never comes near zero (|noise| in [0.008, 0.02] per channel, step +0.03), so no pixel's
error is a near-cancellation.

How a bar is made (no number here comes from the library): the float64 restatement (np_compare, shader order) is the reference;
the same restatement in float32, in the shader's order and in the reversed order of every sum, is what another fp32 evaluation of
the same operations may differ by.  F32_VS_F64_* is the largest per-pixel RELATIVE difference |v32 - v64| / v64 of the MSE
contribution and of the FLIP powered error (a pixel whose float64 value is 0 must be 0 in float32 too).  The powered error is a
cube of a sum of absolute differences: where those nearly cancel (the smallest powered errors are 1e-5 of the mean) its relative
difference reaches 1e-3, which is why the FLIP figures are four orders above the MSE's.  A BOUNDARY pixel is one whose float64
contribution in the reference's fixed-point units u = value / N * 1e9 lies within that relative distance, rel * u, of an integer
>= 1: truncation may fall either way there.  A pair has about 2 * rel * sum(u) of them, so zero is out of reach for FLIP however
the case is drawn (s160, approx: 2 * 3.1e-4 * 0.34 * 19200 = 4; found 4); the sdiff pair uses a low-contrast field so that its
features, hence its units, stay small enough for the 1 % condition."""
import numpy as np

import np_compare as npc

PPD = 67.0
SDIFF_CONTRAST = 0.2  # of the field of the different-size pair (see above)

# name, capture (W, H), current (W, H), flip modes measured on it
SYNTH_CASES = [
    ("s160", (160, 120), (160, 120), (0, 1, 2)),
    ("s320", (320, 240), (320, 240), (0, 1, 2)),
    ("s200", (200, 160), (200, 160), (0, 1, 2)),      # wider than 2 * 65 + a few pixels in both axes: every channel has interior pixels
    ("sdiff", (160, 120), (320, 240), (0, 1, 2)),     # the current image has another size: sampler and int(uv * size)
    ("s1080", (1920, 1080), (1920, 1080), (0, 1)),    # MSE and FLIP approx only (the brute-force restatement would take hours)
]

# ---- recorded by test_compare_cpu.py::test_bars_from_the_reference_alone (measured value in the comment, recorded value rounded up)
F32_VS_F64_MSE = 1.25e-7          # measured 1.12e-7 (s1080, equal sizes: the differences of fp16 values are exact, the squares round)
F32_VS_F64_MSE_SAMPLED = 5.0e-6   # measured 3.77e-6 (sdiff: the bilinear weights round before the difference is taken)
F32_VS_F64_FLIP_APPROX = 6.0e-4   # measured 5.69e-4 (s1080; 3.1e-4 .. 4.2e-4 on the small pairs)
F32_VS_F64_FLIP_REF = 5.0e-3      # measured 4.36e-3 (s320)
SEP_VS_2D_FLIP_REF = 5.0e-3       # measured 4.12e-3 (s320): the separable form against the 2-D form, both float32, same measure
MAX_BOUNDARY_SHARE = 0.01        # the issue's condition: at most 1 % of a case's pixels
GPU_MARGIN = 4.0                 # the lighting test's margin: another order of the same fp32 operations, fast exp / pow excluded
# the composite's modes, float32 against float64 of the restatement on the case images (absolute, values in [0, 1])
F32_VS_F64_COMPOSITE = 6.0e-6    # measured 5.07e-6 (heat map of sdiff; 3.4e-6 on s200)


def smooth_field(W, H, seed=1, contrast=1.0):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, size=(3, 4))
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    U, V = np.meshgrid(u, v)
    img = np.ones((H, W, 4), np.float64)
    for c in range(3):
        img[..., c] = 0.5 + contrast * 0.17 * np.sin(2 * np.pi * (1.5 + c) * U + ph[c, 0]) * np.cos(2 * np.pi * (1.0 + 0.5 * c) * V + ph[c, 1]) \
            + contrast * 0.13 * np.sin(2 * np.pi * (3.0 * U + 2.0 * V) + ph[c, 2]) + contrast * 0.05 * np.cos(2 * np.pi * 7.0 * V + ph[c, 3])
    return fp16_values(img)


def fp16_values(img):
    out = np.clip(img, 0.1, 0.9).astype(np.float16).astype(np.float32)
    out[..., 3] = 1.0
    return out


def perturb(img, seed=2):
    """noise of magnitude 0.008..0.02 with a random sign on every colour channel, plus a step of 0.03 on the right half"""
    rng = np.random.default_rng(seed)
    H, W = img.shape[:2]
    noise = rng.uniform(0.008, 0.02, size=(H, W, 3)) * rng.choice([-1.0, 1.0], size=(H, W, 3))
    out = img.astype(np.float64).copy()
    out[..., :3] += noise
    out[:, W // 2:, :3] += 0.03
    return fp16_values(out)


def synthetic_pair(name):
    """(capture, current) float32 [H, W, 4] of a SYNTH_CASES entry"""
    for n, (cw, ch), (w, h), _ in SYNTH_CASES:
        if n == name:
            contrast = 1.0 if (cw, ch) == (w, h) else SDIFF_CONTRAST
            cur = smooth_field(w, h, contrast=contrast)
            cap = perturb(smooth_field(cw, ch, contrast=contrast), seed=2 + cw)
            return cap, cur
    raise KeyError(name)


def rel_diff(v32, v64):
    """largest per-pixel relative difference; where the float64 value is 0 the other must be 0"""
    v32 = np.asarray(v32, np.float64)
    nz = v64 > 0
    assert (v32[~nz] == 0).all()
    return float(np.max(np.abs(v32[nz] - v64[nz]) / v64[nz])) if nz.any() else 0.0


def boundary_count(u64, rel):
    """pixels whose float64 units lie within rel * u of an integer >= 1"""
    k = np.rint(u64)
    return int(np.count_nonzero((k >= 1) & (np.abs(u64 - k) <= rel * u64)))


def recorded(key, sampled=False):
    """the recorded per-pixel relative difference of a quantity measure() names"""
    if key == "mse":
        return F32_VS_F64_MSE_SAMPLED if sampled else F32_VS_F64_MSE
    return F32_VS_F64_FLIP_APPROX if key == "flip1" else F32_VS_F64_FLIP_REF


def flip_bar(flip_mode):
    if flip_mode == 1:
        return F32_VS_F64_FLIP_APPROX
    return F32_VS_F64_FLIP_REF


def gpu_bar(flip_mode=None, sampled=False):
    """relative bar of a GPU sum against the float64 restatement; None: the MSE (sampled: the current image has another size)"""
    if flip_mode is None:
        return GPU_MARGIN * (F32_VS_F64_MSE_SAMPLED if sampled else F32_VS_F64_MSE)
    if flip_mode == 1:
        return GPU_MARGIN * F32_VS_F64_FLIP_APPROX
    return GPU_MARGIN * F32_VS_F64_FLIP_REF + SEP_VS_2D_FLIP_REF


def measure(cap, cur, modes, ppd=PPD):
    """{quantity: (largest relative difference float32 vs float64 over two orders, boundary pixels, bit-equal fixed sums)}"""
    out = {}
    ref = {m: npc.contributions(cap, cur, m, ppd, np.float64, 0) for m in modes}
    alt = {(m, o): npc.contributions(cap, cur, m, ppd, np.float32, o) for m in modes for o in (0, 1)}
    m0 = modes[0]
    u64 = ref[m0][1]
    rel = max(rel_diff(alt[(m0, o)][1], u64) for o in (0, 1))
    same = all(int(npc.to_fixed(alt[(m0, o)][1]).sum()) == int(npc.to_fixed(u64).sum()) for o in (0, 1))
    out["mse"] = (rel, u64, same)
    for m in modes:
        if m == 0:
            continue
        u64 = ref[m][3]
        rel = max(rel_diff(alt[(m, o)][3], u64) for o in (0, 1))
        same = all(int(npc.to_fixed(alt[(m, o)][3]).sum()) == int(npc.to_fixed(u64).sum()) for o in (0, 1))
        out["flip%d" % m] = (rel, u64, same)
    return out
