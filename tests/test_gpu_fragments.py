"""GPU tests (-m gpu): which pixel receives which fragment, exactly.

With the opacity gaussian disabled (debug_flags = 4) every fragment has alpha 1 and the only fragment rule is A <= 8, so the additive
alpha (MGS_ALPHA_SUM) of an RGBA32F frame is the integer NUMBER of fragments of each pixel.  It is compared with the float64 count of
tests/np_fragments.py on the cases of tests/fragment_cases.py: equal on every pixel that has no fragment within DELTA of the
threshold, within the number of such fragments elsewhere.  tests/test_fragments_cpu.py shows from the CPU side alone that the oracle
meets the same comparison, that at most 1 % of a case's pixels are borderline, and where EPS_FRAG comes from.

The two cases added to the issue's ("crowded", "crowded_opaque": the only ones whose regions walk a second batch) also set aside
the fragments that the direction of a nearly axis-aligned splat's basis leaves open in fp32 (fragment_cases.BASIS_ULPS): the kernel
counted 26 fragments where float64 has 25 at pixel (251,81) of "crowded", whose only near miss is splat 6286 at A = 8.00287, a splat
whose basis the oracle's own fp32 puts 3.9e-4 rad from the float64 one.

Every walk of k_composite has to arrive at the same number: the additive mode's own walks (per-wave sum walk, the all-saturated
batches' polynomial walk), the general walk (surface outputs, occluder), and — as coverage — the default mode's early-out walk; on
both binning paths and with the smallest bins."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vk_gaussian_splatting_amd import capi
import fragment_cases as fc
import gpu_fragments as gf
import np_fragments as nf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    """one committed scene per case, built on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = gf.build_scene(name)
        return made[name]

    yield get
    for s in made.values():
        s.close()


def check_counts(what, fr, alpha, out=None):
    """alpha == count off the borderline pixels, within borderline_count on them, a non-negative integer everywhere"""
    if out is not None:
        assert out.error_flags == 0, (what, out.error_flags)
    clear = ~fr.borderline
    print(f"fragments {what}: {int(clear.sum())} pixels compared exactly, {int(fr.borderline.sum())} borderline "
          f"({100 * fr.borderline.mean():.3f} %), {int((alpha != fr.count).sum())} of them differ by a fragment")
    assert np.isfinite(alpha).all(), what
    whole = (alpha >= 0) & (alpha == np.floor(alpha))
    assert whole.all(), what + ": not a non-negative integer\n" + nf.describe(fr, alpha, fr.count, ~whole)
    bad = (alpha != fr.count) & clear
    assert not bad.any(), what + "\n" + nf.describe(fr, alpha, fr.count, bad)
    off = np.abs(alpha.astype(np.float64) - fr.count) > fr.borderline_count
    assert not off.any(), what + ": beyond the borderline fragments\n" + nf.describe(fr, alpha, fr.count, off)


# ---- the additive mode's own walks (compositor modes 1 | 2) ------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.COUNT_CASES)
def test_counts_sum_walk(scenes, ob, name):
    fr = fc.reference(ob, name).fragments()
    alpha, out = gf.render_alpha(scenes(name), name, alpha_mode=capi.ALPHA_SUM, debug_flags=4)
    check_counts(f"{name}, sum walk", fr, alpha, out)


# ---- the general walk: the instantiations where sum_walk() is false must count the same -----------------------------------------------
@pytest.mark.parametrize("name", fc.COUNT_CASES)
def test_counts_general_walk_with_surface_outputs(scenes, ob, name):
    fr = fc.reference(ob, name).fragments()
    alpha, out = gf.render_alpha(scenes(name), name, alpha_mode=capi.ALPHA_SUM, debug_flags=4, surface_outputs=1)
    check_counts(f"{name}, surface outputs", fr, alpha, out)


@pytest.mark.parametrize("level", ["beyond", "median"])
@pytest.mark.parametrize("name", fc.COUNT_CASES)
def test_counts_general_walk_with_an_occluder(scenes, ob, name, level):
    """a constant occluder depth: beyond every splat (1.0) the count is unchanged; at the median key depth it is the fragments with
    z <= D, z = the key depth (bit-exact with the oracle's: test_depth_keys_cull_and_sort_bit_exact), D in a gap of the key depths"""
    ref = fc.reference(ob, name)
    D = np.float32(1.0) if level == "beyond" else ref.median_level()
    fr = ref.fragments(depth_level=D)
    if level == "beyond":
        assert np.array_equal(fr.count, ref.fragments().count)
    scene = scenes(name)
    scene.upload_occluder(np.full((ref.c["H"], ref.c["W"]), D, np.float32))
    try:
        alpha, out = gf.render_alpha(scene, name, alpha_mode=capi.ALPHA_SUM, debug_flags=4)
    finally:
        scene.clear_occluder()
    check_counts(f"{name}, occluder at {level} depth {float(D):.6f}", fr, alpha, out)


# ---- the default mode's early-out walk: a wave that retires early or a quarter masked out wrongly leaves a hole --------------------
@pytest.mark.parametrize("name", fc.COVERAGE_CASES)
def test_coverage_early_out(scenes, ob, name):
    fr = fc.reference(ob, name).fragments()
    alpha, out = gf.render_alpha(scenes(name), name, debug_flags=4)
    assert out.error_flags == 0
    covered = (fr.count > 0).astype(np.float32)
    clear = ~fr.borderline
    print(f"fragments {name}, coverage: {int(clear.sum())} pixels compared, {100 * covered.mean():.1f} % covered")
    bad = (alpha != covered) & clear
    assert not bad.any(), name + "\n" + nf.describe(fr, alpha, covered, bad)
    assert np.isin(alpha, (0.0, 1.0)).all()


# ---- the real-valued sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.GAUSSIAN_CASES)
def test_alpha_sum_with_the_gaussian(scenes, ob, name):
    """|alpha - alpha_sum| <= 8 EPS_FRAG count + 4e-7 alpha_sum off the borderline pixels: the oracle's own per-fragment error
    (fragment_cases.EPS_FRAG, measured on the CPU) with a margin of 8 for v_exp_f32 / v_log_f32 and the 2^(log2 a - q) form, plus
    fp32 summation; widened by borderline_count (1 + DELTA) / 255 on the borderline pixels."""
    fr = fc.reference(ob, name).fragments(gaussian=True)
    alpha, out = gf.render_alpha(scenes(name), name, alpha_mode=capi.ALPHA_SUM)
    assert out.error_flags == 0
    bound = 8.0 * fc.EPS_FRAG * fr.count + 4e-7 * fr.alpha_sum
    wide = bound + fr.borderline_count * (1.0 + fc.DELTA) / 255.0
    err = np.abs(alpha.astype(np.float64) - fr.alpha_sum)
    clear = ~fr.borderline
    ratio = err / np.maximum(bound, 1e-30)
    print(f"fragments {name}, gaussian on: worst error / bound {float(ratio[clear & (fr.count > 0)].max()):.4f} on {int(clear.sum())} pixels "
          f"(mean alpha sum {fr.alpha_sum.mean():.2f}); {int(fr.borderline.sum())} borderline pixels, worst error / widened bound "
          f"{float((err / np.maximum(wide, 1e-30))[fr.borderline].max()) if fr.borderline.any() else 0.0:.4f}")
    bad = (err > bound) & clear
    assert not bad.any(), name + "\n" + nf.describe(fr, alpha, fr.alpha_sum, bad)
    off = (err > wide) & fr.borderline
    assert not off.any(), name + ": borderline pixels\n" + nf.describe(fr, alpha, fr.alpha_sum, off)


# ---- both binning paths and the smallest bins ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_hashes(scenes, ob):
    """SHA-1 of the count-mode alpha plane of this (default) process, whose planes are the ones compared with the counts"""
    res = {}
    for name in fc.CHILD_CASES:
        alpha, out = gf.render_alpha(scenes(name), name, alpha_mode=capi.ALPHA_SUM, debug_flags=4)
        check_counts(f"{name}, default binning", fc.reference(ob, name).fragments(), alpha, out)
        res[name] = gf.sha1(alpha)
    return res


@pytest.mark.parametrize("env", [{"MGS_DIRECT_BIN": "0"}, {"MGS_BIN_SHIFT": "1,0"}, {"MGS_DIRECT_BIN": "0", "MGS_BIN_SHIFT": "1,0"}],
                         ids=["pair_sort", "bins_32x16", "pair_sort_bins_32x16"])
def test_binning_paths_give_the_same_counts(default_hashes, env):
    """the record + pair-sort path and 32x16-px bins (one region per bin) hand the compositor the same lists restricted to a bin: the
    alpha planes are the default process's, bit for bit"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_fragments.py")
    e = {k: v for k, v in os.environ.items() if k not in ("MGS_DIRECT_BIN", "MGS_BIN_SHIFT")}
    e.update(env)
    r = subprocess.run([sys.executable, child], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    got = {l.split()[1]: l.split()[2] for l in r.stdout.splitlines() if l.startswith("ALPHA_SHA1")}
    assert got == default_hashes, (env, got, default_hashes)
