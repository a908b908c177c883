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
both binning paths and with the smallest bins.

The last section holds the binning stage to the same counts on every bin grid at which it changes its path: the limits of the direct
binning (32 bins along an axis, 256 bins, binsX + binsY = 40), masks by ballots and by transpose at their edges, the frames that fall
to the record path, the three placement paths of k_dbin_emit around its stage of 3072 entries, chunk boundaries, and strips that begin
and end inside a bin."""
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


# ---- every bin-grid regime of the binning stage --------------------------------------------------------------------------------------
# What the binning hands the compositor, exactly, on the grids where k_dbin_count / k_dbin_emit change their path
# (fragment_cases.GRIDS, STACK_CASES; test_fragments_cpu.py shows from the CPU side that each case reaches its regime).
def check_binning(what, name, ref, stats, ids, rects, rides):
    """the frame's statistics against the sorted splats' own rectangles: every list entry counted once (exactly), the over-sized
    splat over the whole grid (the frame had the grid the case was built for), the escapes where the rectangles ride"""
    sorted_count, tile_pairs, escape_count, error_flags = (int(v) for v in stats)
    bx, by = ref.c["bins"]
    assert error_flags == 0, (what, error_flags)
    assert sorted_count == ref.total == ids.size, (what, sorted_count, ref.total)
    entries = fc.rect_entries(rects)
    assert tile_pairs == int(entries.sum()), (what, tile_pairs, int(entries.sum()))
    over = rects[ids == ref.c["tags"]["oversized"][0]]
    assert over.shape[0] == 1 and tuple(over[0]) == (0, 0, bx - 1, by - 1), (what, over)
    escapes = int(((rects[:, 2] - rects[:, 0] > 1) | (rects[:, 3] - rects[:, 1] > 1)).sum())
    if rides:
        assert escape_count == escapes, (what, escape_count, escapes)
    per_chunk = [int(entries[i:i + 1024].sum()) for i in range(0, ids.size, 1024)]
    print(f"fragments {what}: {sorted_count} sorted, {tile_pairs} list entries, {escapes} escapes, entries per chunk {per_chunk}")
    if name == "stage_edge":
        assert per_chunk == fc.STAGE_EDGE_ENTRIES, (what, per_chunk)


@pytest.mark.parametrize("name", list(fc.DEFAULT_BIN_GRIDS))
def test_counts_default_bins(scenes, ob, name):
    """2048x1024 (16x16) and 4096x512 (32x8) at the additive alpha's own 128x64-px bins: no switch set"""
    ref = fc.reference(ob, name)
    fr = ref.fragments()
    alpha, out = gf.render_counts(scenes(name), name)
    check_counts(f"{name}, default bins", fr, alpha, out)
    ids, rects = gf.sorted_rects(scenes(name), out)
    check_binning(name, name, ref, (out.sorted_count, out.tile_pairs, out.escape_count, out.error_flags), ids, rects, rides=True)


class Rows:
    """the pixel rows [y0, y1) of a Fragments, for check_counts"""

    def __init__(self, fr, y0, y1):
        self.fr, self.y0 = fr, y0
        self.count, self.borderline_count = fr.count[y0:y1], fr.borderline_count[y0:y1]
        self.borderline = self.borderline_count > 0

    def covering(self, x, y):
        return self.fr.covering(x, y + self.y0)


@pytest.mark.parametrize("strip", [(0, 1), (1, 6), (5, 7), (7, 64), (8, 12)], ids=lambda s: f"rows_{s[0]}_{s[1]}")
def test_counts_of_strips_inside_bins(scenes, ob, strip):
    """tile rows [r0, r1) of the 16x16 default-bin frame (a bin is 4 tile rows: the strips begin and end inside bins, (8, 12) is one
    bin row): the strip's own pixel rows hold the full frame's counts"""
    name = "bins128_16x16"
    fr = fc.reference(ob, name).fragments()
    assert (fc.case(name)["H"] + 15) // 16 == 64
    y0, y1 = 16 * strip[0], 16 * strip[1]
    # the frame buffer outlives a frame: first fill it with a frame that is no count anywhere on the strip's rows (the same frame with
    # the gaussian on: every pixel lies under the over-sized splat and gets a non-integer alpha), so that a pixel the strip's frame
    # does not write cannot pass
    before, _ = gf.render_alpha(scenes(name), name, alpha_mode=capi.ALPHA_SUM)
    assert (before[y0:y1] != fr.count[y0:y1]).all() and (before[y0:y1] != np.floor(before[y0:y1])).all()
    alpha, out = gf.render_alpha(scenes(name), name, strip=strip, alpha_mode=capi.ALPHA_SUM, debug_flags=4)
    check_counts(f"{name}, tile rows {strip}", Rows(fr, y0, y1), alpha[y0:y1], out)


GRID_ENVS = {"default": {}, "ballots": {"MGS_DB_TRANSPOSE": "0"}, "gather": {"MGS_RECT_RIDE": "0"}, "split": {"MGS_RIDE_SPLIT": "2"},
             "records": {"MGS_DIRECT_BIN": "0"}}


@pytest.fixture(scope="module")
def grid_children(tmp_path_factory):
    """one child per environment (all with 32x16-px bins), started on first use: name -> the child's npz as a dict"""
    done = {}

    def get(env_id):
        if env_id not in done:
            import time
            child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_fragment_grids.py")
            out = str(tmp_path_factory.mktemp("grids") / f"{env_id}.npz")
            e = {k: v for k, v in os.environ.items() if k not in ("MGS_DIRECT_BIN", "MGS_BIN_SHIFT", "MGS_DB_TRANSPOSE", "MGS_RECT_RIDE", "MGS_RIDE_SPLIT")}
            e.update(GRID_ENVS[env_id], MGS_BIN_SHIFT="1,0")
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, child, out], env=e, capture_output=True, text=True, timeout=300)
            print(f"fragments grids, {env_id}: child took {time.perf_counter() - t0:.1f} s")
            assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
            with np.load(out) as z:
                done[env_id] = {k: z[k] for k in z.files}
        return done[env_id]

    return get


@pytest.mark.parametrize("env_id", list(GRID_ENVS))
def test_grid_counts(grid_children, ob, env_id):
    """every grid, chunk and stage case with 32x16-px bins against the float64 counts, and the frame's statistics against the sorted
    splats' rectangles: masks by transpose or ballots as the grid decides with the rectangles riding (default), ballots everywhere,
    every rectangle gathered by id (staged without ride), the codes split, and the record + pair-sort path.  A frame of 257 bin
    columns is refused and the scene's next frame holds its counts."""
    got = grid_children(env_id)
    for name in fc.GRID_CASES:
        ref = fc.reference(ob, name)
        what = f"{name}, {env_id}"
        check_counts(what, ref.fragments(), got[name + "/alpha"])
        rides = env_id in ("default", "ballots", "split") and fc.direct_binning_takes(*ref.c["bins"])
        check_binning(what, name, ref, got[name + "/stats"], got[name + "/ids"], got[name + "/rects"], rides)
    # the refused frame: the buffer held a frame that is no count anywhere (the gaussian on) when it was refused, the frame after it
    # holds the counts again
    first = fc.GRID_CASES[0]
    fr = fc.reference(ob, first).fragments()
    assert int(got["invalid/code"]) == capi.ERR_INVALID_ARG
    assert (got["invalid/alpha_before"] != fr.count).all()
    check_counts(f"{first}, {env_id}, after the refused frame", fr, got["invalid/alpha_after"])
    assert np.array_equal(got["invalid/alpha_after"].view(np.uint32), got[first + "/alpha"].view(np.uint32))


def test_grid_counts_identical_across_settings(grid_children):
    """the five settings' alpha planes are the same bit for bit"""
    base = grid_children("default")
    for env_id in GRID_ENVS:
        got = grid_children(env_id)
        for name in fc.GRID_CASES:
            assert np.array_equal(got[name + "/alpha"].view(np.uint32), base[name + "/alpha"].view(np.uint32)), (env_id, name)
