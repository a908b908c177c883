"""CPU side of the fragment-count tests (no GPU): the oracle against the float64 count of tests/np_fragments.py on the cases of
tests/fragment_cases.py, the borderline share of every case, and the measurement behind fragment_cases.EPS_FRAG.  What is
established here from the two CPU implementations alone is what tests/test_gpu_fragments.py holds the compositor to."""
import numpy as np
import pytest

import fragment_cases as fc
import np_fragments as nf

ALL_CASES = (["dense", "sparse", "hand_made", "hand_made_open", "opaque_gaussian", "two_instances", "crowded", "crowded_opaque"]
             + fc.GRID_CASES + list(fc.DEFAULT_BIN_GRIDS))


def oracle_alpha(ob, ref, order, **kw):
    """the oracle's additive alpha (fp32 target, back to front: alpha = sum of the fragments' alphas) of the splats `order`"""
    img, _ = ob.render(ob.make_frame(**dict(ref.frame_kw, **kw)), ref.inst, order=np.ascontiguousarray(order, np.uint32))
    return img[..., 3]


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_alpha_is_the_fragment_count(ob, name):
    ref = fc.reference(ob, name)
    fr = ref.fragments()
    # the per-splat decisions (dist-stage cull) of float64 and of the oracle's fp32 agree on every splat of these cases
    drawn64 = np.concatenate(ref.survivors)
    assert np.array_equal(drawn64, ref.oracle_survivors), np.flatnonzero(drawn64 != ref.oracle_survivors)
    alpha = oracle_alpha(ob, ref, np.flatnonzero(ref.oracle_survivors), debug_flags=4)
    share = float(fr.borderline.mean())
    print(f"fragments {name}: {fr.count.size} pixels, {fr.count.mean():.2f} fragments per pixel, max {fr.count.max()}, "
          f"borderline share {100 * share:.3f} % ({int(fr.borderline.sum())} pixels)")
    assert share <= fc.BORDERLINE_CAP, share
    bad = (alpha != fr.count) & ~fr.borderline
    assert not bad.any(), nf.describe(fr, alpha, fr.count, bad)
    on_edge = np.abs(alpha - fr.count) <= fr.borderline_count
    assert on_edge.all(), nf.describe(fr, alpha, fr.count, ~on_edge)
    assert fr.count.max() > 0


def test_hand_made_case_covers_what_it_is_made_for(ob):
    """the placement the hand-made splats exist for, checked on the float64 projection: centres on the edges, the clamp, the stacks"""
    ref = fc.reference(ob, "hand_made")
    pr, fr = ref.projected[0], ref.fragments()
    assert pr["valid"].all() and ref.survivors[0].all()
    c = pr["center_px"]
    for ex, ey in ((32.0, 16.0), (48.0, 24.0), (128.0, 64.0)):
        for dx in (0.0, -0.5, 0.5):
            assert (np.abs(c - [ex + dx, ey + dx]).max(axis=1) < 1e-4).any(), (ex, ey, dx)
    lengths = np.hypot(pr["b1"][:, 0], pr["b1"][:, 1])
    assert np.isclose(lengths.max(), 2048.0) and (lengths > 1000).sum() == 1             # one splat at the clamp
    assert ((c[:, 0] < 0) | (c[:, 1] > fc.HH)).sum() == 2                                   # two centres outside the frame
    assert (np.hypot(pr["b2"][:, 0], pr["b2"][:, 1]) < 0.5).sum() == 2                      # two sub-pixel splats
    in_regions = np.zeros(fr.count.shape, bool)
    for n, (cx, cy), _ in fc.STACKS:  # each stack lies inside its one region, where nothing else adds more than a few fragments
        x, y = int(cx), int(cy)
        assert n <= fr.count[y, x] <= n + 2, (n, fr.count[y, x])
        in_regions[y // 16 * 16:y // 16 * 16 + 16, x // 32 * 32:x // 32 * 32 + 32] = True
    assert not ((fr.count >= 449) & ~in_regions).any()
    assert fr.count.min() == 1 and fr.count.max() >= 513  # (the splat at the clamp covers the frame)
    assert (fc.reference(ob, "hand_made_open").fragments().count == 0).mean() > 0.5


def rects_by_id(ref):
    """the bin rectangles of a grid case's splats from the restatement's footprint boxes, indexed by splat id (every splat is drawn)"""
    c, t = ref.c, ref.fragments().table
    assert np.array_equal(t["id"], np.arange(ref.total)), "a splat of the case is culled"
    r, hit = fc.bin_rects(t, c["W"], c["H"], *c["bin_px"])
    assert hit.all()
    return r


@pytest.mark.parametrize("name", list(fc.GRIDS) + list(fc.DEFAULT_BIN_GRIDS))
def test_grid_case_reaches_its_regime(ob, name):
    """each grid case's premise from reference data alone: the bin grid that W, H and the shifts give, whether the direct binning takes
    it, and the rectangles its groups were placed for (float64 footprint boxes)"""
    ref = fc.reference(ob, name)
    c, tags = ref.c, ref.c["tags"]
    (bx, by), (bw, bh) = c["bins"], c["bin_px"]
    assert fc.bin_grid(c["W"], c["H"], {32: 1, 128: 3}[bw], {16: 0, 64: 2}[bh]) == (bx, by)
    if name in fc.GRIDS:
        assert (bx, by) == fc.GRIDS[name][:2]
        assert fc.direct_binning_takes(bx, by) == (not name.startswith(fc.RECORD_GRIDS)), name
    r = rects_by_id(ref)
    wide, high = r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1
    assert tuple(r[tags["oversized"][0]]) == (0, 0, bx - 1, by - 1)
    inside = {int(r[i, 1] * bx + r[i, 0]) for i in tags["inside"] if wide[i] == 1 and high[i] == 1}
    assert inside == set(range(bx * by)), inside   # every bin, the four corner bins and bin nb - 1 among them
    shapes = {"corner": (2, 2), "edge_x": (2, 1), "edge_y": (1, 2), "ends_x_2": (2, 1), "ends_y_2": (1, 2), "3x1": (3, 1), "1x3": (1, 3), "3x3": (3, 3)}
    for tag, (nx, ny) in shapes.items():
        for i in tags.get(tag, ()):
            assert (wide[i], high[i]) == (nx, ny), (tag, i, r[i])
    for tag in ("ends_x_1", "ends_y_1"):   # one bin, up to the last (from the first) pixel of it
        for i in tags.get(tag, ()):
            assert (wide[i], high[i]) == (1, 1), (tag, i, r[i])
    assert ("corner" in tags) == (bx >= 2 and by >= 2) and ("3x1" in tags) == (bx >= 3) and ("1x3" in tags) == (by >= 3)
    assert all(wide[i] == bx for i in tags.get("all_columns", ())) and ("all_columns" in tags) == (bx >= 2)
    assert all(high[i] == by for i in tags.get("all_rows", ())) and ("all_rows" in tags) == (by >= 2)
    cpx = ref.projected[0]["center_px"][tags["outside"]]
    assert cpx[0, 0] < 0 and cpx[1, 0] > c["W"] and cpx[2, 1] < 0 and cpx[3, 1] > c["H"]
    n_esc = int(((wide > 2) | (high > 2)).sum())
    print(f"fragments {name}: {c['W']}x{c['H']} px, {bx}x{by} bins (sum {bx + by}), {ref.total} splats, {n_esc} escapes, "
          f"{int(fc.rect_entries(r).sum())} list entries")


@pytest.mark.parametrize("name", list(fc.STACK_CASES))
def test_stack_case_fills_its_chunks(ob, name):
    """the chunk and stage premises from the oracle's sorted order and the restatement's footprint boxes: the sorted count, and the
    list entries of every chunk of 1024 sorted splats"""
    ref = fc.reference(ob, name)
    assert fc.bin_grid(ref.c["W"], ref.c["H"], 1, 0) == (16, 16)
    r = rects_by_id(ref)
    keys, ids = ob.key_cull(ob.make_frame(**ref.frame_kw), ref.inst)
    _, order = ob.sort_stable(keys, ids)
    assert order.size == ref.total == sum(n for n, _, _ in fc.STACK_CASES[name])
    entries = fc.rect_entries(r)[order]
    per_chunk = [int(entries[i:i + 1024].sum()) for i in range(0, order.size, 1024)]
    print(f"fragments {name}: {order.size} sorted splats, list entries per chunk {per_chunk}")
    assert tuple(r[order[0]]) == (0, 0, 15, 15)
    if name == "stage_edge":
        assert per_chunk == fc.STAGE_EDGE_ENTRIES and per_chunk[1] == 3072 and per_chunk[2] == 3073 and per_chunk[0] > 3072
    else:
        assert order.size == int(name.split("_")[1]) and len(per_chunk) == (order.size + 1023) // 1024
        assert name == "chunks_1024" or entries[1024 * (len(per_chunk) - 1):].size == 1   # a last chunk of one splat


def test_staged_records_per_region(ob):
    """which cases reach the compositor's batch edges: a region that stages more than MGS_SUM_GO = 192 records walks a second batch
    (after the first every wave is saturated in the count mode: the polynomial walk), more than MGS_SUM_CAP = 448 fills a batch"""
    staged = {name: fc.reference(ob, name).staged_per_region() for name in ("dense", "sparse", "crowded", "hand_made")}
    for name, s in staged.items():
        print(f"fragments {name}: staged records per region: median {int(np.median(s))}, max {s.max()}, {(s > 192).sum()} regions above 192, {(s > 448).sum()} above 448")
    assert staged["dense"].max() <= 192           # (as the issue sets the case: one batch per region)
    assert (staged["crowded"] > 192).sum() >= 20 and (staged["crowded"] > 448).sum() >= 2
    assert (staged["hand_made"] > 448).sum() == 3  # the three stacks


def test_occluder_levels_split_the_counts(ob):
    """a constant occluder depth beyond every splat changes no count; one at the median key depth keeps the nearer half"""
    ref = fc.reference(ob, "sparse")
    full, far, med = ref.fragments(), ref.fragments(depth_level=1.0), ref.fragments(depth_level=ref.median_level())
    assert np.array_equal(full.count, far.count) and np.array_equal(full.borderline_count, far.borderline_count)
    assert (med.count <= full.count).all() and 0.2 * full.count.sum() < med.count.sum() < 0.8 * full.count.sum()
    # against the oracle, which has no depth test: the draw order filtered by the key depth
    keep = np.flatnonzero(ref.oracle_survivors & (ref.key_depth <= ref.median_level()))
    alpha = oracle_alpha(ob, ref, keep, debug_flags=4)
    bad = (alpha != med.count) & ~med.borderline
    assert not bad.any(), nf.describe(med, alpha, med.count, bad)


def measure_eps_frag(ob, name):
    """largest |oracle alpha - float64 alpha| over the fragments of a case that are clear of the thresholds: every splat is drawn
    alone by the oracle (additive alpha of one splat = its fragments' alphas), windowed to its footprint"""
    ref = fc.reference(ob, name)
    t = ref.fragments(gaussian=True).table
    Wc, Hc = ref.c["W"], ref.c["H"]
    frame = ob.make_frame(**ref.frame_kw)
    worst, n = 0.0, 0
    ex = np.abs(t["b1"][:, 0]) + np.abs(t["b2"][:, 0])
    ey = np.abs(t["b1"][:, 1]) + np.abs(t["b2"][:, 1])
    for i in range(t["id"].shape[0]):
        x0, x1 = int(max(0, np.floor(t["c"][i, 0] - ex[i] - 1))), int(min(Wc - 1, np.ceil(t["c"][i, 0] + ex[i] + 1)))
        y0, y1 = int(max(0, np.floor(t["c"][i, 1] - ey[i] - 1))), int(min(Hc - 1, np.ceil(t["c"][i, 1] + ey[i] + 1)))
        if x1 < x0 or y1 < y0:
            continue
        img, _ = ob.render_window(frame, ref.inst, np.array([t["id"][i]], np.uint32), (x0, y0, x1, y1))
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        A, alpha = nf._eval(t["c"][i], t["b1"][i], t["b2"][i], t["opacity"][i], xx + 0.5, yy + 0.5, True)
        keep, edge = nf._rule(A, alpha, True, fc.DELTA)
        clear = ~edge
        assert np.array_equal((img[..., 3] > 0)[clear], keep[clear]), (name, int(t["id"][i]))
        m = keep & clear
        if m.any():
            worst = max(worst, float(np.abs(img[..., 3].astype(np.float64) - alpha)[m].max()))
            n += int(m.sum())
    return worst, n


def test_eps_frag_is_the_oracles_own_error(ob):
    worst = 0.0
    for name in fc.EPS_CASES:
        e, n = measure_eps_frag(ob, name)
        fr = fc.reference(ob, name).fragments(gaussian=True)
        print(f"fragments {name} (gaussian on): {n} fragments, worst per-fragment alpha error of the oracle {e:.3e}; "
              f"borderline share {100 * fr.borderline.mean():.3f} %, mean alpha sum {fr.alpha_sum.mean():.2f}")
        assert fr.borderline.mean() <= fc.BORDERLINE_CAP
        worst = max(worst, e)
    print(f"EPS_FRAG measured {worst:.3e}, fragment_cases.EPS_FRAG = {fc.EPS_FRAG:.3e}")
    assert fc.EPS_FRAG / 2 <= worst <= fc.EPS_FRAG, (worst, fc.EPS_FRAG)


@pytest.mark.parametrize("name", fc.GAUSSIAN_CASES)
def test_oracle_alpha_sum_with_the_gaussian(ob, name):
    """the bound tests/test_gpu_fragments.py gives the compositor, met by the oracle with its own error (margin 1 instead of 8) on
    every pixel that is not borderline.  On the borderline pixels the figures are printed only: a fragment on the A = 8 edge weighs
    exp(-4) * opacity, up to 0.018, which is more than the 1 / 255 per borderline fragment that the widened bound allows — the
    oracle's fp32 itself lands on the other side than float64 for two such fragments of "crowded_opaque"."""
    ref = fc.reference(ob, name)
    fr = ref.fragments(gaussian=True)
    alpha = oracle_alpha(ob, ref, np.flatnonzero(ref.oracle_survivors)).astype(np.float64)
    bound = fc.EPS_FRAG * fr.count + 4e-7 * fr.alpha_sum
    wide = bound + fr.borderline_count * (1.0 + fc.DELTA) / 255.0
    err = np.abs(alpha - fr.alpha_sum)
    clear = ~fr.borderline
    print(f"fragments {name} (gaussian on): oracle's worst error / bound {float((err / np.maximum(bound, 1e-30))[clear].max()):.3f} on {int(clear.sum())} pixels; "
          f"{int((err > wide).sum())} of {int(fr.borderline.sum())} borderline pixels beyond the widened bound")
    bad = (err > bound) & clear
    assert not bad.any(), nf.describe(fr, alpha, fr.alpha_sum, bad)


def test_basis_direction_of_nearly_axis_aligned_splats(ob):
    """what fragment_cases.BASIS_ULPS stands on, from the two CPU implementations alone: how far the direction of the oracle's fp32
    basis is from the float64 one, in the units of np_fragments.basis_turn, over every drawn splat of "crowded" — and that for the
    least determined splats it is off by far more than the 1e-6 that lengths and centres agree to (a turn that moves A by more than
    DELTA at some pixels)"""
    ref = fc.reference(ob, "crowded")
    t = ref.fragments().table
    unit = nf.basis_turn(ref.projected[0], 1)[t["id"]]
    frame = ob.make_frame(**ref.frame_kw)
    turn = np.zeros(t["id"].shape[0])
    for i in range(turn.size):
        p = ob.project(frame, ref.inst, 0, int(t["id"][i]))
        assert p.valid
        b1 = np.array(list(p.basis1), np.float64)
        cross = b1[0] * t["b1"][i, 1] - b1[1] * t["b1"][i, 0]
        turn[i] = abs(np.arcsin(np.clip(cross / (np.hypot(*b1) * np.hypot(*t["b1"][i])), -1, 1)))
    steps = float((turn / unit).max())
    print(f"fragments crowded: oracle's basis direction off by up to {turn.max():.2e} rad; BASIS_ULPS measured {steps:.2f}, "
          f"fragment_cases.BASIS_ULPS = {fc.BASIS_ULPS}")
    assert turn.max() > 1e-4
    assert fc.BASIS_ULPS / 2 <= steps <= fc.BASIS_ULPS, steps
    assert np.array_equal(t["theta"], fc.BASIS_MARGIN * fc.BASIS_ULPS * unit)
