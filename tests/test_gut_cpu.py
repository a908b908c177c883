"""CPU tests (no GPU) of the 3DGUT restatement tests/np_gut.py and of the cases of tests/gut_cases.py: every case's premise from the
restatement alone, the oracle (orc_project_gut, orc_gut_fragment through orc_render_gut_order) held to the restatement — same decisions
off the fragile particles, the record's fields within what fp32 leaves, counts and nearest ids equal off the borderline pixels —, the
caps on the fragile and borderline shares, and the oracle's own per-field deviations, which are the yardstick of the kernels' bars
(gut_cases.ORACLE_DEV).  Run with -s to see the figures."""
import numpy as np
import pytest

import gut_cases as gc
import np_gut as ng

BOX_RULES = [ng.REJECTIONS.index(k) for k in ("no_pixel_centre", "off_screen", "off_strip")]


def oracle_scene(ob, name, **fkw):
    """(frame, instances, far-to-near draw order of the dist-stage survivors) of the case for the oracle"""
    c = gc.case(name)
    V, P, eye = c["cam"]
    st = c["st"]
    inst = ob.make_instances([(ob.PreparedSet(a), m) for a, m in c["sets"]])
    kw = dict(camera_model=st["camera_model"], extent_method=st["extent_method"], ms_antialiasing=st["ms_antialiasing"],
              splat_scale=st["splat_scale"], pipeline_3dgut=1)
    kw.update(fkw)
    fr = ob.make_frame(V, P, eye, c["W"], c["H"], **kw)
    ok, oi = ob.key_cull(fr, inst)
    _, ois = ob.sort_stable(ok, oi)
    return fr, inst, ois


def oracle_records(ob, name):
    """(valid[n], rec[n, 24] in the layout of mgs_frame_download_projected_gut) of every particle of the case, from what orc_project_gut
    exposes: centre, half axes, opacity as they are; B and ro from its scale, inverse rotation and the instance's inverse matrix"""
    c = gc.case(name)
    fr, inst, _ = oracle_scene(ob, name)
    o = np.linalg.inv(np.asarray(c["cam"][0], np.float64))[:3, 3]
    valid, rows = [], []
    for k, (a, _) in enumerate(c["sets"]):
        Mi = np.array(list(inst[k].transform_inv), np.float64).reshape(4, 4).T
        for i in range(a["positions"].shape[0]):
            P = ob.project_gut(fr, inst, k, i)
            valid.append(bool(P.valid))
            if not P.valid:
                rows.append(np.zeros(24))
                continue
            h1, h2 = np.array(list(P.half1), np.float64), np.array(list(P.half2), np.float64)
            R = np.array(list(P.inv_rot), np.float64).reshape(3, 3).T           # rows = principal axes
            A = R / np.array(list(P.scale), np.float64)[:, None]
            B = A @ Mi[:3, :3]
            ro = A @ (Mi[:3, :3] @ o + Mi[:3, 3] - np.array(list(P.position), np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                rows.append(np.concatenate([list(P.center_px), h1 / (h1 @ h1), h2 / (h2 @ h2),
                                            [abs(h1[0]) + abs(h2[0]) + 0.01, abs(h1[1]) + abs(h2[1]) + 0.01], B.reshape(-1), ro, [0, 0, 0, P.rgba[3]]]))
    return np.array(valid), np.array(rows)


PREMISES = {
    "cloud": lambda pr, c: pr["emits"].sum() >= 250,
    "trs": lambda pr, c: pr["emits"].sum() >= 100,
    # camera inside the cloud: particles with 1-6 invalid sigma points of both kinds, quads larger than the frame
    "inside": lambda pr, c: (((pr["n_valid"] >= 1) & (pr["n_valid"] <= 6) & (pr["behind"] >= 1)).sum() >= 10
                             and ((pr["n_valid"] >= 1) & (pr["n_valid"] <= 6) & (pr["behind"] == 0)).sum() >= 10
                             and (pr["emits"] & (pr["box"][:, 0] > c["W"] / 2) & (pr["box"][:, 1] > c["H"] / 2)).sum() >= 5),
    # needles and discs that emit; sub-pixel particles that cover no pixel centre (conic) or fall under the 0.1 floor (eigen); the 2048
    # clamp (eigen); boxes that end on tile / region / bin edges (conic, where the box is the quad)
    "shapes": lambda pr, c: (pr["emits"][0:120].sum() >= 60 and
                             ((pr["reason"] == ng.REJECTIONS.index("ev2")).sum() >= 5 and np.linalg.norm(pr["half1"][170]) >= 2047.0
                              if c["st"]["extent_method"] == 0 else
                              (pr["reason"] == ng.REJECTIONS.index("no_pixel_centre")).sum() >= 5 and pr["emits"][171:180].all()
                              and np.abs(pr["cx"][171:180] + pr["box"][171:180, 0] - np.repeat(gc.SHAPES_EDGES[0], 3)).max() < 1e-3
                              and np.abs(pr["cy"][171:180] + pr["box"][171:180, 1] - np.tile(gc.SHAPES_EDGES[1], 3)).max() < 1e-3)),
    "opacity": lambda pr, c: ((pr["reason"] == ng.REJECTIONS.index("alpha_cull")).sum() >= 5
                              and (c["st"]["extent_method"] == 0 or (pr["reason"] == ng.REJECTIONS.index("wop")).sum() >= 5) and pr["emits"].sum() >= 80),
    "strip": lambda pr, c: (pr["reason"] == ng.REJECTIONS.index("off_strip")).sum() >= 5 and pr["emits"].sum() >= 50,
}
for _k in ("fisheye150", "fisheye175"):
    # particles on both sides of the max angle (some with points on either side), the centre of the image, pixels without a ray
    PREMISES[_k] = lambda pr, c: (((pr["n_valid"] >= 1) & (pr["n_valid"] <= 6)).sum() >= 10 and (pr["n_valid"] == 0).sum() >= 5
                                  and pr["emits"].sum() >= 100 and (~ng.pixel_rays(c["cam"][0], c["cam"][1], c["W"], c["H"], c["st"])[1]).sum() >= 100
                                  and (pr["emits"] & (np.hypot(pr["cx"] - c["W"] / 2, pr["cy"] - c["H"] / 2) < 12)).sum() >= 1)


@pytest.mark.parametrize("name", gc.CASES)
def test_case_covers_what_it_is_for(name):
    c = gc.case(name)
    prs = gc.projected(name)
    pr = {k: gc.stack(prs, k) for k in ("emits", "reason", "fragile", "n_valid", "behind", "box", "half1", "cx", "cy")}
    counts = {ng.REJECTIONS[r]: int((pr["reason"] == r).sum()) for r in np.unique(pr["reason"]) if r >= 0}
    share = pr["fragile"][pr["emits"]].mean()
    print(f"\n3DGUT case {name}: {pr['emits'].size} particles, {int(pr['emits'].sum())} emit, rejected {counts}, "
          f"1-6 valid points {int(((pr['n_valid'] >= 1) & (pr['n_valid'] <= 6)).sum())}, behind-camera points on {int((pr['behind'] > 0).sum())}, "
          f"fragile {int(pr['fragile'].sum())} ({share:.4f} of the emitted)")
    assert PREMISES[name.split("+")[0]](pr, c), "the case no longer covers what it is for"
    assert share <= gc.FRAGILE_CAP
    fr = gc.reference_fragments(name)
    cap = gc.BORDERLINE_CAP.get(name.split("+")[0], gc.BORDERLINE_CAP["default"])
    print(f"  fragments {int(fr.count.sum())}, covered pixels {(fr.count > 0).mean():.3f}, max count {fr.count.max()}, "
          f"borderline pixels {fr.borderline.mean():.4f} (cap {cap}), nearest open {fr.nearest_open.mean():.4f}")
    assert fr.borderline.mean() <= cap and fr.count.max() >= 3
    if name in ("cloud", "trs"):   # the occluder cases of the GPU file: the depth images cut through the cloud
        for kind in ("plane", "step"):
            fo = gc.reference_fragments(name, 2, kind)
            print(f"  occluder {kind}: fragments {int(fo.count.sum())}, borderline pixels {fo.borderline.mean():.4f}")
            assert fo.borderline.mean() <= cap and 0.2 * fo.count.sum() < fr.count.sum() - fo.count.sum()


@pytest.mark.parametrize("name", gc.CASES)
def test_oracle_records_match_the_restatement(ob, name):
    prs = gc.projected(name)
    emits, reason, fragile = (gc.stack(prs, k) for k in ("emits", "reason", "fragile"))
    valid, rec = oracle_records(ob, name)
    # the oracle emits every quad the shader emits: the restatement's box rules are the rasteriser's, not orc_project_gut's
    mine = emits | np.isin(reason, BOX_RULES)
    dist = reason == ng.REJECTIONS.index("dist")   # (orc_project_gut is not asked about the dist stage)
    differ = (valid != mine) & ~fragile & ~dist
    assert not differ.any(), [(int(i), ng.REJECTIONS[reason[i]] if reason[i] >= 0 else "emits", bool(valid[i])) for i in np.flatnonzero(differ)[:8]]
    pr = {k: gc.stack(prs, k) for k in ("cx", "cy", "half1", "half2", "box", "B", "ro", "opacity")}
    idx = np.flatnonzero(emits & valid & ~fragile)
    dev, worst = ng.record_deviation(pr, idx, rec[idx])
    print(f"\n3DGUT oracle vs float64, {name} ({idx.size} particles): " + ", ".join(f"{k} {dev[k]:.2e} (#{worst[k]})" for k in ng.FIELDS))
    # the recorded yardstick is the measurement, rounded up: never exceeded (a stale, too large entry shows in the printed line)
    print("  recorded / measured: " + ", ".join(f"{k} {gc.ORACLE_DEV[name][k] / max(dev[k], 1e-300):.2f}" for k in ng.FIELDS))
    for k in ng.FIELDS:
        assert dev[k] <= gc.ORACLE_DEV[name][k], (k, dev[k], worst[k])


@pytest.mark.parametrize("name", gc.CASES)
def test_oracle_counts_and_nearest_ids_match_the_restatement(ob, name):
    """orc_render_gut_order with the opacity gaussian disabled, far to near: the alpha channel is the number of fragments, the colour
    that of the nearest"""
    c = gc.case(name)
    fr, inst, order = oracle_scene(ob, name, debug_flags=4, sh_degree=0)
    img, _ = ob.render_gut(fr, inst, order)
    if c["st"]["strip"] is not None:
        r0, r1 = c["st"]["strip"]
        img[:r0 * 16], img[r1 * 16:] = 0, 0
    ref = gc.reference_fragments(name)
    got = np.rint(img[..., 3]).astype(np.int64)
    off = np.abs(got - ref.count) > np.where(ref.borderline, ref.borderline_count, 0)
    assert not off.any(), ng.describe(ref, got, ref.count, off)
    n0 = c["sets"][0][0]["positions"].shape[0]
    ids = gc.decode_colour(img[..., :3])
    want = np.where(ref.nearest_id >= 0, ref.nearest_id % n0, -1)
    bad = (ids != want) & ~ref.nearest_open & ~ref.borderline
    print(f"\n3DGUT oracle counts, {name}: {int(ref.count.sum())} fragments, {int(ref.borderline.sum())} borderline pixels, "
          f"{int((got != ref.count).sum())} of them differ, nearest id open on {int(ref.nearest_open.sum())}")
    assert not bad.any(), ng.describe(ref, ids, want, bad)


# every rejection of np_gut.REJECTIONS that a particle can reach, and the case that is there for it.  Not reachable by any particle, so
# no case has them: det_zero (the dilated determinant is at least 0.3^2), radius and degenerate (the extent factor is 0 only for an
# opacity of exactly 0.01, and both eigen lengths are positive once ev2 > 0)
RULE_CASES = {"dist": "inside", "alpha_cull": "opacity", "no_valid_point": "fisheye175", "wop": "opacity", "ev2": "shapes+eigen",
              "ndc_z": "inside", "no_pixel_centre": "shapes", "off_screen": "inside", "off_strip": "strip"}


@pytest.mark.parametrize("rule", list(RULE_CASES))
def test_each_reachable_rejection_has_its_case(rule):
    prs = gc.projected(RULE_CASES[rule])
    reason = gc.stack(prs, "reason")
    if rule == "no_valid_point":   # the dist stage's fisheye cull takes these first: the front end's own test is counted before it
        n = int((gc.stack(prs, "n_valid") == 0).sum())
    else:
        n = int((reason == ng.REJECTIONS.index(rule)).sum())
    print(f"\n3DGUT rejection {rule}: {n} particles of {RULE_CASES[rule]}")
    assert n >= 5


@pytest.mark.parametrize("name", gc.GAUSS_CASES)
def test_oracle_blend_lies_in_the_interval(ob, name):
    """the opacity gaussian on: orc_render_gut_order's fp32 frame against the float64 blend evaluated with every borderline fragment in
    and with every one out; its largest distance from that interval is the yardstick of the kernels' tolerance (gut_cases.GAUSS_DEV)"""
    fr, inst, order = oracle_scene(ob, name, sh_degree=0, front_to_back=1)   # nearest first, the "under" blend: alpha is the coverage
    img, _ = ob.render_gut(fr, inst, order)
    lo, hi, fragile = gc.reference_blend(name)
    d = gc.interval_distance(img.astype(np.float64), lo, hi, fragile)
    print(f"\n3DGUT oracle blend, {name}: distance from the interval {d:.2e} (recorded {gc.GAUSS_DEV.get(name)}), widest interval "
          f"{(hi - lo).max():.3f}, fragile pixels {fragile.mean():.4f}, covered {(hi[..., 3] > 0).mean():.3f}")
    assert fragile.mean() <= gc.GAUSS_FRAGILE_CAP and (hi[..., 3] > 0.5).mean() > 0.05
    assert d <= gc.GAUSS_DEV[name]
