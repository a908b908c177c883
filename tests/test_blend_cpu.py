"""CPU side of the blend tests (no GPU): the fp32 oracle against the float64 interval of tests/np_blend.py on the cases of
tests/blend_cases.py — the check, made without the kernel, that the derived interval is not too tight for an honest fp32
implementation —, the cap on what the comparison sets aside, and the mutants: deliberately wrong float64 blends of the same cases
that the comparison function of tests/test_gpu_blend.py has to reject."""
import numpy as np
import pytest

import blend_cases as bc
import np_blend as nb

F16 = 2.0 ** -11


def oracle(ob, ref, order, **kw):
    img, _ = ob.render(ob.make_frame(**dict(ref.frame_kw, **kw)), ref.inst, order=np.ascontiguousarray(order, np.uint32))
    return img


def check(ref, b, what, lo, hi, img):
    bad, ex, frac, width = nb.compare(lo, hi, b.n, img)
    print(f"blend {ref.name}, {what}: widest interval {width:.3e}, oracle at most {frac:.3f} of the half-width from the midpoint, "
          f"{int(ex.sum())} pixels excluded ({100 * ex.mean():.3f} %)")
    assert ex.mean() <= nb.EXCLUDE_CAP and not nb.whole_quarter_excluded(ex), (what, ex.mean())
    assert not bad.any(), f"{ref.name}, {what}\n" + nb.describe(b, img, lo, hi, bad, ref.order)


@pytest.mark.parametrize("name", bc.CASES)
def test_oracle_lies_in_the_interval(ob, name):
    """both draw directions of the oracle (back to front: colour and the additive alpha; front to back: colour and 1 - T, accumulated
    as A = 1 - T) in an fp32 target"""
    ref = bc.reference(ob, name)
    b = ref.blend()
    check(ref, b, "back to front, fp32 target", *b.image(alpha_sum=True), oracle(ob, ref, ref.order_btf))
    bf = ref.blend(t_abs=nb.U)
    check(ref, bf, "front to back, fp32 target", *bf.image(), oracle(ob, ref, ref.order, front_to_back=1))


@pytest.mark.parametrize("name", ["layers", "faint"])
def test_oracle_lies_in_the_interval_fp16_target(ob, name):
    """the RGBA16F target is rounded after every blend: the same derivation with the accumulates' unit roundoff 2^-11"""
    ref = bc.reference(ob, name)
    b = ref.blend(acc_u=F16)
    check(ref, b, "back to front, fp16 target", *b.image(alpha_sum=True), oracle(ob, ref, ref.order_btf, target_fp16=1))
    bf = ref.blend(acc_u=F16, t_abs=F16)
    check(ref, bf, "front to back, fp16 target", *bf.image(), oracle(ob, ref, ref.order, front_to_back=1, target_fp16=1))


@pytest.mark.parametrize("name", bc.CASES)
def test_oracle_lies_in_the_interval_under_an_occluder(ob, name):
    """a constant occluder depth in a gap of the key depths next to their median: the fragments with z <= D, the caller's colour
    under the remaining T (the oracle has no depth test: its frame of the filtered stream, plus T x colour in fp32)"""
    ref = bc.reference(ob, name)
    D, bg = ref.median_level(), ref.background()
    seen = ref.key_depth[ref.order] <= D
    assert seen.any() and not seen.all()
    f = oracle(ob, ref, ref.order[seen], front_to_back=1)
    f[..., :3] += (np.float32(1.0) - f[..., 3:4]) * bg[..., :3]
    b = ref.blend(occluder=True, t_abs=nb.U)
    check(ref, b, "occluder, front to back", *b.image(), f)
    a = oracle(ob, ref, ref.order[seen][::-1].copy())
    a[..., :3], a[..., 3] = f[..., :3], a[..., 3] + bg[..., 3]
    check(ref, b, "occluder, additive alpha", *b.image(alpha_sum=True), a)


@pytest.mark.parametrize("name", bc.SURFACE_CASES)
def test_oracle_picks_an_admissible_fragment(ob, name):
    ref = bc.reference(ob, name)
    """the picked (id, depth) is admissible, and the integrated normal (the oracle's own per-splat normals, not quantised, under
    the colour's weights) lies in its interval"""
    b = ref.blend(iso=bc.ISO, t_abs=nb.U, normals=True)
    depth, ids, nrm = ob.render_surface(ob.make_frame(**dict(ref.frame_kw, front_to_back=1)), ref.inst, ref.order, bc.ISO,
                                        quantize_normals=False, normals=True)
    bad = nb.compare_picks(b, np.where(depth == 0, nb.NONE_ID, ids), depth, ref.ndc_z)
    several = ((b.pick_ids >= 0).sum(axis=2) + b.pick_none > 1)
    print(f"blend {name}, surface: {int((ids != nb.NONE_ID).sum())} picks, {int(several.sum())} pixels with more than one admissible, "
          f"{int(b.pick_open.sum())} open")
    assert (depth != 0).any() and b.pick_open.mean() <= nb.EXCLUDE_CAP and several.mean() <= 0.05
    assert not bad.any(), nb.describe(b, np.stack([ids, depth], 2), b.lo, b.hi, bad, ref.order)
    assert np.abs(nrm[..., :3]).max() > 0.5
    check(ref, b, "integrated normal", b.nlo, b.nhi, nrm)


# ---- the cases have the structure they are named for ----------------------------------------------------------------------------------
def test_cases_have_their_structure(ob):
    lay = bc.reference(ob, "layers").blend()
    assert (lay.T_hi < nb.T_SAT).all()                      # every pixel saturates (behind the 6th layer) ...
    sat = bc.reference(ob, "layers").simulate(t_sat=1e-3)[0]
    assert (1.0 - sat[..., 3] > nb.T_SAT).all()            # ... and a retirement at 1e-3 stops all of them above 1e-4
    hole = bc.reference(ob, "hole")
    front = hole.order[hole.order < hole.total - bc.HOLE_BEHIND]    # the eight front layers alone
    q = (1.0 - hole.simulate(order=front)[0][..., 3])[bc.HOLE_QUARTER] < nb.T_SAT
    assert 96 <= q.sum() < 128 and not q[bc.HOLE[1] - 16, bc.HOLE[0] - 32], q.sum()   # 3/4 and more of the quarter saturate, the hole does not
    for name in ("second_batch", "faint"):
        assert (bc.reference(ob, name).blend().T_lo > 1e-3).all(), name               # nothing saturates
    sb = bc.reference(ob, "second_batch")
    t = sb.table
    ex, ey = np.hypot(t["b1"][:, 0], t["b2"][:, 0]), np.hypot(t["b1"][:, 1], t["b2"][:, 1])
    staged = int(((np.abs(t["c"][:, 0] - 16) <= ex + 15.5) & (np.abs(t["c"][:, 1] - 8) <= ey + 7.5)).sum())
    assert staged == bc.SECOND_BATCH_RECORDS > 512 and sb.blend().n.max() > 448
    part = bc.reference(ob, "partial")
    edge = part.blend()
    # the ragged last region column (x >= 320) holds saturated pixels next to live ones (the ragged last row holds live ones only)
    assert part.W % 32 and part.H % 16 and (edge.T_hi[:, 320:] < nb.T_SAT).any() and (edge.T_lo[:, 320:] > nb.T_SAT).any()
    assert (edge.n[208:] > 0).any()


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def rejected(ref, b, img, alpha_sum=False):
    lo, hi = b.image(alpha_sum)
    return bool(nb.compare(lo, hi, b.n, img)[0].any())


def frame_of(sim, alpha_sum=False):
    img, s, _ = sim
    if alpha_sum:
        img = img.copy()
        img[..., 3] = s
    return img


@pytest.mark.parametrize("name", bc.CASES)
def test_honest_retirement_is_accepted(ob, name):
    """simulate() with the kernel's own rule (all 128 pixels below 1e-4) lies in the interval, in both alpha modes"""
    ref = bc.reference(ob, name)
    b, sim = ref.blend(), ref.simulate()
    assert not rejected(ref, b, frame_of(sim)) and not rejected(ref, b, frame_of(sim, True), True)


MUTANTS = [("retires at T < 1e-3", "layers", dict(t_sat=1e-3), False),
           ("retires a quarter when any pixel is saturated", "hole", dict(share=0), False),
           ("retires a quarter when 3/4 of it are saturated", "hole", dict(share=0.75), False),
           ("drops record 288 of a region's staged list", "second_batch", dict(drop=288), False),
           ("drops record 512 of a region's staged list", "second_batch", dict(drop=512), False),
           ("drops record 448 of a region's staged list (additive)", "second_batch", dict(drop=448), True),
           ("cutoff 1/128 instead of 1/255", "faint", dict(alpha_min=1.0 / 128.0), False),
           ("additive alpha stops at saturation", "layers", dict(sum_stops=True), True)]


@pytest.mark.parametrize("what,name,kw,alpha_sum", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_mutant_is_rejected(ob, what, name, kw, alpha_sum):
    ref = bc.reference(ob, name)
    assert rejected(ref, ref.blend(), frame_of(ref.simulate(**kw), alpha_sum), alpha_sum), what


def test_mutant_swapped_pair_is_rejected(ob):
    """two adjacent records of the order swapped behind a layer of alpha 0.8: front layers 2 and 3 of "layers" """
    ref = bc.reference(ob, "layers")
    order = ref.order.copy()
    assert ref.table["opacity"][0] > 0.5 and set(order[:3].tolist()) == {0, 1, 2}
    order[[1, 2]] = order[[2, 1]]
    assert rejected(ref, ref.blend(), frame_of(ref.simulate(order=order)))


@pytest.mark.parametrize("name", bc.SURFACE_CASES)
def test_mutant_late_pick_is_rejected(ob, name):
    ref = bc.reference(ob, name)
    b = ref.blend(iso=bc.ISO)
    for late in (False, True):
        _, _, pid = ref.simulate(iso=bc.ISO, late_pick=late)
        depth = np.where(pid == nb.NONE_ID, 0.0, ref.ndc_z[np.where(pid == nb.NONE_ID, 0, pid)])
        assert bool(nb.compare_picks(b, pid, depth, ref.ndc_z).any()) == late, (name, late)
