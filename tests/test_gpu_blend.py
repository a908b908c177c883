"""GPU tests (-m gpu): the blend of k_composite — alpha in the folded form, the transmittance chain, the saturation rule and the wave's
retirement, the additive mode's switch to summing, the depth pick, the occluder's colour under the remaining T — held to the float64
interval of tests/np_blend.py on the cases of tests/blend_cases.py.  The interval is built from the records the frame itself
projected (mgs_frame_download_projected) and from the colours the scene holds (download_set), in the frame's own sorted order:
what is compared is the blend alone.  tests/test_blend_cpu.py shows from the CPU side that the oracle meets the same comparison, that
at most 1 % of a case's pixels are set aside, and that the comparison rejects every wrong blend it was built for.

The dependence on the device's records is closed here: Device.__init__ holds them to the oracle's own projection at the bars of
mixed_scene.check_projected_records, so a wrong record cannot hide in both the frame and its interval."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from vk_gaussian_splatting_amd import capi
import blend_cases as bc
import gpu_blend as gb
import np_blend as nb

pytestmark = pytest.mark.gpu


class Device:
    """one committed scene per case and, from its first frame, the device's own records as the splat table of the float64 blend"""

    def __init__(self, ob, name):
        self.name, self.ref = name, bc.reference(ob, name)
        self.scene = gb.build_scene(name)
        self.default, out, _ = gb.render(self.scene, name)
        assert out.error_flags == 0, out.error_flags
        # the frame's own sorted stream, nearest first: ties of the fp32 depth key fall in the library's storage order, which
        # test_depth_keys_cull_and_sort_bit_exact holds against the oracle; the blend is given the order the frame drew in
        _, ids = self.scene.sort_download(out.sorted_count)
        self.order = ids[::-1].copy()
        assert np.array_equal(np.sort(self.order), np.sort(self.ref.order[np.isin(self.ref.order, ids)])) and self.order.size > 0
        rec, _ = self.scene.download_projected(self.order)
        self.table = self.ref.table_of(self.order, rec.astype(np.float64))
        # the records against the oracle's projection (fp32 both; bars of mixed_scene.check_projected_records)
        t, o = self.table, self.ref.table
        mine, theirs = {int(g): r for r, g in enumerate(t["id"])}, {int(g): r for r, g in enumerate(o["id"])}
        both = sorted(set(mine) & set(theirs))
        # a splat the oracle projects but the frame did not sort (the front end culls footprints that reach no pixel) leaves no fragment
        gone = np.array(sorted(set(theirs) - set(mine)), np.int64)
        x0, x1, y0, y1 = nb._windows(o, self.ref.W, self.ref.H, 0.0)
        for g in gone:
            r = theirs[int(g)]
            if x1[r] >= x0[r] and y1[r] >= y0[r]:
                yy, xx = np.mgrid[y0[r]:y1[r] + 1, x0[r]:x1[r] + 1]
                assert not nb._fragment(o, r, xx, yy, 0.0)[1].any(), f"splat {g} leaves fragments but the frame did not sort it"
        assert len(both) > 0 and not set(mine) - set(int(g) for g in self.ref.order)
        a, b = np.array([mine[g] for g in both]), np.array([theirs[g] for g in both])

        def ext(tb, r):
            return np.einsum("ni,nj->nij", tb["b1"][r], tb["b1"][r]) + np.einsum("ni,nj->nij", tb["b2"][r], tb["b2"][r])
        Ew = ext(o, b)
        assert np.abs(t["c"][a] - o["c"][b]).max() <= 2e-3 and np.abs(t["opacity"][a] - o["opacity"][b]).max() <= 1e-5
        assert (np.abs(ext(t, a) - Ew) / np.abs(Ew).max(axis=(1, 2))[:, None, None]).max() <= 3e-3
        # colours and opacities as the committed scene holds them (dequantised), per instance, concatenated by global id
        self.rgba = np.concatenate([self.scene.download_set(k, 2, 4 * c).reshape(c, 4) for k, c in enumerate(self.ref.counts)]).astype(np.float64)
        assert self.rgba.shape[0] == self.ref.total

    @functools.lru_cache(maxsize=None)
    def blend(self, occluder=False, iso=None):
        """with iso: the integrated normal too, from the oracle's per-splat normals with the allowance for another fp32 evaluation"""
        return self.ref.blend(table=self.table, colours=self.rgba[:, :3], order=self.order, occluder=occluder, iso=iso,
                              normals="other" if iso is not None else False)

    def check(self, what, b, img, out, alpha_sum=False, normal=False):
        assert out is None or out.error_flags == 0, (what, out.error_flags)
        lo, hi = (b.nlo, b.nhi) if normal else b.image(alpha_sum)
        bad, ex, frac, width = nb.compare(lo, hi, b.n, img)
        print(f"blend {self.name}, {what}: widest interval {width:.3e}, kernel at most {frac:.3f} of the half-width from the midpoint, "
              f"{int(ex.sum())} pixels excluded ({100 * ex.mean():.3f} %)")
        assert ex.mean() <= nb.EXCLUDE_CAP and not nb.whole_quarter_excluded(ex), (what, ex.mean())
        assert not bad.any(), f"{self.name}, {what}\n" + nb.describe(b, img, lo, hi, bad, self.order)

    def check_picks(self, what, b, p):
        depth, ids, nrm = self.scene.download_surface(p, normals=True)
        bad = nb.compare_picks(b, ids, depth, self.ref.ndc_z)
        several = ((b.pick_ids >= 0).sum(axis=2) + b.pick_none > 1)
        print(f"blend {self.name}, {what}: {int((ids != nb.NONE_ID).sum())} picks, {int(several.sum())} pixels with more than one "
              f"admissible, {int(b.pick_open.sum())} pixels open")
        assert b.pick_open.mean() <= nb.EXCLUDE_CAP and several.mean() <= 0.05
        self.check(what + ", integrated normal", b, nrm, None, normal=True)
        assert not bad.any(), f"{self.name}, {what}\n" + nb.describe(b, np.stack([ids, depth], 2), b.lo, b.hi, bad, self.order)
        return ids


@pytest.fixture(scope="module")
def devices(ob):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Device(ob, name)
        return made[name]

    yield get
    for d in made.values():
        d.scene.close()


@pytest.mark.parametrize("name", bc.CASES)
def test_default_mode(devices, name):
    d = devices(name)
    d.check("default mode", d.blend(), d.default, None)


@pytest.mark.parametrize("name", bc.CASES)
def test_alpha_sum(devices, name):
    """the colour is the default mode's bit for bit; the additive alpha has its own interval (it never stops)"""
    d = devices(name)
    img, out, _ = gb.render(d.scene, name, alpha_mode=capi.ALPHA_SUM)
    assert np.array_equal(img[..., :3].view(np.uint32), d.default[..., :3].view(np.uint32))
    d.check("MGS_ALPHA_SUM", d.blend(), img, out, alpha_sum=True)


@pytest.mark.parametrize("alpha_sum", [False, True], ids=["default", "alpha_sum"])
@pytest.mark.parametrize("name", bc.CASES)
def test_surface_outputs(devices, name, alpha_sum):
    """the general walk: the image in its interval, every picked (id, depth) admissible"""
    d = devices(name)
    b = d.blend(iso=bc.ISO)
    img, out, p = gb.render(d.scene, name, surface_outputs=1, depth_iso_threshold=bc.ISO, quantize_normals=0, alpha_mode=capi.ALPHA_SUM if alpha_sum else 0)
    d.check("surface outputs", b, img, out, alpha_sum)
    ids = d.check_picks("surface outputs", b, p)
    assert (ids != nb.NONE_ID).any() or name not in bc.SURFACE_CASES


@pytest.mark.parametrize("surface", [0, 1], ids=["plain", "surface_outputs"])
@pytest.mark.parametrize("name", bc.CASES)
def test_occluder_at_the_median_level(devices, name, surface):
    """a constant occluder depth in a gap of the key depths with a caller colour image: the fragments with z <= D, the caller's
    colour under the remaining T; both alpha modes"""
    d = devices(name)
    ref = d.ref
    b = d.blend(occluder=True, iso=bc.ISO if surface else None)
    d.scene.upload_occluder(np.full((ref.H, ref.W), ref.median_level(), np.float32), ref.background())
    try:
        for alpha_sum in (False, True):
            img, out, p = gb.render(d.scene, name, surface_outputs=surface, depth_iso_threshold=bc.ISO, quantize_normals=0, alpha_mode=capi.ALPHA_SUM if alpha_sum else 0)
            d.check(f"occluder, surface outputs {surface}, alpha sum {alpha_sum}", b, img, out, alpha_sum)
            if surface:
                d.check_picks("occluder", b, p)
    finally:
        d.scene.clear_occluder()


@pytest.mark.parametrize("name", bc.CHILD_CASES)
def test_strips_are_bit_identical(devices, name):
    """tile rows of the frame rendered alone (they begin and end inside the frame's one bin): a long-lived wave's pixels must not
    depend on where the batches of a strip's frame fall"""
    d = devices(name)
    rows = (d.ref.H + 15) // 16
    for alpha_sum in (False, True):
        kw = dict(alpha_mode=capi.ALPHA_SUM) if alpha_sum else {}
        full, _, _ = gb.render(d.scene, name, **kw)
        for r in range(rows):
            img, out, _ = gb.render(d.scene, name, strip=(r, r + 1), **kw)
            assert out.error_flags == 0
            y0, y1 = 16 * r, min(16 * r + 16, d.ref.H)
            assert np.array_equal(img[y0:y1].view(np.uint32), full[y0:y1].view(np.uint32)), (name, alpha_sum, r)


@pytest.mark.parametrize("env", [{"MGS_DIRECT_BIN": "0"}, {"MGS_BIN_SHIFT": "1,0"}, {"MGS_DIRECT_BIN": "0", "MGS_BIN_SHIFT": "1,0"}],
                         ids=["pair_sort", "bins_32x16", "pair_sort_bins_32x16"])
def test_binning_paths_blend_the_same(devices, tmp_path, env):
    """the record + pair-sort path and 32x16-px bins (one region per bin) hand the compositor the same lists restricted to a bin: the
    frames lie in the same intervals"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_child_blend.py")
    e = {k: v for k, v in os.environ.items() if k not in ("MGS_DIRECT_BIN", "MGS_BIN_SHIFT")}
    e.update(env)
    out = str(tmp_path / "frames.npz")
    r = subprocess.run([sys.executable, child, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_DONE" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    with np.load(out) as z:
        for name in bc.CHILD_CASES:
            d = devices(name)
            for mode in ("default", "sum"):
                assert int(z[f"{name}/{mode}/flags"]) == 0
                d.check(f"{mode}, {env}", d.blend(), z[f"{name}/{mode}"], None, alpha_sum=mode == "sum")
