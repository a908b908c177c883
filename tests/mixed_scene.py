"""Scenes made of several DIFFERENT splat sets (test helper, not a test module): the sets, the scene builder and the
per-splat projected-record check shared by test_gpu_mixed_sets.py and test_gpu_fullsize.py.

Every other GPU test adds one SplatSet object again and again, and mgs_instance_add de-duplicates sets by their handle, so
those scenes hold one DeviceSet: same count, SH degree, storage order and buffers in every instance.  The scenes here mix
splat counts around the 2048-splat partition, SH degrees 0..3 (degree 0 without SH: sh == nullptr on the device) and
storage permutations, and reuse one set in two instances."""
import numpy as np

import vk_gaussian_splatting_amd as mgs
from vk_gaussian_splatting_amd import capi, synth

CPC = {0: 0, 1: 3, 2: 8, 3: 15}   # f_rest coefficients per channel of an SH degree


def make_set(n, seed, degree):
    """a synthetic set of the given SH degree; degree 0 has f_rest = None (no SH buffer at all)"""
    sc = synth.make_scene(n, seed=seed, sh_coeffs_per_channel=CPC[degree])
    if degree == 0:
        sc["f_rest"] = None
    return sc


def one_big_splat():
    """set B: one large, nearly opaque, anisotropic splat of SH degree 0"""
    rot = np.array([[0.9, 0.1, 0.3, 0.2]], np.float32)
    return dict(positions=np.zeros((1, 3), np.float32), f_dc=np.array([[1.4, -0.9, 0.6]], np.float32), f_rest=None,
                opacity=np.array([3.5], np.float32), scale=np.log(np.array([[0.30, 0.18, 0.24]], np.float32)),
                rotation=rot / np.linalg.norm(rot))


def distinct_sets():
    """A: 3*2048 + 777 (degree 3, partial last partition), B: 1 splat (degree 0), C: exactly 2048 (degree 1),
    D: 2049 (degree 2, one splat into a second partition), E: 30 000 (degree 3, other buffers than A)"""
    return dict(A=make_set(3 * 2048 + 777, 101, 3), B=one_big_splat(), C=make_set(2048, 102, 1), D=make_set(2049, 103, 2),
                E=make_set(30_000, 104, 3))


def projective(M, a=1.0e-3, b=-5.0e-4):
    """M with a last row that is not (0, 0, 0, 1): modelIsAffine is false for it"""
    M = np.array(M, np.float32, copy=True)
    M[3, 2], M[3, 0] = a, b
    return M


def mixed_layout():
    """[(set name, transform)] of the six-instance scene: A twice (de-duplicated) among four other sets; identity,
    affine TRS and one projective model"""
    T = lambda s, r, t: mgs.compute_transform(s, r, t)[0]
    return [("A", None),
            ("B", T([1.0, 1.0, 1.0], [0.0, 25.0, 0.0], [0.2, 1.3, 0.4])),
            ("C", T([0.7, 0.7, 0.7], [0.0, 30.0, 0.0], [1.5, 0.2, -1.0])),
            ("D", projective(T([0.9, 1.1, 1.0], [10.0, -20.0, 5.0], [-1.2, 0.0, 0.8]))),
            ("A", T([1.2, 0.8, 1.0], [0.0, -40.0, 15.0], [-1.5, -0.3, -1.2])),
            ("E", T([1.0, 1.0, 1.0], [5.0, 60.0, 0.0], [0.5, 0.1, 1.5]))]


class MixedScene:
    """a committed mgs.Scene over [(set name, transform)] plus what the oracle needs to follow it"""

    def __init__(self, sets, layout, sh_format=capi.FORMAT_FLOAT32, rgba_format=capi.FORMAT_FLOAT32):
        self.sets, self.layout = sets, list(layout)
        self.handles = {name: mgs.SplatSet.from_arrays(**sets[name]) for name in {nm for nm, _ in self.layout}}
        self.scene = mgs.Scene(0)
        for name, M in self.layout:
            self.scene.add_instance(self.handles[name], M)
        self.scene.commit(sh_format, rgba_format)
        self.sh_format, self.rgba_format = sh_format, rgba_format
        self.counts = [sets[name]["positions"].shape[0] for name, _ in self.layout]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        assert self.scene.splat_count == self.offsets[-1]
        self.perms = [self.scene.storage_order(i, c) for i, c in enumerate(self.counts)]

    def transforms(self):
        return [M for _, M in self.layout]

    def set_transform(self, i, M):
        self.scene.set_transform(i, M)
        self.layout[i] = (self.layout[i][0], M)

    def oracle_stream(self, ob, frame):
        """(keys, caller ids, storage ids, oracle instances in storage order) of the oracle's stable sort"""
        insts = [(self.sets[name], perm, M) for (name, M), perm in zip(self.layout, self.perms)]
        return ob.storage_sorted_stream(frame, insts, self.sh_format, self.rgba_format)

    def instance_of(self, global_ids):
        return np.searchsorted(self.offsets, np.asarray(global_ids, np.int64), side="right") - 1

    def close(self):
        self.scene.close()
        for h in self.handles.values():
            h.close()


def check_projected_records(ob, fr, inst_s, sids, inst_k, rec, rect, W, H, label, bins=(256, 128), records=True):
    """the projected per-splat records of the frame (download_projected, in the order of the sorted stream) against
    orc_project, at the tolerances of test_projected_records_match_oracle_per_splat, WORST SPLAT PER INSTANCE (a wrong
    instance offset shows up in one instance only).  sids: oracle storage ids aligned with rec; inst_k: their instance;
    inst_s: the oracle's storage-order instances.  records=False: the bin-rectangle containment alone (the record levels
    are printed)."""
    want = np.zeros((sids.size, 7))
    offs = {}
    for j, s in enumerate(sids):
        k = int(inst_k[j])
        if k not in offs:
            offs[k] = sum(int(inst_s[q].count) for q in range(k))
        q = ob.project(fr, inst_s, k, int(s) - offs[k])
        assert q.valid, f"{label}: splat {s} of instance {k} was sorted by the frame but the oracle rejects it"
        want[j] = [q.center_px[0], q.center_px[1], q.basis1[0], q.basis1[1], q.basis2[0], q.basis2[1], q.rgba[3]]
    got = rec[:, :7].astype(np.float64)

    def ext(b):
        return np.einsum("ni,nj->nij", b[:, 2:4], b[:, 2:4]) + np.einsum("ni,nj->nij", b[:, 4:6], b[:, 4:6])
    Ew = ext(want)
    eall = (np.abs(ext(got) - Ew) / np.abs(Ew).max(axis=(1, 2))[:, None, None]).max(axis=(1, 2))
    cerr = np.abs(got[:, :2] - want[:, :2]).max(axis=1)
    aerr = np.abs(got[:, 6] - want[:, 6])
    l1, l2 = np.hypot(want[:, 2], want[:, 3]), np.hypot(want[:, 4], want[:, 5])
    gl1, gl2 = np.hypot(got[:, 2], got[:, 3]), np.hypot(got[:, 4], got[:, 5])
    for k in np.unique(inst_k):
        m = inst_k == k
        print(f"{label}: instance {k}: {int(m.sum())} records, worst centre {cerr[m].max():.2e} px, opacity {aerr[m].max():.2e}, "
              f"extent matrix rel {eall[m].max():.2e}, lengths rel {max(np.abs(gl1[m] / l1[m] - 1).max(), np.abs(gl2[m] / l2[m] - 1).max()):.2e}")
    # bars of test_projected_records_match_oracle_per_splat (fp32 FMA-contracted vs unfused IEEE)
    if records:
        assert cerr.max() <= 2e-3 and aerr.max() <= 1e-5
        assert eall.max() <= 3e-3 and np.percentile(eall, 99) <= 5e-5 and np.percentile(eall, 99.9) <= 2e-4
        assert np.allclose(gl1, l1, rtol=1e-4) and np.allclose(gl2, l2, rtol=1e-4)
    # the conservative extents and the bin rectangle contain the visible footprint's box
    ex, ey = rec[:, 7].astype(np.float64), rec[:, 8].astype(np.float64)
    shrink = np.sqrt(np.minimum(4.0, np.log(np.maximum(want[:, 6] * 255.0, 1.0))) / 4.0)
    exw, eyw = shrink * np.hypot(want[:, 2], want[:, 4]) * 0.999, shrink * np.hypot(want[:, 3], want[:, 5]) * 0.999
    assert np.all(ex >= exw) and np.all(ey >= eyw)
    bw, bh = bins
    bxn, byn = (W + bw - 1) // bw, (H + bh - 1) // bh
    x0b, y0b = (rect & 255).astype(np.int64), ((rect >> 8) & 255).astype(np.int64)
    x1b, y1b = ((rect >> 16) & 255).astype(np.int64), (rect >> 24).astype(np.int64)
    assert np.all(x0b <= x1b) and np.all(y0b <= y1b) and np.all(x1b < bxn) and np.all(y1b < byn)
    fx0, fx1 = np.ceil(want[:, 0] - exw - 0.5), np.floor(want[:, 0] + exw - 0.5)
    fy0, fy1 = np.ceil(want[:, 1] - eyw - 0.5), np.floor(want[:, 1] + eyw - 0.5)
    vis = (fx1 >= fx0) & (fy1 >= fy0) & (fx1 >= 0) & (fx0 <= W - 1) & (fy1 >= 0) & (fy0 <= H - 1)
    cx0, cx1 = np.clip(fx0, 0, W - 1), np.clip(fx1, 0, W - 1)
    cy0, cy1 = np.clip(fy0, 0, H - 1), np.clip(fy1, 0, H - 1)
    assert np.all((x0b * bw <= cx0)[vis]) and np.all(((x1b + 1) * bw > cx1)[vis])
    assert np.all((y0b * bh <= cy0)[vis]) and np.all(((y1b + 1) * bh > cy1)[vis])
    # tight as well: the rectangle is the box of the kernel's own (fp16-rounded-up) extents at most
    gx0, gx1 = np.clip(np.ceil(got[:, 0] - ex - 0.5), 0, W - 1), np.clip(np.floor(got[:, 0] + ex - 0.5), 0, W - 1)
    gy0, gy1 = np.clip(np.ceil(got[:, 1] - ey - 0.5), 0, H - 1), np.clip(np.floor(got[:, 1] + ey - 0.5), 0, H - 1)
    assert np.all((x0b >= gx0 // bw)[vis]) and np.all((x1b <= gx1 // bw)[vis])
    assert np.all((y0b >= gy0 // bh)[vis]) and np.all((y1b <= gy1 // bh)[vis])
    return want, vis
