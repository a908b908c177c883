"""The per-splat radiance cases (radiance_cases.py) without a device: the builder's premises hold for every case, and the oracle's own
fp32 shading (orc_project) is compared with the float64 reference on all of them.  That comparison validates the cases and measures
K_REF, the yardstick of the device bar of test_gpu_radiance.py: this module holds the figure written in radiance_cases.py."""
import numpy as np
import pytest

import np_reference as npr
import radiance_cases as rc

SCENES = [("four", p) for p in rc.POSE_NAMES] + [("twenty", rc.TWENTY_POSE)]


def test_basis_suprema():
    """BMAX against a dense sample of the sphere: never below the sampled maximum, and within 1e-4 of it"""
    rng = np.random.Generator(np.random.PCG64(5))
    d = rng.standard_normal((400_000, 3))
    th, ph = np.meshgrid(np.linspace(0, np.pi, 721), np.linspace(0, 2 * np.pi, 1441))
    d = np.concatenate([d, np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1).reshape(-1, 3)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(15):
        sh = np.zeros((1, 15, 3))
        sh[0, k, 0] = 1.0
        b = np.abs(npr.sh_radiance(np.broadcast_to(sh, (d.shape[0], 15, 3)), 3, d)[:, 0]).max()
        assert b <= rc.BMAX[k] * (1 + 1e-12) and b >= rc.BMAX[k] * (1 - 1e-4), (k, b, rc.BMAX[k])


def test_layouts():
    four, twenty = rc.four_layout(), rc.twenty_layout()
    assert [d for d, _ in four] == [3, 0, 1, 2] and len(twenty) == 20 and {d for d, _ in twenty} == {0, 1, 2, 3}
    for _, M in four + twenty:
        s = np.linalg.svd(M[:3, :3].astype(np.float64), compute_uv=False)
        assert s.min() >= 0.25 * (1 - 1e-6) and s.max() <= 4.0 * (1 + 1e-6) and np.abs(M[:3, 3]).max() > 0
    assert sum(np.ptp(np.linalg.svd(M[:3, :3].astype(np.float64), compute_uv=False)) > 0.1 for _, M in four) == 4   # non-uniform, all four
    # instance 0: a rotation about (1, 1, 1), exactly representable
    M0 = four[0][1].astype(np.float64)
    R = M0[:3, :3] / np.linalg.norm(M0[:3, :3], axis=0)
    assert np.allclose(R @ np.ones(3), np.ones(3)) and np.isclose(np.linalg.det(R), 1.0) and not np.allclose(R, np.eye(3))
    assert np.array_equal(M0 * 4, np.round(M0 * 4))


@pytest.mark.parametrize("kind,pose", SCENES)
def test_builder_invariants(kind, pose):
    sc, g = rc.scene(kind, pose), rc.geometry(kind, pose)       # geometry() asserts the premises of the read-out
    n = g["read"].shape[0]
    assert n == rc.N == sc["cell"].size
    assert np.unique(g["read"], axis=0).shape[0] == n
    assert not rc.border_mask()[g["read"][:, 1], g["read"][:, 0]].any()
    assert np.ptp(g["dist"]) > 2.0                               # depths vary over the grid
    counts = [a["positions"].shape[0] for a, _ in sc["sets"]]
    assert min(counts) >= 8 and sum(counts) == n                 # the first and the last splat of every instance are read: all are
    for (a, _), d in zip(sc["sets"], sc["degrees"]):
        assert (a["f_rest"] is None) == (d == 0)
        assert d == 0 or a["f_rest"].shape[1] == 3 * rc.CPC[d]
        assert np.ptp(a["scale"], axis=1).max() == 0             # isotropic
    if kind == "four" and pose in ("+x", "-x", "+y", "-y", "+z", "-z"):
        # the splat at the image centre: its model-space view direction is an exact coordinate axis
        a, M = sc["sets"][0]
        i = int(np.flatnonzero(sc["cell"][:a["positions"].shape[0]] == 82)[0])
        assert tuple(g["read"][i]) == (127, 95)
        cam = (np.append(sc["eye"].astype(np.float64), 1.0) @ np.linalg.inv(M.astype(np.float64)).T)[:3]
        d = a["positions"][i].astype(np.float64) - cam
        assert np.count_nonzero(d) == 1, d


def test_every_coefficient_and_channel_is_alone_somewhere():
    seen = set()
    for pose in rc.POSE_NAMES:
        sc = rc.scene("four", pose)
        at = 0
        for (a, _), d in zip(sc["sets"], sc["degrees"]):
            n = a["positions"].shape[0]
            for i in np.flatnonzero(sc["single"][at:at + n] >= 0):
                fr = a["f_rest"][i].reshape(3, rc.CPC[d])
                ch, k = np.nonzero(fr)
                assert ch.size == 1 and abs(fr[ch[0], k[0]]) >= 0.35
                seen.add((int(k[0]), int(ch[0])))
            at += n
    assert seen == {(k, ch) for k in range(15) for ch in range(3)}


def test_negative_radiance_and_band_three_weight():
    rgb, _ = rc.reference("four", "+x", "f32", 3)
    assert (rgb < -0.05).any(axis=0).all()                       # negative in every channel somewhere
    lo, _ = rc.reference("four", "+x", "f32", 2)
    n0 = rc.scene("four", "+x")["sets"][0][0]["positions"].shape[0]
    assert np.abs(rgb[:n0] - lo[:n0]).max() > 0.2                # band 3 carries weight on the degree-3 set
    assert np.array_equal(rgb[n0:], lo[n0:])                     # ... and nothing on the others


def test_ray_batch():
    r = rc.rays()                                                # rays() asserts lengths, origins and isolation
    assert r["origin"].shape == (rc.N, 3) and r["exact"].sum() == 14
    md = r["model_dir"][r["exact"]]
    ax = md[np.count_nonzero(md, axis=1) == 1]
    assert sorted(map(tuple, ax)) == sorted(map(lambda t: tuple(map(float, t)), rc.AXES))
    oc = md[np.count_nonzero(md, axis=1) == 3]
    assert oc.shape[0] == 8 and np.unique(np.sign(oc), axis=0).shape[0] == 8 and np.ptp(np.abs(oc)) == 0
    free = r["model_dir"][~r["exact"]]
    assert all((free @ np.asarray(o, np.float64) > 0.5).any() for o in rc.AXES)   # the spread reaches every side of the sphere


def _oracle_rgb(ob, kind, pose, fmt, sh_degree, flags, origins=None):
    sc = rc.scene(kind, pose)
    pss = rc.prepared(kind, pose, fmt)
    inst = ob.make_instances([(ps, M) for ps, (_, M) in zip(pss, sc["sets"])])
    fr = ob.make_frame(sc["V"], sc["P"], sc["eye"], rc.W, rc.H, sh_degree=sh_degree, debug_flags=flags)
    out, at = [], 0
    for k, ps in enumerate(pss):
        for i in range(ps.count):
            if origins is not None:
                fr = ob.make_frame(sc["V"], sc["P"], origins[at + i], rc.W, rc.H, sh_degree=sh_degree, debug_flags=flags)
            q = ob.project(fr, inst, k, i)
            assert q.valid
            out.append([q.rgba[0], q.rgba[1], q.rgba[2]])
        at += ps.count
    return np.array(out, np.float64)


def test_oracle_fp32_against_float64(ob):
    """K_REF = max |oracle fp32 - float64| / u over every case the device test reads: all scenes, storage formats and frame degrees, the
    SH-only variant and the ray batch (the oracle shades from a camera position: the ray's origin is handed in as one)"""
    worst = 0.0
    for fmt in rc.FORMATS:
        for kind, pose in SCENES:
            for deg in range(4):
                for sh_only in ((False, True) if pose == rc.EXTRAS_POSE and kind == "four" and deg == 3 else (False,)):
                    want, u = rc.reference(kind, pose, fmt, deg, sh_only)
                    got = _oracle_rgb(ob, kind, pose, fmt, deg, 4 | (2 if sh_only else 0))
                    k = float(rc.in_units(np.abs(got - want), u).max())
                    worst = max(worst, k)
        for deg, sh_only in ((0, False), (1, False), (2, False), (3, False), (3, True)):
            want, u = rc.ray_reference(fmt, deg, sh_only)
            got = _oracle_rgb(ob, "four", rc.EXTRAS_POSE, fmt, deg, 4 | (2 if sh_only else 0), origins=rc.rays()["origin"])
            k = float(rc.in_units(np.abs(got - want), u).max())
            worst = max(worst, k)
        print(f"{fmt}: K_ref so far {worst:.3f}")
    print(f"K_ref = {worst:.3f} (radiance_cases.K_REF = {rc.K_REF}, K = {rc.K})")
    assert worst <= rc.K_REF
    assert rc.K == 2 ** int(np.ceil(np.log2(4 * rc.K_REF))) and rc.K <= 64
