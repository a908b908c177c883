"""np_hierarchy.py checked on the CPU, and the finding the GPU test rests on: an fp32 numpy emulation of k_bvh_leaves' arithmetic
(unfused; contraction changes the bits, not the class of error) with the formula the kernel had, and of the double path it has now.

The inflation the kernel had, 8 ulps of the half extent + 2 ulps of |c|, FAILS containment on group d (the centre's transform rounds
at the magnitude of its terms, about 1e3, while |c| is about 1) and on group e for low degrees (kmr / density just below the clamp:
the quotient's rounding, a quarter ulp of 1, is amplified by 1 / (n |ln 0.97|) in the radius) wherever the centre's own 2 ulps do not
happen to hide it; on group b the rotation's rounding alone is worth more than 1e3 ulps of a half extent.  The present box, that one
united with the double evaluation rounded outward (restated here on its own and held to a long-double reference), holds containment and tightness on every group, degree and clamping mode."""
import os
import re

import numpy as np
import pytest

import hierarchy_cases as hc
import np_hierarchy as nh
import np_mesh_rays as nr
from vk_gaussian_splatting_amd import capi

F = np.float32
ULP = F(1.1920929e-7)
OLD = (F(8), F(2), False)   # (ulps of the half extent, ulps of the centre term, centre term = sum of |terms| instead of |c|)
NEW = "double"              # the double evaluation, h widened by 8 ulps of h + 2 ulps of T + SLACK * 2^-53 * (h + T), rounded outward
SLACK = 64.0


def double_leaves(pl, M, degree, kmr, adaptive):
    """leafBoundDouble of k_bvh.hip in float64 numpy, in the kernel's order of operations (its own normalisation, rotation, pow / log /
    exp and sums, none of np_hierarchy's) -> (c, h, T) [n, 3]"""
    M = np.asarray(M, F).astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.asarray(pl["quats"], F).astype(np.float64)
        ql = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        w, x, y, z = (q[:, i] / ql for i in range(4))
        R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
             [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
        dens = np.asarray(pl["density"], F).astype(np.float64)
        thr = np.minimum(np.float64(F(kmr)) / dens if adaptive else np.full_like(dens, np.float64(F(kmr))), np.float64(F(0.97)))
        if degree == 0:
            r = (1.0 - thr) / 0.329630334487
        else:
            n = float(degree)
            r = np.power(np.log(thr) / (-4.5 / np.power(3.0, n)), 1.0 / n)
        rs = r[:, None] * np.exp(np.asarray(pl["scales"], F).astype(np.float64))
        p = np.asarray(pl["centers"], F).astype(np.float64)
        c, h, T = np.empty_like(p), np.empty_like(p), np.empty_like(p)
        for ax in range(3):
            acc = np.zeros_like(dens)
            for j in range(3):
                e = (M[ax, 0] * R[0][j] + M[ax, 1] * R[1][j] + M[ax, 2] * R[2][j]) * rs[:, j]
                acc = acc + e * e
            h[:, ax] = np.sqrt(acc)
            t = [M[ax, 0] * p[:, 0], M[ax, 1] * p[:, 1], M[ax, 2] * p[:, 2], np.full_like(dens, M[ax, 3])]
            c[:, ax] = t[0] + t[1] + t[2] + t[3]
            T[:, ax] = np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]) + np.abs(t[3])
    return c, h, T


def emulate_leaves(pl, M, degree, kmr, adaptive, cull, formula, raw=False):
    """k_bvh_leaves in fp32 numpy, operation for operation and unfused -> (lo [n, 3], hi [n, 3] fp32, ok [n]); raw: the centre and
    the half extent before the inflation in place of lo and hi"""
    kh, kc, terms = formula
    M = np.asarray(M, F)
    p, dens = np.asarray(pl["centers"], F), np.asarray(pl["density"], F)
    with np.errstate(all="ignore"):
        s = np.exp(np.asarray(pl["scales"], F))
        q = np.asarray(pl["quats"], F)
        ql = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        w, x, y, z = (q[:, i] / ql for i in range(4))
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        one, two = F(1), F(2)
        R = [[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)], [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
             [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]]
        thr = np.minimum(F(kmr) / dens if adaptive else np.full_like(dens, F(kmr)), F(0.97))
        if degree == 0:
            r = (one - thr) / F(0.329630334487)
        else:
            n = F(degree)
            r = np.power(np.log(thr) / (F(-4.5) / np.power(F(3), n)), one / n)
        lo, hi, ok = np.empty_like(p), np.empty_like(p), dens > F(cull)
        for ax in range(3):
            acc = np.zeros_like(dens)
            for j in range(3):
                mr = M[ax, 0] * R[0][j] + M[ax, 1] * R[1][j] + M[ax, 2] * R[2][j]
                e = mr * (r * s[:, j])
                acc = acc + e * e
            h = np.sqrt(acc)
            c = M[ax, 0] * p[:, 0] + M[ax, 1] * p[:, 1] + M[ax, 2] * p[:, 2] + M[ax, 3]
            t = np.abs(M[ax, 0] * p[:, 0]) + np.abs(M[ax, 1] * p[:, 1]) + np.abs(M[ax, 2] * p[:, 2]) + np.abs(M[ax, 3]) if terms else np.abs(c)
            hh = h * (one + kh * ULP) + t * (kc * ULP)
            lo[:, ax], hi[:, ax] = (c, h) if raw else (c - hh, c + hh)
            ok = ok & np.isfinite(lo[:, ax]) & np.isfinite(hi[:, ax]) & (hh >= 0)
    assert lo.dtype == F and hi.dtype == F
    return lo, hi, ok


def planes_of(sets, cull_from=None):
    """[(storage planes, M)] of a splat scene with the identity as storage order, and the cull threshold"""
    out = [(hc.storage_planes(a, np.arange(a["positions"].shape[0])), M) for a, M in sets]
    cull = hc.CULL if cull_from is None else out[0][0]["density"][cull_from]
    return out, cull


def emulated_margins(name, degree, adaptive, formula):
    """-> (margin [leaves, 6] of the emulated boxes over the float64 boxes, h, bound, valid-set agreement)"""
    pls, cull = planes_of(hc.splat_groups()[name], hc.E_CULL_FROM if name == "e_thresholds" else None)
    ref = nh.scene_splats(pls, degree, hc.KMR, adaptive, cull)
    if formula is NEW:   # the double path restated on its own (double_leaves), not taken from the reference it is held to
        cd, hd, Td = (np.concatenate(x) for x in zip(*[double_leaves(pl, M, degree, hc.KMR, adaptive) for pl, M in pls]))
        with np.errstate(all="ignore"):
            hh = hd * (1.0 + 8.0 * 2.0 ** -23) + Td * (2.0 * 2.0 ** -23) + SLACK * 2.0 ** -53 * (hd + Td)
            xl, xu = cd - hh, cd + hh
            lo, hi = xl.astype(F), xu.astype(F)
            lo = np.where(lo.astype(np.float64) > xl, np.nextafter(lo, F(-np.inf)), lo)
            hi = np.where(hi.astype(np.float64) < xu, np.nextafter(hi, F(np.inf)), hi)
            ok = (np.concatenate([pl["density"] for pl, _ in pls]) > F(cull)) & np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
    else:
        parts = [emulate_leaves(pl, M, degree, hc.KMR, adaptive, cull, formula) for pl, M in pls]
        lo, hi, ok = (np.concatenate(x) for x in zip(*parts))
    v = ref["valid"]
    nodes = np.zeros((int(v.sum()), 8), np.uint32)
    nodes[:, 0:3], nodes[:, 4:7], nodes[:, 3] = lo[v].view(np.uint32), hi[v].view(np.uint32), np.nonzero(v)[0]
    return nh.splat_containment(nodes, ref), np.array_equal(ok, v)


def test_the_hook_is_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mgs.h")).read()
    assert re.search(r"\bmgs_debug_download_hierarchy\(", hdr) and "#define MGS_HAS_DEBUG_HIERARCHY 1" in hdr
    assert "mgs_debug_download_hierarchy" in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), "mgs_debug_download_hierarchy")
    import ctypes
    assert ctypes.sizeof(capi.HierarchyInfo) == 4 * (4 + 11 + 11 + 3 + 3)


@pytest.mark.parametrize("degree", nh.DEGREES)
def test_radius_inverts_the_forward_response(degree):
    thr = np.concatenate([np.geomspace(1e-6, 0.9, 400), np.linspace(0.9, nh.CLAMP, 100)[1:]])
    r = nh.proxy_radius(degree, thr)
    assert (r > 0).all() and (np.diff(r) < 0).all()
    assert (np.abs(nh.response(degree, r) - thr) <= 1e-12 * thr + 1e-15).all()
    # and the threshold: clamped at 0.97f, divided by the density only with adaptive clamping
    d = np.array([0.004, 0.0116, 0.0117, 0.5, 1.0], np.float32)
    assert np.array_equal(nh.proxy_threshold(hc.KMR, d, 0), np.full(5, np.float64(hc.KMR)))
    assert np.allclose(nh.proxy_threshold(hc.KMR, d, 1), np.minimum(np.float64(hc.KMR) / d.astype(np.float64), nh.CLAMP), rtol=0, atol=0)


@pytest.mark.parametrize("name", ["b_anisotropic", "c_affine", "d_cancelling"])
def test_ellipsoid_box_against_a_dense_sampling_of_the_surface(name):
    """x = M (p + R diag(r s) u) over 200 000 unit vectors u: no sample outside the box, and the samples reach every face to within the
    sampling's own resolution (the nearest of N random directions to a given one is within about 2 / sqrt(N) rad: 1 - cos < 1e-4)"""
    r = np.random.Generator(np.random.PCG64(5))
    u = r.standard_normal((200_000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for a, M in hc.splat_groups()[name]:
        pl = hc.storage_planes(a, np.arange(0, a["positions"].shape[0], 37))
        c, h, _ = nh.ellipsoid_boxes(pl["centers"], pl["scales"], pl["quats"], pl["density"], M, 2, hc.KMR, 1)
        Md = np.asarray(M, np.float32).astype(np.float64)
        rad = nh.proxy_radius(2, nh.proxy_threshold(hc.KMR, pl["density"], 1))
        Rm = nh.rotations(pl["quats"])
        for i in range(c.shape[0]):
            local = (u * (np.exp(pl["scales"][i].astype(np.float64)) * rad[i])) @ Rm[i].T      # R diag(r s) u, about the centre
            x = local @ Md[:3, :3].T                                                           # the affine image, about M p
            ext = np.abs(x).max(0)
            assert (ext <= h[i] * (1 + 1e-12)).all() and (ext >= h[i] * (1 - 1e-4)).all(), (name, i)
        # the canonical distance of the surface is the radius: the response there is the threshold
        assert np.allclose(nh.response(2, rad), nh.proxy_threshold(hc.KMR, pl["density"], 1), rtol=1e-12)


def test_the_old_inflation_fails_containment_on_the_cancelling_transform():
    m, same = emulated_margins("d_cancelling", 2, 1, OLD)
    worst = m["margin"][:hc.D_N].min()
    inside = (m["margin"][:hc.D_N] >= 0).all(1)
    print(f"old formula, d_cancelling: worst face {worst:.3e} (negative = the exact box sticks out), boxes that contain: {inside.mean():.1%}")
    assert same and worst < -1e-5 and inside.mean() < 0.5


@pytest.mark.parametrize("name", list(hc.splat_groups()))
def test_the_present_inflation_holds_containment_and_tightness(name):
    worst_m, worst_x = np.inf, 0.0
    for degree, adaptive in hc.PROXIES:
        m, same = emulated_margins(name, degree, adaptive, NEW)
        assert same, (degree, adaptive)
        if m["margin"].size == 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            ulps, ratio = m["margin"] / (2 * nh.EPS * m["h"]), m["margin"] / m["bound"]
        worst_m, worst_x = min(worst_m, ulps.min()), max(worst_x, ratio.max())
        assert (m["margin"] >= 0).all(), (degree, adaptive, ulps.min())
        assert (m["margin"] <= m["bound"]).all(), (degree, adaptive, ratio.max())
    print(f"{name}: worst containment margin {worst_m:.2f} ulps of h, worst excess / bound {worst_x:.3f}")


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2.0 ** -60, reason="needs an extended-precision long double")
@pytest.mark.parametrize("name", ["b_anisotropic", "c_affine", "d_cancelling", "e_thresholds"])
def test_the_double_path_lies_within_its_slack_of_an_extended_precision_reference(name):
    """leafBoundDouble restated in float64 (double_leaves) against np_hierarchy evaluated in long double, on the groups where the
    double path's own errors are largest (cancellation, anisotropy, the clamp): the faces differ by less than SLACK * 2^-53 * (h + T),
    so the slack the kernel subtracts covers its evaluation; and np_hierarchy's own float64 lies as close, so it may serve as the
    reference.  Printed: the worst difference in units of 2^-53 * (h + T)."""
    L = np.longdouble
    worst = 0.0
    for degree, adaptive in hc.PROXIES:
        pls, cull = planes_of(hc.splat_groups()[name], hc.E_CULL_FROM if name == "e_thresholds" else None)
        for pl, M in pls:
            cx, hx, _ = nh.ellipsoid_boxes(pl["centers"], pl["scales"], pl["quats"], pl["density"], M, degree, hc.KMR, adaptive, dtype=L)
            cr, hr, Tr = nh.ellipsoid_boxes(pl["centers"], pl["scales"], pl["quats"], pl["density"], M, degree, hc.KMR, adaptive)
            cd, hd, Td = double_leaves(pl, M, degree, hc.KMR, adaptive)
            v = nh.splat_valid(pl["density"], cull, cr, hr)
            unit = (2.0 ** -53 * (hr + Tr))[v]
            for c, h in ((cd, hd), (cr, hr)):
                err = np.maximum(np.abs((c - h).astype(L) - (cx - hx)), np.abs((c + h).astype(L) - (cx + hx)))[v].astype(np.float64) / unit
                worst = max(worst, float(err.max()))
            assert np.allclose(Td[v], Tr[v], rtol=1e-15)
    print(f"{name}: double evaluation off by at most {worst:.1f} x 2^-53 (h + T)")
    assert worst < SLACK / 2


def test_what_no_count_of_ulps_covers():
    """the three errors of the fp32 evaluation that the kernel's comment names, measured on the emulation: the half extent's in ulps
    (2^-23) of itself, the centre's in ulps of |c| and of the sum of its terms"""
    worst = {}
    for name in ("b_anisotropic", "d_cancelling", "e_thresholds", "a_isotropic"):
        for degree, adaptive in hc.PROXIES:
            pls, cull = planes_of(hc.splat_groups()[name], hc.E_CULL_FROM if name == "e_thresholds" else None)
            ref = nh.scene_splats(pls, degree, hc.KMR, adaptive, cull)
            parts = [emulate_leaves(pl, M, degree, hc.KMR, adaptive, cull, OLD, raw=True) for pl, M in pls]
            c, h, _ = (np.concatenate(x) for x in zip(*parts))
            v = ref["valid"]
            eh = (np.abs(h[v].astype(np.float64) - ref["h"][v]) / (2 * nh.EPS * ref["h"][v])).max()
            dc = np.abs(c[v].astype(np.float64) - ref["c"][v])
            w = worst.setdefault(name, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], eh), max(w[1], (dc / (2 * nh.EPS * np.abs(ref["c"][v]))).max()), max(w[2], (dc / (2 * nh.EPS * ref["T"][v])).max())
    for name, w in worst.items():
        print(f"{name}: half extent off by {w[0]:.1f} ulps of h; centre off by {w[1]:.1f} ulps of |c|, {w[2]:.2f} ulps of the sum of its terms")
    assert worst["a_isotropic"][0] < 4 and worst["b_anisotropic"][0] > 100 and worst["e_thresholds"][0] > 8
    assert worst["d_cancelling"][1] > 100 and worst["d_cancelling"][2] < 1


@pytest.mark.parametrize("n", hc.COUNTS)
def test_tree_shape_and_the_node_checks_on_a_numpy_tree(n):
    levels, total, off, cnt = nh.tree_shape(n)
    assert cnt[0] == n and (levels == 0) == (n == 0) and levels <= 6 and (n == 0 or cnt[levels - 1] == 1)
    assert all(cnt[l] == -(-int(cnt[l - 1]) // 8) and off[l] == off[l - 1] + cnt[l - 1] for l in range(1, levels))
    r = np.random.Generator(np.random.PCG64(n))
    lo = r.uniform(-1, 1, (n, 3)).astype(F)
    level = np.zeros((n, 8), F)
    level[:, 0:3], level[:, 4:7] = lo, lo + F(0.1)
    level[:, 3] = np.arange(n, dtype=np.uint32).view(F)
    parts = [level]
    for l in range(1, levels):
        b, pad = parts[-1], (-parts[-1].shape[0]) % 8
        up = np.zeros((int(cnt[l]), 8), F)
        up[:, 0:3] = np.concatenate([b[:, 0:3], np.full((pad, 3), np.inf, F)]).reshape(-1, 8, 3).min(1)
        up[:, 4:7] = np.concatenate([b[:, 4:7], np.full((pad, 3), -np.inf, F)]).reshape(-1, 8, 3).max(1)
        parts.append(up)
    nodes = np.concatenate(parts).view(np.uint32)
    info = dict(levels=levels, total_nodes=total, leaves=n, level_offset=off, level_count=cnt)
    nh.check_nodes(info, nodes, n)
    if levels > 1:   # the check bites: a parent one ulp too tight
        bad = nodes.copy()
        bad[int(off[1]), 4] ^= 1
        with pytest.raises(AssertionError):
            nh.check_nodes(info, bad, n)


def reference_order(centre, lo, inv):
    return np.argsort(nh.morton(nh.quantised(centre, lo, inv)), kind="stable")


def frame_of(points):
    lo, hi = points.min(0), points.max(0)
    with np.errstate(divide="ignore"):
        return lo.astype(F), np.where(hi > lo, 1.0 / (hi - lo), 0.0).astype(F)


def test_the_cases_keep_the_excused_pairs_under_the_cap():
    scenes = dict(hc.splat_groups(), **{f"count_{n}": hc.count_scene(n) for n in hc.COUNTS})
    for name, sets in scenes.items():
        pls, cull = planes_of(sets, hc.E_CULL_FROM if name == "e_thresholds" else None)
        ref = nh.scene_splats(pls, 2, hc.KMR, 1, cull)
        if not ref["valid"].any():
            continue
        lo, inv = hc.morton_frame([(a["positions"], M) for a, M in sets])
        ids = np.nonzero(ref["valid"])[0]
        order = reference_order(ref["c"][ids], lo, inv)
        excused, pairs = nh.check_order(ref["c"][ids][order], lo, inv, ids[order])
        print(f"{name}: {excused} of {pairs} pairs excused")
        assert excused <= hc.EXCUSED_CAP * pairs, name
    meshes, _ = hc.mesh_content()
    for name, ms in dict(content=meshes, **{f"count_{n}": hc.count_mesh(n) for n in hc.COUNTS}).items():
        ref = nh.scene_triangles(ms)
        if not ref["valid"].any():
            continue
        cen = ref["tri32"][ref["valid"]].astype(np.float64).mean(1)
        lo, inv = hc.morton_frame([(m["positions"], m.get("transform")) for m in ms])
        excused, pairs = nh.check_order(cen[reference_order(cen, lo, inv)], lo, inv)
        print(f"mesh {name}: {excused} of {pairs} pairs excused")
        assert excused <= hc.EXCUSED_CAP * pairs, name


def test_order_check_bites():
    c = np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, (500, 3))
    lo, inv = frame_of(c)
    order = reference_order(c, lo, inv)
    swapped = order.copy()
    swapped[[10, 400]] = swapped[[400, 10]]
    with pytest.raises(AssertionError):
        nh.check_order(c[swapped], lo, inv)


def test_triangle_reference_and_the_leaf_formula():
    meshes, names = hc.mesh_content()
    ref = nh.scene_triangles(meshes)
    first = np.cumsum([0] + [len(m["indices"]) for m in meshes])
    deg = names.index("degenerate")
    assert ref["valid"][first[deg]:first[deg + 1]].tolist() == hc.MESH_VALID["degenerate"]
    assert ref["valid"].sum() == ref["valid"].size - 3
    # the fp32 vertex stage lies within its bound of the float64 transform, and is what np_mesh_rays (written independently) uses
    assert (np.abs(ref["tri32"].astype(np.float64) - ref["tri64"]) <= ref["bound"]).all()
    tri, _, inst, mat, _, valid, _, _ = nr.world_triangles(meshes)
    assert tri.tobytes() == ref["tri32"].tobytes() and np.array_equal(valid, ref["valid"]) and np.array_equal(inst, ref["inst"]) and np.array_equal(mat, ref["mat"])
    # the leaf formula in fp32: strictly outside the vertices on every axis, the planes through 0 included
    lo, hi = nr.leaf_boxes(ref["tri32"][ref["valid"]])
    t = ref["tri32"][ref["valid"]].astype(np.float64)
    assert (lo.astype(np.float64) < t.min(1)).all() and (hi.astype(np.float64) > t.max(1)).all()
    ap = names.index("axis_parallel")
    flat = ref["tri32"][first[ap]:first[ap + 1]]
    assert ((flat.max(1) == flat.min(1)).sum(1) == 1).all() and (flat == 0).all(1).any()
