"""Mesh ray queries restated in numpy (include/mgs.h, "mesh ray queries"): every ray against every triangle.

trace()      float64 brute force: plane intersection and barycentrics from areas, the window (max(t_min, 0), t_max) with both ends open,
             ties in t to the lower global primitive id, visibility, position and normal as the closest-hit shader writes them; plus
             the fragile-ray mask (and which of its rays are fragile for a window end) and the second-nearest candidate.
trace_f32()  the kernel's arithmetic (k_mesh_rays.hip) in float32, operation for operation where it decides hit / miss and id: the
             shear to ray space, the edge functions with every product and difference rounded once, the double fallback at an exact
             zero, t = T / det.

A mesh is a dict: positions [V,3] f32, indices [T,3], normals [V,3] f32, material_ids [T] or None, transform 4x4 (row-major, as
capi takes it) or None, visible.  The triangle both see is the WORLD triangle in float32, M p with the products in the mesh pass's
order; a triangle with a non-finite vertex or a float cross product of exactly 0 is no triangle."""
import numpy as np

NONE = 0xFFFFFFFF
FRAGILE = 1e-5


def world_triangles(meshes):
    """(tri [N,3,3] f32 world, prim [N], inst [N], mat [N], visible [N] bool, valid [N] bool, local (P [N,3,3], Nrm [N,3,3]) f32, M [N,4,4] f32)"""
    T, inst, mat, vis, LP, LN, MM = [], [], [], [], [], [], []
    for k, m in enumerate(meshes):
        M = np.eye(4, dtype=np.float32) if m.get("transform") is None else np.asarray(m["transform"], np.float32)
        p = np.asarray(m["positions"], np.float32).reshape(-1, 3)
        idx = np.asarray(m["indices"]).reshape(-1, 3)
        w = np.empty_like(p)
        for r in range(3):   # ((x m0 + y m4) + z m8) + m12, each operation rounded once
            w[:, r] = ((p[:, 0] * M[r, 0] + p[:, 1] * M[r, 1]) + p[:, 2] * M[r, 2]) + M[r, 3]
        T.append(w[idx])
        LP.append(p[idx])
        LN.append(np.asarray(m["normals"], np.float32).reshape(-1, 3)[idx])
        inst.append(np.full(idx.shape[0], k, np.uint32))
        mid = m.get("material_ids")
        mat.append(np.zeros(idx.shape[0], np.uint32) if mid is None else np.asarray(mid, np.uint32))
        vis.append(np.full(idx.shape[0], bool(m.get("visible", True))))
        MM.append(np.broadcast_to(M, (idx.shape[0], 4, 4)))
    if not T:
        z = np.zeros((0, 3, 3), np.float32)
        return z, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, bool), np.zeros(0, bool), (z, z), np.zeros((0, 4, 4), np.float32)
    tri = np.concatenate(T).astype(np.float32)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    valid = np.isfinite(tri).all((1, 2)) & np.isfinite(c).all(1) & ~(c == 0).all(1)
    return (tri, np.arange(tri.shape[0], dtype=np.uint32), np.concatenate(inst), np.concatenate(mat), np.concatenate(vis), valid,
            (np.concatenate(LP), np.concatenate(LN)), np.concatenate(MM))


def ray_valid(O, D, tmin, tmax):
    fin = np.isfinite(O).all(1) & np.isfinite(D).all(1) & np.isfinite(tmin) & np.isfinite(tmax)
    with np.errstate(invalid="ignore"):
        return fin & (D != 0).any(1) & (tmin <= tmax)


def _shade(hit, prim, b1, b2, local, MM, dt):
    """position and normal of the winning hits (rchit.slang:50-59) in dtype dt"""
    n = hit.shape[0]
    pos, nrm = np.zeros((n, 3), dt), np.zeros((n, 3), dt)
    if not hit.any():
        return pos, nrm
    g = prim[hit].astype(np.int64)
    P, N = local[0][g].astype(dt), local[1][g].astype(dt)
    M = MM[g].astype(dt)
    c1, c2 = b1[hit].astype(dt)[:, None], b2[hit].astype(dt)[:, None]
    c0 = dt(1.0) - c1 - c2
    pl = P[:, 0] * c0 + P[:, 1] * c1 + P[:, 2] * c2
    nl = N[:, 0] * c0 + N[:, 1] * c1 + N[:, 2] * c2
    pos[hit] = np.einsum("nij,nj->ni", M[:, :3, :3], pl) + M[:, :3, 3]
    # transformRotScaleInverse = inverse(mat3(transform)) in double rounded once to f32 (the library's); the normal takes its transpose
    inv = np.linalg.inv(MM[g][:, :3, :3].astype(np.float64)).astype(np.float32).astype(dt)
    nw = np.einsum("nji,nj->ni", inv, nl)
    nrm[hit] = nw / np.linalg.norm(nw, axis=1, keepdims=True)
    return pos, nrm


CHUNK = 512   # rays per block of the brute force (memory: rays x triangles x a few vectors)


def _chunked(fn, meshes, O, D, tmin, tmax):
    O, D = np.asarray(O, np.float32).reshape(-1, 3), np.asarray(D, np.float32).reshape(-1, 3)
    tmin, tmax = np.broadcast_to(np.asarray(tmin, np.float32), O.shape[:1]), np.broadcast_to(np.asarray(tmax, np.float32), O.shape[:1])
    parts = [fn(meshes, O[i:i + CHUNK], D[i:i + CHUNK], tmin[i:i + CHUNK], tmax[i:i + CHUNK]) for i in range(0, max(O.shape[0], 1), CHUNK)]
    return {k: (v if np.isscalar(v) else np.concatenate([p[k] for p in parts])) for k, v in parts[0].items()}


def trace(meshes, O, D, tmin, tmax):
    return _chunked(_trace, meshes, O, D, tmin, tmax)


def _trace(meshes, O, D, tmin, tmax):
    """float64 brute force.  Returns a dict: hit, t, prim, inst, mat, b1, b2, pos, nrm, valid (the ray), fragile, and prim2 / hit2: the
    second-nearest candidate; window_end: a candidate's t is within FRAGILE of an end of the window.  Exact duplicates of a lower-id triangle never win (the tie rule) and are no candidates."""
    tri, prim, inst, mat, vis, valid, local, MM = world_triangles(meshes)
    O, D = np.asarray(O, np.float32).astype(np.float64), np.asarray(D, np.float32).astype(np.float64)
    tmin, tmax = np.asarray(tmin, np.float32).astype(np.float64), np.asarray(tmax, np.float32).astype(np.float64)
    R = O.shape[0]
    rv = ray_valid(O, D, tmin, tmax)
    t0 = np.maximum(tmin, 0.0)
    dup = np.zeros(tri.shape[0], bool)
    seen = {}
    for i in range(tri.shape[0]):
        key = (tri[i].tobytes(), bool(vis[i]))
        dup[i] = key in seen
        seen.setdefault(key, i)
    use = valid & vis & ~dup
    V = tri[use].astype(np.float64)
    gid = prim[use]
    res = dict(valid=rv, hit=np.zeros(R, bool), t=np.full(R, np.inf), prim=np.full(R, NONE, np.uint32), inst=np.full(R, NONE, np.uint32),
               mat=np.full(R, NONE, np.uint32), b1=np.zeros(R), b2=np.zeros(R), fragile=np.zeros(R, bool), window_end=np.zeros(R, bool), prim2=np.full(R, NONE, np.uint32),
               hit2=np.zeros(R, bool), triangles=int(tri.shape[0]), leaves=int(valid.sum()))
    if V.shape[0] and R:
        Od, Dd = np.where(rv[:, None], O, 0.0), np.where(rv[:, None], D, 1.0)
        e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        n = np.cross(e1, e2)                                                   # [T,3]
        nn = (n * n).sum(1)
        den = Dd @ n.T                                                         # [R,T]
        num = ((V[:, 0][None] - Od[:, None]) * n[None]).sum(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        p = Od[:, None] + t[..., None] * Dd[:, None]                           # [R,T,3]
        q = p - V[None, :, 0]
        with np.errstate(invalid="ignore"):
            b1 = (np.cross(q, e2[None]) * n[None]).sum(2) / nn[None]
            b2 = (np.cross(e1[None], q) * n[None]).sum(2) / nn[None]
            b0 = 1.0 - b1 - b2
            bmin = np.minimum(np.minimum(b0, b1), b2)
            ok = np.isfinite(t) & (den != 0)
            inside = ok & (bmin >= 0)
            near_in = ok & (bmin >= -FRAGILE)
            inwin = (t > t0[:, None]) & (t < tmax[:, None])
            cand = inside & inwin & rv[:, None]
            tc = np.where(cand, t, np.inf)
        # nearest and second nearest by (t, id)
        key_t = tc
        first = np.argmin(key_t, axis=1)                                       # lowest index among equal t = lowest id (gid ascending)
        rr = np.arange(R)
        hit = np.isfinite(key_t[rr, first])
        tc2 = key_t.copy()
        tc2[rr, first] = np.inf
        second = np.argmin(tc2, axis=1)
        hit2 = np.isfinite(tc2[rr, second])
        res["hit"], res["hit2"] = hit, hit2
        res["t"] = np.where(hit, key_t[rr, first], np.inf)
        res["prim"] = np.where(hit, gid[first], NONE).astype(np.uint32)
        res["prim2"] = np.where(hit2, gid[second], NONE).astype(np.uint32)
        res["inst"] = np.where(hit, inst[use][first], NONE).astype(np.uint32)
        res["mat"] = np.where(hit, mat[use][first], NONE).astype(np.uint32)
        res["b1"], res["b2"] = np.where(hit, b1[rr, first], 0.0), np.where(hit, b2[rr, first], 0.0)
        # fragile rays
        tbest = res["t"]
        with np.errstate(invalid="ignore"):
            upto = t <= np.where(hit, tbest * (1 + FRAGILE), np.inf)[:, None]  # candidates that could change the answer
            f_edge = (near_in & (np.abs(bmin) <= FRAGILE) & (t > t0[:, None] * (1 - FRAGILE)) & (t < tmax[:, None] * (1 + FRAGILE)) & upto).any(1)
            t2 = tc2[rr, second]
            f_pair = hit & hit2 & (np.abs(t2 - tbest) <= FRAGILE * np.abs(tbest))
            near_end = near_in & upto & ((np.abs(t - t0[:, None]) <= FRAGILE * np.maximum(np.abs(t), t0[:, None]))
                                         | (np.abs(t - tmax[:, None]) <= FRAGILE * np.abs(tmax[:, None])))
            f_end = near_end.any(1)
        res["fragile"] = rv & (f_edge | f_pair | f_end)
        res["window_end"] = rv & f_end          # the fragile rays on which a miss is a legitimate answer
    res["pos"], res["nrm"] = _shade(res["hit"], res["prim"], res["b1"], res["b2"], local, MM, np.float64)
    return res


def trace_f32(meshes, O, D, tmin, tmax):
    return _chunked(_trace_f32, meshes, O, D, tmin, tmax)


def _trace_f32(meshes, O, D, tmin, tmax):
    """the kernel's arithmetic in float32 (see the module's docstring); the same keys as trace() without fragile / second"""
    f = np.float32
    tri, prim, inst, mat, vis, valid, local, MM = world_triangles(meshes)
    O, D = np.asarray(O, f), np.asarray(D, f)
    tmin, tmax = np.asarray(tmin, f), np.asarray(tmax, f)
    R = O.shape[0]
    rv = ray_valid(O, D, tmin, tmax)
    t0 = np.maximum(tmin, f(0))
    use = valid & vis
    V, gid = tri[use], prim[use]
    res = dict(valid=rv, hit=np.zeros(R, bool), t=np.full(R, np.inf, f), prim=np.full(R, NONE, np.uint32), inst=np.full(R, NONE, np.uint32),
               mat=np.full(R, NONE, np.uint32), b1=np.zeros(R, f), b2=np.zeros(R, f), leaf_ok=np.ones(R, bool))
    if V.shape[0] and R:
        Os, Ds = np.where(rv[:, None], O, f(0)), np.where(rv[:, None], D, f(1))
        a = np.abs(Ds)
        kz = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        rr = np.arange(R)
        neg = Ds[rr, kz] < 0
        kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
        dz = Ds[rr, kz]
        sx, sy, sz = Ds[rr, kx] / dz, Ds[rr, ky] / dz, f(1) / dz

        V = np.ascontiguousarray(V)
        Pb = np.broadcast_to(V[None], (R,) + V.shape)                          # [R,T,3,3]

        def comp(c, k):
            return np.take_along_axis(Pb[:, :, c, :], np.broadcast_to(k[:, None, None], (R, V.shape[0], 1)), 2)[..., 0]

        def sheared(c):
            z = comp(c, kz) - Os[rr, kz][:, None]
            x = (comp(c, kx) - Os[rr, kx][:, None]) - sx[:, None] * z
            y = (comp(c, ky) - Os[rr, ky][:, None]) - sy[:, None] * z
            return x, y, z

        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ax, ay, az = sheared(0)
            bx, by, bz = sheared(1)
            cx, cy, cz = sheared(2)
            u = cx * by - cy * bx
            v = ax * cy - ay * cx
            w = bx * ay - by * ax
            zero = (u == 0) | (v == 0) | (w == 0)
            d = np.float64
            du = cx.astype(d) * by.astype(d) - cy.astype(d) * bx.astype(d)
            dv = ax.astype(d) * cy.astype(d) - ay.astype(d) * cx.astype(d)
            dw = bx.astype(d) * ay.astype(d) - by.astype(d) * ax.astype(d)
            u, v, w = np.where(zero, du.astype(f), u), np.where(zero, dv.astype(f), v), np.where(zero, dw.astype(f), w)
            su, sv, sw = np.where(zero, du, u.astype(d)), np.where(zero, dv, v.astype(d)), np.where(zero, dw, w.astype(d))
            mixed = ((su < 0) | (sv < 0) | (sw < 0)) & ((su > 0) | (sv > 0) | (sw > 0))
            det = (u + v) + w
            T = (u * (sz[:, None] * az) + v * (sz[:, None] * bz)) + w * (sz[:, None] * cz)
            t = T / det
            b1, b2 = v / det, w / det
            cand = ~mixed & (det != 0) & (t > t0[:, None]) & (t < tmax[:, None]) & rv[:, None]
        tc = np.where(cand, t, f(np.inf))
        first = np.argmin(tc, axis=1)                                          # equal t: the lowest index = the lowest id
        hit = np.isfinite(tc[rr, first])
        res["hit"] = hit
        res["t"] = np.where(hit, tc[rr, first], f(np.inf)).astype(f)
        res["prim"] = np.where(hit, gid[first], NONE).astype(np.uint32)
        res["inst"] = np.where(hit, inst[use][first], NONE).astype(np.uint32)
        res["mat"] = np.where(hit, mat[use][first], NONE).astype(np.uint32)
        res["b1"], res["b2"] = np.where(hit, b1[rr, first], f(0)).astype(f), np.where(hit, b2[rr, first], f(0)).astype(f)
        # the winning triangle's own leaf (k_mesh_bvh_leaves' box) under the traversal's node test (slabHit) with the window and the hit's
        # t as the cut: a hit the triangle test accepts must not be refused by its leaf
        lo, hi = leaf_boxes(V[first])
        res["leaf_ok"] = ~hit | slab_hit(Os, Ds, lo, hi, t0, tmax, res["t"])
    res["pos"], res["nrm"] = _shade(res["hit"], res["prim"], res["b1"], res["b2"], local, MM, np.float32)
    return res


def leaf_boxes(tri):
    """the box k_mesh_bvh_leaves gives world triangles [N,3,3] f32, for leaf_ok's slab test.  A restatement of the device formula: it
    cannot disagree with what it copies.  The device's boxes themselves are checked directly, against the records' vertices, by
    tests/test_gpu_hierarchy.py on the downloaded hierarchy."""
    f, ulp, tiny = np.float32, np.float32(1.1920929e-7), np.float32(1e-37)
    l, u = tri.min(1), tri.max(1)
    ext = u - l
    return l - (ext * (f(4) * ulp) + np.abs(l) * (f(2) * ulp) + tiny), u + (ext * (f(4) * ulp) + np.abs(u) * (f(2) * ulp) + tiny)


def slab_hit(O, D, lo, hi, t0, t1, cut):
    """slabHit of trace_traverse.h in float32, per ray against its own box, and the walk's te <= cut"""
    f, ulp = np.float32, np.float32(1.1920929e-7)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f(1) / D
        a, b = (lo - O) * inv, (hi - O) * inv
        tn = np.fmax(np.fmax(np.fmin(a[:, 0], b[:, 0]), np.fmin(a[:, 1], b[:, 1])), np.fmax(np.fmin(a[:, 2], b[:, 2]), f(0)))
        tf = np.fmin(np.fmin(np.fmax(a[:, 0], b[:, 0]), np.fmax(a[:, 1], b[:, 1])), np.fmax(a[:, 2], b[:, 2])) * (f(1) + f(4) * ulp)
        te = tn * (f(1) - f(4) * ulp)
        return (te <= tf) & (tf >= t0) & (te <= t1) & (te <= cut)


def errors(got, ref, mask):
    """largest differences of t (relative to max(1, |t|)), barycentrics, position (relative to max(1, |p|)) and normal on `mask` rays
    where both hit"""
    m = mask & ref["hit"] & got["hit"]
    if not m.any():
        return dict(t=0.0, bary=0.0, pos=0.0, nrm=0.0)
    t = np.abs(got["t"][m].astype(np.float64) - ref["t"][m]) / np.maximum(1.0, np.abs(ref["t"][m]))
    b = np.maximum(np.abs(got["b1"][m].astype(np.float64) - ref["b1"][m]), np.abs(got["b2"][m].astype(np.float64) - ref["b2"][m]))
    p = np.abs(got["pos"][m].astype(np.float64) - ref["pos"][m]) / np.maximum(1.0, np.abs(ref["pos"][m]))
    nr = np.abs(got["nrm"][m].astype(np.float64) - ref["nrm"][m])
    return dict(t=float(t.max()), bary=float(b.max()), pos=float(p.max()), nrm=float(nr.max()))
